"""What a beam call costs (slimt_hip_translate_beam_async) against the comparable existing calls, same process, alternating
rounds, one context.

Shape: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 sources, beam k = 4 and 8 (128 and 256 decoder rows), EOS bias 0
(no source ends early: every call runs its 48 steps). Three kinds of round per k:
  beam      -- slimt_hip_translate_beam_async: k rows per source, one selection launch per step (beam_select.hip);
  truncated -- slimt_hip_translate_fanout_async of the same rows, sampled at T = 1 with top-k 40 / top-p 0.9: it also stores
               each step's logits and runs one selection launch per step (sample_truncate.hip) plus the step's record /
               embed launch -- the comparable existing call;
  greedy    -- slimt_hip_translate_async of the 32 sources in the context's default mode (the persistent decoder).
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); medians and every repeat's value are printed, then
one JSON line per k.

  python tools/beam_bench.py [--rounds 10] [--repeats 3] [--sources 32] [--beams 4,8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="tiny11")
    ap.add_argument("--sources", type=int, default=32)
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, S = args.sources, args.src_len
    beams = [int(x) for x in args.beams.split(",")]
    sl = synth.make_shortlist(m.V, args.shortlist)
    ids, lens = synth.make_batch(m.V, B, S, seed=4321)
    kinds = ("beam", "truncated", "greedy")
    for k in beams:
        N = B * k
        ctx = capi.Context(gm, N, S)
        bm = ctx.beam_buffers(B, S, k)
        fo = ctx.fanout_buffers(B, S, N)
        gr = ctx.pinned_buffers(B, S)
        keys = capi._Pinned()
        keys_a = keys.array(np.uint64, (N,))
        keys_a[...] = capi.sampling_keys(7, N)
        for dst in (bm, fo, gr):
            dst[0][...] = ids
            dst[1][...] = lens
        fo[2][...] = np.repeat(np.arange(B, dtype=np.uint32), k)
        T = bm[2].shape[2]

        def submit(kind):
            if kind == "beam":
                ctx.translate_beam_async(bm, sl)
            elif kind == "truncated":
                ctx.translate_fanout_async(fo, sl, sampling=(1.0, keys_a), truncation=(40, 0.9))
            else:
                ctx.translate_async(gr, sl)
            ctx.synchronize()

        for _ in range(args.warmup):
            for kind in kinds:
                submit(kind)
        assert (bm[3] == T).all() and (fo[4] == T).all()  # (every row ran all its steps)
        times = {kind: [] for kind in kinds}
        for _ in range(args.repeats):
            per = {kind: [] for kind in kinds}
            for _ in range(args.rounds):
                for kind in kinds:
                    t0 = time.perf_counter()
                    submit(kind)
                    per[kind].append(time.perf_counter() - t0)
            for kind in kinds:
                times[kind].append(statistics.median(per[kind]))
        out = {"preset": args.preset, "sources": B, "beam": k, "rows": N, "S": S, "Tmax": T, "shortlist": args.shortlist,
               "rounds": args.rounds, "repeats": args.repeats, "hw_queues": capi.lib().slimt_hip_hw_queues()}
        for kind in kinds:
            med = statistics.median(times[kind])
            out[kind] = {"call_ms_median": round(med * 1e3, 3), "call_ms_repeats": [round(t * 1e3, 3) for t in times[kind]]}
            print("k = %d %-9s %.3f ms per call (repeats %s)" % (k, kind, med * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind])))
        med = {kind: statistics.median(times[kind]) for kind in kinds}
        out["beam_step_over_truncated_step_us"] = round((med["beam"] - med["truncated"]) / T * 1e6, 2)
        out["beam_over_truncated"] = round(med["beam"] / med["truncated"], 4)
        out["beam_over_greedy"] = round(med["beam"] / med["greedy"], 4)
        print("k = %d: a beam step costs %+.2f us against the truncated call's step; the beam call takes %.2f x the greedy call "
              "on the %d sources" % (k, out["beam_step_over_truncated_step_us"], out["beam_over_greedy"], B))
        print(json.dumps(out))
        keys.free()
        ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
