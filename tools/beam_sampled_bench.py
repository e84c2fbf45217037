"""What sampling without replacement costs on a beam call (slimt_hip_ctx_set_beam_sampling) against the un-armed beam call
and the truncated sampled fan-out of the same row count: same process, alternating rounds, one context, pinned asynchronous
calls -- tools/beam_bench.py's shape (tiny11, S = 32, Tmax 48, a 4096-id shortlist, 32 sources, EOS bias 0) and manner.

  sampled   -- slimt_hip_translate_beam_async armed: one launch of beam_sampled.hip's selection per step;
  beam      -- the same call un-armed: beam_select.hip's selection;
  truncated -- slimt_hip_translate_fanout_async of the same rows, sampled at T = 1 with top-k 40 / top-p 0.9.
With EOS bias 0 a sampled hypothesis may still draw EOS early; the armed call is submitted with a fixed step budget like the
others, so every call runs its 48 steps' launches.

  python tools/beam_sampled_bench.py [--rounds 10] [--repeats 3] [--sources 32] [--beams 4,8]
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
    ap.add_argument("--sources", type=int, default=32)
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model("tiny11", eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, S = args.sources, 32
    sl = synth.make_shortlist(m.V, 4096)
    ids, lens = synth.make_batch(m.V, B, S, seed=4321)
    kinds = ("sampled", "beam", "truncated")
    for k in [int(x) for x in args.beams.split(",")]:
        N = B * k
        ctx = capi.Context(gm, N, S)
        bm = ctx.beam_buffers(B, S, k)
        fo = ctx.fanout_buffers(B, S, N)
        pins = [capi._Pinned() for _ in range(3)]
        row_keys = pins[0].array(np.uint64, (N,))
        row_keys[...] = capi.sampling_keys(7, N)
        src_keys = pins[1].array(np.uint64, (B,))
        src_keys[...] = capi.sampling_keys(7, B)
        pert = pins[2].array(np.float32, (B, k))
        for dst in (bm, fo):
            dst[0][...] = ids
            dst[1][...] = lens
        fo[2][...] = np.repeat(np.arange(B, dtype=np.uint32), k)
        T = bm[2].shape[2]

        def submit(kind):
            if kind == "sampled":
                ctx.translate_beam_async(bm, sl, sampling_keys=src_keys, perturbed=pert)
            elif kind == "beam":
                ctx.translate_beam_async(bm, sl)
            else:
                ctx.translate_fanout_async(fo, sl, sampling=(1.0, row_keys), truncation=(40, 0.9))
            ctx.synchronize()

        for _ in range(args.warmup):
            for kind in kinds:
                submit(kind)
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
        med = {kind: statistics.median(times[kind]) for kind in kinds}
        out = {"sources": B, "beam": k, "rows": N, "S": S, "Tmax": T, "rounds": args.rounds, "repeats": args.repeats,
               "hw_queues": capi.lib().slimt_hip_hw_queues()}
        for kind in kinds:
            out[kind] = {"call_ms_median": round(med[kind] * 1e3, 3), "call_ms_repeats": [round(t * 1e3, 3) for t in times[kind]]}
            print("k = %d %-9s %.3f ms per call (repeats %s)" % (k, kind, med[kind] * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind])))
        out["sampled_step_over_beam_step_us"] = round((med["sampled"] - med["beam"]) / T * 1e6, 2)
        out["sampled_over_truncated"] = round(med["sampled"] / med["truncated"], 4)
        print(json.dumps(out))
        for p in pins:
            p.free()
        ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
