"""What drawing several samples per source from one encoding saves (slimt_hip_translate_fanout_async) against the same work
done with every row carrying a copy of its source (slimt_hip_translate_async on the duplicated rows), same process,
alternating rounds.

Headline shape: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 sources x 8 rows per call (256 decoder rows), truncated
sampling (top-k 40, top-p 0.9) at T = 1, rows sorted by source; `--workers` contexts (HIP streams) each submitting one pinned
asynchronous call per round, at the hardware-queue setting the process starts with. Three kinds of round, alternating so
that clocks and neighbours drift into all alike:
  fanout     -- slimt_hip_translate_fanout_async: 32 rows encoded, their K / V projected once, 256 rows decoded step-wise;
  duplicated -- slimt_hip_translate_async on src_ids[row_src] in decode mode 1, truncated alike: 256 rows encoded; the same
                decoder kernels but for the attention, so the difference is what fan-out saves;
  persistent -- the duplicated call in the context's default mode, sampled WITHOUT truncation: the persistent decoder, which
                truncated sampling cannot take -- the upper reference for a fan-out inside that kernel.
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); the medians, every repeat's value and the spread of
the duplicated call's own repeats are printed, then one JSON line. Tokens of fanout and duplicated are compared bit for bit.

  python tools/fanout_bench.py [--workers 4] [--rounds 10] [--repeats 3] [--sources 32] [--per-source 8]
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
    ap.add_argument("--per-source", type=int, default=8)
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, C, S, W = args.sources, args.per_source, args.src_len, args.workers
    N = B * C
    sl = synth.make_shortlist(m.V, args.shortlist)
    trunc = (args.top_k, args.top_p)
    kinds = ("fanout", "duplicated", "persistent")
    ctxs = [capi.Context(gm, N, S) for _ in range(W)]  # (max_batch N: the duplicated calls need it)
    T = ctxs[0].pinned_buffers(1, S)[2].shape[1]
    pins, work = [], []

    def pinned(dt, shape):
        p = capi._Pinned()
        pins.append(p)
        return p.array(dt, shape)

    for w in range(W):
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        src = np.repeat(np.arange(B, dtype=np.uint32), C)
        keys = pinned(np.uint64, (N,))
        keys[...] = capi.sampling_keys(7 + w, N)
        fan = (pinned(np.uint32, (B, S)), pinned(np.uint32, (B,)), pinned(np.uint32, (N,)), pinned(np.uint32, (N, T)),
               pinned(np.uint32, (N,)), None)
        for dst, val in zip(fan, (ids, lens, src)):
            dst[...] = val
        dup = {}
        for kind in ("duplicated", "persistent"):
            dup[kind] = (pinned(np.uint32, (N, S)), pinned(np.uint32, (N,)), pinned(np.uint32, (N, T)), pinned(np.uint32, (N,)), None)
            dup[kind][0][...] = ids[src]
            dup[kind][1][...] = lens[src]
        work.append((fan, dup, keys))

    def submit(kind):
        for ctx, (fan, dup, keys) in zip(ctxs, work):
            if kind == "fanout":
                ctx.translate_fanout_async(fan, sl, sampling=(1.0, keys), truncation=trunc)
            elif kind == "duplicated":
                ctx.set_decode_mode(1)
                ctx.translate_async(dup[kind], sl, sampling=(1.0, keys), truncation=trunc)
                ctx.set_decode_mode(0)
            else:
                ctx.translate_async(dup[kind], sl, sampling=(1.0, keys))

    def sync():
        for ctx in ctxs:
            ctx.synchronize()

    for _ in range(args.warmup):
        for kind in kinds:
            submit(kind)
            sync()
    for fan, dup, _ in work:  # the two step-wise kinds drew the same bits
        assert np.array_equal(fan[4], dup["duplicated"][3]) and np.array_equal(fan[3], dup["duplicated"][2])
    times = {k: [] for k in kinds}  # per repeat: median seconds of a round
    for _ in range(args.repeats):
        per = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind in kinds:
                t0 = time.perf_counter()
                submit(kind)
                sync()
                per[kind].append(time.perf_counter() - t0)
        for kind in kinds:
            times[kind].append(statistics.median(per[kind]))
    out = {"preset": args.preset, "sources": B, "per_source": C, "S": S, "Tmax": T, "shortlist": args.shortlist, "top_k": trunc[0],
           "top_p": trunc[1], "workers": W, "rounds": args.rounds, "repeats": args.repeats,
           "hw_queues": capi.lib().slimt_hip_hw_queues()}
    for kind in kinds:
        med = statistics.median(times[kind])
        out[kind] = {"round_ms_median": round(med * 1e3, 3), "round_ms_repeats": [round(t * 1e3, 3) for t in times[kind]]}
        print("%-10s round %.3f ms (repeats %s)" % (kind, med * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind])))
    med = {k: statistics.median(times[k]) for k in kinds}
    spread = max(times["duplicated"]) - min(times["duplicated"])
    out["duplicated_spread_ms"] = round(spread * 1e3, 3)
    out["fanout_gain"] = round(1.0 - med["fanout"] / med["duplicated"], 4)
    out["not_slower"] = bool(med["fanout"] <= med["duplicated"] + spread)
    out["persistent_over_fanout"] = round(med["persistent"] / med["fanout"], 4)
    print("fanout against duplicated: %.1f%% less time; the duplicated call's own repeats spread over %.3f ms; the persistent "
          "decoder on the duplicated rows takes %.2f x the fan-out call's time" % (out["fanout_gain"] * 100, spread * 1e3,
                                                                                 out["persistent_over_fanout"]))
    print(json.dumps(out))
    for ctx in ctxs:
        ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
