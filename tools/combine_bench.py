"""What the combined selection costs a fan-out call (slimt_hip_ctx_set_fanout_combine: combine_step.hip, one launch per step
that selects, records and embeds for every row of a group), same process, alternating rounds.

Shape: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 groups of m = 2 and m = 4 rows (group g reads the sources g, g + 1,
...), scores on, EOS bias 0 so that rows rarely end before Tmax (each kind's count of recorded tokens is printed); one context,
one pinned asynchronous call per round. Per m three kinds of round, alternating so that clocks drift into all alike:
  combined  -- weights (1, -0.5, ...) and a gap of -4
  stored    -- the same rows un-armed but under a step constraint that bans nothing (a suppressed id outside the shortlist):
               the stored-logits greedy path, step_constrain.hip's selection per row: the like-for-like baseline
  plain     -- the same rows un-armed: the logits gemm's own arg-max epilogue, no stored row
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); the medians, every repeat's value and each kind's
spread over its repeats are printed, then one JSON line.

  python tools/combine_bench.py [--rounds 10] [--repeats 3] [--groups 32]
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
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    G, S = args.groups, args.src_len
    sl = synth.make_shortlist(m.V, args.shortlist)
    outside = int(np.setdiff1d(np.arange(m.V, dtype=np.uint32), sl)[0])
    ids, lens = synth.make_batch(m.V, G, S, seed=4321)
    ctx = capi.Context(gm, 4 * G, S)
    T = ctx.pinned_buffers(1, S)[2].shape[1]
    pins, work, kinds = [], {}, []

    def pinned(dt, shape):
        p = capi._Pinned()
        pins.append(p)
        return p.array(dt, shape)

    for members in (2, 4):
        N = G * members
        fan = (pinned(np.uint32, (G, S)), pinned(np.uint32, (G,)), pinned(np.uint32, (N,)), pinned(np.uint32, (N, T)),
               pinned(np.uint32, (N,)), None)
        rows = np.asarray([(g + j) % G for g in range(G) for j in range(members)], np.uint32)
        for dst, val in zip(fan, (ids, lens, rows)):
            dst[...] = val
        sc = pinned(np.float32, (N, T))
        w = (1.0, -0.5, 0.25, -0.25)[:members]
        for kind, opt in (("combined", dict(combine=(w, -4.0))), ("stored", dict(constraints=dict(suppress=(outside,)))), ("plain", {})):
            work["%s%d" % (kind, members)] = (fan, sc, opt)
            kinds.append("%s%d" % (kind, members))

    def run(kind):
        fan, sc, opt = work[kind]
        ctx.translate_fanout_async(fan, sl, scores=sc, **opt)
        ctx.synchronize()

    tokens = {}
    for _ in range(args.warmup):
        for kind in kinds:
            run(kind)
            tokens[kind] = int(work[kind][0][4].sum())
    times = {k: [] for k in kinds}  # per repeat: median seconds of a call
    for _ in range(args.repeats):
        per = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind in kinds:
                t0 = time.perf_counter()
                run(kind)
                per[kind].append(time.perf_counter() - t0)
        for kind in kinds:
            times[kind].append(statistics.median(per[kind]))
    out = {"preset": args.preset, "groups": G, "S": S, "Tmax": T, "shortlist": args.shortlist, "rounds": args.rounds,
           "repeats": args.repeats, "hw_queues": capi.lib().slimt_hip_hw_queues()}
    med = {}
    for kind in kinds:
        med[kind] = statistics.median(times[kind])
        spread = max(times[kind]) - min(times[kind])
        out[kind] = {"call_ms_median": round(med[kind] * 1e3, 3), "call_ms_repeats": [round(t * 1e3, 3) for t in times[kind]],
                     "spread_ms": round(spread * 1e3, 3), "tokens": tokens[kind]}
        print("%-10s call %.3f ms (repeats %s; spread %.3f ms; %d tokens)" % (
            kind, med[kind] * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind]), spread * 1e3, tokens[kind]))
    for members in (2, 4):
        a, b, c = (med["%s%d" % (k, members)] for k in ("combined", "stored", "plain"))
        out["m%d_combined_over_stored" % members], out["m%d_combined_over_plain" % members] = round(a / b, 4), round(a / c, 4)
        print("m = %d: combined / stored = %.4f, combined / plain = %.4f" % (members, a / b, a / c))
    print(json.dumps(out))
    ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
