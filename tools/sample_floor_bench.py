"""What a step's selection costs a sampled fan-out call by the kind of truncation: the min-p / epsilon floor
(slimt_hip_ctx_set_sampling_floor: sample_floor.hip, one read of the row) against top-k / top-p
(slimt_hip_ctx_set_sampling_truncation: sample_truncate.hip, a radix select over several reads), against locally typical
sampling (slimt_hip_ctx_set_sampling_typical: sample_typical.hip, one read and a radix descent in registers) and against none,
same process, alternating rounds.

Shape: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 sources x 8 rows per call (256 decoder rows), T = 1, EOS bias 0 so
that rows rarely end before Tmax (each kind's count of recorded tokens is printed); `--workers` contexts (HIP streams) each
submitting one pinned asynchronous fan-out call per round, at the hardware-queue setting the process starts with. Four kinds
of round, alternating so that clocks and neighbours drift into all alike:
  floored    -- min_p 0.05, epsilon 0.02
  truncated  -- top-k 40, top-p 0.9, the same rows and keys
  nucleus    -- top-p 0.9 alone (the weighted radix descent typical sampling is compared with)
  typical    -- mass 0.9
  plain      -- the untruncated sampled call (the logits gemm's own arg-max epilogue, no stored row)
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); the medians, every repeat's value and each kind's
spread over its repeats are printed, then one JSON line.

  python tools/sample_floor_bench.py [--workers 4] [--rounds 10] [--repeats 3] [--sources 32] [--per-source 8]
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
    ap.add_argument("--min-p", type=float, default=0.05)
    ap.add_argument("--epsilon", type=float, default=0.02)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--typical", type=float, default=0.9)
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
    options = {"floored": dict(floor=(args.min_p, args.epsilon)), "truncated": dict(truncation=(args.top_k, args.top_p)),
               "nucleus": dict(truncation=(0, args.top_p)), "typical": dict(typical=args.typical), "plain": {}}
    kinds = tuple(options)
    ctxs = [capi.Context(gm, N, S) for _ in range(W)]
    T = ctxs[0].pinned_buffers(1, S)[2].shape[1]
    pins, work = [], []

    def pinned(dt, shape):
        p = capi._Pinned()
        pins.append(p)
        return p.array(dt, shape)

    for w in range(W):
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        keys = pinned(np.uint64, (N,))
        keys[...] = capi.sampling_keys(7 + w, N)
        fan = (pinned(np.uint32, (B, S)), pinned(np.uint32, (B,)), pinned(np.uint32, (N,)), pinned(np.uint32, (N, T)),
               pinned(np.uint32, (N,)), None)
        for dst, val in zip(fan, (ids, lens, np.repeat(np.arange(B, dtype=np.uint32), C))):
            dst[...] = val
        work.append((fan, keys))

    def submit(kind):
        for ctx, (fan, keys) in zip(ctxs, work):
            ctx.translate_fanout_async(fan, sl, sampling=(1.0, keys), **options[kind])

    def sync():
        for ctx in ctxs:
            ctx.synchronize()

    tokens = {}
    for _ in range(args.warmup):
        for kind in kinds:
            submit(kind)
            sync()
            tokens[kind] = int(sum(int(fan[4].sum()) for fan, _ in work))
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
    out = {"preset": args.preset, "sources": B, "per_source": C, "S": S, "Tmax": T, "shortlist": args.shortlist,
           "min_p": args.min_p, "epsilon": args.epsilon, "top_k": args.top_k, "top_p": args.top_p, "typical_mass": args.typical, "workers": W,
           "rounds": args.rounds, "repeats": args.repeats, "hw_queues": capi.lib().slimt_hip_hw_queues()}
    med = {}
    for kind in kinds:
        med[kind] = statistics.median(times[kind])
        spread = max(times[kind]) - min(times[kind])
        out[kind] = {"round_ms_median": round(med[kind] * 1e3, 3), "round_ms_repeats": [round(t * 1e3, 3) for t in times[kind]],
                     "spread_ms": round(spread * 1e3, 3), "tokens": tokens[kind]}
        print("%-10s round %.3f ms (repeats %s; spread %.3f ms; %d tokens)" % (
            kind, med[kind] * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind]), spread * 1e3, tokens[kind]))
    out["floored_over_truncated"] = round(med["floored"] / med["truncated"], 4)
    out["floored_over_plain"] = round(med["floored"] / med["plain"], 4)
    print("floored / truncated = %.4f, floored / plain = %.4f" % (out["floored_over_truncated"], out["floored_over_plain"]))
    out["typical_over_nucleus"] = round(med["typical"] / med["nucleus"], 4)
    out["typical_over_plain"] = round(med["typical"] / med["plain"], 4)
    print("typical / nucleus = %.4f, typical / plain = %.4f" % (out["typical_over_nucleus"], out["typical_over_plain"]))
    print(json.dumps(out))
    for ctx in ctxs:
        ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
