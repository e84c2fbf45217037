"""Sampled decoding (slimt_hip_ctx_set_sampling) against the scored greedy call, same process, interleaved rounds.

Headline shape: tiny11, B = 256, S = 32, a 4096-id shortlist, `--workers` contexts (HIP streams) each submitting one
pinned asynchronous scored translate per round. Two kinds of round, alternating so that clocks and neighbours drift into
both alike:
  scored  -- greedy, scored (the reference point);
  sampled -- the same batches drawn at `--temperature` under per-sentence keys, scored.
Target tokens/s counts out_len of the round's own outputs (sampled sentences end where their draws put EOS). With
`--merge K` every context submits K sub-batches of B / K in one merged launch.

  python tools/sampling_bench.py [--workers 20] [--rounds 10] [--merge 1] [--batch 256] [--temperature 1.0]
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--merge", type=int, default=1)
    ap.add_argument("--eos-bias", type=float, default=0.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    capi.request_hw_queues(32)
    m = synth.make_model(args.preset, eos_bias=args.eos_bias)
    gm = capi.Model(m, device=0)
    gm.set_decoder_budget(256)
    B, S, W, K = args.batch, args.src_len, args.workers, args.merge
    T = max(int(np.float32(1.5) * np.float32(S)), 1)
    sl = synth.make_shortlist(m.V, args.shortlist)
    sub = max(1, B // K)
    rows = B if K == 1 else max(B, capi.translate_many_rows([sub] * K))  # (sub-batches start at aligned rows)
    ctxs = [capi.Context(gm, rows, S) for _ in range(W)]
    pins, work = [], []  # per context: K parts of (bufs, scores, keys)
    for w, c in enumerate(ctxs):
        parts = []
        for j in range(K):
            ids, lens = synth.make_batch(m.V, sub, S, seed=4321 + 31 * w + j)
            arrs = []
            for dt_, shape in ((np.uint32, (sub, S)), (np.uint32, (sub,)), (np.uint32, (sub, T)), (np.uint32, (sub,)),
                               (np.float32, (sub, T))):
                p = capi._Pinned()
                pins.append(p)
                arrs.append(p.array(dt_, shape))
            arrs[0][...] = ids
            arrs[1][...] = lens
            kp = capi._Pinned()
            pins.append(kp)
            keys = kp.array(np.uint64, (sub,))
            keys[...] = capi.sampling_keys(w * K + j, sub)
            parts.append([tuple(arrs[:4]) + (None,), arrs[4], keys])
        work.append(parts)

    def submit(kind):
        for c, parts in zip(ctxs, work):
            sm = None if kind == "scored" else (args.temperature, [p[2] for p in parts])
            if K == 1:
                c.translate_async(parts[0][0], sl, scores=parts[0][1], sampling=None if sm is None else (sm[0], sm[1][0]))
            else:
                c.translate_many_async([p[0] for p in parts], sl, scores=[p[1] for p in parts], sampling=sm)

    def run(kind):
        t0 = time.perf_counter()
        submit(kind)
        for c in ctxs:
            c.synchronize()
        dt = time.perf_counter() - t0
        return sum(int(p[0][3].sum()) for parts in work for p in parts) / dt

    kinds = ("scored", "sampled")
    for _ in range(args.warmup):
        for k in kinds:
            run(k)
    res = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k in kinds[r % 2:] + kinds[:r % 2]:
            res[k].append(run(k))
    for c in ctxs:
        c.close()
    for k, v in res.items():
        print(json.dumps({"run": k, "merge": K, "median_tok_s": statistics.median(v), "min": min(v), "max": max(v),
                          "rounds": [round(x) for x in v]}))
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"summary": f"{args.preset} B={B} S={S} shortlist={args.shortlist} workers={W} merge={K}",
                      "temperature": args.temperature, "sampled_over_scored": med["sampled"] / med["scored"],
                      "scored_tok_s": med["scored"], "sampled_tok_s": med["sampled"]}))
    for p in pins:
        p.free()
    gm.close()


if __name__ == "__main__":
    main()
