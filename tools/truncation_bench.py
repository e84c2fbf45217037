"""Truncated sampling (slimt_hip_ctx_set_sampling_truncation) against the untruncated sampled call, same process,
interleaved rounds.

Headline shape: tiny11, B = 256, S = 32, a 4096-id shortlist, `--workers` contexts (HIP streams) each submitting one
pinned asynchronous scored translate per round. Four kinds of round, alternating so that clocks and neighbours drift
into all alike:
  fused     -- sampled at `--temperature` by the persistent decoder (decode mode 0);
  stage     -- the same draws by the per-stage kernels (decode mode 1): the path a truncated call takes, without the
               truncation (logits gemm with the sampled arg-max epilogue);
  truncated_m1 -- the same batches with `--top-k` / `--top-p` on a context in decode mode 1: stage's kernels, but the logits
               gemm stores the row and the selection kernel (sample_truncate.hip) draws;
  truncated -- ... on a context in decode mode 0, what a caller gets by default: the per-stage decoder behind the
               persistent encoder.
Target tokens/s counts out_len of the round's own outputs (a truncated sentence ends where its draws put EOS).

  python tools/truncation_bench.py [--workers 20] [--rounds 6] [--batch 256] [--top-k 40] [--top-p 0.9]
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
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--eos-bias", type=float, default=0.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--kinds", default="fused,stage,truncated_m1,truncated")
    args = ap.parse_args()

    from slimt_amd import capi, synth
    capi.request_hw_queues(32)
    m = synth.make_model(args.preset, eos_bias=args.eos_bias)
    gm = capi.Model(m, device=0)
    gm.set_decoder_budget(256)
    B, S, W = args.batch, args.src_len, args.workers
    T = max(int(np.float32(1.5) * np.float32(S)), 1)
    sl = synth.make_shortlist(m.V, args.shortlist)
    ctxs = [capi.Context(gm, B, S) for _ in range(W)]
    pins, work = [], []  # per context: (bufs, scores, keys)
    for w, c in enumerate(ctxs):
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        arrs = []
        for dt_, shape in ((np.uint32, (B, S)), (np.uint32, (B,)), (np.uint32, (B, T)), (np.uint32, (B,)), (np.float32, (B, T))):
            p = capi._Pinned()
            pins.append(p)
            arrs.append(p.array(dt_, shape))
        arrs[0][...] = ids
        arrs[1][...] = lens
        kp = capi._Pinned()
        pins.append(kp)
        keys = kp.array(np.uint64, (B,))
        keys[...] = capi.sampling_keys(w, B)
        work.append((tuple(arrs[:4]) + (None,), arrs[4], keys))

    def run(kind):
        for c in ctxs:
            c.set_decode_mode(0 if kind in ("fused", "truncated") else 1)
        t0 = time.perf_counter()
        for c, (bufs, sc, keys) in zip(ctxs, work):
            c.translate_async(bufs, sl, scores=sc, sampling=(args.temperature, keys),
                              truncation=(args.top_k, args.top_p) if kind.startswith("truncated") else None)
        for c in ctxs:
            c.synchronize()
        dt = time.perf_counter() - t0
        return sum(int(bufs[3].sum()) for bufs, _, _ in work) / dt, dt

    kinds = tuple(args.kinds.split(","))
    for _ in range(args.warmup):
        for k in kinds:
            run(k)
    res = {k: [] for k in kinds}
    secs = {k: [] for k in kinds}
    for r in range(args.rounds):
        o = r % len(kinds)
        for k in kinds[o:] + kinds[:o]:
            tok_s, dt = run(k)
            res[k].append(tok_s)
            secs[k].append(dt)
    for c in ctxs:
        c.close()
    for k, v in res.items():
        print(json.dumps({"run": k, "median_tok_s": statistics.median(v), "min": min(v), "max": max(v),
                          "median_round_ms": 1e3 * statistics.median(secs[k]), "rounds": [round(x) for x in v]}))
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": f"{args.preset} B={B} S={S} shortlist={args.shortlist} workers={W}", "temperature": args.temperature,
               "top_k": args.top_k, "top_p": args.top_p}
    if "truncated_m1" in med and "stage" in med:
        summary["truncated_m1_over_stage"] = med["truncated_m1"] / med["stage"]
    if "truncated" in med and "stage" in med:
        summary["truncated_over_stage"] = med["truncated"] / med["stage"]
    if "truncated" in med and "fused" in med:
        summary["truncated_over_fused"] = med["truncated"] / med["fused"]
    print(json.dumps(summary))
    for p in pins:
        p.free()
    gm.close()


if __name__ == "__main__":
    main()
