"""Teacher-forced scoring in one pass (slimt_hip_score_async) against the forced-prefix scored call, same process,
interleaved rounds.

Headline shape: tiny11, B = 256, S = 32, T = 48 (= floor(1.5 S): what the prefix path can still take), a 4096-id
shortlist, targets of T tokens from the shortlist ending in EOS at T; `--workers` contexts (HIP streams) each submitting
one pinned asynchronous call per round, at the hardware-queue setting the process starts with. Two kinds of round,
alternating so that clocks and neighbours drift into both alike:
  forced -- slimt_hip_translate_async with the targets as forced prefixes, scored (the baseline: the persistent decoder,
            one step per target token);
  tall   -- slimt_hip_score_async on the same sources and targets (every target position in one pass).
Both score B T target tokens per context and round; target tokens/s counts those.

  python tools/score_bench.py [--workers 20] [--rounds 10] [--batch 256] [--src-len 32] [--tgt-len 48] [--only tall]
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
    ap.add_argument("--tgt-len", type=int, default=0, help="0: floor(1.5 * src-len)")
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("forced", "tall"), default=None, help="one kind of round only (profiling runs)")
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    gm.set_decoder_budget(256)
    B, S, W = args.batch, args.src_len, args.workers
    Tmax = max(int(np.float32(1.5) * np.float32(S)), 1)
    T = args.tgt_len or Tmax
    sl = synth.make_shortlist(m.V, args.shortlist)
    pool = sl[sl != 0]
    kinds = (args.only,) if args.only else ("forced", "tall")
    if "forced" in kinds and T != Tmax:
        raise SystemExit(f"the forced-prefix baseline takes targets of {Tmax} tokens at S = {S}, not {T} (--only tall)")
    ctxs = [capi.Context(gm, B, S) for _ in range(W)]
    pins, work = [], []
    for w in range(W):
        rng = np.random.default_rng(99 + w)
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        arrs = {}
        for name, dt_, shape in (("ids", np.uint32, (B, S)), ("len", np.uint32, (B,)), ("out", np.uint32, (B, T)),
                                 ("ol", np.uint32, (B,)), ("fsc", np.float32, (B, T)), ("tg", np.uint32, (B, T)),
                                 ("tl", np.uint32, (B,)), ("sc", np.float32, (B, T))):
            p = capi._Pinned()
            pins.append(p)
            arrs[name] = p.array(dt_, shape)
        arrs["ids"][...] = ids
        arrs["len"][...] = lens
        arrs["tg"][...] = rng.choice(pool, size=(B, T))
        arrs["tg"][:, T - 1] = 0  # EOS at T
        arrs["tl"][...] = T
        work.append(arrs)

    def submit(kind):
        for c, a in zip(ctxs, work):
            if kind == "forced":
                c.translate_async((a["ids"], a["len"], a["out"], a["ol"], None), sl, scores=a["fsc"], prefix=(a["tg"], a["tl"]))
            else:
                c.score_async((a["ids"], a["len"], a["tg"], a["tl"], a["sc"], None), sl)

    def run(kind):
        t0 = time.perf_counter()
        submit(kind)
        for c in ctxs:
            c.synchronize()
        return W * B * T / (time.perf_counter() - t0)

    for _ in range(args.warmup):
        for k in kinds:
            run(k)
    if len(kinds) == 2:  # the two paths score the same tokens: how far apart are they?
        err = max(float(np.max(np.abs(a["fsc"].astype(np.float64) - a["sc"]))) for a in work)
        assert all(int(a["ol"].min()) == T for a in work)
        print(json.dumps({"max_abs_score_difference_forced_vs_tall": err}))
    res = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k in kinds[r % 2:] + kinds[:r % 2]:
            res[k].append(run(k))
    for c in ctxs:
        c.close()
    for k, v in res.items():
        print(json.dumps({"run": k, "median_tok_s": statistics.median(v), "min": min(v), "max": max(v),
                          "rounds": [round(x) for x in v]}))
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": f"{args.preset} B={B} S={S} T={T} shortlist={args.shortlist} workers={W} hw_queues={capi.lib().slimt_hip_hw_queues()}"}
    summary.update({k + "_tok_s": v for k, v in med.items()})
    if len(kinds) == 2:
        summary["tall_over_forced"] = med["tall"] / med["forced"]
    print(json.dumps(summary))
    for p in pins:
        p.free()
    gm.close()


if __name__ == "__main__":
    main()
