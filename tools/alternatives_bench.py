"""What arming the scorer's alternatives costs (slimt_hip_ctx_set_score_alternatives): the same slimt_hip_score_async call
armed and unarmed, same process, interleaved rounds.

Headline shape: tiny11, B = 256, S = 32, T = 48, a 4096-id shortlist, targets of T random tokens from the
shortlist; `--workers` contexts (HIP streams) each submitting one pinned asynchronous call per round, at the
hardware-queue setting the process starts with. Two kinds of round, alternating so that clocks and neighbours drift into
both alike:
  plain -- slimt_hip_score_async;
  armed -- the same call with k alternatives (ids, scores and ranks, pinned like the scores).
Both score B T target tokens per context and round; target tokens/s counts those. After the rounds the output-layer
kernel families of each kind are timed on one context alone with the library's event profile, next to the call's wall
time on that context: the per-kernel split.

  python tools/alternatives_bench.py [--workers 20] [--rounds 10] [--k 8] [--batch 256] [--src-len 32] [--tgt-len 48]
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
    ap.add_argument("--k", type=int, default=8)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, S, W, k = args.batch, args.src_len, args.workers, args.k
    T = args.tgt_len or max(int(np.float32(1.5) * np.float32(S)), 1)
    sl = synth.make_shortlist(m.V, args.shortlist)
    ctxs = [capi.Context(gm, B, S) for _ in range(W)]
    pins, work = [], []
    for w in range(W):
        rng = np.random.default_rng(99 + w)
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        arrs = {}
        for name, dt_, shape in (("ids", np.uint32, (B, S)), ("len", np.uint32, (B,)), ("tg", np.uint32, (B, T)),
                                 ("tl", np.uint32, (B,)), ("sc", np.float32, (B, T)), ("sc2", np.float32, (B, T)),
                                 ("ai", np.uint32, (B, T, k)), ("as", np.float32, (B, T, k)), ("ar", np.uint32, (B, T))):
            p = capi._Pinned()
            pins.append(p)
            arrs[name] = p.array(dt_, shape)
        arrs["ids"][...] = ids
        arrs["len"][...] = lens
        arrs["tg"][...] = rng.choice(sl, size=(B, T))
        arrs["tl"][...] = T
        work.append(arrs)
    kinds = ("plain", "armed")

    def submit(kind, c, a):
        if kind == "plain":
            c.score_async((a["ids"], a["len"], a["tg"], a["tl"], a["sc"], None), sl)
        else:
            c.score_async((a["ids"], a["len"], a["tg"], a["tl"], a["sc2"], None), sl, alternatives=(a["ai"], a["as"], a["ar"]))

    def run(kind):
        t0 = time.perf_counter()
        for c, a in zip(ctxs, work):
            submit(kind, c, a)
        for c in ctxs:
            c.synchronize()
        return W * B * T / (time.perf_counter() - t0)

    for _ in range(args.warmup):
        for kd in kinds:
            run(kd)
    for a in work:  # the armed call's scores are the plain call's bits; the ranks agree with the ids
        assert np.array_equal(a["sc"].view(np.uint32), a["sc2"].view(np.uint32))
        hit = a["ar"] < k
        assert np.array_equal(np.take_along_axis(a["ai"], np.minimum(a["ar"], k - 1)[..., None], 2)[..., 0][hit], a["tg"][hit])
    res = {kd: [] for kd in kinds}
    for r in range(args.rounds):
        for kd in kinds[r % 2:] + kinds[:r % 2]:
            res[kd].append(run(kd))
    for kd, v in res.items():
        print(json.dumps({"run": kd, "median_tok_s": statistics.median(v), "min": min(v), "max": max(v),
                          "rounds": [round(x) for x in v]}))
    med = {kd: statistics.median(v) for kd, v in res.items()}
    summary = {"summary": f"{args.preset} B={B} S={S} T={T} shortlist={args.shortlist} k={k} workers={W} "
                          f"hw_queues={capi.lib().slimt_hip_hw_queues()}"}
    summary.update({kd + "_tok_s": v for kd, v in med.items()})
    summary["armed_time_over_plain"] = med["plain"] / med["armed"]
    print(json.dumps(summary))
    # one context alone: the call's wall time and, family by family, its kernels' summed time (event profile), medians
    c, a = ctxs[0], work[0]
    fams = {"output_layer": capi.K_LOGITS, "decoder_gemms": capi.K_GEMM_DEC, "attention": capi.K_ATTN_DEC, "ssru_scan": capi.K_SSRU}
    split = {}
    for kd in kinds:
        wall = []
        for _ in range(max(args.rounds, 8)):
            t0 = time.perf_counter()
            submit(kd, c, a)
            c.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        split[kd] = {"call_ms": statistics.median(wall)}
        for name, fam in fams.items():
            ms = []
            for _ in range(max(args.rounds, 8)):
                c.profile_enable(fam)
                c.profile_reset()
                submit(kd, c, a)
                c.synchronize()
                ms.append(c.profile_read()["total_ms"])
            c.profile_enable(capi.K_NONE)
            split[kd][name + "_ms"] = statistics.median(ms)
    split["output_layer_armed_over_plain"] = split["armed"]["output_layer_ms"] / split["plain"]["output_layer_ms"]
    print(json.dumps({"one_context": split}))
    for c in ctxs:
        c.close()
    for p in pins:
        p.free()
    gm.close()


if __name__ == "__main__":
    main()
