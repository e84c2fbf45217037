"""Scored against unscored translation (slimt_hip_ctx_set_scores), same process, interleaved rounds.

Headline shape: tiny11, B = 256, S = 32, a 4096-id shortlist, `--workers` contexts (HIP streams) each submitting one
pinned asynchronous translate per round; rounds alternate unscored / scored so that clocks and neighbours drift into
both alike. Also one merged launch per context (slimt_hip_translate_many_async, `--merge` batches of B / merge each),
scored and unscored; and the batching service (BatchService, merged launches on, workers x B sentences per request),
scored and unscored. Prints one JSON line per measurement and a summary line with the ratios.

  python tools/scores_bench.py [--workers 20] [--rounds 10] [--merge 4]
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
    ap.add_argument("--merge", type=int, default=4)
    ap.add_argument("--eos-bias", type=float, default=0.0)
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
    bufs, scs = [], []
    for w, c in enumerate(ctxs):
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + w)
        b = c.pinned_buffers(B, S)
        b[0][...] = ids
        b[1][...] = lens
        bufs.append(b)
        scs.append(c._pinned.setdefault("sc", capi._Pinned()).array(np.float32, (B, T)))

    def run_round(scored):
        t0 = time.perf_counter()
        for c, b, s in zip(ctxs, bufs, scs):
            c.translate_async(b, sl, scores=s if scored else None)
        for c in ctxs:
            c.synchronize()
        dt = time.perf_counter() - t0
        return sum(int(b[3].sum()) for b in bufs) / dt

    # merged: `merge` sub-batches of B / merge sentences per context, one launch pair
    sub = max(1, B // args.merge)
    assert capi.translate_many_rows([sub] * args.merge) <= B
    mctx = ctxs  # (the same contexts: more than 22 in one process time-slice the hardware queues)
    mbufs, mscs, pins = [], [], []
    for w, c in enumerate(mctx):
        lst, sc_l = [], []
        for j in range(args.merge):
            ids, lens = synth.make_batch(m.V, sub, S, seed=9000 + 31 * w + j)
            arrs = []
            for dt_, shape in ((np.uint32, (sub, S)), (np.uint32, (sub,)), (np.uint32, (sub, T)), (np.uint32, (sub,)),
                               (np.float32, (sub, T))):
                p = capi._Pinned()
                pins.append(p)
                arrs.append(p.array(dt_, shape))
            arrs[0][...] = ids
            arrs[1][...] = lens
            lst.append(tuple(arrs[:4]) + (None,))
            sc_l.append(arrs[4])
        mbufs.append(lst)
        mscs.append(sc_l)

    def run_merged(scored):
        t0 = time.perf_counter()
        for c, lst, s in zip(mctx, mbufs, mscs):
            c.translate_many_async(lst, sl, scores=s if scored else None)
        for c in mctx:
            c.synchronize()
        dt = time.perf_counter() - t0
        return sum(int(b[3].sum()) for lst in mbufs for b in lst) / dt

    for _ in range(args.warmup):
        run_round(False), run_round(True), run_merged(False), run_merged(True)
    res = {"plain": [], "scored": [], "merged_plain": [], "merged_scored": []}
    for r in range(args.rounds):
        order = (False, True) if r % 2 == 0 else (True, False)
        for scored in order:
            res["scored" if scored else "plain"].append(run_round(scored))
        for scored in order:
            res["merged_scored" if scored else "merged_plain"].append(run_merged(scored))
    for c in ctxs:
        c.close()
    # the batching service (host/Service, merged launches on): one request of workers x B sentences per round; two services
    # of 5 double-buffered workers each (20 contexts, like the rounds above)
    n_sent = W * B
    rng = np.random.Generator(np.random.PCG64(17))
    sents = [list(rng.integers(3, m.V, S - 1)) + [0] for _ in range(n_sent)]
    svcs = {sc: capi.BatchService([gm], max_words=8192, workers_per_device=5, limit_factor=1.5, shortlist=sl,
                                  alignments=False, scores=sc) for sc in (False, True)}

    def run_service(scored):
        t0 = time.perf_counter()
        r = svcs[scored].translate(sents)
        dt = time.perf_counter() - t0
        tok = int(r.target_offsets[-1])
        r.close()
        return tok / dt

    for _ in range(args.warmup):
        run_service(False), run_service(True)
    res["service_plain"], res["service_scored"] = [], []
    for r in range(args.rounds):
        for scored in ((False, True) if r % 2 == 0 else (True, False)):
            res["service_scored" if scored else "service_plain"].append(run_service(scored))
    for v in svcs.values():
        v.close()
    for k, v in res.items():
        print(json.dumps({"run": k, "median_tok_s": statistics.median(v), "min": min(v), "max": max(v),
                          "rounds": [round(x) for x in v]}))
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"summary": f"{args.preset} B={B} S={S} shortlist={args.shortlist} workers={W}",
                      "scored_over_plain": med["scored"] / med["plain"],
                      "merged_scored_over_plain": med["merged_scored"] / med["merged_plain"],
                      "service_scored_over_plain": med["service_scored"] / med["service_plain"],
                      "plain_tok_s": med["plain"], "scored_tok_s": med["scored"]}))
    for p in pins:
        p.free()
    gm.close()


if __name__ == "__main__":
    main()
