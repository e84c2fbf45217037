"""What scoring several candidates per source from one encoding saves (slimt_hip_score_candidates_async) against the same work
done with every candidate carrying a copy of its source (slimt_hip_score_async on the duplicated rows), same process,
alternating rounds.

Headline shape: tiny11, S = 32, T = 48, a 4096-id shortlist, 32 sources x 8 candidates per call (256 target rows), targets of
T random tokens from the shortlist, sorted by source; `--workers` contexts (HIP streams) each submitting one pinned
asynchronous call per round, at the hardware-queue setting the process starts with. Three kinds of round, alternating so
that clocks and neighbours drift into all alike:
  duplicated -- slimt_hip_score_async on src_ids[cand_src]: B = 256 rows encoded, one attention workgroup per row and head;
  candidates -- slimt_hip_score_candidates_async, candidates sorted by source: 32 rows encoded;
  shuffled   -- the same call with the candidates in a random order (more K / V stagings, the same bits).
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); the medians, every repeat's value and the spread of
the duplicated call's own repeats are printed, then one JSON line. Scores of the three kinds are compared bit for bit.

  python tools/candidates_bench.py [--workers 4] [--rounds 20] [--repeats 3] [--sources 32] [--per-source 8]
  rocprofv3 --kernel-trace --stats -- python tools/candidates_bench.py --workers 1 --rounds 5 --repeats 1   (per-kernel split)
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
    ap.add_argument("--tgt-len", type=int, default=48)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, C, S, T, W = args.sources, args.per_source, args.src_len, args.tgt_len, args.workers
    N = B * C
    sl = synth.make_shortlist(m.V, args.shortlist)
    kinds = ("duplicated", "candidates", "shuffled")
    ctxs = [capi.Context(gm, N, S) for _ in range(W)]  # (max_batch N: the duplicated call needs it)
    pins, work = [], []

    def pinned(dt, shape):
        p = capi._Pinned()
        pins.append(p)
        return p.array(dt, shape)

    for w in range(W):
        rng = np.random.default_rng(99 + w)
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        src = np.repeat(np.arange(B, dtype=np.uint32), C)
        tg = rng.choice(sl, size=(N, T)).astype(np.uint32)
        tl = np.full(N, T, np.uint32)
        perm = rng.permutation(N)
        a = {}
        for kind, (i, l, t, n, s) in (("duplicated", (ids[src], lens[src], tg, tl, None)), ("candidates", (ids, lens, tg, tl, src)),
                                      ("shuffled", (ids, lens, tg[perm], tl[perm], src[perm]))):
            bufs = [pinned(np.uint32, i.shape), pinned(np.uint32, l.shape), pinned(np.uint32, t.shape), pinned(np.uint32, n.shape)]
            for dst, val in zip(bufs, (i, l, t, n)):
                dst[...] = val
            if s is not None:
                bufs.append(pinned(np.uint32, s.shape))
                bufs[-1][...] = s
            bufs += [pinned(np.float32, t.shape), None]
            a[kind] = tuple(bufs)
        work.append((a, perm))

    def submit(kind):
        for ctx, (a, _) in zip(ctxs, work):
            if kind == "duplicated":
                ctx.score_async(a[kind], sl)
            else:
                ctx.score_candidates_async(a[kind], sl)

    def sync():
        for ctx in ctxs:
            ctx.synchronize()

    for _ in range(args.warmup):
        for kind in kinds:
            submit(kind)
            sync()
    for a, perm in work:  # the three kinds computed the same bits
        ref = a["duplicated"][4].view(np.uint32)
        assert np.array_equal(a["candidates"][5].view(np.uint32), ref)
        assert np.array_equal(a["shuffled"][5].view(np.uint32), ref[perm])
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
    tokens = W * N * T
    out = {"preset": args.preset, "sources": B, "per_source": C, "S": S, "T": T, "shortlist": args.shortlist, "workers": W,
           "rounds": args.rounds, "repeats": args.repeats, "hw_queues": capi.lib().slimt_hip_hw_queues()}
    for kind in kinds:
        med = statistics.median(times[kind])
        out[kind] = {"round_ms_median": round(med * 1e3, 4), "round_ms_repeats": [round(t * 1e3, 4) for t in times[kind]],
                     "target_tokens_per_s": round(tokens / med)}
        print("%-10s round %.3f ms (repeats %s) %d target tokens/s" % (kind, med * 1e3,
              ", ".join("%.3f" % (t * 1e3) for t in times[kind]), tokens / med))
    spread = max(times["duplicated"]) - min(times["duplicated"])
    gain = 1.0 - statistics.median(times["candidates"]) / statistics.median(times["duplicated"])
    out["duplicated_spread_ms"] = round(spread * 1e3, 4)
    out["candidates_gain"] = round(gain, 4)
    out["not_slower"] = bool(statistics.median(times["candidates"]) <= statistics.median(times["duplicated"]) + spread)
    print("candidates against duplicated: %.1f%% less time; the duplicated call's own repeats spread over %.3f ms" % (gain * 100, spread * 1e3))
    print(json.dumps(out))
    for ctx in ctxs:
        ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
