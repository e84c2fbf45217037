"""What the consensus pick over unit rows -- the character n-gram F, slimt_hip_ctx_set_fanout_consensus_units -- costs behind a
fan-out call, against the plain call and the call armed with the token utility. Same process, alternating rounds, after
tools/consensus_bench.py.

Headline shape, as there: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 sources x 8 rows per call, truncated sampling
(top-k 40, top-p 0.9) at T = 1, rows sorted by source; `--workers` contexts each submitting one pinned asynchronous call per
round, at the hardware-queue setting the process starts with. The unit table is synthetic: every id a piece of 1..6 units
(3.5 on average, a SentencePiece vocabulary's) over 64 symbols. Three kinds of round:
  plain   -- (i)   slimt_hip_translate_fanout_async, nothing armed;
  tokens  -- (ii)  the same call with the token selection armed (max_order 4, beta2 4): one launch behind the last step;
  units   -- (iii) the same call with the unit selection armed (max_order 6, beta2 4): a clear and three launches behind the last
                   step.
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); medians, every repeat and the plain call's own
min-max spread are printed. The armed units call's picks are checked against slimt_hip_consensus_select_units on its rows.
Then those launches alone, through slimt_hip_profile_* (kernel family SLIMT_HIP_K_CONSENSUS), on synthetic rows: 32 x 8
rows of 48 tokens (168 units), and the worst admitted case, 64 rows x 1024 units, on one source and on 32.

  python tools/consensus_units_bench.py [--workers 1,4] [--rounds 10] [--repeats 3] [--out profiles/r25_consensus_units_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G_TOKENS, G_UNITS, BETA2 = 4, 6, 4


def table(V, lengths, seed=5):
    rnd = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(rnd.choice(lengths, V))]).astype(np.uint32)
    return off, rnd.integers(0x61, 0x61 + 64, int(off[-1])).astype(np.uint32)


def headline(args, W, say):
    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    off, units = table(m.V, [1, 2, 3, 4, 5, 6])
    gm.set_consensus_units(off, units)
    B, C, S = args.sources, args.per_source, args.src_len
    N = B * C
    sl = synth.make_shortlist(m.V, args.shortlist)
    trunc = (args.top_k, args.top_p)
    kinds = ("plain", "tokens", "units")
    ctxs = [capi.Context(gm, N, S) for _ in range(W)]
    T = ctxs[0].pinned_buffers(1, S)[2].shape[1]
    pins, work = [], []

    def pinned(dt, shape):
        q = capi._Pinned()
        pins.append(q)
        return q.array(dt, shape)

    for w in range(W):
        ids, lens = synth.make_batch(m.V, B, S, seed=4321 + 31 * w)
        src = np.repeat(np.arange(B, dtype=np.uint32), C)
        keys = pinned(np.uint64, (N,))
        keys[...] = capi.sampling_keys(7 + w, N)
        fan = (pinned(np.uint32, (B, S)), pinned(np.uint32, (B,)), pinned(np.uint32, (N,)), pinned(np.uint32, (N, T)),
               pinned(np.uint32, (N,)), None)
        for dst, val in zip(fan, (ids, lens, src)):
            dst[...] = val
        picked = {k: (pinned(np.uint32, (B,)), pinned(np.float64, (N,))) for k in ("tokens", "units")}
        work.append((fan, keys, picked))

    def round_of(kind):
        for ctx, (fan, keys, picked) in zip(ctxs, work):
            if kind == "tokens":
                ctx.set_fanout_consensus(G_TOKENS, BETA2, *picked["tokens"])
            elif kind == "units":
                ctx.set_fanout_consensus_units(G_UNITS, BETA2, *picked["units"])
            ctx.translate_fanout_async(fan, sl, sampling=(1.0, keys), truncation=trunc)
        for ctx in ctxs:
            ctx.synchronize()

    for _ in range(args.warmup):
        for kind in kinds:
            round_of(kind)
    row_units = []
    for fan, _, picked in work:  # the armed call picked what the stand-alone call picks on its rows, bit for bit
        util, best = capi.consensus_select_units(fan[3], fan[4], fan[2], B, off, units, G_UNITS, BETA2)
        assert np.array_equal(picked["units"][0], best) and np.array_equal(picked["units"][1].view(np.uint64), util.view(np.uint64))
        row_units += [int(sum(off[v + 1] - off[v] for v in fan[3][r, :fan[4][r]])) for r in range(N)]
    times = {k: [] for k in kinds}  # per repeat: median seconds of a round
    for _ in range(args.repeats):
        per = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind in kinds:
                t0 = time.perf_counter()
                round_of(kind)
                per[kind].append(time.perf_counter() - t0)
        for kind in kinds:
            times[kind].append(statistics.median(per[kind]))
    out = {"preset": args.preset, "sources": B, "per_source": C, "S": S, "Tmax": T, "shortlist": args.shortlist, "top_k": trunc[0],
           "top_p": trunc[1], "workers": W, "rounds": args.rounds, "repeats": args.repeats, "hw_queues": capi.lib().slimt_hip_hw_queues(),
           "mean_row_tokens": round(float(np.mean([w[0][4].mean() for w in work])), 1), "mean_row_units": round(float(np.mean(row_units)), 1)}
    say("---- %d context(s), %d hardware queues, rows of %.1f tokens, %.1f units on average"
        % (W, out["hw_queues"], out["mean_row_tokens"], out["mean_row_units"]))
    for kind in kinds:
        med = statistics.median(times[kind])
        out[kind] = {"round_ms_median": round(med * 1e3, 3), "round_ms_repeats": [round(t * 1e3, 3) for t in times[kind]]}
        say("%-7s round %.3f ms (repeats %s)" % (kind, med * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind])))
    med = {k: statistics.median(times[k]) for k in kinds}
    out["plain_spread_ms"] = round((max(times["plain"]) - min(times["plain"])) * 1e3, 3)
    out["tokens_minus_plain_ms"] = round((med["tokens"] - med["plain"]) * 1e3, 3)
    out["units_minus_plain_ms"] = round((med["units"] - med["plain"]) * 1e3, 3)
    say("units - plain %+.3f ms and tokens - plain %+.3f ms against the plain call's own min-max spread of %.3f ms"
        % (out["units_minus_plain_ms"], out["tokens_minus_plain_ms"], out["plain_spread_ms"]))
    say(json.dumps(out))
    for ctx in ctxs:
        ctx.close()
    gm.close()


def kernels_alone(args, say):
    import torch
    from slimt_amd import capi, synth
    m = synth.make_model("micro", eos_bias=3.0)
    gm = capi.Model(m, device=0)
    ctx = capi.Context(gm, 4, 8)
    rnd = np.random.default_rng(3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    say("---- the launches alone (slimt_hip_profile_*, %d calls each; rows are mutations of one sentence per source)" % args.launches)
    for B, C, T, per_id in ((32, 8, 48, [1, 2, 3, 4, 5, 6]), (1, 64, 256, [4]), (32, 64, 256, [4])):
        gm.set_consensus_units(*table(m.V, per_id))
        N = B * C
        base = rnd.integers(1, m.V, size=(B, T))
        ids = np.repeat(base, C, axis=0)
        swap = rnd.random((N, T)) < 0.25
        ids = np.where(swap, rnd.integers(1, m.V, size=(N, T)), ids).astype(np.uint32)
        lens = np.full(N, T, np.uint32)
        src = np.repeat(np.arange(B, dtype=np.uint32), C)
        d_ids, d_len, d_src = dev(ids), dev(lens), dev(src)
        d_util = torch.zeros((N,), dtype=torch.float64, device="cuda")
        d_best = torch.zeros((B,), dtype=torch.int32, device="cuda")
        call = lambda: ctx.consensus_select_units_device(d_ids.data_ptr(), d_len.data_ptr(), d_src.data_ptr(), N, T, B, G_UNITS,
                                                         BETA2, d_util.data_ptr(), d_best.data_ptr())
        call()
        ctx.synchronize()
        assert (d_best.cpu().numpy().view(np.uint32) != capi.NO_ROW).all()  # (no source over a limit: the pairs were counted)
        ctx.profile_enable(capi.K_CONSENSUS)
        ctx.profile_reset()
        for _ in range(args.launches):
            call()
        ctx.synchronize()
        r = ctx.profile_read()
        ctx.profile_enable(capi.K_NONE)
        say("%2d source(s) x %2d rows of %3d tokens, %s units per id: %.1f us per call (%d calls)"
            % (B, C, T, "1..6" if len(per_id) > 1 else str(per_id[0]), 1e3 * r["total_ms"] / max(1, r["launches"]), r["launches"]))
    ctx.close()
    gm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="tiny11")
    ap.add_argument("--sources", type=int, default=32)
    ap.add_argument("--per-source", type=int, default=8)
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--workers", default="1,4")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("consensus_units_bench: %s, %d sources x %d rows, S %d, shortlist %d, top-k %d, top-p %g; tokens: max_order %d, units: "
        "max_order %d, beta2 %d; %d rounds x %d repeats" % (args.preset, args.sources, args.per_source, args.src_len, args.shortlist,
                                                            args.top_k, args.top_p, G_TOKENS, G_UNITS, BETA2, args.rounds, args.repeats))
    for W in [int(w) for w in args.workers.split(",") if w]:  # (--workers "": the launches alone)
        headline(args, W, say)
    kernels_alone(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
