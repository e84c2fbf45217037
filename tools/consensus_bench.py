"""What the consensus pick among a fan-out call's rows costs on the device (slimt_hip_ctx_set_fanout_consensus) against the
ways to get a pick without it, same process, alternating rounds.

Headline shape, as tools/fanout_bench.py: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 sources x 8 rows per call,
truncated sampling (top-k 40, top-p 0.9) at T = 1, rows sorted by source; `--workers` contexts (HIP streams) each submitting
one pinned asynchronous call per round, at the hardware-queue setting the process starts with. Four kinds of round,
alternating so that clocks and neighbours drift into all alike:
  plain   -- (i)   slimt_hip_translate_fanout_async, nothing armed;
  armed   -- (ii)  the same call with the selection armed (max_order 4, beta2 4): one more launch behind the last step and
                   two small copies;
  host    -- (iii) the plain call, then the same selection as a C++ host loop over the returned rows
                   (tools/consensus_host.cc, one thread per context, outside the interpreter lock);
  rerank  -- (iv)  the engine part of sample_and_rerank: the plain call, then slimt_hip_score_candidates_async over the
                   returned rows (a second encoding and a scorer pass), then the totals and the best row (numpy).
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); medians, every repeat and the plain call's own
min-max spread are printed. armed and host must pick the same rows with the same utility bits (checked).
Then the kernel alone, through slimt_hip_profile_* (kernel family SLIMT_HIP_K_CONSENSUS), on synthetic rows: 32 x 8 rows of
48 tokens, and the worst admitted case, 64 rows x T = 192, on one source and on 32.

  python tools/consensus_bench.py [--workers 1,4,20] [--rounds 10] [--repeats 3] [--out profiles/r18_consensus_bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G, BETA2 = 4, 4


def host_loop():
    """tools/consensus_host.cc as a shared library beside the engine's (built when missing or older than its source)"""
    src = os.path.join(ROOT, "tools", "consensus_host.cc")
    so = os.path.join(ROOT, "slimt_amd", "lib", "consensus_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", so])
    fn = ctypes.CDLL(so).consensus_host
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    fn.argtypes = [vp, vp, vp, sz, sz, sz, ctypes.c_int, ctypes.c_int, vp, vp]
    return fn


def headline(args, W, say):
    from slimt_amd import capi, synth
    m = synth.make_model(args.preset, eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, C, S = args.sources, args.per_source, args.src_len
    N = B * C
    sl = synth.make_shortlist(m.V, args.shortlist)
    trunc = (args.top_k, args.top_p)
    kinds = ("plain", "armed", "host", "rerank")
    ctxs = [capi.Context(gm, N, S) for _ in range(W)]
    T = ctxs[0].pinned_buffers(1, S)[2].shape[1]
    pins, work = [], []
    loop = host_loop()
    pool = ThreadPoolExecutor(max_workers=W)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

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
        picked = {k: (pinned(np.uint32, (B,)), pinned(np.float64, (N,))) for k in ("armed", "host")}
        scores = pinned(np.float32, (N, T))
        work.append((fan, keys, picked, scores))

    def fanout(armed):
        for ctx, (fan, keys, picked, _) in zip(ctxs, work):
            if armed:
                ctx.set_fanout_consensus(G, BETA2, *picked["armed"])
            ctx.translate_fanout_async(fan, sl, sampling=(1.0, keys), truncation=trunc)

    def sync():
        for ctx in ctxs:
            ctx.synchronize()

    def host_pick(item):
        fan, _, picked, _ = item
        best, util = picked["host"]
        assert loop(p(fan[3]), p(fan[4]), p(fan[2]), N, T, B, G, BETA2, p(util), p(best)) == 0

    def round_of(kind):
        fanout(kind == "armed")
        sync()
        if kind == "host":
            list(pool.map(host_pick, work))
        elif kind == "rerank":
            for ctx, (fan, _, _, scores) in zip(ctxs, work):
                ctx.score_candidates_async((fan[0], fan[1], fan[3], fan[4], fan[2], scores, None), sl)
            sync()
            for fan, _, _, scores in work:
                live = np.arange(T)[None, :] < fan[4][:, None]
                totals = np.where(live, scores, np.float32(0)).sum(axis=1, dtype=np.float32).reshape(B, C)
                totals.argmax(axis=1)

    for _ in range(args.warmup):
        for kind in kinds:
            round_of(kind)
    for fan, _, picked, _ in work:  # the device and the host loop picked the same rows with the same utility bits
        assert np.array_equal(picked["armed"][0], picked["host"][0])
        assert np.array_equal(picked["armed"][1].view(np.uint64), picked["host"][1].view(np.uint64))
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
           "top_p": trunc[1], "workers": W, "rounds": args.rounds, "repeats": args.repeats, "max_order": G, "beta2": BETA2,
           "hw_queues": capi.lib().slimt_hip_hw_queues(),
           "mean_row_tokens": round(float(np.mean([w[0][4].mean() for w in work])), 1)}
    say("---- %d context(s), %d hardware queues, rows of %.1f tokens on average" % (W, out["hw_queues"], out["mean_row_tokens"]))
    for kind in kinds:
        med = statistics.median(times[kind])
        out[kind] = {"round_ms_median": round(med * 1e3, 3), "round_ms_repeats": [round(t * 1e3, 3) for t in times[kind]]}
        say("%-7s round %.3f ms (repeats %s)" % (kind, med * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind])))
    med = {k: statistics.median(times[k]) for k in kinds}
    spread = max(times["plain"]) - min(times["plain"])
    out["plain_spread_ms"] = round(spread * 1e3, 3)
    out["armed_minus_plain_ms"] = round((med["armed"] - med["plain"]) * 1e3, 3)
    out["host_minus_plain_ms"] = round((med["host"] - med["plain"]) * 1e3, 3)
    out["rerank_minus_plain_ms"] = round((med["rerank"] - med["plain"]) * 1e3, 3)
    say("armed - plain %+.3f ms against the plain call's own min-max spread of %.3f ms; host loop - plain %+.3f ms; "
        "rerank - plain %+.3f ms" % (out["armed_minus_plain_ms"], out["plain_spread_ms"], out["host_minus_plain_ms"],
                                     out["rerank_minus_plain_ms"]))
    say(json.dumps(out))
    pool.shutdown()
    for ctx in ctxs:
        ctx.close()
    gm.close()


def kernel_alone(args, say):
    import torch
    from slimt_amd import capi, synth
    gm = capi.Model(synth.make_model("micro", eos_bias=3.0), device=0)
    ctx = capi.Context(gm, 4, 8)
    rnd = np.random.default_rng(3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    say("---- the kernel alone (slimt_hip_profile_*, %d launches each; rows are mutations of one sentence per source)" % args.launches)
    for B, C, T, L in ((32, 8, 48, 48), (1, 64, 192, 192), (32, 64, 192, 192)):
        N = B * C
        base = rnd.integers(1, 200, size=(B, T))
        ids = np.repeat(base, C, axis=0)
        swap = rnd.random((N, T)) < 0.25
        ids = np.where(swap, rnd.integers(1, 200, size=(N, T)), ids).astype(np.uint32)
        lens = rnd.integers(max(1, L - 8), L + 1, size=N).astype(np.uint32)
        src = np.repeat(np.arange(B, dtype=np.uint32), C)
        d_ids, d_len, d_src = dev(ids), dev(lens), dev(src)
        d_util = torch.zeros((N,), dtype=torch.float64, device="cuda")
        d_best = torch.zeros((B,), dtype=torch.int32, device="cuda")
        call = lambda: ctx.consensus_select_device(d_ids.data_ptr(), d_len.data_ptr(), d_src.data_ptr(), N, T, B, G, BETA2,
                                                   d_util.data_ptr(), d_best.data_ptr())
        call()
        ctx.synchronize()
        ctx.profile_enable(capi.K_CONSENSUS)
        ctx.profile_reset()
        for _ in range(args.launches):
            call()
        ctx.synchronize()
        r = ctx.profile_read()
        ctx.profile_enable(capi.K_NONE)
        say("%2d source(s) x %2d rows, T = %3d (lengths %d..%d): %.1f us per launch (%d launches)"
            % (B, C, T, max(1, L - 8), L, 1e3 * r["total_ms"] / max(1, r["launches"]), r["launches"]))
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
    ap.add_argument("--workers", default="1,4,20")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("consensus_bench: %s, %d sources x %d rows, S %d, shortlist %d, top-k %d, top-p %g, max_order %d, beta2 %d; %d rounds x %d "
        "repeats" % (args.preset, args.sources, args.per_source, args.src_len, args.shortlist, args.top_k, args.top_p, G, BETA2,
                     args.rounds, args.repeats))
    for W in [int(w) for w in args.workers.split(",") if w]:  # (--workers "": the kernel alone)
        headline(args, W, say)
    kernel_alone(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
