"""What step constraints (slimt_hip_ctx_set_step_constraints: step_constrain.hip, one more launch per step that reads the
stored row once) cost a fan-out call, on the workload of tools/sample_floor_bench.py, same process, alternating rounds.

Shape: tiny11, S = 32 (Tmax 48), a 4096-id shortlist, 32 sources x 8 rows per call (256 decoder rows), EOS bias 0;
`--workers` contexts in decode mode 1 each submitting one pinned asynchronous fan-out call per round. Four kinds of round:
  constrained-greedy   -- no repeated trigram, penalty 1.2, min length 8, 4 suppressed ids; the logits gemm stores the row
  greedy               -- the plain greedy call (the gemm's fused arg-max)
  constrained-sampled  -- the same setting under T = 1
  sampled              -- the plain sampled call
With --beam the rounds are beam calls instead (slimt_hip_translate_beam_async, the sources x k = per-source slots):
  constrained-beam     -- slimt_hip_ctx_set_beam_constraints: no repeated trigram, penalty 1.2, min length 4;
                          beam_constrained.hip's selection in the place of beam_select.hip's, still one launch per step
  beam                 -- the plain beam call
Each kind is repeated `--repeats` times (a repeat = `--rounds` rounds); medians, every repeat and spreads are printed, then
one JSON line.

  python tools/step_constrain_bench.py [--workers 4] [--rounds 10] [--repeats 3] [--beam]
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
    ap.add_argument("--sources", type=int, default=32)
    ap.add_argument("--per-source", type=int, default=8)
    ap.add_argument("--src-len", type=int, default=32)
    ap.add_argument("--shortlist", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--beam", action="store_true")
    args = ap.parse_args()

    from slimt_amd import capi, synth
    m = synth.make_model("tiny11", eos_bias=0.0)
    gm = capi.Model(m, device=0)
    B, C, S, W = args.sources, args.per_source, args.src_len, args.workers
    N = B * C
    sl = synth.make_shortlist(m.V, args.shortlist)
    cn = dict(no_repeat_ngram=3, repetition_penalty=1.2, min_length=8, suppress=[int(v) for v in sl[1:5]])
    ctxs = [capi.Context(gm, N, S) for _ in range(W)]
    for ctx in ctxs:
        ctx.set_decode_mode(1)
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
    options = {"constrained-greedy": lambda keys: dict(constraints=cn), "greedy": lambda keys: {},
               "constrained-sampled": lambda keys: dict(sampling=(1.0, keys), constraints=cn),
               "sampled": lambda keys: dict(sampling=(1.0, keys))}
    kinds = ("constrained-beam", "beam") if args.beam else tuple(options)
    bcn = dict(no_repeat_ngram=3, repetition_penalty=1.2, min_length=4)
    beams = []
    for ctx, (fan, _) in zip(ctxs, work if args.beam else ()):
        bufs = ctx.beam_buffers(B, S, C)
        bufs[0][...], bufs[1][...] = fan[0], fan[1]
        beams.append(bufs)

    def run(kind):
        t0 = time.perf_counter()
        for i, (ctx, (fan, keys)) in enumerate(zip(ctxs, work)):
            if args.beam:
                if kind == "constrained-beam":
                    ctx.set_beam_constraints(**bcn)
                ctx.translate_beam_async(beams[i], sl)
            else:
                ctx.translate_fanout_async(fan, sl, **options[kind](keys))
        for ctx in ctxs:
            ctx.synchronize()
        return time.perf_counter() - t0

    tokens = {}
    for _ in range(args.warmup):
        for kind in kinds:
            run(kind)
            tokens[kind] = int(sum(int(b[3].sum()) for b in beams) if args.beam else sum(int(fan[4].sum()) for fan, _ in work))
    times = {k: [] for k in kinds}  # per repeat: median seconds of a round
    for _ in range(args.repeats):
        per = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind in kinds:
                per[kind].append(run(kind))
        for kind in kinds:
            times[kind].append(statistics.median(per[kind]))
    out = {"sources": B, "per_source": C, "S": S, "Tmax": T, "shortlist": args.shortlist, "workers": W, "rounds": args.rounds,
           "repeats": args.repeats, "constraints": bcn if args.beam else cn, "hw_queues": capi.lib().slimt_hip_hw_queues()}
    med = {}
    for kind in kinds:
        med[kind] = statistics.median(times[kind])
        spread = max(times[kind]) - min(times[kind])
        out[kind] = {"round_ms_median": round(med[kind] * 1e3, 3), "round_ms_repeats": [round(t * 1e3, 3) for t in times[kind]],
                     "spread_ms": round(spread * 1e3, 3), "tokens": tokens[kind]}
        print("%-20s round %.3f ms (repeats %s; spread %.3f ms; %d tokens)" % (
            kind, med[kind] * 1e3, ", ".join("%.3f" % (t * 1e3) for t in times[kind]), spread * 1e3, tokens[kind]))
    if args.beam:
        out["beam_ratio"] = round(med["constrained-beam"] / med["beam"], 4)
        print("constrained / plain: beam %.4f" % out["beam_ratio"])
    else:
        out["greedy_ratio"] = round(med["constrained-greedy"] / med["greedy"], 4)
        out["sampled_ratio"] = round(med["constrained-sampled"] / med["sampled"], 4)
        print("constrained / plain: greedy %.4f, sampled %.4f" % (out["greedy_ratio"], out["sampled_ratio"]))
    print(json.dumps(out))
    for ctx in ctxs:
        ctx.close()
    gm.close()


if __name__ == "__main__":
    main()
