"""Beam search (include/slimt_hip.h, slimt_hip_translate_beam*): the rule restated in NumPy, the checkers and the cases.

  * `tr_exp`, `sm_log`, `weights`, `row_scores`: slimt_amd/csrc/beam.h operation by operation in float32 -- a fused
    multiply-add is the exact product and sum in float64, rounded to odd and then once to float32, which is the correctly
    rounded fmaf. tests/test_beam_checker.py compares them bit for bit with the header compiled for the host.
  * `beam_step_host`: one selection as a brute-force sort over ALL candidates (every column of every live slot) -- the
    checker of slimt_hip_beam_step; it shares nothing with the kernel's per-slot lists and wave-wide rounds but the scores.
  * `beam_translate`: the search over the oracle's decode_step in PORTABLE mode with the states reordered by parent, each
    hypothesis keeping its own token, score and alignment lists (no back-pointers: another structure than the engine's).
  * PARITY: the cases tests/test_gpu_beam.py compares bit for bit; tests/test_beam_case_fixtures.py proves on the CPU that
    they show a reorder, a carried finished slot, a rank 0 that differs from greedy, a slot live at Tmax and an order that
    depends on the length mode."""
from collections import namedtuple

import numpy as np

DEAD, LIVE, FINISHED = 0, 1, 2
NONE = 0xFFFFFFFF
MAX_BEAM = 8
f32 = np.float32


# ---- the arithmetic (beam.h, truncation.h, sampling.h) ---------------------------------------------------------------------
def fmaf(a, b, c):
    """float32 fma of float32 arrays: a * b is exact in float64; the sum is rounded to odd there, then once to float32"""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):
        p = a * b
        t = p + c
        bb = t - p
        e = (p - (t - bb)) + (c - bb)  # TwoSum: t + e == p + c exactly
        bits = t.copy().view(np.int64)
        fix = np.isfinite(t) & (e != 0) & ((bits & 1) == 0)
        up = (e > 0) == (t > 0)  # the exact sum lies further from zero than t
        bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _float(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def tr_exp(d):
    """truncation.h: exp(d) of float32 d in (-28, 0]"""
    d = np.asarray(d, dtype=np.float32)
    t = d * f32(1.44269504088896341)
    n = (t + f32(12582912.0)) - f32(12582912.0)
    r = fmaf(n, f32(-0.693359375), d)
    r = fmaf(n, f32(2.12194440e-4), r)
    z = r * r
    p = np.full(d.shape, f32(1.9875691500e-4), np.float32)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = fmaf(p, r, f32(c))
    y = fmaf(p, z, r) + f32(1.0)
    return _float(_bits(y) + (n.astype(np.int32).astype(np.uint32) << np.uint32(23)))


def sm_log(x):
    """sampling.h: log(x) of positive, finite, normal float32 x"""
    x = np.asarray(x, dtype=np.float32)
    b = _bits(x) - np.uint32(0x3f3504f3)
    e = (b.view(np.int32) >> 23).astype(np.float32)
    f = _float((b & np.uint32(0x007fffff)) + np.uint32(0x3f3504f3)) - f32(1.0)
    z = f * f
    p = np.full(x.shape, f32(7.0376836292e-2), np.float32)
    for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1,
              -2.4999993993e-1, 3.3333331174e-1):
        p = fmaf(p, f, f32(c))
    y = (f * z) * p
    y = fmaf(e, f32(-2.12194440e-4), y)
    y = fmaf(f32(-0.5), z, y)
    return fmaf(e, f32(0.693359375), f + y)


def row_max(l):
    """(usable, M): no NaN and a finite maximum, -0 read as +0"""
    l = np.asarray(l, dtype=np.float32)
    if np.isnan(l).any():
        return False, f32(np.nan)
    M = f32(l.max() + f32(0.0))
    return bool(np.isfinite(M)), M


def weights(l, M):
    """uint64 bm_weight(l_c, M) of a usable row"""
    l = np.asarray(l, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = l - f32(M)
        w = np.zeros(l.shape, np.uint64)
        mid = (l != M) & (d > f32(-28.0))
        w[mid] = (tr_exp(d[mid]).astype(np.float64) * 1099511627776.0).astype(np.uint64)
        w[l == M] = np.uint64(1) << np.uint64(40)
    return w


def row_scores(l):
    """(usable, M, Q, L, lp float32 [N]) of one row of float32 logits; lp is None for an unusable row"""
    l = np.asarray(l, dtype=np.float32)
    usable, M = row_max(l)
    if not usable:
        return False, M, 0, f32(0), None
    Q = int(weights(l, M).sum(dtype=np.uint64))
    L = sm_log(np.asarray([f32(np.float64(Q) * 2.0 ** -40)], np.float32))[0]
    with np.errstate(all="ignore"):
        lp = (l - M) - L
    return True, M, Q, L, lp.astype(np.float32)


# ---- one selection, by sorting every candidate -----------------------------------------------------------------------------
def beam_step_host(logits, totals, flags, beam, eos_id=0, ids=None):
    """slimt_hip_beam_step's outputs (parent, token, token_score, totals, flags), each [B * beam], by a brute-force sort"""
    logits = np.asarray(logits, dtype=np.float32)
    totals, flags = np.asarray(totals, dtype=np.float32), np.asarray(flags, dtype=np.uint32)
    R, N = logits.shape
    k = int(beam)
    parent, token = np.full(R, NONE, np.uint32), np.full(R, NONE, np.uint32)
    score, tot = np.zeros(R, np.float32), np.full(R, -np.inf, np.float32)
    fl = np.zeros(R, np.uint32)
    for b in range(R // k):
        cands = []  # (cand, slot, logit, column, lp, carried)
        for s in range(k):
            r = b * k + s
            if flags[r] == FINISHED:
                cands.append((totals[r], s, f32(0), 0, f32(0), True))
            elif flags[r] == LIVE:
                usable, _, _, _, lp = row_scores(logits[r])
                if not usable:
                    continue
                with np.errstate(all="ignore"):
                    cand = (totals[r] + lp).astype(np.float32)
                for c in np.nonzero(cand != -np.inf)[0]:
                    cands.append((cand[c], s, logits[r, c], int(c), lp[c], False))
        # cand descending (+0 == -0), slot ascending, logit descending, column ascending: Python compares floats as floats
        cands.sort(key=lambda x: (-float(x[0]), x[1], -float(x[2]), x[3]))
        for i, (cand, s, _, c, lp, carried) in enumerate(cands[:k]):
            r = b * k + i
            parent[r], tot[r] = s, cand
            if carried:
                fl[r] = FINISHED
            else:
                token[r] = c if ids is None else ids[c]
                score[r] = lp
                fl[r] = FINISHED if token[r] == eos_id else LIVE
    return parent, token, score, tot, fl


def start_state(B, beam):
    totals = np.full((B, beam), -np.inf, np.float32)
    flags = np.zeros((B, beam), np.uint32)
    totals[:, 0], flags[:, 0] = 0.0, LIVE
    return totals.reshape(-1), flags.reshape(-1)


# ---- the search over the oracle ------------------------------------------------------------------------------------------
def tmax_of(S, limit_factor=1.5):
    return max(int(np.float32(limit_factor) * np.float32(S)), 1)


def final_order(totals, lens, flags, mode):
    """the final slots, best first: live or finished before dead, key descending, ties to the lower slot"""
    def key(s):
        if flags[s] == DEAD:
            return (1, 0.0, s)
        with np.errstate(all="ignore"):
            v = totals[s] / f32(lens[s]) if mode == 1 else totals[s]
        return (0, -float(f32(v)), s)
    return sorted(range(len(totals)), key=key)


def beam_translate(oracle, om, m, ids, lens, sl, k, mode=0, limit_factor=1.5, eos=0, trace=None):
    """(out_ids [B,k,T], out_len [B,k], totals [B,k], token_scores [B,k,T], align [B,k,T,S]) of the contract's search.
    trace (a dict): gets what the case fixtures assert -- reorders, carries, slots live at the end."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lens = np.asarray(lens, dtype=np.uint32)
        B, S = ids.shape
        T = tmax_of(S, limit_factor)
        R = B * k
        row_src = np.repeat(np.arange(B), k)
        mask1 = oracle.make_mask(lens, S)
        enc1 = om.encode(om.embed(ids), mask1)
        enc, mask = np.ascontiguousarray(enc1[row_src]), np.ascontiguousarray(mask1[row_src])
        states = np.zeros((m.dec_layers, R, m.D), np.float32)
        totals, flags = start_state(B, k)
        hyps = [dict(tok=[], sc=[], al=[]) for _ in range(R)]
        prev = None
        if trace is not None:
            trace.update(reorders=0, carried_beside_live=set(), live_at_end=set())
        for t in range(T):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            logits = np.ascontiguousarray(logits, dtype=np.float32)
            parent, token, score, totals, new_flags = beam_step_host(logits, totals, flags, k, eos, sl)
            new_hyps, new_states = [], np.zeros_like(states)
            prev = np.zeros(R, np.uint32)
            for r in range(R):
                b, i = divmod(r, k)
                if new_flags[r] == DEAD:
                    new_hyps.append(dict(tok=[], sc=[], al=[]))
                    continue
                p = b * k + int(parent[r])
                h = hyps[p]
                if token[r] == NONE:  # a carried finished slot
                    new_hyps.append(h)
                else:
                    row = np.zeros(S, np.float32)
                    row[: int(lens[b])] = attn[p, 0, 0, : int(lens[b])]
                    new_hyps.append(dict(tok=h["tok"] + [int(token[r])], sc=h["sc"] + [score[r]], al=h["al"] + [row]))
                    if trace is not None and int(parent[r]) != i and new_flags[r] == LIVE:
                        trace["reorders"] += 1
                new_states[:, r] = states[:, p]
                if new_flags[r] == LIVE:
                    prev[r] = token[r]
            if trace is not None:
                for b in range(B):
                    fl = new_flags[b * k:(b + 1) * k]
                    if (fl == LIVE).any() and (fl == FINISHED).any():
                        trace["carried_beside_live"].add(b)
            hyps, states, flags = new_hyps, new_states, new_flags
            if not (flags == LIVE).any():
                break
        out = np.zeros((B, k, T), np.uint32)
        ln = np.zeros((B, k), np.uint32)
        tot = np.full((B, k), -np.inf, np.float32)
        sc = np.zeros((B, k, T), np.float32)
        al = np.zeros((B, k, T, S), np.float32)
        for b in range(B):
            rows = slice(b * k, (b + 1) * k)
            lens_b = [len(h["tok"]) for h in hyps[rows]]
            if trace is not None and (flags[rows] == LIVE).any():
                trace["live_at_end"].add(b)
            for j, s in enumerate(final_order(totals[rows], lens_b, flags[rows], mode)):
                if flags[b * k + s] == DEAD:
                    continue
                h = hyps[b * k + s]
                n = len(h["tok"])
                out[b, j, :n], ln[b, j], tot[b, j] = h["tok"], n, totals[b * k + s]
                sc[b, j, :n] = h["sc"]
                if n:
                    al[b, j, :n] = np.stack(h["al"])
        return out, ln, tot, sc, al
    finally:
        oracle.set_mode(oracle.FAITHFUL)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# preset + dims + eos_bias + model_seed: the synthetic model; S, B, ragged: the sources; k, mode; n_sl: the shortlist's size
# (None: the full vocabulary); seed: of the batch; max_batch: the context's (None: B * k + 3); kv_format: the model's K/V form
Case = namedtuple("Case", "name preset dims eos_bias model_seed S B ragged k mode n_sl seed max_batch kv_format")


def case(name, preset, eos_bias, S, B, k, n_sl, mode=0, ragged=True, dims=None, model_seed=1234, seed=None, max_batch=None,
         kv_format=None):
    return Case(name, preset, dims, eos_bias, model_seed, S, B, ragged, k, mode, n_sl, 71 + S + B if seed is None else seed,
                max_batch, kv_format)


PARITY = [
    case("k6", "tiny11", 6.0, 8, 3, 6, 4096),              # 18 rows: a source's rows straddle the attention's 16-row workgroup
    case("k8", "tiny11", 7.0, 8, 2, 8, 4096, ragged=False),
    case("full", "tiny11", 7.0, 8, 2, 2, None),
    case("sl1000", "tiny11", 6.0, 8, 2, 3, 1000),           # a shortlist that is no multiple of 16
    case("base", "base", 14.0, 8, 2, 3, 4096, ragged=False),
    case("s70", "tiny11", 8.0, 70, 2, 2, 4096),             # two keys per lane
    case("exact", "tiny11", 6.0, 8, 2, 4, 4096, max_batch=8),  # B * k == max_batch
    case("mean", "tiny11", 6.0, 8, 3, 6, 4096, mode=1),     # k6 under the mean: another order
]
# K/V cache format 3 keeps the reference's literal float order in the cross-attention, which is not PORTABLE's (DESIGN.md
# section 2): no oracle mode has its bits, so this case is compared with the device's own step-wise translate and with itself
KV3 = case("kv3", "tiny11", 6.0, 8, 2, 3, 4096, kv_format=3)


def parity(name):
    return next(c for c in PARITY + [KV3] if c.name == name)


def model_of(c, synth_models=None):
    from slimt_amd import synth
    if c.dims is not None:
        return synth.make_model(c.preset, seed=c.model_seed, eos_bias=c.eos_bias, dims=c.dims)
    if synth_models is not None:
        return synth_models(c.preset, c.eos_bias, c.model_seed)
    return synth.make_model(c.preset, seed=c.model_seed, eos_bias=c.eos_bias)


def inputs(c, V):
    """(ids [B, S], lens [B], shortlist | None)"""
    from slimt_amd import synth
    ids, lens = synth.make_batch(V, c.B, c.S, seed=c.seed, ragged=c.ragged)
    return ids, lens, (None if c.n_sl is None else synth.make_shortlist(V, c.n_sl))


# ---- crafted rows for slimt_hip_beam_step ------------------------------------------------------------------------------------
def crafted_step(N, k, B, seed=0):
    """(logits [B k, N], totals, flags, eos, ids | None): random rows with the contract's edges planted where N and k allow"""
    r = np.random.default_rng(1000 * N + 10 * k + B + seed)
    R = B * k
    logits = r.normal(0, 3, size=(R, N)).astype(np.float32)
    logits = np.round(logits * 4) / 4  # quarter steps: equal logits within and across rows
    totals = -np.round(r.uniform(0, 6, size=R) * 2).astype(np.float32) / 2  # half steps: equal cand across slots
    flags = np.full(R, LIVE, np.uint32)
    eos = 0
    ids = None if N < 17 else r.permutation(N).astype(np.uint32)
    eos_col = 0 if ids is None else int(np.nonzero(ids == eos)[0][0])
    for b in range(B):
        rows = np.arange(b * k, (b + 1) * k)
        if b == 0:
            totals[rows], flags[rows] = start_state(1, k)  # the step-0 state
            logits[rows[0], eos_col] = logits[rows[0]].max() + 1  # ... and EOS is chosen
            continue
        if k >= 3:
            logits[rows[0]] = logits[rows[1]]  # equal rows with equal totals: ties across slots
            totals[rows[0]] = totals[rows[1]]
            flags[rows[2]] = FINISHED          # a finished slot that beats every live candidate
            totals[rows[2]] = 0.5
        if k >= 8:
            logits[rows[3], N // 2] = np.nan   # a NaN row
            logits[rows[4]] = -np.inf          # a row of all -inf
            logits[rows[5], N - 1] = np.inf    # M = +inf
            flags[rows[6]] = DEAD
            totals[rows[6]] = -np.inf
            logits[rows[7], : N // 2] = -np.inf
        if N >= 17:
            z = rows[0] if k < 3 else rows[k - 1]
            logits[z, np.arange(N) % 8 != 1] -= 40  # most of a row out of the weights' range ...
            logits[z, [3, 9]] = [0.0, -0.0]         # ... and +0 / -0 at its top
    if B >= 3 and k >= 3:  # fewer than k candidates: one live slot of two usable columns
        rows = np.arange(2 * k, 3 * k)
        flags[rows[1:]] = DEAD
        totals[rows[1:]] = -np.inf
        if N > 2:
            logits[rows[0], 2:] = -np.inf
    return logits, totals, flags, eos, ids
