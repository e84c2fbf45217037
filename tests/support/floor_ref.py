"""A NumPy restatement of slimt_amd/csrc/floor.h (slimt_hip_ctx_set_sampling_floor): tr_exp and tr_weight of truncation.h
in float32 arithmetic with an exactly rounded fmaf, Python-int sums, float64 products. It shares no code with the header;
tests/test_floor_checker.py holds the two together bit for bit. Also the crafted rows both floor tests use."""
import numpy as np

from test_forced_prefix_checker import tmax_of
from test_sampling_checker import first_max, row_keys
from test_truncation_checker import kept_scores

F = np.float32


def fmaf(a, b, c):
    """float32 fma: the exact a b + c rounded once. a b is exact in float64; the sum's rounding error (two-sum) moves a
    float64 result that sits on a float32 midpoint off it, so the second rounding cannot go the wrong way."""
    p, c = np.asarray(a, np.float64) * np.asarray(b, np.float64), np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    mid = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    s = np.where(mid & (err != 0), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def tr_exp(d):
    d = np.asarray(d, F)
    n = (d * F(1.44269504088896341) + F(12582912.0)) - F(12582912.0)
    r = fmaf(n, F(2.12194440e-4), fmaf(n, F(-0.693359375), d))
    p = F(1.9875691500e-4)
    for k in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = fmaf(p, r, F(k))
    y = (fmaf(p, r * r, r) + F(1.0)).astype(F)
    return (y.view(np.uint32) + (n.astype(np.int32).view(np.uint32) << np.uint32(23))).view(F)


def tr_weight(z, M):
    """uint32 weights of a float32 array of valid z against M"""
    z = np.asarray(z, F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (z - F(M)).astype(F)
        live = (z != F(M)) & (d > F(-17.0))
        w = np.zeros(z.shape, np.uint32)
        w[live] = (tr_exp(d[live]) * F(16777216.0)).astype(np.uint32)
    w[z == F(M)] = 16777216
    return w


def kept_set(z32, min_p, epsilon):
    """(kept bool [N], Q int, M float32) of one row of float32 z"""
    z32 = np.asarray(z32, F)
    valid = ~np.isnan(z32)
    if not valid.any():
        return valid, 0, F(-np.inf)
    M = z32[valid].max()
    w = np.zeros(z32.size, np.uint32)
    w[valid] = tr_weight(z32[valid], M)
    Q = sum(int(x) for x in w)
    kept = valid.copy()
    if F(min_p) != 0:
        kept &= w.astype(np.float64) >= np.float64(F(min_p)) * 16777216.0
    if F(epsilon) != 0:
        kept &= w.astype(np.float64) >= np.float64(F(epsilon)) * np.float64(Q)
    with np.errstate(invalid="ignore"):
        return kept | (valid & (z32 == M)), Q, M


def floored_row(key, t, logits, ids, inv_T, min_p, epsilon, forced=False):
    """one step of one sentence: (column, none, kept, M, float64 score of the drawn column)"""
    logits = np.ascontiguousarray(logits, dtype=F)
    z32 = (logits * F(inv_T)).astype(F)
    kept, _, M = kept_set(z32, 0.0, 0.0) if forced else kept_set(z32, min_p, epsilon)
    col, none = first_max(np.where(kept, row_keys(key, t, logits, ids, inv_T), F(-np.inf)), logits[0])
    return col, none, kept, M, kept_scores(z32, kept, none)[col]


def floored_translate(oracle, om, m, ids, lens, sl, keys, T, min_p, epsilon, sizes=None):
    """the sampled checker's loop with the floor applied to every step: out, lengths, alignment, float64 scores.
    sizes (a list): gets (row, step, |K|, n_valid) of every step."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        B, S = ids.shape
        Tm, inv_T = tmax_of(S), F(1.0) / F(T)
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(ids), mask)
        states = np.zeros((m.dec_layers, B, m.D), F)
        out, ln = np.zeros((B, Tm), np.uint32), np.zeros(B, np.uint32)
        al, sc = np.zeros((B, Tm, S), F), np.full((B, Tm), np.nan)
        done, prev = np.zeros(B, bool), None
        for t in range(Tm):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            tok = np.zeros(B, np.uint32)
            for b in np.flatnonzero(~done):
                col, none, kept, _, s = floored_row(keys[b], ln[b], logits[b], sl, inv_T, min_p, epsilon)
                if sizes is not None:
                    sizes.append((b, t, int(kept.sum()), int((~np.isnan(logits[b])).sum())))
                tok[b] = col if sl is None else sl[col]
                sc[b, t] = s
                al[b, t, : int(lens[b])] = attn[b, 0, 0, : int(lens[b])]
                out[b, t] = tok[b]
                ln[b] += 1
                done[b] = tok[b] == 0
            prev = tok
            if done.all():
                break
        return out, ln, al, sc
    finally:
        oracle.set_mode(oracle.FAITHFUL)


def _step_down_to(z, pred):
    """the first float32 at or below z, walking down ulp by ulp, for which pred(weight against M = 0) holds"""
    z = F(z)
    while not pred(int(tr_weight(np.array([z]), F(0.0))[0])):
        z = np.nextafter(z, F(-np.inf))
    return z


def crafted_rows(N, seed, min_p, epsilon):
    """[(kind, logits float32 [N], (min_p, epsilon))]: the rows of the floor tests at inverse temperature 1. Special values
    sit in the leading columns and a row is cut to N, so a short row keeps what fits. 'gauss' comes at the first scale
    at which the restatement keeps a strict subset of more than one column (where one exists)."""
    rng = np.random.default_rng(seed)
    n = max(N, 8)
    low = np.full(n, -30.0, F)  # weight 0 against a maximum of 0
    rows = []
    g = rng.normal(0.0, 1.0, n).astype(F)
    for scale in (1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0):
        k = int(kept_set((g * F(scale))[:N], min_p, epsilon)[0].sum())
        if 1 < k < N:
            break
    rows.append(("gauss", g * F(scale), (min_p, epsilon)))
    mp = min_p if min_p else 0.1  # two columns on the min-p boundary (the least weight that passes), one just under
    floor = np.float64(F(mp)) * 16777216.0
    on = _step_down_to(np.log(mp) + 1e-5, lambda w: w - 1 < floor) if mp < 1 else F(0.0)
    under = _step_down_to(on, lambda w: w < floor) if mp < 1 else np.nextafter(F(0.0), F(-1.0))
    x = low.copy()
    x[:4] = (on, 0.0, under, on)
    rows.append(("min-p boundary", x, (mp, 0.0)))
    half = _step_down_to(-0.69314, lambda w: w <= 1 << 23)  # weight 2^23: with the maximum and a twin, Q = 2^25
    assert int(tr_weight(np.array([half]), F(0.0))[0]) == 1 << 23
    for kind, twin in (("w == epsilon Q", half), ("w just under epsilon Q", _step_down_to(half, lambda w: w < 1 << 23))):
        x = low.copy()
        x[:3] = (half, 0.0, twin)
        rows.append((kind, x, (0.0, 0.25)))
    x = (g * F(0.05)).astype(F)
    x[1] = x[5] = F(1.0)
    rows.append(("epsilon above every probability", x, (min_p, 0.9)))
    for kind, at, v in (("nan at 0", [0], np.nan), ("nan in the middle", [N // 2], np.nan),
                        ("all nan", slice(None), np.nan), ("all -inf", slice(None), -np.inf), ("+inf maximum", [3 % N], np.inf)):
        x = (g * F(2.0)).astype(F)
        x[at] = v
        rows.append((kind, x, (min_p, epsilon)))
    rows.append(("+0 against -0", np.where(np.arange(n) % 3 == 0, F(0.0), np.where(np.arange(n) % 3 == 1, F(-0.0), F(-1.0))).astype(F),
                 (min_p, epsilon)))
    x = (g * F(2.0)).astype(F)
    x[[0, 2 % N, N - 1]] = x[:N].max() + F(0.5)
    rows.append(("duplicated maxima", x, (min_p, epsilon)))
    return [(kind, np.ascontiguousarray(x[:N], dtype=F), p) for kind, x, p in rows]
