"""A NumPy restatement of slimt_amd/csrc/typical.h on floor_ref's tr_weight (Python-int totals, a float64 product for the
mass; tests/test_typical_checker.py holds it to the header bit for bit), the typical tests' crafted rows and translate loop."""
import numpy as np

from support.floor_ref import F, tr_weight
from test_forced_prefix_checker import tmax_of
from test_sampling_checker import first_max, row_keys
from test_truncation_checker import kept_scores


def typical_set(z32, mass):
    """(kept bool [N], Ebar int, M float32) of one row of float32 z"""
    z32 = np.asarray(z32, F)
    valid = ~np.isnan(z32)
    if not valid.any():
        return valid, 0, F(-np.inf)
    M = z32[valid].max()
    w = np.zeros(z32.size, np.int64)
    w[valid] = tr_weight(z32[valid], M)
    gapped = (w > 0) & (z32 != M)  # (z == M: gap 0, and no inf - inf)
    G = np.zeros(z32.size, np.int64)
    G[gapped] = (-(z32[gapped] - M).astype(F) * F(65536.0)).astype(np.uint32)
    Q, A = sum(int(x) for x in w), sum(int(x) * int(g) for x, g in zip(w, G))
    Ebar = A // Q
    key = np.abs(G - Ebar)
    live = np.flatnonzero(w > 0)
    live = live[np.argsort(key[live], kind="stable")]
    reached = np.cumsum(w[live]).astype(np.float64) >= np.float64(F(mass)) * np.float64(Q)  # (sums below 2^53: exact)
    kappa = key[live][np.argmax(reached)]  # the first key at which the weight up to it reaches the mass
    return (w > 0) & (key <= kappa), Ebar, M


def typical_row(key, t, logits, ids, inv_T, mass):
    """one step of one sentence: (column, none, kept, M, Ebar, float64 score of the drawn column)"""
    logits = np.ascontiguousarray(logits, dtype=F)
    z32 = (logits * F(inv_T)).astype(F)
    kept, Ebar, M = typical_set(z32, mass)
    col, none = first_max(np.where(kept, row_keys(key, t, logits, ids, inv_T), F(-np.inf)), logits[0])
    return col, none, kept, M, Ebar, kept_scores(z32, kept, none)[col]


def typical_translate(oracle, om, m, ids, lens, sl, keys, T, mass, sizes=None):
    """the sampled checker's loop under the typical set: out, lengths, alignment, float64 scores; sizes gets each step's (|K|, n_valid)"""
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
            prev = np.zeros(B, np.uint32)
            for b in np.flatnonzero(~done):
                col, _, kept, _, _, sc[b, t] = typical_row(keys[b], ln[b], logits[b], sl, inv_T, mass)
                if sizes is not None:
                    sizes.append((int(kept.sum()), int((~np.isnan(logits[b])).sum())))
                out[b, t] = prev[b] = col if sl is None else sl[col]
                al[b, t, : int(lens[b])] = attn[b, 0, 0, : int(lens[b])]
                ln[b] += 1
                done[b] = prev[b] == 0
            if done.all():
                break
        return out, ln, al, sc
    finally:
        oracle.set_mode(oracle.FAITHFUL)


def crafted_rows(N, seed):
    """[(kind, z float32 [N])] at inverse temperature 1; a row is cut to N, so a short row keeps what fits"""
    rng = np.random.default_rng(seed)
    n = max(N, 8)
    g = rng.normal(0.0, 1.0, n).astype(F)
    rows = [("gauss sd 1", g), ("gauss sd 3", g * F(3.0)), ("all equal", np.full(n, 0.25, F)),
            ("two values", np.where(np.arange(n) % 3 == 0, F(1.0), F(-0.5)).astype(F))]
    for kind, at, v in (("one nan", [n // 2 % N], np.nan), ("all nan", slice(None), np.nan),
                        ("some -inf", [0, 2 % N, N - 1], -np.inf), ("+inf maximum", [3 % N], np.inf)):
        x = (g * F(2.0)).astype(F)
        x[at] = v
        rows.append((kind, x))
    x = np.full(n, -1.5, F)  # one column at 0: below the entropy's surprisal when the rest outweigh it
    x[1 % N] = 0.0
    rows.append(("peaked", x))
    # p = (.475, .175, .175, .175, 0 ...): the three twins share the smallest key, and masses 1e-6 and 0.2 are reached at
    # the first and the second of them -- all three are in
    x = np.full(n, -30.0, F)
    x[:4] = (0.0, -1.0, -1.0, -1.0)
    rows.append(("boundary tie", x))
    return [(kind, np.ascontiguousarray(x[:N], dtype=F)) for kind, x in rows]
