"""A NumPy restatement of slimt_amd/csrc/constraints.h (slimt_hip_ctx_set_step_constraints), sharing no code with it
(tests/test_constraints_checker.py holds the two together), the crafted rows of both kernel tests and the checker loop of
the translate test. A setting is the tuple (no_repeat_ngram, repetition_penalty, min_length, suppress)."""
from unittest import mock

import numpy as np

from support import floor_ref
from test_sampling_checker import first_max, row_keys
from test_truncation_checker import kept_scores

F = np.float32
OFF = (0, 1.0, 0, ())
as_dict = lambda cn: dict(zip(("no_repeat_ngram", "repetition_penalty", "min_length", "suppress"), cn))


def layout(N, with_ids):
    """(the columns' vocabulary ids or None, an eos id that has a column); id 2 has none under the ids"""
    ids = ((np.arange(N, dtype=np.uint64) * 3 + 1) % (1 << 32)).astype(np.uint32) if with_ids else None
    return ids, min(5, N - 1) if ids is None else int(ids[min(5, N - 1)])


def sets(h, cn, N, ids, eos):
    """(banned by the n-gram rule, banned otherwise, seen) bool [N] of a row with history h"""
    n, _, min_length, suppress = cn
    h, L = [int(x) for x in h], len(h)
    grams = {h[q + n - 1] for q in range(L - n + 1) if h[q:q + n - 1] == h[L - n + 1:]} if n >= 1 else set()

    def columns(bad):
        a, out = np.array(sorted(set(bad)), np.int64), np.zeros(N, bool)
        at = a if ids is None else np.searchsorted(ids, a)
        out[at[(at < N) & ((np.asarray(ids)[np.minimum(at, N - 1)] == a) if ids is not None else True)]] = True
        return out
    return columns(grams), columns(set(suppress) | ({eos} if L < min_length else set())), columns(h)


def constrained_row(logits, h, cn, ids, eos, inv_T=F(1.0), key=None, t=0, forced=False):
    """one step of one row: (column, none, banned count, fallback, float64 score, C, hits). key None: greedy. hits: whether
    the unconstrained choice was banned by the n-gram rule, by the EOS rule, and whether the penalty alone moved it."""
    l = np.ascontiguousarray(logits, dtype=F)
    grams, other, seen = sets([] if forced else h, OFF if forced else cn, l.size, ids, eos)
    banned, theta = grams | other, F(cn[1])
    with np.errstate(invalid="ignore", over="ignore"):
        lp = np.where(seen, np.where(l > 0, l * (F(1.0) / theta), l * theta), l).astype(F)
        z = (lp * F(inv_T)).astype(F)
    valid = ~np.isnan(z)
    C = valid & ~banned
    fallback = bool(valid.any() and not C.any())
    C = valid if fallback else C

    def pick(x, keep):
        v = (x * F(inv_T)).astype(F) if key is None else row_keys(key, t, x, ids, inv_T)
        return first_max(np.where(keep, v, F(-np.inf)), l[0])
    (col, none), plain, penalised = pick(lp, C), pick(l, ~np.isnan(l))[0], pick(lp, valid)[0]
    hits = (bool(grams[plain]), bool(len(h) < cn[2] and (plain if ids is None else ids[plain]) == eos), penalised != plain)
    return col, none, int(banned.sum()), fallback, kept_scores(z, C, none)[col], C, hits


def crafted_rows(N, ids, eos, seed):
    """[(kind, logits float32 [N], history, setting)] of both kernel tests; eos has a column, `absent` is an id without one"""
    rng = np.random.default_rng(seed)
    tok = (lambda c: int(c)) if ids is None else (lambda c: int(ids[c]))
    g, absent = rng.normal(0.0, 2.0, N).astype(F), 2 if ids is not None else N + 5
    top, low, e = int(np.argmax(g)), int(np.argmin(g)), int(np.flatnonzero((np.arange(N) if ids is None else ids) == eos)[0])
    few = [tok(c) for c in rng.integers(0, N, 4)] + [absent]
    first = [tok(c) for c in range(min(N, 64))]
    tie, early, nan = g.copy(), g.copy(), g.copy()
    tie[[0, N // 2, N - 1]] = early[e] = g.max() + F(1.0)
    nan[[top, N // 3]] = np.nan
    rows = [("maximum banned", g, [tok(top)], (1, 1.0, 0, ())),
            ("every column banned (N <= 64)", g, first[::-1], (1, 1.0, 0, first)),
            ("tie of a banned and an unbanned column", tie, [tok(0)], (1, 1.0, 0, ())),
            ("nan on the banned maximum", nan, [tok(top)], (1, 1.0, 0, ()))]
    # top and low are seen twice: one product each, a positive and a negative logit wherever N >= 2
    rows += [("penalty %.1f" % th, g, [tok(top), tok(low), tok(top), absent, tok(low), tok(N // 2)], (0, th, 0, ())) for th in (1.3, 0.7)]
    rows += [("a a a a, n = %d" % n, g, [tok(top)] * 4, (n, 1.0, 0, ())) for n in (2, 3)]
    rows += [("min_length 3 at L = %d" % L, early, [tok(low)] * L, (0, 1.2, 3, ())) for L in (2, 3)]
    # n = 3: L in {0, n - 1, n, one wave of windows and either side, the bound}
    rows += [("L = %d" % L, g, [few[i] for i in rng.integers(0, len(few), L)], (3, 1.1, 0, (absent,))) for L in (0, 2, 3, 63, 64, 65, 1024)]
    return [(kind, np.ascontiguousarray(x, dtype=F), [int(v) for v in h], (n, th, ml, tuple(int(v) for v in sup)))
            for kind, x, h, (n, th, ml, sup) in rows]


def constrained_translate(oracle, om, m, ids, lens, sl, cn, keys, T=None, p_ids=None, p_len=None, trace=None):
    """floor_ref.floored_translate with constrained_row in place of floored_row, sampled at T or greedy (T None: the keys only
    name the rows), under an optional forced prefix of shortlisted tokens. trace (a list): gets every unforced step's hits."""
    row_of, hist = {int(k): b for b, k in enumerate(keys)}, {}

    def row(key, t, logits, sl, inv_T, *_):
        b, h = row_of[int(key)], hist.setdefault(int(key), [])
        forced = p_len is not None and t < int(p_len[b])
        col, none, _, _, s, C, hits = constrained_row(logits, h, cn, sl, 0, inv_T, None if T is None else key, t, forced)
        if forced:  # (scored over the whole layer, like every forced step)
            col = int(np.searchsorted(sl, p_ids[b, t]))
            s = kept_scores((logits * inv_T).astype(F), C, none)[col]
        elif trace is not None:
            trace.append(hits)
        h.append(int(sl[col]))
        return col, none, C, None, s
    with mock.patch.object(floor_ref, "floored_row", row):
        return floor_ref.floored_translate(oracle, om, m, ids, lens, sl, keys, 1.0 if T is None else T, 0.0, 0.0)
