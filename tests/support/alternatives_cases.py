"""The cases tests/test_gpu_score_alternatives.py compares with the checker of tests/test_alternatives_checker.py, and
tests/test_alternatives_case_fixtures.py checks for being worth comparing (CPU). One table, so that the GPU test and the CPU
proof of its coverage cannot drift.

Targets are built step by step on the oracle: the targets at t only influence rows > t, so step t's tokens are chosen from
step t's own logits. Row (b, t) takes slot (5 b + t) % 16 of SLOTS: a place in the row's order (0 = the checker's top-1),
"R" = a random id of the output layer, "O" = an id outside it (a random id of the layer where the layer is the whole
vocabulary: no id is outside). The places are chosen for k in KS = (1, 5, 8) at once -- ranks k - 1 and k for each of them
-- so that one pass over the oracle serves all three: the alternatives for k are the first k of those for 8."""
from collections import namedtuple

import numpy as np

from support import model_shapes as MS

KS = (1, 5, 8)
NONE = 0xFFFFFFFF
FILL = np.float32(-7.25)   # what the float output buffers hold before a call
FILL_U = np.uint32(0xABCD1234)  # ... and the integer ones: neither an id, a rank nor NONE
# rank 0 in five slots of sixteen (more than a quarter below k = 1), ranks >= 8 in six (more than a quarter not below k = 8)
SLOTS = (0, 8, 0, "R", 1, 11, 0, "O", 4, 9, 0, "R", 5, 8, 7, 0)

# name: (preset or model_shapes id, S, B, T or None = tmax_of(S) | 1, shortlist size or None). The issue's table, then one shape
# per embedding size 64 / 128 / 256 / 512 of tests/support/model_shapes.py
TABLE = {
    "tiny11-S32": ("tiny11", 32, 17, 48, 4096),
    "tiny11-full": ("tiny11", 8, 17, None, None),
    "tiny11-S64": ("tiny11", 64, 9, None, 4096),
    "base": ("base", 32, 9, None, 4096),
}
EMB_SHAPES = {}  # emb size -> the first model_shapes.SHAPES entry of that size
for _s in MS.SHAPES:
    EMB_SHAPES.setdefault(_s.dims[0], _s)
EMB_B, EMB_S, EMB_T = 5, 13, 21

Case = namedtuple("Case", "name m ids lens sl t_ids t_len alt")  # alt: the checker's result at k = 8, logits kept


def case_names():
    return list(TABLE) + ["emb%d" % d for d in sorted(EMB_SHAPES)]


def _spread(B, hi, lo=0):
    return [lo + (b * (hi - lo)) // max(1, B - 1) for b in range(B)]


def chooser(sl, V, seed):
    """choose(t, logits) of test_alternatives_checker.alternatives: the slots above"""
    rng = np.random.default_rng(seed)
    outside = None if sl is None else np.setdiff1d(np.arange(1, V, dtype=np.uint32), sl)

    def choose(t, logits):
        B, N = logits.shape
        toks = np.zeros(B, np.uint32)
        for b in range(B):
            slot = SLOTS[(5 * b + t) % 16]
            if slot == "O" and outside is not None and len(outside):
                toks[b] = rng.choice(outside)
                continue
            if isinstance(slot, str):
                col = int(rng.integers(N))
            else:
                cols = np.arange(N)
                order = cols[np.lexsort((cols, -logits[b].astype(np.float64)))]
                col = int(order[min(slot, N - 1)])
            toks[b] = col if sl is None else sl[col]
        return toks

    return choose


_CACHE = {}


def build(oracle, name):
    """the case and its reference, computed once per session"""
    if name in _CACHE:
        return _CACHE[name]
    from slimt_amd import synth
    from test_alternatives_checker import alternatives
    from test_forced_prefix_checker import tmax_of
    if name in TABLE:
        preset, S, B, T, n_sl = TABLE[name]
        m = synth.make_model(preset, seed=1234, eos_bias=6.0)
        T = T if T is not None else tmax_of(S) | 1
    else:
        s = EMB_SHAPES[int(name[3:])]
        m = MS.make(s)
        S, B, T, n_sl = EMB_S, EMB_B, EMB_T, MS.SHORTLIST
    ids, lens = synth.make_batch(m.V, B, S, seed=43 + S + B, ragged=True)
    lens[0], lens[-1] = 0, S
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    t_len = np.asarray(_spread(B, T, 0), np.uint32)  # 0 .. T, both included
    t_ids = np.zeros((B, T), np.uint32)
    om = oracle.OracleModel(m)
    alt = alternatives(oracle, om, m, ids, lens, sl, t_ids, t_len, max(KS), choose=chooser(sl, m.V, S + B), keep_logits=True)
    _CACHE[name] = Case(name, m, ids, lens, sl, t_ids, t_len, alt)
    return _CACHE[name]


def live(c):
    return np.arange(c.t_ids.shape[1])[None, :] < c.t_len[:, None]


def expected(c, k):
    """(alt_ids [B,T,k], alt_scores float64 [B,T,k], rank [B,T]) of the checker for k <= 8"""
    return c.alt.ids[:, :, :k], c.alt.scores[:, :, :k], c.alt.rank
