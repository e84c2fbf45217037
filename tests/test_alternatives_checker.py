"""Alternatives of teacher-forced scoring (include/slimt_hip.h, slimt_hip_ctx_set_score_alternatives): the checker and the
CPU-side checks.

The checker (`alternatives`) loops over the oracle's decode_step in PORTABLE mode like `teacher_forced` of
tests/test_score_checker.py, and per live row sorts the valid (non-NaN) columns by (-logit, column) -- float comparison, so
+0 equals -0 and the infinities order like any value --, takes the float64 log-softmax of the first k and counts the
columns ordered before the target's. Here it is checked against `teacher_forced` (the score at index `rank`) and the
oracle's greedy_sample (the first alternative), `row_alternatives` is checked on hand-made rows, and the new entry points
are checked to be declared, exported, wrapped and loud without a context."""
import ctypes
import inspect
import os
from collections import namedtuple

import numpy as np
import pytest

from test_score_checker import teacher_forced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF

Alternatives = namedtuple("Alternatives", "ids scores rank logits")


def row_alternatives(lg, k, col):
    """One row of float32 logits lg [N]: (columns [k] int64, -1 past the valid ones; scores [k] float64, -inf there; rank,
    NONE when col < 0 or its logit is NaN). Scores are lg[c] - logsumexp(lg) in float64, with teacher_forced's expression:
    a row holding a NaN gives NaN scores."""
    lg = np.asarray(lg, np.float32)
    cols = np.flatnonzero(~np.isnan(lg))
    order = cols[np.lexsort((cols, -lg[cols].astype(np.float64)))]  # (-0.0 == 0.0 under <: ties fall to the column)
    l64 = lg.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = l64.max()
        lse = mx + np.log(np.exp(l64 - mx).sum())
        out_c = np.full(k, -1, np.int64)
        out_s = np.full(k, -np.inf)
        n = min(k, len(order))
        out_c[:n] = order[:n]
        out_s[:n] = l64[order[:n]] - lse
    if col < 0 or np.isnan(lg[col]):
        return out_c, out_s, NONE
    y = lg[col]
    before = (lg[cols] > y) | ((lg[cols] == y) & (cols < col))
    return out_c, out_s, int(before.sum())


def column_of(sl, tok, N):
    if sl is None:
        return int(tok) if tok < N else -1
    i = int(np.searchsorted(sl, tok))
    return i if i < len(sl) and sl[i] == tok else -1


def alternatives(oracle, om, m, ids, lens, sl, t_ids, t_len, k, choose=None, keep_logits=False):
    """Alternatives(ids [B,T,k] uint32, scores [B,T,k] float64, rank [B,T] uint32, logits) of the given targets; entries
    with t >= t_len[b] hold NONE / NaN / NONE (the calls do not write them). choose(t, logits) -> tokens [B]: the targets
    of step t are chosen from the step's own logits and written into t_ids before its rows are evaluated (the targets at t
    only influence rows > t). logits: the steps' [B, N] float32 arrays when keep_logits, else None."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        assert t_ids.dtype == np.uint32 and t_ids.flags.c_contiguous
        B, S = ids.shape
        T = t_ids.shape[1]
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(ids), mask)
        states = np.zeros((m.dec_layers, B, m.D), np.float32)
        a_ids = np.full((B, T, k), NONE, np.uint32)
        a_sc = np.full((B, T, k), np.nan)
        rank = np.full((B, T), NONE, np.uint32)
        kept = []
        for t in range(int(np.max(t_len, initial=0))):
            prev = None if t == 0 else np.ascontiguousarray(t_ids[:, t - 1])
            logits, _ = om.decode_step(enc, mask, states, prev, sl)
            if keep_logits:
                kept.append(np.array(logits, np.float32))
            if choose is not None:
                t_ids[:, t] = choose(t, logits)
            N = logits.shape[1]
            for b in range(B):
                if t >= int(t_len[b]):
                    continue
                c, s, r = row_alternatives(logits[b], k, column_of(sl, t_ids[b, t], N))
                a_ids[b, t] = [NONE if x < 0 else (x if sl is None else sl[x]) for x in c]
                a_sc[b, t] = s
                rank[b, t] = r
        return Alternatives(a_ids, a_sc, rank, kept if keep_logits else None)
    finally:
        oracle.set_mode(oracle.FAITHFUL)


# ---- the checker against the score checker and the greedy arg-max -------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(oracle, synth_models):
    m = synth_models("tiny11", 6.0)
    return m, oracle.OracleModel(m)


@pytest.mark.parametrize("n_sl", [4096, None])
def test_checker_agrees_with_the_score_checker_and_the_greedy_sample(oracle, tiny, n_sl):
    from slimt_amd import synth
    m, om = tiny
    B, S, T, k = 4, 8, 6, 5
    ids, lens = synth.make_batch(m.V, B, S, seed=11, ragged=True)
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    rng = np.random.default_rng(3)

    def choose(t, logits):  # top-1, the third and the sixth of the order, a random id of the layer
        order = np.argsort(-logits.astype(np.float64), axis=1, kind="stable")
        col = np.array([order[0, 0], order[1, 2], order[2, 5], rng.integers(logits.shape[1])])
        return (col if sl is None else sl[col]).astype(np.uint32)

    t_ids = np.zeros((B, T), np.uint32)
    t_len = np.array([T, T, T - 1, 3], np.uint32)
    alt = alternatives(oracle, om, m, ids, lens, sl, t_ids, t_len, k, choose=choose, keep_logits=True)
    if sl is not None:
        t_ids[3, 1] = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)[0]  # (row (3, 1) only: it feeds row (3, 2))
        alt = alternatives(oracle, om, m, ids, lens, sl, t_ids, t_len, k, keep_logits=True)
        assert alt.rank[3, 1] == NONE
    sc, _ = teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len)
    hits = 0
    for b in range(B):
        for t in range(int(t_len[b])):
            r = int(alt.rank[b, t])
            if r < k:
                assert alt.scores[b, t, r] == sc[b, t], (b, t)  # the same expression on the same logits
                assert alt.ids[b, t, r] == t_ids[b, t]
                hits += 1
            else:
                assert t_ids[b, t] not in alt.ids[b, t]
            assert np.all(np.diff(alt.scores[b, t]) <= 0)
        assert np.all(alt.ids[b, t_len[b]:] == NONE) and np.all(np.isnan(alt.scores[b, t_len[b]:]))
        assert np.all(alt.rank[b, t_len[b]:] == NONE)
    assert hits >= 2 * T - 1 and np.all(alt.rank[0, :T] == 0) and np.all(alt.rank[1, :T] == 2) and np.all(alt.rank[2, :T - 1] == 5)
    for t, lg in enumerate(alt.logits):
        top = oracle.greedy_sample(lg, sl)
        live = t < t_len
        assert np.array_equal(alt.ids[live, t, 0], top[live]), t


# ---- hand-made rows -------------------------------------------------------------------------------------------------------
def _lsm(row):
    l = np.asarray(row, np.float64)
    return l - (l.max() + np.log(np.exp(l - l.max()).sum()))


def test_rows_with_ties_go_to_the_lower_column():
    lg = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 3.0, 0.5], np.float32)
    c, s, r = row_alternatives(lg, 5, 3)
    assert c.tolist() == [1, 3, 5, 2, 4] and r == 1
    assert np.array_equal(s, _lsm(lg)[[1, 3, 5, 2, 4]])
    assert row_alternatives(lg, 5, 5)[2] == 2 and row_alternatives(lg, 5, 4)[2] == 4 and row_alternatives(lg, 5, 6)[2] == 6
    assert row_alternatives(lg, 1, 1)[0].tolist() == [1]


def test_rows_with_signed_zeros_compare_equal():
    lg = np.array([-1.0, 0.0, -0.0, 0.0, -0.0], np.float32)
    assert np.signbit(lg[2]) and not np.signbit(lg[1])
    c, s, r = row_alternatives(lg, 4, 2)
    assert c.tolist() == [1, 2, 3, 4] and r == 1  # by column, whatever the sign
    lg = lg[[0, 2, 1, 4, 3]]
    assert row_alternatives(lg, 4, 4)[0].tolist() == [1, 2, 3, 4] and row_alternatives(lg, 4, 4)[2] == 3


def test_rows_with_infinities_order_like_any_value():
    lg = np.array([2.0, -np.inf, 7.0, -np.inf, 1.0], np.float32)
    c, s, r = row_alternatives(lg, 5, 3)
    assert c.tolist() == [2, 0, 4, 1, 3] and r == 4
    assert s[3] == -np.inf and s[4] == -np.inf and np.all(np.isfinite(s[:3]))  # probability 0, still valid columns
    assert row_alternatives(lg, 5, 1)[2] == 3
    c, s, r = row_alternatives(np.array([2.0, np.inf, 7.0, np.inf], np.float32), 3, 3)
    assert c.tolist() == [1, 3, 2] and r == 1
    assert np.all(np.isnan(s))  # inf - inf: the float64 log-softmax itself is NaN


def test_rows_with_nan_keep_the_order_of_the_valid_columns():
    lg = np.array([2.0, np.nan, 7.0, 1.0, np.nan], np.float32)
    c, s, r = row_alternatives(lg, 4, 3)
    assert c.tolist() == [2, 0, 3, -1] and r == 2
    assert np.all(np.isnan(s[:3])) and s[3] == -np.inf
    assert row_alternatives(lg, 4, 1)[2] == NONE and row_alternatives(lg, 4, -1)[2] == NONE
    c, s, r = row_alternatives(np.full(3, np.nan, np.float32), 2, 0)
    assert c.tolist() == [-1, -1] and np.all(s == -np.inf) and r == NONE


def test_rows_narrower_than_k_and_of_one_column():
    lg = np.array([0.25, 1.5, -3.0], np.float32)
    c, s, r = row_alternatives(lg, 8, 2)
    assert c.tolist() == [1, 0, 2, -1, -1, -1, -1, -1] and r == 2
    assert np.array_equal(s[:3], _lsm(lg)[[1, 0, 2]]) and np.all(s[3:] == -np.inf)
    c, s, r = row_alternatives(np.array([-4.0], np.float32), 5, 0)
    assert c.tolist() == [0, -1, -1, -1, -1] and s[0] == 0.0 and np.all(s[1:] == -np.inf) and r == 0
    assert row_alternatives(np.array([-4.0], np.float32), 5, -1)[2] == NONE


# ---- the entry points without a device -----------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_wrapped():
    from slimt_amd import build, capi
    dll = ctypes.CDLL(build.build())
    with open(os.path.join(ROOT, "include", "slimt_hip.h")) as f:
        header = f.read()
    name = "slimt_hip_ctx_set_score_alternatives"
    assert hasattr(dll, name) and name in capi.SYMBOLS
    assert "int %s(slimt_hip_ctx *ctx, uint32_t k, uint32_t *alt_ids, float *alt_scores," % name in header
    assert "#define SLIMT_HIP_MAX_ALTERNATIVES 8" in header and capi.MAX_ALTERNATIVES == 8
    assert "#define SLIMT_HIP_ABI_VERSION 3" in header and capi.lib().slimt_hip_abi_version() == 3
    for fn in (capi.Context.score, capi.Context.score_async, capi.Context.score_device):
        assert inspect.signature(fn).parameters["alternatives"].default is None
    assert inspect.signature(capi.BatchService.score).parameters["alternatives"].default == 0
    assert callable(capi.Context.set_score_alternatives) and callable(capi.ServiceResult.alternatives)
    from slimt_amd import frontend
    assert inspect.signature(frontend.Service.score).parameters["alternatives"].default == 0
    fields = {f.name: f for f in frontend.PairScore.__dataclass_fields__.values()}
    assert fields["ranks"].default is None and fields["alternatives"].default is None


def test_entry_point_fails_loudly_without_a_context():
    from slimt_amd import capi
    L = capi.lib()
    ids = (ctypes.c_uint32 * 8)()
    assert L.slimt_hip_ctx_set_score_alternatives(None, 1, ids, None, None) != 0
    assert b"null argument" in L.slimt_hip_last_error()
    assert L.slimt_hip_ctx_set_score_alternatives(None, 0, None, None, None) != 0
    assert b"null argument" in L.slimt_hip_last_error()
    assert L.slimt_hip_ctx_set_score_alternatives(None, 9, ids, None, None) != 0  # (the value first)
    assert b"exceeds SLIMT_HIP_MAX_ALTERNATIVES" in L.slimt_hip_last_error()


def test_wrappers_refuse_mismatched_shapes():
    """refused in Python before anything reaches the library (no device needed: the checks come first)"""
    from slimt_amd import capi
    ctx = capi.Context.__new__(capi.Context)
    ids, lens = np.zeros((2, 4), np.uint32), np.zeros(2, np.uint32)
    tg, tl = np.zeros((2, 5), np.uint32), np.zeros(2, np.uint32)
    for k in (9, -1, 2.5, True):
        with pytest.raises(ValueError):
            ctx.score(ids, lens, None, tg, tl, alternatives=k)
    with pytest.raises(ValueError):
        ctx.score(ids, lens, None, np.zeros((3, 5), np.uint32), tl, alternatives=3)
    bufs = (ids, lens, tg, tl, np.zeros((2, 5), np.float32), None)
    u32, f32 = np.uint32, np.float32
    for alt in ((np.zeros((2, 5, 9), u32), None, None),                                # k = 9
                (np.zeros((2, 4, 3), u32), None, None),                                # T
                (np.zeros((2, 5, 3), np.int64), None, None),                           # dtype
                (None, np.zeros((2, 5, 3), f32), None),                                # no ids
                (np.zeros((2, 5, 3), u32), np.zeros((2, 5, 4), f32), None),            # scores' k
                (np.zeros((2, 5, 3), u32), np.zeros((2, 5, 3), f32), np.zeros((2, 4), u32)),  # rank's T
                (np.zeros((2, 5, 3), u32), np.zeros((2, 5, 3), f32))):                 # two arrays
        with pytest.raises(ValueError):
            ctx.score_async(bufs, alternatives=alt)
    with pytest.raises(ValueError):
        ctx.score_async(bufs, alternatives=9)
    with pytest.raises(ValueError):
        ctx.score_device(1, 1, 2, 4, 0, 0, 1, 1, 5, 1, alternatives=(9, 1, 0, 0))
    with pytest.raises(ValueError):
        ctx.score_device(1, 1, 2, 4, 0, 0, 1, 1, 5, 1, alternatives=(3, 0, 0, 0))
    svc = capi.BatchService.__new__(capi.BatchService)
    with pytest.raises(ValueError):
        svc.score([[1, 2, 0]], [[3, 0]], alternatives=9)
    with pytest.raises(ValueError):
        svc.score([[1, 2, 0]], [[3, 0], [4, 0]], alternatives=3)


def test_service_entry_points_are_exported_declared_and_refuse_bad_arguments():
    """include/slimt_hip_service_alternatives.h against libslimt_hip_host.so: without a GPU no service can be created, so
    the entry points are checked on their argument errors"""
    import re
    from slimt_amd import build, capi
    build.build_host_lib()
    H = capi.host_lib()
    with open(os.path.join(ROOT, "include", "slimt_hip_service_alternatives.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(slimt_hip_(?:service|result)_[a-z0-9_]+)\s*\(", text)))
    assert names == ["slimt_hip_result_alternatives", "slimt_hip_service_score_alternatives"]
    for n in names:
        assert hasattr(H, n), n
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_score_alternatives(None, None, None, None, None, 0, 3, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert H.slimt_hip_service_score_alternatives(None, None, None, None, None, 0, 9, ctypes.byref(out)) != 0
    assert b"not in 1..8" in H.slimt_hip_service_last_error()
    assert H.slimt_hip_service_score_alternatives(None, None, None, None, None, 0, 0, ctypes.byref(out)) != 0
    assert H.slimt_hip_result_alternatives(None, 0, None, None, None, None) != 0
    assert b"result is NULL" in H.slimt_hip_service_last_error()
