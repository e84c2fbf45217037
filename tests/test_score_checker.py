"""Teacher-forced scoring (include/slimt_hip.h, slimt_hip_score*): the checker and the CPU-side checks.

The checker (`teacher_forced`) is a loop over the oracle's decode_step in PORTABLE mode with prev = t_ids[:, t - 1] -- the
given targets, never the arg-max -- that does not stop at EOS. Scores are the float64 log_softmax at the target column,
-inf where the token is not in the shortlist; alignment rows are head 0 of the last layer. Here it is checked against the
forced-prefix checker (targets ending in EOS) and against a decode loop that is simply not stopped (EOS in the middle), and
the new entry points are checked to be declared, exported, wrapped and loud without a GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from test_forced_prefix_checker import forced_translate, tmax_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slimt_hip_score", "slimt_hip_score_async", "slimt_hip_score_device", "slimt_hip_score_async_generated")


def teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len):
    """(scores [B,T] float64, align [B,T,S] float32) of the given targets; entries with t >= t_len[b] are NaN, alignment
    columns j >= lens[b] NaN as well (the calls do not write them)."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        t_ids = np.ascontiguousarray(t_ids, dtype=np.uint32)
        B, S = ids.shape
        T = t_ids.shape[1]
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(ids), mask)
        states = np.zeros((m.dec_layers, B, m.D), np.float32)
        sc = np.full((B, T), np.nan)
        al = np.full((B, T, S), np.nan, np.float32)
        for t in range(int(np.max(t_len, initial=0))):
            prev = None if t == 0 else np.ascontiguousarray(t_ids[:, t - 1])
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            lg = logits.astype(np.float64)
            mx = lg.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(axis=1))
            for b in range(B):
                if t >= int(t_len[b]):
                    continue
                tok = t_ids[b, t]
                if sl is None:
                    col = int(tok) if tok < lg.shape[1] else -1
                else:
                    i = int(np.searchsorted(sl, tok))
                    col = i if i < len(sl) and sl[i] == tok else -1
                sc[b, t] = lg[b, col] - lse[b] if col >= 0 else -np.inf
                al[b, t, : int(lens[b])] = attn[b, 0, 0, : int(lens[b])]
        return sc, al
    finally:
        oracle.set_mode(oracle.FAITHFUL)


@pytest.fixture(scope="module")
def tiny(oracle, synth_models):
    m = synth_models("tiny11", 6.0)
    return m, oracle.OracleModel(m)


@pytest.mark.parametrize("S", [8, 32])
def test_checker_is_the_forced_prefix_checker_on_targets_ending_in_eos(oracle, tiny, S):
    from slimt_amd import synth
    m, om = tiny
    B = 5
    ids, lens = synth.make_batch(m.V, B, S, seed=5 + S, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    T = tmax_of(S)
    rng = np.random.default_rng(S)
    pool = sl[sl != 0]
    t_ids = rng.choice(pool, size=(B, T)).astype(np.uint32)
    t_len = np.array([1, 2, T // 2, T - 1, T], np.uint32)
    for b in range(B):
        t_ids[b, t_len[b] - 1] = 0  # EOS ends each target
    sc, al = teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len)
    w_out, w_ln, w_al, w_sc = forced_translate(oracle, om, m, ids, lens, sl, t_ids, t_len)
    assert np.array_equal(w_ln, t_len)
    for b in range(B):
        n, L = int(t_len[b]), int(lens[b])
        assert np.array_equal(sc[b, :n], w_sc[b, :n]), b  # the same formula on the same logits
        assert np.array_equal(al[b, :n, :L].view(np.uint32), w_al[b, :n, :L].view(np.uint32)), b
        assert np.all(np.isnan(sc[b, n:])) and np.all(np.isnan(al[b, n:])) and np.all(np.isnan(al[b, :, L:]))


def test_checker_goes_on_behind_an_eos_in_the_middle(oracle, tiny):
    """the rows behind an EOS are those of the oracle's decode loop fed the same tokens and not stopped"""
    from slimt_amd import synth
    m, om = tiny
    B, S, T = 3, 8, 7
    ids, lens = synth.make_batch(m.V, B, S, seed=21, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    rng = np.random.default_rng(2)
    t_ids = rng.choice(sl[sl != 0], size=(B, T)).astype(np.uint32)
    t_ids[:, 2] = 0
    t_len = np.full(B, T, np.uint32)
    sc, al = teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len)
    oracle.set_mode(oracle.PORTABLE)
    try:
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(np.ascontiguousarray(ids, dtype=np.uint32)), mask)
        states = np.zeros((m.dec_layers, B, m.D), np.float32)
        prev = None
        for t in range(T):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            lg = logits.astype(np.float64)
            for b in range(B):
                col = int(np.searchsorted(sl, t_ids[b, t]))
                mx = lg[b].max()
                want = lg[b, col] - (mx + np.log(np.exp(lg[b] - mx).sum()))
                assert sc[b, t] == want, (b, t)
                assert np.array_equal(al[b, t, : lens[b]].view(np.uint32), attn[b, 0, 0, : lens[b]].view(np.uint32))
            prev = np.ascontiguousarray(t_ids[:, t])
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    assert np.all(np.isfinite(sc[:, 3:]))


def test_score_entry_points_are_declared_exported_and_wrapped():
    from slimt_amd import build, capi
    dll = ctypes.CDLL(build.build())
    with open(os.path.join(ROOT, "include", "slimt_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(dll, name), name
        assert name in capi.SYMBOLS, name
        assert "int %s(slimt_hip_ctx *ctx," % name in header, name
    assert "#define SLIMT_HIP_ABI_VERSION 3" in header
    for name in ("score", "score_async", "score_device"):
        assert callable(getattr(capi.Context, name)), name
    assert inspect.signature(capi.Context.score).parameters["want_align"].default is False
    assert list(inspect.signature(capi.BatchService.score).parameters)[1:3] == ["sentences", "targets"]


def test_score_entry_points_fail_loudly_without_a_context():
    from slimt_amd import capi
    L = capi.lib()
    one = (ctypes.c_uint32 * 1)(0)
    sc = (ctypes.c_float * 1)(0)
    for fn in (L.slimt_hip_score, L.slimt_hip_score_async, L.slimt_hip_score_device):
        assert fn(None, one, one, 1, 1, None, 0, one, one, 1, sc, None) != 0
        assert b"null argument" in L.slimt_hip_last_error()
    assert L.slimt_hip_score_async_generated(None, None, one, one, 1, 1, one, one, 1, sc, None) != 0
    assert b"null argument" in L.slimt_hip_last_error()


def test_wrappers_refuse_mismatched_shapes():
    """refused in Python before anything reaches the library (no device needed: the checks come first)"""
    from slimt_amd import capi
    ctx = capi.Context.__new__(capi.Context)
    ids, lens = np.zeros((2, 4), np.uint32), np.zeros(2, np.uint32)
    with pytest.raises(ValueError):
        ctx.score(ids, lens, None, np.zeros((3, 5), np.uint32), np.zeros(3, np.uint32))
    with pytest.raises(ValueError):
        ctx.score(ids, lens, None, np.zeros((2, 5), np.uint32), np.zeros(3, np.uint32))
    with pytest.raises(ValueError):
        ctx.score(ids, np.zeros(3, np.uint32), None, np.zeros((2, 5), np.uint32), np.zeros(2, np.uint32))
    with pytest.raises(ValueError):
        ctx.score_async((ids, lens, np.zeros((2, 5), np.uint32), np.zeros(2, np.uint32), np.zeros((2, 4), np.float32), None))
    with pytest.raises(ValueError):
        ctx.score_async((ids, lens, np.zeros((2, 5), np.uint32), np.zeros(2, np.uint32), np.zeros((2, 5), np.float32),
                         np.zeros((2, 5, 3), np.float32)))
    svc = capi.BatchService.__new__(capi.BatchService)
    with pytest.raises(ValueError):
        svc.score([[1, 2, 0]], [[3, 0], [4, 0]])


def test_service_score_is_exported_declared_and_refuses_null_arguments():
    """include/slimt_hip_service_score.h against libslimt_hip_host.so: without a GPU no service can be created, so the
    entry point is checked on its argument errors (it fails loudly; there is no CPU fallback)"""
    from slimt_amd import build, capi
    build.build_host_lib()
    H = capi.host_lib()
    assert hasattr(H, "slimt_hip_service_score")
    with open(os.path.join(ROOT, "include", "slimt_hip_service_score.h")) as f:
        assert "int slimt_hip_service_score(slimt_hip_service *service," in f.read()
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_score(None, None, None, None, None, 0, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
