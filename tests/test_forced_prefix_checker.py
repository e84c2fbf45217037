"""Forced target prefixes (include/slimt_hip.h, slimt_hip_ctx_set_target_prefix): the checker and the CPU-side checks.

The checker (`forced_translate`) is the decode loop of Model.cc:111-185 over the oracle's decode_step in PORTABLE mode,
changed in one place: at step t < P_b sentence b records and feeds prefix[b][t] instead of the arg-max. Alignment rows
are head 0 of the last layer, as so_translate copies them; scores are the float64 log_softmax at the recorded column,
-inf where the token is not in the shortlist. Here it is checked against the oracle's own translate (no prefix, and the
greedy output as the prefix), and the new entry point is checked to be exported, wrapped and loud without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest


def tmax_of(S, limit_factor=1.5):
    return max(1, int(np.float32(limit_factor) * np.float32(S)))


def forced_translate(oracle, om, m, ids, lens, sl, p_ids, p_len, limit_factor=1.5, eos=0):
    """(out_ids [B,T], out_len [B], align [B,T,S], scores [B,T] float64) of the forced-then-greedy decode loop."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        B, S = ids.shape
        T = tmax_of(S, limit_factor)
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(ids), mask)
        states = np.zeros((m.dec_layers, B, m.D), np.float32)
        out = np.zeros((B, T), np.uint32)
        ln = np.zeros(B, np.uint32)
        al = np.zeros((B, T, S), np.float32)
        sc = np.full((B, T), np.nan)
        done = np.zeros(B, bool)
        prev = None
        for t in range(T):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            tok = oracle.greedy_sample(logits, sl)
            lg = logits.astype(np.float64)
            mx = lg.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(axis=1))
            for b in range(B):
                if done[b]:
                    continue
                if t < int(p_len[b]):
                    tok[b] = p_ids[b, t]
                if sl is None:
                    col = int(tok[b]) if tok[b] < lg.shape[1] else -1
                else:
                    i = int(np.searchsorted(sl, tok[b]))
                    col = i if i < len(sl) and sl[i] == tok[b] else -1
                sc[b, t] = lg[b, col] - lse[b] if col >= 0 else -np.inf
                al[b, t, : int(lens[b])] = attn[b, 0, 0, : int(lens[b])]
                out[b, t] = tok[b]
                ln[b] += 1
                done[b] = tok[b] == eos
            prev = tok
            if done.all():
                break
        return out, ln, al, sc
    finally:
        oracle.set_mode(oracle.FAITHFUL)


@pytest.fixture(scope="module")
def tiny(oracle, synth_models):
    m = synth_models("tiny11", 6.0)
    return m, oracle.OracleModel(m)


@pytest.mark.parametrize("S", [8, 32])
def test_checker_without_prefix_and_with_its_own_output_is_the_oracle(oracle, tiny, S):
    from slimt_amd import synth
    m, om = tiny
    B = 9
    ids, lens = synth.make_batch(m.V, B, S, seed=3 + S, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    oracle.set_mode(oracle.PORTABLE)
    try:
        w_out, w_ln, w_al, _ = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    T = tmax_of(S)
    for p_ids, p_len in ((np.zeros((B, T), np.uint32), np.zeros(B, np.uint32)),
                         (w_out, np.minimum(w_ln, T).astype(np.uint32))):
        out, ln, al, sc = forced_translate(oracle, om, m, ids, lens, sl, p_ids, p_len)
        assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out)
        assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32))
        for b in range(B):
            assert np.all(sc[b, : ln[b]] <= 0.0)


def test_checker_forces_its_prefix_and_scores_missing_tokens_minus_inf(oracle, tiny):
    from slimt_amd import synth
    m, om = tiny
    B, S = 4, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=11, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    missing = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)[0]
    T = tmax_of(S)
    p_ids = np.zeros((B, T), np.uint32)
    p_ids[:, 0] = sl[5]
    p_ids[:, 1] = missing
    p_ids[2, 2] = 0  # EOS inside the prefix ends sentence 2 there
    p_len = np.array([0, 2, 4, T], np.uint32)
    p_ids[3, :] = sl[7]
    out, ln, _, sc = forced_translate(oracle, om, m, ids, lens, sl, p_ids, p_len)
    assert out[1, 0] == sl[5] and out[1, 1] == missing and sc[1, 1] == -np.inf and np.isfinite(sc[1, 0])
    assert ln[2] == 3 and out[2, 2] == 0
    assert ln[3] == T and np.all(out[3] == sl[7])


def test_set_target_prefix_is_exported_declared_and_wrapped():
    import os
    from slimt_amd import build, capi
    dll = ctypes.CDLL(build.build())
    assert hasattr(dll, "slimt_hip_ctx_set_target_prefix")
    assert "slimt_hip_ctx_set_target_prefix" in capi.SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "slimt_hip.h")) as f:
        assert "int slimt_hip_ctx_set_target_prefix(slimt_hip_ctx *ctx, const uint32_t *const *prefix_ids," in f.read()
    for name in ("translate", "translate_pinned", "translate_async", "translate_generated", "translate_device",
                 "translate_device_generated", "translate_many_device", "translate_many_async"):
        assert inspect.signature(getattr(capi.Context, name)).parameters["prefix"].default is None


def test_set_target_prefix_fails_loudly_without_a_context():
    from slimt_amd import capi
    L = capi.lib()
    arr = (ctypes.c_void_p * 1)(None)
    assert L.slimt_hip_ctx_set_target_prefix(None, arr, arr, 1) != 0
    assert b"null argument" in L.slimt_hip_last_error()


def test_wrappers_check_prefix_shapes_and_counts():
    """refused in Python before anything is armed on the context (no device needed: the checks come first)"""
    from slimt_amd import capi
    ctx = capi.Context.__new__(capi.Context)
    with pytest.raises(ValueError):
        capi.Context._prefix_host((np.zeros((2, 3), np.uint32), np.zeros(2, np.uint32)), 2, 4)
    with pytest.raises(ValueError):
        ctx.translate_many_async([(np.zeros((1, 8), np.uint32), np.zeros(1, np.uint32), np.zeros((1, 12), np.uint32),
                                   np.zeros(1, np.uint32), None)] * 2,
                                 prefix=[(np.zeros((1, 12), np.uint32), np.zeros(1, np.uint32))])


def test_service_prefixed_is_exported_declared_and_refuses_null_arguments():
    """include/slimt_hip_service_prefix.h against libslimt_hip_host.so: without a GPU no service can be created, so the
    entry point is checked on its argument errors (it fails loudly; there is no CPU fallback)"""
    import os
    from slimt_amd import build, capi
    build.build_host_lib()
    H = capi.host_lib()
    assert hasattr(H, "slimt_hip_service_translate_prefixed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "slimt_hip_service_prefix.h")) as f:
        assert "int slimt_hip_service_translate_prefixed(slimt_hip_service *service," in f.read()
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_translate_prefixed(None, None, None, None, None, 0, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert inspect.signature(capi.BatchService.translate).parameters["prefixes"].default is None
