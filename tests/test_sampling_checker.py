"""Sampled decoding (include/slimt_hip.h, slimt_hip_ctx_set_sampling): the noise, the checker and the CPU-side checks.

slimt_amd/csrc/sampling.h is compiled here for the host (g++ -O2 -ffp-contract=off), so the Gumbel noise the kernels add
is available bit for bit: its accuracy and monotony over all 2^23 uniforms, the hash's uniformity, and the draw's
distribution are checked on it. The checker (`sampled_translate`) is forced_translate of test_forced_prefix_checker.py
with the token rule of the header: at step t (the sentence's count of recorded tokens) the token is the vocabulary id of
the first maximum of fmaf(logit, 1 / T, g(key, t, id)); its scores are the float64 log_softmax of z = logit * (1 / T) at
the recorded column."""
import atexit
import ctypes
import inspect
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_forced_prefix_checker import tmax_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include "sampling.h"
using namespace slimt_hip;
extern "C" {
void gumbel_all(float *out, uint32_t h0, uint32_t n) { for (uint32_t i = 0; i < n; ++i) out[i] = sm_gumbel_of(sm_uniform(h0 + i)); }
void uniform_all(float *out, uint32_t h0, uint32_t n) { for (uint32_t i = 0; i < n; ++i) out[i] = sm_uniform(h0 + i); }
uint64_t sentence_key(uint64_t seed, uint64_t index) { return sm_sentence_key(seed, index); }
// u of (key, t, ids[i])
void hash_u(uint64_t key, uint32_t t, const uint32_t *ids, uint32_t n, float *out) {
  const uint64_t w = sm_step_words(key, t);
  for (uint32_t i = 0; i < n; ++i) out[i] = sm_uniform(sm_hash23((uint32_t)w, (uint32_t)(w >> 32), ids[i]));
}
// the compared values of one row of logits (ids == nullptr: the column is the id)
void keys_row(uint64_t key, uint32_t t, const float *l, const uint32_t *ids, uint32_t n, float inv_T, float *out) {
  const uint64_t w = sm_step_words(key, t);
  for (uint32_t i = 0; i < n; ++i) out[i] = sm_key(l[i], inv_T, (uint32_t)w, (uint32_t)(w >> 32), ids ? ids[i] : i);
}
// one draw per key at step 0: the first maximum from the arg-max's start value (-FLT_MAX, strict >)
void draw_many(const uint64_t *keys, uint32_t n_keys, const float *l, const uint32_t *ids, uint32_t n, float inv_T, uint32_t *out) {
  for (uint32_t k = 0; k < n_keys; ++k) {
    const uint64_t w = sm_step_words(keys[k], 0);
    float best = -3.402823466e+38f;
    uint32_t bi = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const float v = sm_key(l[i], inv_T, (uint32_t)w, (uint32_t)(w >> 32), ids ? ids[i] : i);
      if (v > best) { best = v; bi = i; }
    }
    out[k] = bi;
  }
}
}
"""

_lib = None


def harness():
    """sampling.h compiled for the host, once per process"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="slimt_sampling_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = os.path.join(d, "h.cc")
        with open(src, "w") as f:
            f.write(_HARNESS)
        so = os.path.join(d, "h.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "slimt_amd", "csrc"), src, "-o", so])
        h = ctypes.CDLL(so)
        vp, u32, u64, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
        h.gumbel_all.argtypes = [vp, u32, u32]
        h.uniform_all.argtypes = [vp, u32, u32]
        h.sentence_key.argtypes = [u64, u64]
        h.sentence_key.restype = u64
        h.hash_u.argtypes = [u64, u32, vp, u32, vp]
        h.keys_row.argtypes = [u64, u32, vp, vp, u32, f32, vp]
        h.draw_many.argtypes = [vp, u32, vp, vp, u32, f32, vp]
        _lib = h
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def keys_of(seed, n, first=0):
    h = harness()
    return np.array([h.sentence_key(seed, first + i) for i in range(n)], dtype=np.uint64)


def row_keys(key, t, logits, ids, inv_T):
    """float32 compared values of one row: fmaf(logit, inv_T, g(key, t, id)), the header's own bits"""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    out = np.empty(l.size, np.float32)
    i = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    harness().keys_row(int(key), int(t), _ptr(l), _ptr(i), l.size, ctypes.c_float(inv_T), _ptr(out))
    return out


def first_max(keys, logit0):
    """the arg-max's rules on the keys: from -FLT_MAX with strict >, NaNs skipped; class 0 when nothing beats the start
    value or logit 0 is NaN. Returns (column, none)"""
    ok = keys > np.float32(-3.402823466e+38)  # (NaN compares false)
    if np.isnan(logit0) or not ok.any():
        return 0, True
    return int(np.argmax(np.where(ok, keys, -np.inf))), False  # (argmax: the first maximum)


def sampled_translate(oracle, om, m, ids, lens, sl, keys, T, p_ids=None, p_len=None, limit_factor=1.5, eos=0, trace=None):
    """(out_ids [B,T], out_len [B], align [B,T,S], scores [B,T] float64) of the forced-then-sampled decode loop.
    keys: uint64 [B] (None: the row indices). trace (a list): gets every active row's gap between its two largest logits."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        B, S = ids.shape
        Tm = tmax_of(S, limit_factor)
        keys = np.arange(B, dtype=np.uint64) if keys is None else np.asarray(keys, dtype=np.uint64)
        inv_T = np.float32(1.0) / np.float32(T)
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(ids), mask)
        states = np.zeros((m.dec_layers, B, m.D), np.float32)
        out = np.zeros((B, Tm), np.uint32)
        ln = np.zeros(B, np.uint32)
        al = np.zeros((B, Tm, S), np.float32)
        sc = np.full((B, Tm), np.nan)
        done = np.zeros(B, bool)
        prev = None
        for t in range(Tm):
            logits, attn = om.decode_step(enc, mask, states, prev, sl)
            logits = np.ascontiguousarray(logits, dtype=np.float32)
            z = (logits * inv_T).astype(np.float32).astype(np.float64)  # (one float32 product, like the kernels')
            mx = z.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(z - mx).sum(axis=1))
            tok = np.zeros(B, np.uint32)
            for b in range(B):
                col, none = first_max(row_keys(keys[b], ln[b], logits[b], sl, inv_T), logits[b, 0])
                tok[b] = col if sl is None else sl[col]
                if done[b]:
                    continue
                if trace is not None:
                    top = np.sort(logits[b])[-2:]
                    trace.append(float(top[1] - top[0]))
                if p_len is not None and t < int(p_len[b]):
                    tok[b] = p_ids[b, t]
                    if sl is None:
                        col = int(tok[b]) if tok[b] < z.shape[1] else -1
                    else:
                        i = int(np.searchsorted(sl, tok[b]))
                        col = i if i < len(sl) and sl[i] == tok[b] else -1
                sc[b, t] = np.nan if none else (z[b, col] - lse[b] if col >= 0 else -np.inf)
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


def chi2_quantile_9999(k):
    """the 99.99 % quantile of chi-square with k degrees of freedom (Wilson-Hilferty)"""
    zq = 3.719016485  # the standard normal's 99.99 % quantile
    return k * (1.0 - 2.0 / (9.0 * k) + zq * np.sqrt(2.0 / (9.0 * k))) ** 3


# ---- 1: the noise ---------------------------------------------------------------------------------------------------------
def test_gumbel_of_every_uniform_is_accurate_finite_and_monotone():
    h = harness()
    n = 1 << 23
    g, u = np.empty(n, np.float32), np.empty(n, np.float32)
    h.gumbel_all(_ptr(g), 0, n)
    h.uniform_all(_ptr(u), 0, n)
    u64 = (np.arange(n, dtype=np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u.astype(np.float64), u64)  # every u an exact float in (0, 1)
    assert u.max() < 1.0 and u.min() > 0.0
    assert np.all(np.isfinite(g))
    err = np.abs(g.astype(np.float64) + np.log(-np.log(u64)))
    print("gumbel: max |g - float64| = %.3g at h23 = %d" % (err.max(), err.argmax()))
    assert err.max() <= 2e-4
    assert np.all(np.diff(g) >= 0)


# ---- 2: the hash ----------------------------------------------------------------------------------------------------------
def _chi2_uniform(u, bins=256):
    counts = np.bincount(np.minimum((u.astype(np.float64) * bins).astype(np.int64), bins - 1), minlength=bins)
    e = u.size / bins
    return float(((counts - e) ** 2 / e).sum())


def test_hash_is_uniform_over_steps_ids_and_keys():
    h = harness()
    ids = np.arange(32000, dtype=np.uint32)
    key = int(keys_of(2026, 1)[0])
    us = []
    for t in range(48):
        u = np.empty(ids.size, np.float32)
        h.hash_u(key, t, _ptr(ids), ids.size, _ptr(u))
        us.append(u)
    stat = _chi2_uniform(np.concatenate(us))
    print("hash: chi-square over (t, id) = %.1f (255 degrees of freedom)" % stat)
    assert stat < chi2_quantile_9999(255)
    # over the 48 keys of one seed at a fixed (t, id): 8 bins, an expectation of 6
    one = np.array([777], np.uint32)
    uk = np.empty(48, np.float32)
    for i, k in enumerate(keys_of(11, 48)):
        h.hash_u(int(k), 3, _ptr(one), 1, _ptr(uk[i:i + 1]))
    stat = _chi2_uniform(uk, bins=8)
    print("hash: chi-square over 48 keys = %.1f (7 degrees of freedom)" % stat)
    assert stat < chi2_quantile_9999(7)
    assert np.unique(uk).size >= 47


# ---- 3: the draw ----------------------------------------------------------------------------------------------------------
def test_the_draw_follows_softmax_of_logits_over_temperature():
    h = harness()
    rng = np.random.default_rng(12)
    l = rng.normal(0.0, 1.5, 64).astype(np.float32)
    ids = (np.arange(64, dtype=np.uint32) * 37 + 5).astype(np.uint32)
    p1 = np.exp(l.astype(np.float64) - l.max())
    p1 /= p1.sum()
    assert 0.1 <= p1.max() <= 0.5, p1.max()
    n = 200000
    keys = keys_of(5, n)
    assert np.unique(keys).size == n
    for T in (0.7, 1.0, 1.5):
        inv_T = np.float32(1.0) / np.float32(T)
        out = np.empty(n, np.uint32)
        h.draw_many(_ptr(keys), n, _ptr(l), _ptr(ids), 64, ctypes.c_float(inv_T), _ptr(out))
        z = l.astype(np.float64) * float(inv_T)
        p = np.exp(z - z.max())
        p /= p.sum()
        counts = np.bincount(out, minlength=64).astype(np.float64)
        e = p * n
        small = e < 5.0  # pooled into one category
        obs = np.append(counts[~small], counts[small].sum()) if small.any() else counts
        exp = np.append(e[~small], e[small].sum()) if small.any() else e
        stat = float(((obs - exp) ** 2 / exp).sum())
        print("draw: T = %.1f chi-square %.1f over %d categories" % (T, stat, exp.size))
        assert stat < chi2_quantile_9999(exp.size - 1), T


# ---- 4: the checker -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(oracle, synth_models):
    m = synth_models("tiny11", 6.0)
    return m, oracle.OracleModel(m)


def test_checker_at_a_low_temperature_is_the_oracles_greedy_translate(oracle, tiny):
    from slimt_amd import synth
    m, om = tiny
    B, S = 5, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=4, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    oracle.set_mode(oracle.PORTABLE)
    try:
        w_out, w_ln, w_al, _ = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    trace = []
    T = 1e-3
    out, ln, al, sc = sampled_translate(oracle, om, m, ids, lens, sl, keys_of(1, B), T, trace=trace)
    # no ties at the maximum, and none the noise could bridge: g lies in [-2.82, 16.64], so at 1 / T = 1000 a gap of
    # 0.02 between the two largest logits keeps the greedy token the first maximum of the keys
    assert min(trace) > 0.02, min(trace)
    assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out)
    assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32))
    for b in range(B):
        assert np.all(sc[b, : ln[b]] <= 0.0)


def test_checker_echoes_a_prefix_that_covers_everything_and_depends_on_the_keys(oracle, tiny):
    from slimt_amd import synth
    m, om = tiny
    B, S = 4, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=11, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    Tm = tmax_of(S)
    p_ids = np.tile(sl[5:5 + Tm], (B, 1)).astype(np.uint32)
    p_len = np.full(B, Tm, np.uint32)
    out, ln, _, sc = sampled_translate(oracle, om, m, ids, lens, sl, keys_of(2, B), 0.7, p_ids, p_len)
    assert np.array_equal(out, p_ids) and np.all(ln == Tm) and np.all(np.isfinite(sc))
    a = sampled_translate(oracle, om, m, ids, lens, sl, keys_of(2, B), 1.0)
    b = sampled_translate(oracle, om, m, ids, lens, sl, keys_of(2, B), 1.0)
    c = sampled_translate(oracle, om, m, ids, lens, sl, keys_of(3, B), 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])
    # a sentence's draw does not depend on its row: the batch reversed, under reversed keys
    r = sampled_translate(oracle, om, m, ids[::-1], lens[::-1], sl, keys_of(2, B)[::-1], 1.0)
    assert np.array_equal(r[0][::-1], a[0]) and np.array_equal(r[1][::-1], a[1])


# ---- 5: the interface -----------------------------------------------------------------------------------------------------
def test_sampling_symbols_are_exported_declared_and_wrapped():
    from slimt_amd import build, capi
    dll = ctypes.CDLL(build.build())
    for name in ("slimt_hip_ctx_set_sampling", "slimt_hip_sampling_key"):
        assert hasattr(dll, name)
        assert name in capi.SYMBOLS
    with open(os.path.join(ROOT, "include", "slimt_hip.h")) as f:
        text = f.read()
    assert "int slimt_hip_ctx_set_sampling(slimt_hip_ctx *ctx, float temperature, const uint64_t *const *keys, size_t n);" in text
    assert "uint64_t slimt_hip_sampling_key(uint64_t seed, uint64_t index);" in text
    assert "#define SLIMT_HIP_ABI_VERSION 3" in text or capi.lib().slimt_hip_abi_version() == 3
    for name in ("translate", "translate_pinned", "translate_async", "translate_generated", "translate_device",
                 "translate_device_generated", "translate_many_device", "translate_many_async"):
        assert inspect.signature(getattr(capi.Context, name)).parameters["sampling"].default is None
    assert "keys" in inspect.signature(capi.Context.set_sampling).parameters


def test_set_sampling_fails_loudly_without_a_context_and_refuses_bad_temperatures():
    from slimt_amd import capi
    L = capi.lib()
    assert L.slimt_hip_ctx_set_sampling(None, 1.0, None, 1) != 0
    assert b"null argument" in L.slimt_hip_last_error()
    # the temperature is checked first, so the refusal shows without a GPU (no context can be made here)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        assert L.slimt_hip_ctx_set_sampling(None, bad, None, 1) != 0
        assert b"temperature" in L.slimt_hip_last_error(), bad


def test_sampling_key_is_the_headers_and_distinct_over_indices():
    from slimt_amd import capi
    h = harness()
    idx = np.arange(1 << 16, dtype=np.uint64)
    keys = np.array([capi.sampling_key(9, int(i)) for i in idx[:4096]], dtype=np.uint64)
    assert np.array_equal(keys, keys_of(9, 4096))
    all_keys = keys_of(9, 1 << 16)
    assert np.unique(all_keys).size == 1 << 16
    assert np.unique(keys_of(10, 1 << 16)).size == 1 << 16
    assert np.intersect1d(all_keys, keys_of(10, 1 << 16)).size == 0
    assert h.sentence_key(0, 0) != 0


def test_wrappers_check_key_shapes():
    from slimt_amd import capi
    with pytest.raises(ValueError):
        capi.Context._sampling_host((1.0, np.zeros(3, np.uint64)), 2)
    t, k = capi.Context._sampling_host((0.7, [1, 2]), 2)
    assert k.dtype == np.uint64 and abs(t - 0.7) < 1e-12
    assert capi.Context._sampling_host((1.0, None), 2)[1] is None


def test_service_sampling_is_exported_declared_and_refuses_null_arguments():
    """include/slimt_hip_service_sampling.h against libslimt_hip_host.so: without a GPU no service can be created, so the
    entry points are checked on their argument errors (they fail loudly; there is no CPU fallback)"""
    from slimt_amd import build, capi, frontend
    build.build_host_lib()
    H = capi.host_lib()
    with open(os.path.join(ROOT, "include", "slimt_hip_service_sampling.h")) as f:
        text = f.read()
    assert "int slimt_hip_service_set_sampling(slimt_hip_service *service, float temperature);" in text
    assert "int slimt_hip_service_translate_sampled(slimt_hip_service *service," in text
    for n in ("slimt_hip_service_set_sampling", "slimt_hip_service_translate_sampled"):
        assert hasattr(H, n)
    assert H.slimt_hip_service_set_sampling(None, 1.0) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_translate_sampled(None, None, None, None, None, 0, 0, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert inspect.signature(capi.BatchService).parameters["temperature"].default == 0.0
    assert inspect.signature(capi.BatchService.translate).parameters["seed"].default is None
    for fn in (frontend.Service.translate, frontend.Service.pivot):
        assert inspect.signature(fn).parameters["sampling"].default is None
