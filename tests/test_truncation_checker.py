"""Truncated sampling (include/slimt_hip.h, slimt_hip_ctx_set_sampling_truncation): the weights, the checker and the
CPU-side checks.

slimt_amd/csrc/truncation.h is compiled here for the host (g++ -O2 -ffp-contract=off), so the integer weights the
selection kernel sums are available bit for bit. The checker finds the kept set by SORTING (`keep_mask`: a descending
sort and cumulative integer weights) -- an algorithm that shares nothing with the kernel's radix select but the weights --
and `truncated_translate` is sampled_translate of test_sampling_checker.py with that set applied before the first
maximum, the float64 log-softmax taken over the kept set, and forced steps left whole."""
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
from test_sampling_checker import chi2_quantile_9999, first_max, keys_of, row_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include "truncation.h"
using namespace slimt_hip;
extern "C" {
// the weights of one row against its maximum M
void weights_row(const float *z, uint32_t n, float M, uint32_t *out) { for (uint32_t i = 0; i < n; ++i) out[i] = tr_weight(z[i], M); }
// tr_weight(d, 0) of the floats whose bits are b0, b0 - stride, ... (negative floats: d grows towards 0)
void weight_sweep(uint32_t b0, uint32_t stride, uint32_t n, float *d, uint32_t *w) {
  for (uint32_t i = 0; i < n; ++i) {
    d[i] = sm_float(b0 - i * stride);
    w[i] = tr_weight(d[i], 0.0f);
  }
}
uint32_t weight_of(float z, float M) { return tr_weight(z, M); }
void ord_all(const float *x, uint32_t n, uint32_t *out) { for (uint32_t i = 0; i < n; ++i) out[i] = tr_ord(x[i]); }
void unord_all(const uint32_t *o, uint32_t n, float *out) { for (uint32_t i = 0; i < n; ++i) out[i] = tr_unord(o[i]); }
// one draw per key at step 0 over the columns with keep[i] != 0: the first maximum from the arg-max's start value
void draw_kept(const uint64_t *keys, uint32_t n_keys, const float *l, const uint32_t *ids, const uint8_t *keep, uint32_t n,
               float inv_T, uint32_t *out) {
  for (uint32_t k = 0; k < n_keys; ++k) {
    const uint64_t w = sm_step_words(keys[k], 0);
    float best = -3.402823466e+38f;
    uint32_t bi = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (!keep[i]) continue;
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
    """truncation.h compiled for the host, once per process"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="slimt_truncation_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = os.path.join(d, "h.cc")
        with open(src, "w") as f:
            f.write(_HARNESS)
        so = os.path.join(d, "h.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "slimt_amd", "csrc"), src, "-o", so])
        h = ctypes.CDLL(so)
        vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
        h.weights_row.argtypes = [vp, u32, f32, vp]
        h.weight_sweep.argtypes = [u32, u32, u32, vp, vp]
        h.weight_of.argtypes = [f32, f32]
        h.weight_of.restype = u32
        h.ord_all.argtypes = [vp, u32, vp]
        h.unord_all.argtypes = [vp, u32, vp]
        h.draw_kept.argtypes = [vp, u32, vp, vp, vp, u32, f32, vp]
        _lib = h
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def weights(z, M):
    """uint32 tr_weight(z_i, M) of a float32 array of valid (non-NaN) z"""
    z = np.ascontiguousarray(z, dtype=np.float32)
    out = np.empty(z.size, np.uint32)
    harness().weights_row(_ptr(z), z.size, ctypes.c_float(float(M)), _ptr(out))
    return out


class KeptSets:
    """The kept sets of one row of float32 z = logit * inv_T under the header's rule, by SORTING: one descending sort of
    the valid z, their integer weights against the maximum and the cumulative integer sums; every (top_k, top_p) is
    then a prefix of that order (ties are taken together: a prefix always ends at the end of a group of equal values)."""

    def __init__(self, z):
        self.z = np.asarray(z, dtype=np.float32)
        self.valid = ~np.isnan(self.z)
        self.zs = np.sort(self.z[self.valid])[::-1]  # descending
        n = self.zs.size
        if n:
            self.cum = np.cumsum(weights(self.zs, self.zs[0]).astype(np.uint64), dtype=np.uint64)  # integer sums: exact
            self.ends = np.flatnonzero(np.append(self.zs[1:] != self.zs[:-1], True))  # each group's last index (+-0: one group)
            self.group_end = self.ends[np.searchsorted(self.ends, np.arange(n))]

    def mask(self, top_k, top_p):
        """(kept bool [N], threshold float32): the threshold is max(tau_k, tau_p), -inf where nothing is cut"""
        top_p = np.float32(top_p)
        n1 = self.zs.size
        tau = np.float32(-np.inf)
        if n1 == 0:
            return self.valid.copy(), tau
        if top_k != 0 and top_k < n1:
            tau = self.zs[top_k - 1]  # the top_k-th largest valid z
            n1 = int(self.group_end[top_k - 1]) + 1  # K1: everything >= it
        if top_p != np.float32(1.0):
            ends = self.ends[: np.searchsorted(self.ends, n1)]  # the groups of K1 (n1 - 1 is the last one's end)
            cum = self.cum[ends]
            target = np.float64(top_p) * np.float64(cum[-1])  # one IEEE double product; cum[-1] = Q
            reach = np.flatnonzero(cum.astype(np.float64) >= target)
            assert reach.size
            tau = max(tau, self.zs[ends[reach[0]]])  # the largest value whose sum from the top reaches the target
        with np.errstate(invalid="ignore"):
            return self.valid & (self.z >= tau), np.float32(tau)


def keep_mask(z, top_k, top_p):
    """(kept bool [N], threshold float32) of one row of float32 z (KeptSets)"""
    return KeptSets(z).mask(top_k, top_p)


def truncated_row(key, t, logits, ids, inv_T, top_k, top_p, forced=False, sets=None, rkeys=None):
    """one step of one sentence: (column, none, kept, threshold, float64 score of the drawn column). sets / rkeys: the
    row's KeptSets and compared values (row_keys), where the caller has them already"""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    z32 = (logits * np.float32(inv_T)).astype(np.float32)
    if forced:
        kept, tau = ~np.isnan(z32), np.float32(-np.inf)
    else:
        kept, tau = (sets if sets is not None else KeptSets(z32)).mask(top_k, top_p)
    if rkeys is None:
        rkeys = row_keys(key, t, logits, ids, inv_T)
    col, none = first_max(np.where(kept, rkeys, np.float32(-np.inf)), logits[0])
    return col, none, kept, tau, kept_scores(z32, kept, none)[col]


def kept_scores(z32, kept, none):
    """float64 log softmax of z over the kept set at every column (NaN for a row that holds a NaN, or with `none`)"""
    z = z32.astype(np.float64)
    if none or np.isnan(z).any() or not kept.any():
        return np.full(z.size, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = z[kept].max()
        return z - (mx + np.log(np.exp(z[kept] - mx).sum()))


def truncated_translate(oracle, om, m, ids, lens, sl, keys, T, top_k, top_p, p_ids=None, p_len=None, limit_factor=1.5, eos=0,
                        sizes=None):
    """sampled_translate (test_sampling_checker.py) with the kept set applied to every drawn step; forced steps whole.
    sizes (a list): gets (row, step, |K|) of every drawn step."""
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
            tok = np.zeros(B, np.uint32)
            for b in range(B):
                if done[b]:
                    continue  # (tok 0 is fed; a finished row's state is never read again)
                forced = p_len is not None and t < int(p_len[b])
                col, none, kept, _, _ = truncated_row(keys[b], ln[b], logits[b], sl, inv_T, top_k, top_p, forced)
                tok[b] = col if sl is None else sl[col]
                if not forced and sizes is not None:
                    sizes.append((b, t, int(kept.sum())))
                if forced:
                    tok[b] = p_ids[b, t]
                    if sl is None:
                        col = int(tok[b]) if tok[b] < logits.shape[1] else -1
                    else:
                        i = int(np.searchsorted(sl, tok[b]))
                        col = i if i < len(sl) and sl[i] == tok[b] else -1
                z32 = (logits[b] * inv_T).astype(np.float32)
                s = kept_scores(z32, kept, none)
                sc[b, t] = np.nan if none else (s[col] if col >= 0 else (np.nan if np.isnan(s[0]) else -np.inf))
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


# ---- 1: the weights -------------------------------------------------------------------------------------------------------
def test_weights_are_within_two_units_of_float64_and_never_decrease():
    h = harness()
    b_hi = int(np.array([-17.0], np.float32).view(np.uint32)[0])  # bits fall as a negative float grows towards 0
    stride, first = 97, b_hi - 1  # from just above -17, every 97th float, down to the smallest negative ones
    n = (first - 0x80000001) // stride + 1
    worst, last = 0, 0
    for at in range(0, n, 1 << 22):
        cnt = min(1 << 22, n - at)
        d, w = np.empty(cnt, np.float32), np.empty(cnt, np.uint32)
        h.weight_sweep(first - at * stride, stride, cnt, _ptr(d), _ptr(w))
        assert d[0] > -17.0 and d[-1] < 0.0 and np.all(np.diff(d) > 0)
        want = np.floor(np.exp(d.astype(np.float64)) * 16777216.0)
        worst = max(worst, int(np.abs(w.astype(np.int64) - want.astype(np.int64)).max()))
        assert w[0] >= last and np.all(np.diff(w.astype(np.int64)) >= 0)  # never decreases as d grows
        last = int(w[-1])
    print("tr_weight: max |w - floor(exp64(d) 2^24)| = %d over %d floats of (-17, 0)" % (worst, n))
    assert worst <= 2
    assert last <= 16777216
    # the edges
    just_above = np.array([b_hi - 1], np.uint32).view(np.float32)[0]
    assert h.weight_of(0.0, 0.0) == 16777216 and h.weight_of(-0.0, 0.0) == 16777216
    assert h.weight_of(-17.0, 0.0) == 0 and h.weight_of(-1e30, 0.0) == 0
    assert abs(int(h.weight_of(float(just_above), 0.0)) - int(np.floor(np.exp(np.float64(just_above)) * 16777216.0))) <= 2
    inf = float("inf")
    assert h.weight_of(inf, inf) == 16777216 and h.weight_of(-inf, -inf) == 16777216  # z == M first: no inf - inf
    assert h.weight_of(1.0, inf) == 0 and h.weight_of(-inf, 3.0) == 0 and h.weight_of(-inf, inf) == 0
    assert h.weight_of(2.5, 2.5) == 16777216 and h.weight_of(2.0, 19.0) == 0


def test_ord_preserves_the_order_of_floats_and_round_trips():
    h = harness()
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(0, 5, 4000), [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38]]).astype(np.float32)
    o, back = np.empty(x.size, np.uint32), np.empty(x.size, np.float32)
    h.ord_all(_ptr(x), x.size, _ptr(o))
    h.unord_all(_ptr(o), x.size, _ptr(back))
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
    by_ord = x[np.argsort(o, kind="stable")]
    assert np.all(np.diff(by_ord.astype(np.float64)) >= 0)
    lt = x[:, None] < x[None, :200]
    assert np.all((o[:, None] < o[None, :200])[lt])


# ---- 2: the kept set ------------------------------------------------------------------------------------------------------
def test_keep_mask_follows_the_rule_on_hand_made_rows():
    z = np.array([1.0, 3.0, 2.0, 3.0, -1.0, np.nan, 2.0], np.float32)
    k, tau = keep_mask(z, 1, 1.0)
    assert list(np.flatnonzero(k)) == [1, 3] and tau == 3.0  # ties at the threshold are all kept
    k, tau = keep_mask(z, 3, 1.0)
    assert list(np.flatnonzero(k)) == [1, 2, 3, 6] and tau == 2.0
    for big in (6, 7, 100, 0):  # top_k >= n_valid (6), or off: every valid column
        k, tau = keep_mask(z, big, 1.0)
        assert list(np.flatnonzero(k)) == [0, 1, 2, 3, 4, 6] and np.isneginf(tau)
    # the nucleus: p(3) = 2 e^0, p(2) = 2 e^-1, p(1) = e^-2, p(-1) = e^-4 of Q
    w = weights(z[[0, 1, 2, 3, 4, 6]], 3.0).astype(np.float64)
    Q = w.sum()
    top2 = 2 * 16777216.0 / Q
    k, tau = keep_mask(z, 0, top2 - 1e-3)
    assert list(np.flatnonzero(k)) == [1, 3] and tau == 3.0
    k, tau = keep_mask(z, 0, top2 + 1e-3)
    assert list(np.flatnonzero(k)) == [1, 2, 3, 6] and tau == 2.0
    k, tau = keep_mask(z, 0, 1e-6)
    assert list(np.flatnonzero(k)) == [1, 3]  # K always holds the maximal columns
    k, tau = keep_mask(z, 2, 0.999999)  # both: the nucleus is taken inside the top-k set
    assert list(np.flatnonzero(k)) == [1, 3] and tau == 3.0
    # all NaN: nothing kept; all -inf: everything kept (z == M)
    assert not keep_mask(np.full(5, np.nan, np.float32), 2, 0.5)[0].any()
    assert keep_mask(np.full(5, -np.inf, np.float32), 0, 0.5)[0].all()
    # +-0 are one value
    k, tau = keep_mask(np.array([0.0, -0.0, -1.0], np.float32), 1, 1.0)
    assert list(np.flatnonzero(k)) == [0, 1] and tau == 0.0
    # the set depends on values alone: a permuted row keeps the permuted set
    rng = np.random.default_rng(8)
    z = rng.normal(0, 3, 257).astype(np.float32)
    perm = rng.permutation(z.size)
    for tk, tp in ((5, 1.0), (0, 0.8), (40, 0.9)):
        a, ta = keep_mask(z, tk, tp)
        b, tb = keep_mask(z[perm], tk, tp)
        assert np.array_equal(a[perm], b) and ta == tb


# ---- 3: the draw ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,top_p", [(8, 1.0), (0, 0.7)])
def test_the_truncated_draw_follows_the_renormalised_kept_distribution(top_k, top_p):
    h = harness()
    rng = np.random.default_rng(12)
    l = rng.normal(0.0, 1.5, 64).astype(np.float32)
    ids = (np.arange(64, dtype=np.uint32) * 37 + 5).astype(np.uint32)
    n = 20000
    keys = keys_of(5, n)
    for T in (0.7, 1.0):
        inv_T = np.float32(1.0) / np.float32(T)
        z32 = (l * inv_T).astype(np.float32)
        kept, _ = keep_mask(z32, top_k, top_p)
        assert 2 <= kept.sum() < 64
        if top_k:
            assert kept.sum() == top_k
        keep8 = np.ascontiguousarray(kept.astype(np.uint8))
        out = np.empty(n, np.uint32)
        h.draw_kept(_ptr(keys), n, _ptr(l), _ptr(ids), _ptr(keep8), 64, ctypes.c_float(inv_T), _ptr(out))
        counts = np.bincount(out, minlength=64).astype(np.float64)
        assert counts[~kept].sum() == 0  # no draw falls outside the set
        z = z32.astype(np.float64)
        p = np.where(kept, np.exp(z - z[kept].max()), 0.0)
        p /= p.sum()
        if not top_k:
            full = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
            assert full[kept].sum() >= top_p - 1e-6  # the nucleus holds the mass asked for
            assert full[kept].sum() - full[kept].min() < top_p + 1e-6  # ... and no more columns than that needs
        e = p[kept] * n
        obs = counts[kept]
        small = e < 5.0  # pooled into one category
        if small.any():
            obs, e = np.append(obs[~small], obs[small].sum()), np.append(e[~small], e[small].sum())
        stat = float(((obs - e) ** 2 / e).sum())
        print("draw: k = %d p = %.2f T = %.1f chi-square %.1f over %d categories" % (top_k, top_p, T, stat, e.size))
        assert stat < chi2_quantile_9999(e.size - 1), T


# ---- 4: the checker -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(oracle, synth_models):
    m = synth_models("tiny11", 6.0)
    return m, oracle.OracleModel(m)


def test_checker_with_truncation_off_is_the_sampled_checker_and_top_1_is_greedy(oracle, tiny):
    from slimt_amd import synth
    from test_sampling_checker import sampled_translate
    m, om = tiny
    B, S = 5, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=4, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(1, B)
    a = sampled_translate(oracle, om, m, ids, lens, sl, keys, 0.7)
    b = truncated_translate(oracle, om, m, ids, lens, sl, keys, 0.7, 0, 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    for r in range(B):
        assert np.allclose(a[3][r, :a[1][r]], b[3][r, :b[1][r]], rtol=0, atol=1e-9)
    oracle.set_mode(oracle.PORTABLE)
    try:
        w_out, w_ln, _, _ = om.translate(ids, lens, sl, 1.5, 0)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    sizes = []
    g = truncated_translate(oracle, om, m, ids, lens, sl, keys, 0.7, 1, 1.0, sizes=sizes)
    assert all(n == 1 for _, _, n in sizes)  # (no tied maxima in this model's rows)
    assert np.array_equal(g[0], w_out) and np.array_equal(g[1], w_ln)
    for r in range(B):
        assert np.all(g[3][r, :g[1][r]] == 0.0)
    # a truncated call differs from the untruncated one somewhere, and is reproducible
    c = truncated_translate(oracle, om, m, ids, lens, sl, keys, 1.0, 3, 0.9)
    d = truncated_translate(oracle, om, m, ids, lens, sl, keys, 1.0, 3, 0.9)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])


# ---- 5: the interface -----------------------------------------------------------------------------------------------------
def test_truncation_symbols_are_exported_declared_and_wrapped():
    from slimt_amd import build, capi, frontend
    dll = ctypes.CDLL(build.build())
    for name in ("slimt_hip_ctx_set_sampling_truncation", "slimt_hip_sample_truncated"):
        assert hasattr(dll, name)
        assert name in capi.SYMBOLS
    with open(os.path.join(ROOT, "include", "slimt_hip.h")) as f:
        text = f.read()
    assert "int slimt_hip_ctx_set_sampling_truncation(slimt_hip_ctx *ctx, uint32_t top_k, float top_p);" in text
    assert "int slimt_hip_sample_truncated(const float *logits, size_t M, size_t N, const uint32_t *ids," in text
    assert capi.lib().slimt_hip_abi_version() == 3
    for name in ("translate", "translate_pinned", "translate_async", "translate_generated", "translate_device",
                 "translate_device_generated", "translate_many_device", "translate_many_async"):
        assert inspect.signature(getattr(capi.Context, name)).parameters["truncation"].default is None
    assert inspect.signature(capi.BatchService).parameters["truncation"].default is None
    for fn in (frontend.Service.translate, frontend.Service.pivot):
        assert inspect.signature(fn).parameters["truncation"].default is None
    assert callable(capi.sample_truncated)


def test_set_truncation_refuses_bad_top_p_at_once_and_fails_loudly_without_a_context():
    from slimt_amd import capi
    L = capi.lib()
    # top_p is checked first, so the refusal shows without a GPU (no context can be made here)
    for bad in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        assert L.slimt_hip_ctx_set_sampling_truncation(None, 4, bad) < 0
        assert b"top_p" in L.slimt_hip_last_error(), bad
    assert L.slimt_hip_ctx_set_sampling_truncation(None, 4, 0.5) < 0
    assert b"null argument" in L.slimt_hip_last_error()
    z = np.zeros((1, 4), np.float32)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(capi.SlimtHipError, match="top_p"):
            capi.sample_truncated(z, 1.0, 2, bad)
    with pytest.raises(capi.SlimtHipError, match="temperature"):
        capi.sample_truncated(z, 0.0, 2, 0.5)


def test_service_truncation_is_exported_declared_apart_and_refuses_null_arguments():
    from slimt_amd import build, capi
    build.build_host_lib()
    H = capi.host_lib()
    with open(os.path.join(ROOT, "include", "slimt_hip_service_sampling.h")) as f:
        text = f.read()
    assert "int slimt_hip_service_set_sampling_truncation(slimt_hip_service *service, uint32_t top_k, float top_p);" in text
    with open(os.path.join(ROOT, "include", "slimt_hip_service.h")) as f:
        assert "truncation" not in f.read()
    assert hasattr(H, "slimt_hip_service_set_sampling_truncation")
    assert H.slimt_hip_service_set_sampling_truncation(None, 4, 0.5) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
