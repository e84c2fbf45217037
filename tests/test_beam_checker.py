"""Beam search (include/slimt_hip.h, slimt_hip_translate_beam*): the arithmetic, the checkers and the API's surface, on the CPU.

slimt_amd/csrc/beam.h is compiled here for the host (g++ -O2 -ffp-contract=off) and compared bit for bit with its NumPy
restatement (tests/support/beam_cases.py), which the step checker `beam_step_host` and the search `beam_translate` are
built on; the accuracy the contract states is measured against float64 and printed before it is asserted."""
import atexit
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from support import beam_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include "beam.h"
using namespace slimt_hip;
extern "C" {
void exp_all(const float *d, uint32_t n, float *out) { for (uint32_t i = 0; i < n; ++i) out[i] = tr_exp(d[i]); }
void log_all(const float *x, uint32_t n, float *out) { for (uint32_t i = 0; i < n; ++i) out[i] = sm_log(x[i]); }
// one row: returns usable; M, Q, L and the columns' weights and scores
int row(const float *l, uint32_t n, float *M, uint64_t *Q, float *L, uint64_t *w, float *lp) {
  bool nan = false;
  float m = -INFINITY;
  for (uint32_t i = 0; i < n; ++i) {
    nan = nan || l[i] != l[i];
    m = fmaxf(m, l[i]);
  }
  *M = bm_max(m);
  if (!bm_usable(nan, *M)) return 0;
  uint64_t q = 0;
  for (uint32_t i = 0; i < n; ++i) {
    w[i] = bm_weight(l[i], *M);
    q += w[i];
  }
  *Q = q;
  *L = bm_normaliser(q);
  for (uint32_t i = 0; i < n; ++i) lp[i] = bm_logprob(l[i], *M, *L);
  return 1;
}
int constants(int which) { return which == 0 ? kBeamMax : which == 1 ? (int)kBeamMaxN : (int)kBeamLive * 10 + (int)kBeamFinished; }
}
"""

_lib = None


def harness():
    """beam.h compiled for the host, once per process"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="slimt_beam_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = os.path.join(d, "h.cc")
        with open(src, "w") as f:
            f.write(_HARNESS)
        so = os.path.join(d, "h.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "slimt_amd", "csrc"), src, "-o", so])
        h = ctypes.CDLL(so)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        h.exp_all.argtypes = [vp, u32, vp]
        h.log_all.argtypes = [vp, u32, vp]
        h.row.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        _lib = h
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def header_row(l):
    l = np.ascontiguousarray(l, dtype=np.float32)
    M, L, Q = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.uint64)
    w, lp = np.zeros(l.size, np.uint64), np.zeros(l.size, np.float32)
    usable = harness().row(_ptr(l), l.size, _ptr(M), _ptr(Q), _ptr(L), _ptr(w), _ptr(lp))
    return bool(usable), M[0], int(Q[0]), L[0], w, lp


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def adversarial_rows():
    m28 = np.float32(-28.0)
    around = [np.nextafter(m28, np.float32(0)), m28, np.nextafter(m28, np.float32(-100)), np.float32(-27.5), np.float32(-40)]
    rows = [np.asarray([0.0] + around, np.float32), np.asarray([3.25] + [3.25 + a for a in around], np.float32),
            np.asarray([0.0, -0.0, -1.0], np.float32), np.asarray([-0.0, -0.0], np.float32), np.asarray([-0.0], np.float32),
            np.asarray([1.5, -np.inf, 1.5, -np.inf], np.float32), np.asarray([7.0], np.float32), np.asarray([-3e38, -3e38], np.float32),
            np.asarray([np.nan, 1.0], np.float32), np.asarray([-np.inf, -np.inf], np.float32), np.asarray([np.inf, 1.0], np.float32),
            np.asarray([-1e-30, 0.0, -1e-8], np.float32), np.full(1000, 2.0, np.float32)]
    return rows


def random_rows():
    r = np.random.default_rng(11)
    for n in (1, 2, 17, 256, 4097, 32000):
        for scale in (0.5, 4.0, 20.0):
            yield (r.normal(0, scale, size=n)).astype(np.float32)


# ---- 1: the header against the NumPy rule ----------------------------------------------------------------------------------
def test_the_numpy_exponential_and_logarithm_have_the_headers_bits():
    h = harness()
    r = np.random.default_rng(3)
    d = np.concatenate([-r.uniform(0, 28, size=200000), -np.exp(r.uniform(-40, 3, size=50000))]).astype(np.float32)
    d = d[d > -28]
    got = np.empty_like(d)
    h.exp_all(_ptr(d), d.size, _ptr(got))
    assert _same_bits(got, BC.tr_exp(d))
    x = np.concatenate([r.uniform(1, 2 ** 20, size=200000), 1 + np.exp(r.uniform(-20, 0, size=50000))]).astype(np.float32)
    got = np.empty_like(x)
    h.log_all(_ptr(x), x.size, _ptr(got))
    assert _same_bits(got, BC.sm_log(x))


@pytest.mark.parametrize("rows", [adversarial_rows, random_rows])
def test_weights_sums_normalisers_and_scores_are_bit_equal(rows):
    n_usable = 0
    for l in rows():
        usable, M, Q, L, w, lp = header_row(l)
        u2, M2, Q2, L2, lp2 = BC.row_scores(l)
        assert usable == u2, l[:8]
        if not usable:
            continue
        n_usable += 1
        assert _same_bits(M, M2) and not (M == 0 and np.signbit(M))  # (-0 is read as +0)
        assert np.array_equal(w, BC.weights(l, M2)) and Q == Q2 and Q == int(w.sum(dtype=np.uint64))
        assert 2 ** 40 <= Q < 2 ** 60
        assert _same_bits(L, L2) and _same_bits(lp, lp2)
        assert np.all(w[l == M] == 2 ** 40) and np.all(w[(l - M) <= np.float32(-28)] == 0)
        assert np.all(lp[np.isneginf(l)] == -np.inf) and L >= 0
    assert n_usable >= 8


def test_the_unusable_rows_are_the_contracts():
    for l, usable in (([np.nan, 1.0], False), ([-np.inf, -np.inf], False), ([np.inf, 1.0], False), ([1.0, -np.inf], True),
                      ([-3.4e38], True)):
        assert header_row(np.asarray(l, np.float32))[0] == usable == BC.row_scores(np.asarray(l, np.float32))[0]
    assert harness().constants(0) == BC.MAX_BEAM == 8 and harness().constants(1) == 1 << 20
    assert harness().constants(2) == BC.LIVE * 10 + BC.FINISHED


# ---- 2: the accuracy the contract states ----------------------------------------------------------------------------------------
def test_the_exponential_is_normal_monotone_and_accurate_on_its_range():
    # every 64th float of (-28, 0) and the ends
    top = np.float32(-28.0).view(np.uint32)
    d = np.arange(np.uint32(0x80000000) + np.uint32(1), top, 64, dtype=np.uint32).view(np.float32)
    d = np.concatenate([d, np.asarray([np.nextafter(np.float32(-28), np.float32(0)), -0.0, 0.0], np.float32)])
    d = np.sort(d)
    e = np.empty_like(d)
    harness().exp_all(_ptr(d), d.size, _ptr(e))
    assert np.all(e >= np.finfo(np.float32).tiny) and np.all(np.diff(e) >= 0) and e[-1] == 1.0
    rel = np.abs(e.astype(np.float64) / np.exp(d.astype(np.float64)) - 1.0)
    print("tr_exp on (-28, 0]: worst relative error %.3g at d = %r" % (rel.max(), d[rel.argmax()]))
    assert rel.max() <= 2e-7


def test_the_scores_are_within_the_projects_tolerance_of_float64():
    worst = 0.0
    r = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 100, 1000, 4096, 32000):
        for scale in (0.3, 2.0, 8.0, 25.0):
            l = r.normal(0, scale, size=n).astype(np.float32)
            _, _, _, _, lp = BC.row_scores(l)
            z = l.astype(np.float64)
            want = z - z.max() - np.log(np.exp(z - z.max()).sum())
            sel = want > -64
            worst = max(worst, float(np.abs(lp[sel].astype(np.float64) - want[sel]).max()))
    print("lp against the float64 log-softmax above -64: worst %.3g" % worst)
    assert worst <= 5e-5


# ---- 3: the step checker ---------------------------------------------------------------------------------------------------
def test_beam_one_is_the_first_maximum():
    r = np.random.default_rng(9)
    logits = np.round(r.normal(0, 2, size=(5, 40)) * 2).astype(np.float32) / 2  # (ties)
    totals, flags = BC.start_state(5, 1)
    parent, token, score, tot, fl = BC.beam_step_host(logits, totals, flags, 1, eos_id=7)
    assert np.array_equal(token, logits.argmax(axis=1)) and np.all(parent == 0)
    assert _same_bits(tot, np.float32(0) + score)
    assert np.array_equal(fl, np.where(token == 7, BC.FINISHED, BC.LIVE))


def test_the_step_checker_orders_ties_carries_and_drops_as_the_contract_says():
    k = 3
    logits = np.full((3, 4), -30.0, np.float32)
    logits[0, [1, 2]] = 2.0      # slot 0: two equal best columns
    logits[1] = logits[0]        # slot 1: the same row, the same total
    totals = np.asarray([-1.0, -1.0, -0.25], np.float32)
    flags = np.asarray([BC.LIVE, BC.LIVE, BC.FINISHED], np.uint32)
    parent, token, score, tot, fl = BC.beam_step_host(logits, totals, flags, k, eos_id=2)
    assert parent.tolist() == [2, 0, 0] and token.tolist() == [BC.NONE, 1, 2]  # the carried slot first, then slot 0's columns in order
    assert fl.tolist() == [BC.FINISHED, BC.LIVE, BC.FINISHED] and tot[0] == np.float32(-0.25) and score[0] == 0
    # fewer candidates than slots: the rest are dead
    flags = np.asarray([BC.LIVE, BC.DEAD, BC.DEAD], np.uint32)
    logits[0] = [0.0, -np.inf, -np.inf, -np.inf]
    parent, token, score, tot, fl = BC.beam_step_host(logits, np.asarray([0, -np.inf, -np.inf], np.float32), flags, k)
    assert fl.tolist() == [BC.FINISHED, BC.DEAD, BC.DEAD] and parent.tolist() == [0, BC.NONE, BC.NONE]
    assert token.tolist() == [0, BC.NONE, BC.NONE] and np.isneginf(tot[1:]).all() and tot[0] == 0


# ---- 4: the search ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(oracle, synth_models):
    from slimt_amd import synth
    m = synth_models("tiny11", 3.0, 1234)
    ids, lens = synth.make_batch(m.V, 2, 6, seed=5, ragged=True)
    return m, oracle.OracleModel(m), ids, lens, synth.make_shortlist(m.V, 512)


def test_beam_one_is_the_oracles_greedy_translate(oracle, tiny):
    m, om, ids, lens, sl = tiny
    out, ln, tot, sc, al = BC.beam_translate(oracle, om, m, ids, lens, sl, 1)
    oracle.set_mode(oracle.PORTABLE)
    try:
        w_out, w_ln, w_al, _ = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    assert np.array_equal(ln[:, 0], w_ln) and np.array_equal(out[:, 0], w_out)
    assert np.array_equal(al[:, 0].view(np.uint32), w_al.view(np.uint32))


@pytest.mark.parametrize("mode", [0, 1])
def test_totals_are_the_ascending_sums_and_the_hypotheses_are_sorted(oracle, tiny, mode):
    m, om, ids, lens, sl = tiny
    k = 4
    out, ln, tot, sc, al = BC.beam_translate(oracle, om, m, ids, lens, sl, k, mode)
    for b in range(ids.shape[0]):
        keys = []
        for j in range(k):
            if ln[b, j] == 0:
                assert np.isneginf(tot[b, j]) and all(ln[b, j:] == 0)
                continue
            s = np.float32(0)
            for t in range(int(ln[b, j])):
                s = np.float32(s + sc[b, j, t])
            assert _same_bits(s, tot[b, j])
            keys.append(tot[b, j] / np.float32(ln[b, j]) if mode else tot[b, j])
        assert all(keys[i] >= keys[i + 1] for i in range(len(keys) - 1)), keys
        assert len({tuple(out[b, j, :ln[b, j]]) for j in range(k) if ln[b, j]}) == sum(ln[b] > 0)  # no hypothesis twice


# ---- 5: the API's surface (no device needed) ------------------------------------------------------------------------------
BEAM = ["slimt_hip_translate_beam", "slimt_hip_translate_beam_async", "slimt_hip_translate_beam_device",
        "slimt_hip_translate_beam_async_generated", "slimt_hip_beam_step"]


def test_beam_symbols_are_declared_exported_and_wrapped():
    from slimt_amd import capi, frontend
    header = open(os.path.join(ROOT, "include", "slimt_hip.h")).read()
    L = capi.lib()
    for name in BEAM:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(L, name).argtypes is not None, name
    assert "#define SLIMT_HIP_MAX_BEAM 8" in header and capi.MAX_BEAM == 8 and L.slimt_hip_abi_version() == 3
    for name in ("translate_beam", "translate_beam_async", "translate_beam_pinned", "translate_beam_device",
                 "translate_beam_generated"):
        assert "mean" in inspect.signature(getattr(capi.Context, name)).parameters, name
    assert inspect.signature(capi.beam_step).parameters["beam"]
    assert inspect.signature(frontend.Service.beam_search).parameters["beam"]
    # the C++ batching service stays on the fixed engine double: it names none of the new symbols
    for f in ("Service.cc", "service_capi.cc", "Model.cc"):
        assert "beam" not in open(os.path.join(ROOT, "slimt_amd", "host", f)).read(), f


def test_host_entry_points_fail_loudly_on_bad_arguments():
    from slimt_amd import capi
    L = capi.lib()
    ids, lens = np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32)
    out, ol, tot = np.zeros((2, 3, 6), np.uint32), np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.float32)

    def call(fn, beam, mode, generated=False):
        mid = () if generated else (None, 0)
        head = (None, None) if generated else (None,)
        return fn(*head, _ptr(ids), _ptr(lens), 2, 4, beam, mode, *mid, 1.5, 0, _ptr(out), _ptr(ol), _ptr(tot), None, None)

    for fn, generated in ((L.slimt_hip_translate_beam, False), (L.slimt_hip_translate_beam_async, False)):
        assert call(fn, 3, 0, generated) != 0 and b"null argument" in L.slimt_hip_last_error()
        for beam in (0, 9):
            assert call(fn, beam, 0, generated) != 0 and b"not in 1..8" in L.slimt_hip_last_error()
        assert call(fn, 3, 2, generated) != 0 and b"length_mode 2" in L.slimt_hip_last_error()
    assert call(L.slimt_hip_translate_beam_async_generated, 3, 0, True) != 0 and b"null argument" in L.slimt_hip_last_error()
    assert L.slimt_hip_translate_beam_device(None, _ptr(ids), _ptr(lens), 2, 4, 9, 0, None, 0, 1.5, 0, _ptr(out), _ptr(ol), _ptr(tot),
                                             None, None, 0) != 0
    assert b"not in 1..8" in L.slimt_hip_last_error()
    assert L.slimt_hip_translate_beam_device(None, _ptr(ids), _ptr(lens), 2, 4, 3, 0, None, 0, 1.5, 0, _ptr(out), _ptr(ol), _ptr(tot),
                                             None, None, 0) != 0
    assert b"null argument" in L.slimt_hip_last_error()
    # the op-level call: its refusals come before the device is touched
    lg, t, f = np.zeros((3, 4), np.float32), np.zeros(3, np.float32), np.asarray([1, 0, 3], np.uint32)
    o = [np.zeros(3, np.uint32), np.zeros(3, np.uint32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.uint32)]
    assert L.slimt_hip_beam_step(_ptr(lg), 1, 9, 4, None, _ptr(t), _ptr(f), 0, *map(_ptr, o)) != 0
    assert b"not in 1..8" in L.slimt_hip_last_error()
    assert L.slimt_hip_beam_step(_ptr(lg), 1, 3, 4, None, _ptr(t), _ptr(f), 0, *map(_ptr, o)) != 0
    assert b"flag 3 of row 2" in L.slimt_hip_last_error()
    f[2], t[0] = 2, np.inf
    assert L.slimt_hip_beam_step(_ptr(lg), 1, 3, 4, None, _ptr(t), _ptr(f), 0, *map(_ptr, o)) != 0
    assert b"live row 0 is not finite" in L.slimt_hip_last_error()
    assert L.slimt_hip_beam_step(_ptr(lg), 1, 3, 1 << 20, None, _ptr(t), _ptr(f), 0, *map(_ptr, o)) != 0
    assert b"2^20 or more" in L.slimt_hip_last_error()


def test_wrappers_check_shapes():
    from slimt_amd import capi, frontend
    ctx = capi.Context.__new__(capi.Context)  # (no device: the checks come before the library is called)
    ctx.h = None
    with pytest.raises(ValueError, match="ids \\[B, S\\]"):
        ctx.translate_beam(np.ones(4, np.uint32), np.full(2, 4, np.uint32), 3)
    with pytest.raises(ValueError, match="mismatched shapes"):
        ctx.translate_beam_async((np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32), np.zeros((2, 3, 5), np.uint32),
                                  np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.float32), None, None))
    with pytest.raises(ValueError, match="float32 array of shape \\(2, 3\\)"):
        ctx.translate_beam_async((np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32), np.zeros((2, 3, 6), np.uint32),
                                  np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.float64), None, None))
    with pytest.raises(ValueError, match="beam_step"):
        capi.beam_step(np.zeros((4, 5), np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint32), 3)
    svc = frontend.Service.__new__(frontend.Service)
    with pytest.raises(ValueError, match="beam"):
        svc.beam_search(None, ["a"], 0)
