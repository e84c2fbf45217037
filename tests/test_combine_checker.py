"""Combined decoding (include/slimt_hip.h, slimt_hip_ctx_set_fanout_combine) on the CPU: slimt_amd/csrc/combine.h compiled for
the host (g++ -O2 -ffp-contract=off, as tests/test_beam_checker.py compiles beam.h) against its NumPy restatement
(tests/support/combine_ref.py) bit for bit, the restatement against float64, and the API's surface."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from support import combine_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [((1.0,), -np.inf), ((1.0, -0.7), -np.inf), ((1.0, -0.7), -2.0), ((0.5, 0.0), -np.inf), ((1.0, 0.5, -1.5), -3.0),
            ((2.0, -16.0, 0.0, 0.25), -np.inf), ((1.0, -1.0, 1.0, -1.0), -0.5)]

_HARNESS = r"""
#include "combine.h"
using namespace slimt_hip;
extern "C" int group(const float *l, int m, uint32_t N, const float *w, float gap, uint32_t *col, float *s_out, float *lp_out) {
  float M[kCombineMax], L[kCombineMax], blp[kCombineMax];
  bool us[kCombineMax];
  for (int j = 0; j < m; ++j) {
    bool nan = false;
    float mx = -INFINITY;
    for (uint32_t c = 0; c < N; ++c) nan = nan || l[j * N + c] != l[j * N + c], mx = fmaxf(mx, l[j * N + c]);
    M[j] = bm_max(mx);
    us[j] = bm_usable(nan, M[j]);
    uint64_t Q = 0;
    for (uint32_t c = 0; us[j] && c < N; ++c) Q += bm_weight(l[j * N + c], M[j]);
    L[j] = us[j] ? bm_normaliser(Q) : 0.0f;
    blp[j] = NAN;
  }
  bool bc = false;
  float bs = NAN, bl = -INFINITY;
  uint32_t bi = kCombineNone;
  for (uint32_t c = 0; c < (us[0] ? N : 1u); ++c) {
    float lp[kCombineMax], s = NAN;
    bool cand = false;
    for (int j = 0; j < m; ++j) lp[j] = us[j] ? bm_logprob(l[j * N + c], M[j], L[j]) : NAN;
    if (us[0]) {
      s = cb_first(w[0], lp[0]);
      for (int j = 1; j < m; ++j)
        if (cb_counted(j, w[j], us[j])) s = cb_add(s, w[j], l[j * N + c], lp[j]);
      cand = cb_plausible(l[c], M[0], gap) && s == s;
    }
    const float l0 = us[0] ? l[c] : -INFINITY;
    if (!cb_before(cand, s, l0, c, bc, bs, bl, bi)) continue;
    bc = cand, bs = s, bl = l0, bi = c;
    for (int j = 0; j < m; ++j) blp[j] = lp[j];
  }
  *col = bi, *s_out = bc ? bs : NAN;
  for (int j = 0; j < m; ++j) lp_out[j] = blp[j];
  return cb_valid(m, w, gap);
}
"""


@pytest.fixture(scope="module")
def header_group(tmp_path_factory):
    d = tmp_path_factory.mktemp("combine")
    (d / "h.cc").write_text(_HARNESS)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "slimt_amd", "csrc"),
                           str(d / "h.cc"), "-o", str(d / "h.so")])
    h = ctypes.CDLL(str(d / "h.so"))
    h.group.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_float] + [ctypes.c_void_p] * 3

    def group(rows, w, gap):
        rows, w = np.ascontiguousarray(rows, np.float32), np.asarray(w, np.float32)
        col, s, lp = np.zeros(1, np.uint32), np.zeros(1, np.float32), np.zeros(len(w), np.float32)
        ok = h.group(rows.ctypes.data, len(w), rows.shape[1], w.ctypes.data, gap, col.ctypes.data, s.ctypes.data, lp.ctypes.data)
        return ok, int(col[0]), s[0], lp
    return group


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("w,gap", SETTINGS)
def test_the_header_equals_the_restatement_bit_for_bit(header_group, w, gap):
    m, seen = len(w), set()
    for N in (1, 2, 5, 64, 513, 4097):
        x = CR.crafted(N, m)
        for g in range(3):
            ok, col, s, lp = header_group(x[g * m:(g + 1) * m], w, gap)
            c2, s2, lp2 = CR.step(x[g * m:(g + 1) * m], w, gap)
            assert ok == 1 and col == c2 and _bits(s) == _bits(s2) and np.array_equal(_bits(lp), _bits(lp2)), (N, g)
            seen.add("nan" if np.isnan(s2) else "primary" if col == np.argmax(x[g * m]) else "other")
    assert seen >= ({"nan", "primary", "other"} if any(v != 0 for v in w[1:]) else {"nan", "primary"})  # the cases bite


def test_the_rules_special_cases(header_group):
    ninf, nan = -np.inf, np.nan
    tie = np.asarray([[1.0, 3.0, 3.0, -0.0], [0.0, 5.0, 1.0, -9.0]], np.float32)
    for group in (header_group, lambda r, w, g: (1,) + CR.step(r, w, g)):
        assert group(tie[:1], [2.0], ninf)[1] == 1 and group(tie, [1.0, 0.0], ninf)[1] == 1     # greedy: the first maximum
        assert group(tie, [1.0, -1.0], ninf)[1] == 3 and group(tie, [1.0, -1.0], -1.0)[1] == 2  # contrasted; cut to {1, 2}
        assert group(tie, [1.0, 1.0], ninf)[1] == 1                                             # ensembled
        flat = np.asarray([[2.0, 2.0, 2.0], [0.0, 0.0, 0.0]], np.float32)                       # equal s and l_0: the lower column
        assert group(flat, [1.0, -0.5], ninf)[1] == 0
        assert group(np.asarray([[1.0, 1.0, 1.0], [ninf, 0.0, 0.0]], np.float32), [1.0, 4.0], ninf)[1] == 0  # a -inf term is left out
        _, col, s, lp = group(np.asarray([[nan, 9.0], [0.0, 1.0]], np.float32), [1.0, -1.0], ninf)  # an unusable primary
        assert col == 0 and np.isnan(s) and np.isnan(lp[0]) and lp[1] < 0
        # l - M overflows to -inf: column 0 is +inf - inf = NaN, column 1 (s = -inf) is cut by the gap: no candidate left
        over = np.asarray([[3e38, -3e38], [-3e38, 3e38], [-3e38, 3e38]], np.float32)
        assert group(over, [1.0, -16.0, 16.0], ninf)[1:3] == (1, -np.inf)
        _, col, s, lp = group(over, [1.0, -16.0, 16.0], -1.0)
        assert col == 0 and np.isnan(s) and lp.tolist() == [0.0, ninf, ninf]  # ... the primary's arg-max, each row's own lp


SEEDS = list(range(100, 100 + 3 * (len(SETTINGS) - 1)))  # picked on the CPU: float64's top-two margin holds on every group


def test_the_restatement_is_within_the_tolerance_of_float64():
    worst, rows = 0.0, 0
    for seed, (w, gap) in enumerate(SETTINGS[1:] * 3):
        r = np.random.default_rng(SEEDS[seed])
        for N, scale in ((17, 2.0), (1000, 4.0), (4096, 1.0), (9001, 3.0)):
            x = r.normal(0, scale, size=(len(w), N)).astype(np.float32)
            z = x.astype(np.float64)
            lp64 = z - z.max(axis=1, keepdims=True) - np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1, keepdims=True))
            s64 = (np.asarray(w, np.float64)[:, None] * lp64).sum(axis=0)
            s64[lp64[0] - lp64[0].max() < gap] = -np.inf  # (seeds keep float64's cut away from the top two)
            bound = 5e-5 * float(np.abs(np.asarray(w, np.float64)).sum())  # the project's score tolerance per term
            top = np.sort(s64)[-2:]
            assert top[1] - top[0] > 2 * bound, (seed, N, "pick another seed")
            col, s, _ = CR.step(x, w, gap)
            assert col == int(s64.argmax()), (seed, N)
            worst, rows = max(worst, abs(float(s) - s64[col]) / bound), rows + 1
    print("s against float64 over %d groups: worst %.3g of the bound" % (rows, worst))
    assert worst <= 1.0


def test_symbols_are_declared_wrapped_and_refuse_bad_settings_at_once():
    from slimt_amd import capi, frontend
    import inspect
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "slimt_hip.h")).read()
    for name in ("slimt_hip_ctx_set_fanout_combine", "slimt_hip_combine_step"):
        assert "int %s(" % name in header and name in capi.SYMBOLS and getattr(L, name).argtypes is not None
    assert "#define SLIMT_HIP_MAX_COMBINE 4" in header and capi.MAX_COMBINE == 4 and L.slimt_hip_abi_version() == 3
    assert "combine" in inspect.signature(capi.Context.translate_fanout).parameters
    assert "contrast" in inspect.signature(frontend.Service.translate).parameters
    for members, weights, gap, message in ((5, (1, 1, 1, 1, 1), 0.0, b"not in 0..4"), (-1, (1,), 0.0, b"not in 0..4"),
                                           (2, (1, 17), 0.0, b"within +-16"), (2, (0, 1), 0.0, b"finite and > 0"),
                                           (1, (1,), 0.5, b"not <= 0"), (1, (1,), np.nan, b"not <= 0"), (2, None, 0.0, b"weights is NULL")):
        w = None if weights is None else np.asarray(weights, np.float32)
        rc = L.slimt_hip_ctx_set_fanout_combine(None, members, None if w is None else w.ctypes.data, gap)
        assert rc < 0 and message in L.slimt_hip_last_error(), message
    with pytest.raises(ValueError, match="combine_step"):
        capi.combine_step(np.zeros((3, 4), np.float32), 2, [1.0, -1.0])
