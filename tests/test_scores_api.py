"""CPU-side checks of per-token scores (include/slimt_hip.h, slimt_hip_ctx_set_scores): the entry point is exported and
wrapped, it fails loudly without a context or a GPU, and the running log-sum-exp the kernels keep beside their arg-max
(slimt_amd/csrc/scores.h) agrees with float64 on adversarial orders -- compiled here for the host from the same header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include "scores.h"
using namespace slimt_hip;
// the kernels' order: one running (max, sum) per part over its columns (lse_push, the arg-max's strict > moving the
// maximum), then the parts merged pairwise (lse_merge); returns -log(sum) = the score of the maximum
extern "C" float score_of(const float *l, int n, int parts) {
  float m[64], s[64];
  for (int p = 0; p < parts; ++p) {
    m[p] = -3.402823466e+38f;
    s[p] = 0.0f;
  }
  for (int i = 0; i < n; ++i) {
    const int p = i % parts;
    const bool better = l[i] > m[p];
    lse_push(l[i], true, better, m[p], s[p]);
    m[p] = better ? l[i] : m[p];
  }
  for (int w = 1; w < parts; w *= 2)
    for (int p = 0; p + w < parts; p += 2 * w) lse_merge(m[p], s[p], m[p + w], s[p + w]);
  bool none = !(m[0] > -3.402823466e+38f);
  return lse_score(s[0], none);
}
// a column outside the layer adds nothing, whatever its value
extern "C" float masked_sum(float v, float m, float s) {
  lse_push(v, false, false, m, s);
  return s;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("scores")
    src = d / "h.cc"
    src.write_text(_HARNESS)
    so = d / "h.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "slimt_amd", "csrc"), str(src), "-o", str(so)])
    h = ctypes.CDLL(str(so))
    h.score_of.restype = ctypes.c_float
    h.score_of.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    h.masked_sum.restype = ctypes.c_float
    h.masked_sum.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
    return h


def _score(h, l, parts):
    l = np.ascontiguousarray(l, dtype=np.float32)
    return float(h.score_of(l.ctypes.data, l.size, parts))


def _ref(l):
    l = np.asarray(l, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if np.isnan(l).any():
            return float("nan")
        mx = l.max()
        if not np.isfinite(mx):
            return float("nan")
        return float(mx - (mx + np.log(np.exp(l - mx).sum())))


@pytest.mark.parametrize("parts", [1, 2, 16, 64])
@pytest.mark.parametrize("case", ["normal", "ascending", "descending", "huge_spread", "tiny_spread", "ties",
                                  "some_minus_inf", "wide_vocabulary"])
def test_running_logsumexp_matches_float64(harness, parts, case):
    r = np.random.Generator(np.random.PCG64(7))
    n = 4096
    l = r.normal(0, 4, n).astype(np.float32)
    if case == "ascending":
        l = np.sort(l)  # the maximum moves at every column: the rescaling path throughout
    elif case == "descending":
        l = np.sort(l)[::-1].copy()
    elif case == "huge_spread":
        l = (r.normal(0, 1, n) * 1e4).astype(np.float32)
        l[123] = 3e4
    elif case == "tiny_spread":
        l = (1000.0 + r.normal(0, 1e-4, n)).astype(np.float32)
    elif case == "ties":
        l = np.round(l).astype(np.float32)
    elif case == "some_minus_inf":
        l[r.integers(0, n, 500)] = -np.inf
    elif case == "wide_vocabulary":
        # (the kernels never add more than a few hundred terms in one running sum: 32,000 columns over 256 lanes, or
        # partials of 256 columns; one f32 sum of all 32,000 drifts by ~6e-5)
        if parts < 16:
            pytest.skip("not an order the kernels use")
        l = r.normal(0, 4, 32000).astype(np.float32)
    got, want = _score(harness, l, parts), _ref(l)
    assert abs(got - want) <= 5e-5 + 2e-6 * abs(want), (got, want)


@pytest.mark.parametrize("parts", [1, 16])
def test_nan_and_all_minus_inf_score_nan(harness, parts):
    l = np.zeros(256, np.float32)
    l[77] = np.nan  # a NaN anywhere: NaN
    assert np.isnan(_score(harness, l, parts))
    l = np.full(256, np.nan, np.float32)
    assert np.isnan(_score(harness, l, parts))
    l = np.full(256, -np.inf, np.float32)  # nothing beats the start value
    assert np.isnan(_score(harness, l, parts))


def test_columns_outside_the_layer_add_nothing(harness):
    for v in (float("nan"), 1e30, -1e30, float("inf"), float("-inf"), 0.0):
        assert harness.masked_sum(v, 2.0, 3.5) == np.float32(3.5)


def test_set_scores_is_exported_and_wrapped():
    from slimt_amd import build, capi
    dll = ctypes.CDLL(build.build())
    assert hasattr(dll, "slimt_hip_ctx_set_scores")
    assert "slimt_hip_ctx_set_scores" in capi.SYMBOLS
    import inspect
    for name in ("translate", "translate_pinned", "translate_generated"):
        assert inspect.signature(getattr(capi.Context, name)).parameters["scores"].default is False
    for name in ("translate_async", "translate_many_async", "translate_many_device"):
        assert inspect.signature(getattr(capi.Context, name)).parameters["scores"].default is None
    for name in ("translate_device", "translate_device_generated"):
        assert inspect.signature(getattr(capi.Context, name)).parameters["scores"].default == 0


def test_set_scores_fails_loudly_without_a_context():
    from slimt_amd import capi
    L = capi.lib()
    dst = (ctypes.c_void_p * 1)(None)
    assert L.slimt_hip_ctx_set_scores(None, dst, 1) != 0
    assert b"null argument" in L.slimt_hip_last_error()


def test_service_scores_are_exported_and_refuse_null_arguments():
    """include/slimt_hip_service_scores.h against libslimt_hip_host.so (without a GPU no service can be created, so
    the entry points are checked on their argument errors)."""
    from slimt_amd import build, capi
    build.build_host_lib()
    H = capi.host_lib()
    for n in ("slimt_hip_service_set_scores", "slimt_hip_result_scores"):
        assert hasattr(H, n)
    assert H.slimt_hip_service_set_scores(None, 1) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    out = ctypes.c_void_p()
    assert H.slimt_hip_result_scores(None, ctypes.byref(out)) != 0
    import inspect
    from slimt_amd import frontend
    assert inspect.signature(capi.BatchService).parameters["scores"].default is False
    assert inspect.signature(frontend.Service.translate).parameters["scores"].default is False
    assert inspect.signature(frontend.Service.pivot).parameters["scores"].default is False
    assert {"token_scores", "sentence_scores"} <= set(frontend.Response.__dataclass_fields__)


def test_wrappers_check_the_number_of_score_destinations():
    """a mismatched list is refused in Python, before anything is armed on the context"""
    from slimt_amd import capi
    ctx = capi.Context.__new__(capi.Context)  # (no device needed: the check comes first)
    with pytest.raises(ValueError):
        ctx.translate_many_device([(0, 0, 1, 0, 0, 0, 0, 0)] * 2, 8, 1.5, 0, scores=[1])
    with pytest.raises(ValueError):
        ctx.translate_many_async([(None,) * 5] * 2, scores=[np.zeros((1, 1), np.float32)])
