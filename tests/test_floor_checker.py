"""Floored sampling (include/slimt_hip.h, slimt_hip_ctx_set_sampling_floor): slimt_amd/csrc/floor.h, compiled for the host
into a stand-alone program, against the NumPy restatement of tests/support/floor_ref.py -- kept set and Q bit for bit, on
random rows and on the crafted rows the GPU test uses. This pins the definition both the kernel and the checker follow."""
import os
import subprocess

import numpy as np
import pytest

from support import floor_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "floor.h"
using namespace slimt_hip;
// stdin: rows of "n min_p epsilon" and n float bit patterns; stdout: per row "Q kept-columns..."
int main() {
  unsigned n;
  float min_p, eps;
  while (scanf("%u %f %f", &n, &min_p, &eps) == 3) {
    std::vector<float> z(n);
    for (unsigned i = 0; i < n; ++i) { unsigned b; if (scanf("%x", &b) != 1) return 1; z[i] = sm_float(b); }
    if (!fl_valid(min_p, eps)) return 2;
    float M = -__builtin_inff();
    unsigned long long Q = 0;
    for (float v : z) if (v == v) M = fmaxf(M, v);
    for (float v : z) if (v == v) Q += tr_weight(v, M);
    const double fm = fl_min(min_p), fe = fl_eps(eps, fl_needs_total(eps) ? Q : 0);
    printf("%llu", Q);
    for (unsigned i = 0; i < n; ++i) if (z[i] == z[i] && fl_keep(z[i], M, tr_weight(z[i], M), fm, fe)) printf(" %u", i);
    printf("\n");
  }
  return 0;
}
"""

PARAMS = [(0.1, 0.0), (0.0, 0.02), (0.1, 0.02), (1.0, 0.0), (0.0, 0.9)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("floor")
    (d / "main.cc").write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "slimt_amd", "csrc"),
                           str(d / "main.cc"), "-o", str(d / "floor")])
    return str(d / "floor")


def test_the_header_and_the_restatement_keep_the_same_set_and_total(program):
    rng = np.random.default_rng(5)
    rows = []
    for N in (1, 2, 63, 257, 4096, 5000):
        for scale in (0.5, 3.0, 9.0):
            rows += [(rng.normal(0.0, scale, N).astype(np.float32), p) for p in PARAMS]
    for i, (N, p) in enumerate((N, p) for N in (1, 65, 4097) for p in PARAMS):
        rows += [(x, q) for _, x, q in floor_ref.crafted_rows(N, i, *p)]
    text = "".join("%d %r %r\n%s\n" % (x.size, float(np.float32(p[0])), float(np.float32(p[1])),
                                       " ".join("%x" % b for b in x.view(np.uint32))) for x, p in rows)
    out = subprocess.run([program], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    strict = 0
    for line, (x, p) in zip(out, rows):
        got = [int(v) for v in line.split()]
        kept, Q, _ = floor_ref.kept_set(x, *p)
        assert got[0] == Q, (x.size, p)
        assert got[1:] == list(np.flatnonzero(kept)), (x.size, p)
        strict += 1 < kept.sum() < (~np.isnan(x)).sum()
    assert strict > len(rows) // 4  # (the floors cut, and not down to the maximum alone, in a good share of the rows)


def test_the_restatement_follows_the_rule_on_a_hand_made_row():
    z = np.array([0.0, np.log(0.5), np.log(0.05), np.nan, -40.0], np.float32)  # p = 1, .5, .05, -, 0 of 1.55
    for params, kept in (((0.1, 0.0), [0, 1]), ((0.0, 0.02), [0, 1, 2]), ((0.0, 0.5), [0]), ((0.0, 0.9), [0]), ((0.0, 0.0), [0, 1, 2, 4])):
        assert list(np.flatnonzero(floor_ref.kept_set(z, *params)[0])) == kept, params  # (0.9: the fallback, the maximum alone)
    assert not floor_ref.kept_set(np.full(3, np.nan, np.float32), 0.1, 0.1)[0].any()
    assert floor_ref.kept_set(np.full(3, -np.inf, np.float32), 1.0, 0.9)[0].all()
