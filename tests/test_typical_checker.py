"""Locally typical sampling (include/slimt_hip.h, slimt_hip_ctx_set_sampling_typical): slimt_amd/csrc/typical.h, compiled for
the host into a stand-alone program, against the NumPy restatement of tests/support/typical_ref.py -- kept set and Ebar bit
for bit, on the crafted rows the GPU test uses. This pins the definition both the kernel and the checker follow."""
import os
import subprocess

import numpy as np
import pytest

from support import typical_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "typical.h"
using namespace slimt_hip;
// stdin: rows of "n mass" and n float bit patterns; stdout: per row "Ebar kept-columns..."
int main() {
  unsigned n;
  float mass;
  while (scanf("%u %f", &n, &mass) == 2) {
    std::vector<float> z(n);
    for (unsigned i = 0; i < n; ++i) { unsigned b; if (scanf("%x", &b) != 1) return 1; z[i] = sm_float(b); }
    if (!ty_valid(mass) || n > (unsigned)kTypicalMaxN) return 2;
    float M = -__builtin_inff();
    for (float v : z) if (v == v) M = fmaxf(M, v);
    uint64_t Q = 0, A = 0;
    std::vector<uint32_t> w(n, 0), key(n, 0);
    for (unsigned i = 0; i < n; ++i) if (z[i] == z[i] && (w[i] = tr_weight(z[i], M)) > 0) {
      key[i] = ty_gap(z[i], M);
      Q += w[i];
      A += (uint64_t)w[i] * key[i];
    }
    if (!Q) { printf("0\n"); continue; }
    const uint32_t Ebar = ty_mean(A, Q);
    for (unsigned i = 0; i < n; ++i) if (w[i]) key[i] = ty_key(key[i], Ebar);
    uint32_t kappa = ~0u;  // the least key whose columns, with all below it, reach the mass
    for (unsigned i = 0; i < n; ++i) if (w[i] && key[i] < kappa) {
      uint64_t sum = 0;
      for (unsigned j = 0; j < n; ++j) if (w[j] && key[j] <= key[i]) sum += w[j];
      if ((double)sum >= ty_target(mass, Q)) kappa = key[i];
    }
    printf("%u", Ebar);
    for (unsigned i = 0; i < n; ++i) if (w[i] && key[i] <= kappa) printf(" %u", i);
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("typical")
    (d / "main.cc").write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "slimt_amd", "csrc"),
                           str(d / "main.cc"), "-o", str(d / "typical")])
    return str(d / "typical")


def test_the_header_and_the_restatement_keep_the_same_set_and_mean_gap(program):
    from slimt_amd import capi
    assert {"slimt_hip_ctx_set_sampling_typical", "slimt_hip_sample_typical"} <= set(capi.SYMBOLS)
    rows = [(x, mass) for i, N in enumerate((1, 2, 65, 1029)) for mass in (1e-6, 0.2, 0.9, 1.0) for _, x in typical_ref.crafted_rows(N, i)]
    text = "".join("%d %r\n%s\n" % (x.size, float(np.float32(mass)), " ".join("%x" % b for b in x.view(np.uint32))) for x, mass in rows)
    out = subprocess.run([program], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    for line, (x, mass) in zip(out, rows):
        got = [int(v) for v in line.split()]
        kept, Ebar, _ = typical_ref.typical_set(x, mass)
        assert got[0] == Ebar, (x.size, mass)
        assert got[1:] == list(np.flatnonzero(kept)), (x.size, mass)


def test_the_restatement_follows_the_rule_on_a_hand_made_row():
    z = np.array([0.0, -1.0, -1.0, -1.0, np.nan, -40.0], np.float32)  # p = .475, .175 x 3, -, 0: Ebar = .525 nats
    kept, Ebar, M = typical_ref.typical_set(z, 0.2)
    assert abs(Ebar / 65536 - 3 * np.exp(-1) / (1 + 3 * np.exp(-1))) < 1e-4 and M == 0
    assert list(np.flatnonzero(kept)) == [1, 2, 3]  # the twins are closest to the entropy: all in, the maximum out
    assert list(np.flatnonzero(typical_ref.typical_set(z, 0.6)[0])) == [0, 1, 2, 3]
    assert not typical_ref.typical_set(np.full(3, np.nan, np.float32), 0.5)[0].any()
