"""Sampling without replacement on a beam call (slimt_hip_ctx_set_beam_sampling), on the CPU: slimt_amd/csrc/beam_sampled.h
compiled for the host (g++ -O2 -ffp-contract=off) against its NumPy restatement (tests/support/beam_sampled_ref.py) bit for
bit, its accuracy against float64 measured and printed before it is asserted, and the draw's statistics on the restatement,
which tests/test_gpu_beam_step_sampled.py compares the device with bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_sampled_ref as SB
from test_sampling_checker import keys_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include "beam_sampled.h"
using namespace slimt_hip;
extern "C" void condition_all(const float *G, const float *Z, const float *psi, uint32_t n, float *out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = sb_condition(G[i], Z[i], psi[i]);
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    d = tmp_path_factory.mktemp("beam_sampled")
    (d / "h.cc").write_text(_HARNESS)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "slimt_amd", "csrc"), str(d / "h.cc"), "-o", str(d / "h.so")])
    h = ctypes.CDLL(str(d / "h.so"))
    h.condition_all.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_void_p]
    return h


def grid():
    """(G, Z, psi) float32: G = +0 and others; psi == Z, one ulp below, near 0 and -0.25, at and around -28 below Z"""
    f = np.float32
    m28 = [f(-28.0), np.nextafter(f(-28.0), f(0)), np.nextafter(f(-28.0), f(-100)), f(-27.5), f(-28.5), f(-40.0)]
    below = [f(0), f(-1e-7), f(-1e-5), f(-1e-3), f(-0.1), f(-0.24999), f(-0.25), f(-0.25001), f(-0.7), f(-1.0), f(-3.25),
             f(-9.5), f(-17.0), f(-26.0)] + m28
    G, Z, P = [], [], []
    for g in (f(0.0), f(-0.5), f(2.75), f(-7.25), f(-31.0)):
        for dz in (f(-12.0), f(-3.5), f(-0.75), f(0.0), f(0.5), f(4.0), f(20.0)):  # (Z is the children's maximum: either side of G)
            z = f(g + dz)
            for d in below:
                G.append(g), Z.append(z), P.append(f(z + d))
            G.append(g), Z.append(z), P.append(np.nextafter(z, f(-np.inf)))
    return np.asarray(G, f), np.asarray(Z, f), np.asarray(P, f)


def test_condition_has_the_restatements_bits_never_exceeds_g_and_is_accurate(header):
    G, Z, psi = grid()
    got = np.empty_like(G)
    header.condition_all(G.ctypes.data, Z.ctypes.data, psi.ctypes.data, G.size, got.ctypes.data)
    want = SB.sb_condition(G, Z, psi)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[psi == Z].view(np.uint32), G[psi == Z].view(np.uint32)) and (psi == Z).sum() >= 35
    assert np.all(got <= G) and np.isfinite(got).all()
    g, z, p = (x.astype(np.float64) for x in (G, Z, psi))
    with np.errstate(all="ignore"):
        v = g - p + np.where(p == z, -np.inf, np.log(-np.expm1(np.minimum(p - z, -1e-300))))
        ref = g - np.maximum(0.0, v) - np.log1p(np.exp(-np.abs(v)))
    err = np.abs(got.astype(np.float64) - ref)
    worst = int(err.argmax())
    print("sb_condition against float64 over %d points: worst %.3g at G %r Z %r psi %r" % (G.size, err.max(), G[worst], Z[worst], psi[worst]))
    assert err.max() <= 5e-5  # (measured 3.0e-6: inside the project's score tolerance, which is asserted)


def test_draws_without_replacement_follow_the_models_distribution():
    """one row of 8 logits, k = 2, step 0, 8192 keys: slot 0's token is a draw from softmax p, and token j is among the two
    with probability p_j + sum_{i != j} p_i p_j / (1 - p_i); each frequency within 5 sigma"""
    n, k, N = 8192, 2, 8
    logits = np.linspace(0, 2.1, N).astype(np.float32)
    keys = keys_of(7, n)
    totals, G, flags = SB.start_state(n, k)
    rows = np.zeros((n * k, N), np.float32)
    rows[0::k] = logits
    parent, token, score, tot, pert, fl = SB.step_sampled_host(rows, totals, G, flags, k, keys, 0, eos_id=99)
    token = token.reshape(n, k)
    assert np.all(fl == BC.LIVE) and np.all(parent == 0) and np.all(token[:, 0] != token[:, 1])
    assert np.all(pert.reshape(n, k)[:, 0] == 0) and np.all(pert.reshape(n, k)[:, 1] < 0)  # (the maximum keeps the parent's G)
    p = np.exp(logits.astype(np.float64))
    p /= p.sum()
    incl = np.array([p[j] + sum(p[i] * p[j] / (1 - p[i]) for i in range(N) if i != j) for j in range(N)])
    for want, got in ((p, np.bincount(token[:, 0], minlength=N) / n), (incl, np.bincount(token.reshape(-1), minlength=N) / n)):
        bound = 5 * np.sqrt(want * (1 - want) / n)
        print(np.abs(got - want) / bound)
        assert np.all(np.abs(got - want) <= bound)
