"""GPU parity of the typical selection kernel alone (slimt_hip_sample_typical; slimt_amd/csrc/sample_typical.hip) with the
NumPy restatement of typical.h (tests/support/typical_ref.py) on crafted rows: kept count, Ebar, column and maximum exact,
the score within 5e-5 of the float64 log-softmax over the kept set. N spans the 4-column groups, one wave, the
register-resident bound (4096) and the streaming variant on either side of it; R is the rows per launch."""
import numpy as np
import pytest

from support import typical_ref
from test_sampling_checker import keys_of

pytestmark = pytest.mark.gpu

TOL = 5e-5
BOUND = 4096  # kTypicalResidentN


@pytest.mark.parametrize("mass", [1e-6, 0.2, 0.9])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, BOUND, BOUND + 1, 32000])
def test_the_typical_kernel_matches_the_restatement(hip, N, R, mass):
    from slimt_amd import capi
    T, inv_T = 0.5, np.float32(2.0)  # (logits = z / 2: exact, so the crafted z are what the kernel sees)
    cases = typical_ref.crafted_rows(N, 7 * N + 1)  # (seeds at which no one column of a gauss row holds a fifth of the mass)
    ids = None if R == 1 else ((np.arange(N, dtype=np.uint64) * 3 + 1) % (1 << 32)).astype(np.uint32)
    worst = 0.0
    for at in range(0, len(cases), R):
        part = cases[at:at + R]
        logits = np.stack([x * np.float32(0.5) for _, x in part])
        keys, steps = keys_of(N + at, len(part)), (np.arange(len(part)) * 9 % 41).astype(np.uint32)
        cols, mx, kept, sc, gap = capi.sample_typical(logits, T, mass, ids=ids, keys=keys, steps=steps)
        for r, (kind, x) in enumerate(part):
            w_col, w_none, w_kept, w_M, w_gap, w_sc = typical_ref.typical_row(keys[r], steps[r], logits[r], ids, inv_T, mass)
            if kind.startswith("gauss") and N >= 64 and mass >= 0.2:
                assert 1 < w_kept.sum() < N, kind
            assert kept[r] == w_kept.sum(), kind
            assert gap[r] == w_gap, kind
            assert cols[r] == (0 if w_none else w_col), kind
            assert mx[r] == w_M or (np.isnan(x).all() and np.isneginf(mx[r])), kind
            assert np.isnan(sc[r]) == np.isnan(w_sc), (kind, sc[r], w_sc)
            if not np.isnan(w_sc):
                assert abs(float(sc[r]) - w_sc) <= TOL, (kind, sc[r], w_sc)
                worst = max(worst, abs(float(sc[r]) - w_sc))
    print("N = %d R = %d mass = %g: scores: max |gpu - float64| = %.3g" % (N, R, mass, worst))
