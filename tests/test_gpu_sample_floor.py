"""GPU parity of the floor selection kernel alone (slimt_hip_sample_floor; slimt_amd/csrc/sample_floor.hip) with the NumPy
restatement of floor.h (tests/support/floor_ref.py) on crafted rows: kept count, column and maximum exact, the score within
5e-5 of the float64 log-softmax over the kept set. N spans the 4-column groups, one wave, the register-resident bound
(4096) and the streaming variant on either side of it; R is the rows per launch.

'gauss' rows keep a strict subset of more than one column wherever a row of distinct values can: not with fewer than three
columns, not at min_p = 1 (only full-weight columns pass) and not at epsilon = 0.9 (at most one probability reaches it)."""
import numpy as np
import pytest

from support import floor_ref
from test_sampling_checker import keys_of

pytestmark = pytest.mark.gpu

TOL = 5e-5
BOUND = 4096  # kFloorResidentN


@pytest.mark.parametrize("min_p,epsilon", [(0.1, 0.0), (0.0, 0.02), (0.1, 0.02), (1.0, 0.0), (0.0, 0.9)])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [1, 63, 64, 65, BOUND, BOUND + 1, 32000])
def test_the_floor_kernel_matches_the_restatement(hip, N, R, min_p, epsilon):
    from slimt_amd import capi
    T, inv_T = 0.5, np.float32(2.0)  # (logits = z / 2: exact, so the crafted z are what the kernel sees)
    cases = floor_ref.crafted_rows(N, 7 * N + R, min_p, epsilon)
    ids = None if R == 1 else ((np.arange(N, dtype=np.uint64) * 3 + 1) % (1 << 32)).astype(np.uint32)
    worst = 0.0
    for params in sorted({p for _, _, p in cases}):
        group = [(k, x) for k, x, p in cases if p == params]
        for at in range(0, len(group), R):
            part = group[at:at + R]
            logits = np.stack([x * np.float32(0.5) for _, x in part])
            keys, steps = keys_of(N + at, len(part)), (np.arange(len(part)) * 9 % 41).astype(np.uint32)
            cols, mx, kept, sc = capi.sample_floor(logits, T, *params, ids=ids, keys=keys, steps=steps)
            for r, (kind, x) in enumerate(part):
                w_col, w_none, w_kept, w_M, w_sc = floor_ref.floored_row(keys[r], steps[r], logits[r], ids, inv_T, *params)
                where = (kind, params)
                if kind == "gauss" and N >= 3 and params[0] < 1 and params[1] < 0.9:
                    assert 1 < w_kept.sum() < (~np.isnan(x)).sum(), where
                assert kept[r] == w_kept.sum(), where
                assert cols[r] == (0 if w_none else w_col), where
                assert mx[r] == w_M or (np.isnan(x).all() and np.isneginf(mx[r])), where
                assert np.isnan(sc[r]) == np.isnan(w_sc), where + (sc[r], w_sc)
                if not np.isnan(w_sc):
                    assert abs(float(sc[r]) - w_sc) <= TOL, where + (sc[r], w_sc)
                    worst = max(worst, abs(float(sc[r]) - w_sc))
    print("N = %d R = %d: scores: max |gpu - float64| = %.3g" % (N, R, worst))
