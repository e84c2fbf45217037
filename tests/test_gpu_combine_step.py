"""slimt_hip_combine_step on the device against the NumPy restatement (tests/support/combine_ref.py), bit for bit: column,
token, combined score and every member's own score. N: one column, two, the wave's and the workgroup's edges (63 / 65,
511 / 513), 2049 (a second 4-column group per thread), 4096 (the widest resident rows), 4097 / 4102 (streamed, scalar loads),
8200 (streamed, 128-bit loads), 9001. The rows are combine_ref.crafted's: duplicated columns on quarter steps (ties in s
resolved by l_0, then by the column), -inf entries in primary and contrast rows, a contrast row and a primary with a NaN."""
import numpy as np
import pytest

from support import combine_ref as CR

pytestmark = pytest.mark.gpu

# per m: mixed signs / a gap that cuts all but a few columns / a zero weight
SETTINGS = {1: [((1.0,), -np.inf), ((0.5,), -0.75)],
            2: [((1.0, -3.0), -np.inf), ((1.0, -3.0), -0.75), ((2.0, 0.0), -np.inf)],
            4: [((1.0, -0.5, 0.25, -16.0), -np.inf), ((1.0, 0.5, 0.0, -1.5), -0.75)]}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("m", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 2, 63, 65, 511, 513, 2049, 4096, 4097, 4102, 8200, 9001])
def test_combined_step_equals_the_restatement(hip, N, m, with_ids):
    x = CR.crafted(N, m, G=3)
    ids = np.random.default_rng(N).permutation(N).astype(np.uint32) if with_ids else None
    kept = []
    for w, gap in SETTINGS[m]:
        want = CR.steps(x, m, w, gap, ids)
        got = hip.combine_step(x, m, w, gap, ids)
        for g, v, name in zip(got, want, ("column", "token", "combined", "member_scores")):
            assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(v) if v.dtype == np.float32 else v), (name, w, gap, g, v)
        kept.append(want)
        assert want[0][2] == 0 and np.isnan(want[2][2]) and np.isnan(want[3][2, 0])  # the primary with a NaN: column 0
    # the cases bite, on the reference alone: a contrast changes a pick, and the gap changes it again
    if m > 1 and N >= 63:
        greedy = CR.steps(x, m, (1.0,) + (0.0,) * (m - 1), -np.inf, ids)[0]
        assert not np.array_equal(kept[0][0], greedy) and not np.array_equal(kept[0][0][:2], kept[1][0][:2])
