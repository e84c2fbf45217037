"""slimt_hip_beam_step on the device against `beam_step_host` (tests/support/beam_cases.py), bit for bit: one selection of
the beam search over crafted rows -- equal totals across slots, equal logits within a slot, +0 / -0, a NaN row, a row of
-inf, a maximum of +inf, a finished slot ahead of every live candidate, fewer candidates than slots, EOS chosen, the
step-0 state. N = 1 (one column), 17 (an odd few), 4097 (more than one sweep of the workgroup and one column over)."""
import numpy as np
import pytest

from support import beam_cases as BC

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(hip, logits, totals, flags, k, eos, ids):
    got = hip.beam_step(logits, totals, flags, k, eos, ids)
    want = BC.beam_step_host(logits, totals, flags, k, eos, ids)
    for g, w, name in zip(got, want, ("parent", "token", "token_score", "totals", "flags")):
        if g.dtype == np.float32:
            assert np.array_equal(_bits(g), _bits(w)), (name, g, w)
        else:
            assert np.array_equal(g, w), (name, g, w)
    return want


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 17, 4097])
def test_beam_step_equals_the_sorting_checker(hip, N, k, B):
    logits, totals, flags, eos, ids = BC.crafted_step(N, k, B)
    parent, token, score, tot, fl = _check(hip, logits, totals, flags, k, eos, ids)
    # the crafted state holds what it is for (on the checker's result)
    assert fl[0] != BC.DEAD and parent[0] == 0  # the step-0 state: every new slot comes from slot 0
    assert token[0] == eos and fl[0] == BC.FINISHED  # EOS chosen
    if B >= 3 and k >= 3:
        rows = slice(k, 2 * k)
        assert token[rows][0] == BC.NONE and parent[rows][0] == 2  # the finished slot first
        assert (fl[2 * k:3 * k] == BC.DEAD).sum() == (k - 2 if N > 1 else k - 1)  # fewer candidates than slots


def test_ties_between_slots_and_signed_zeros(hip):
    """two live slots with the same row and the same total: every candidate ties with its twin, the lower slot first;
    +0 and -0 logits are equal, the lower column first, and each keeps its own bits in the score"""
    k, N = 4, 17
    row = np.full(N, -5.0, np.float32)
    row[[2, 11]] = [-0.0, 0.0]
    logits = np.stack([row, row, row - 1, row])
    totals = np.asarray([-1.0, -1.0, -1.0, -np.inf], np.float32)
    flags = np.asarray([BC.LIVE, BC.LIVE, BC.LIVE, BC.DEAD], np.uint32)
    parent, token, score, tot, fl = _check(hip, logits, totals, flags, k, 99, None)
    assert parent.tolist() == [0, 0, 1, 1] and token.tolist() == [2, 11, 2, 11]


def test_unusable_rows_contribute_nothing(hip):
    k, N = 4, 40
    r = np.random.default_rng(3)
    logits = r.normal(0, 1, size=(2 * k, N)).astype(np.float32)
    logits[0, 7] = np.nan
    logits[1] = -np.inf
    logits[2, 39] = np.inf
    totals = np.zeros(2 * k, np.float32)
    flags = np.full(2 * k, BC.LIVE, np.uint32)
    logits[4:, :] = logits[3]  # the second source: four equal usable rows
    logits[5, 3] = np.nan
    parent, token, score, tot, fl = _check(hip, logits, totals, flags, k, 0, None)
    assert set(parent[:k].tolist()) == {3} and 5 - k not in parent[k:].tolist()
