"""slimt_hip_beam_step_grouped on the device against the sorting reference (tests/support/beam_grouped_ref.py), bit for bit:
the groups' step-0 state in source 0, beam_cases.crafted_step's mid-search state (finished, dead and live slots, NaN rows,
quarter-step logits so ties are everywhere) in the others. N = 1 (one column), 17 (an odd few), 4096 (the widest row a wave
keeps in registers), 4097 (one over it: the streamed sweep)."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_grouped_ref as GR

pytestmark = pytest.mark.gpu

KG = [(1, 1), (2, 2), (4, 2), (6, 3), (8, 1), (8, 2), (8, 4), (8, 8)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _state(N, k, G, B, with_ids):
    logits, totals, flags, eos, ids = BC.crafted_step(N, k, B)
    totals[:k], flags[:k] = GR.start_state(1, k, G)  # source 0: the groups' step-0 state ...
    logits[:k] = logits[0]                           # ... where every slot's row is the same row
    if not with_ids:
        ids = None
    elif ids is None:
        ids = np.arange(N, dtype=np.uint32)[::-1].copy()
    return logits, totals, flags, eos, ids


@pytest.mark.parametrize("penalty", [0.0, 0.5, 64.0])
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k,G", KG)
@pytest.mark.parametrize("N", [1, 17, 4096, 4097])
def test_grouped_step_equals_the_sorting_reference(hip, N, k, G, B, with_ids, penalty):
    logits, totals, flags, eos, ids = _state(N, k, G, B, with_ids)
    want = GR.step(logits, totals, flags, k, G, penalty, eos, ids)
    got = hip.beam_step_grouped(logits, totals, flags, k, G, penalty, eos, ids)
    for g, w, name in zip(got, want, ("parent", "token", "token_score", "totals", "flags")):
        assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(w) if w.dtype == np.float32 else w), (name, g, w)
    if G == 1:  # the plain beam step, bit for bit
        plain = hip.beam_step(logits, totals, flags, k, eos, ids)
        assert all(np.array_equal(g.view(np.uint32), p.view(np.uint32)) for g, p in zip(got, plain))
    # the cases bite, on the reference alone (source 0 is at step 0: one live slot per group)
    parent, token, _, _, fl = (x[:k] for x in want)
    if N == 1:  # every later group still takes the one column, and a group of g > 1 slots has one candidate
        first = np.arange(0, k, k // G)
        assert np.array_equal(token[first], np.full(G, 0 if ids is None else ids[0])) and (fl == BC.DEAD).sum() == k - G
    if (k, G) == (8, 8) and N >= 17 and penalty == 64.0:  # the k best columns of the row in order: list depth k is reached
        best = np.lexsort((np.arange(N), -logits[0].astype(np.float64)))[:8]
        assert np.array_equal(token, best if ids is None else ids[best]) and np.array_equal(parent, np.arange(8))


def test_the_penalty_changes_the_picks_and_no_total():
    """on the reference alone: under penalty 0.5 the groups' picks differ from penalty 0, where they are k copies of one pick;
    a total is the parent's total plus the token score, whatever the penalty"""
    logits, totals, flags, eos, ids = _state(17, 8, 8, 3, True)
    zero, half = (GR.step(logits, totals, flags, 8, 8, p, eos, ids) for p in (0.0, 0.5))
    assert len(set(zero[1][:8].tolist())) == 1 and not np.array_equal(zero[1], half[1])
    live = half[1] != BC.NONE
    rows = np.arange(24) // 8 * 8 + half[0]
    assert np.array_equal(_bits(half[3][live]), _bits((totals[rows[live]] + half[2][live]).astype(np.float32)))
