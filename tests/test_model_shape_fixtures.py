"""The translate comparisons of tests/test_gpu_model_shapes.py must not be vacuous: with an unlucky EOS bias a random model
ends every sentence at step 1 (the comparison then checks one step) or never emits EOS (no EOS bookkeeping is checked). Each
shape of the table carries an eos_bias and a seed chosen on the CPU; this test holds every translate case of the table (but
the few batches the table lists as degenerate) to conditions on the PORTABLE oracle's own output -- conditions on the inputs, nothing measured on the device."""
import numpy as np
import pytest

from support import model_shapes as T


def fixture_problems(B, out, ln, steps):
    """What is wrong with a greedy batch as a test input ([] = nothing). B = 21: at least half of the sentences record 4
    or more tokens, at least one ends early with EOS, at least 3 distinct lengths, at least 8 distinct token ids. B = 5 (five
    sentences often cannot meet those): some sentence records 4 or more tokens and the lengths are not all equal."""
    ln = np.asarray(ln).astype(np.int64)
    bad = []
    if B < 21:
        if not (ln >= 4).any():
            bad.append("no sentence records 4 tokens")
        if np.unique(ln).size < 2:
            bad.append("all lengths equal")
        return bad
    if 2 * int((ln >= 4).sum()) < B:
        bad.append("fewer than half of the sentences record 4 tokens: %s" % ln.tolist())
    if not (ln < steps).any():
        bad.append("no sentence ends early with EOS")
    if np.unique(ln).size < 3:
        bad.append("fewer than 3 distinct lengths: %s" % ln.tolist())
    tokens = np.unique(np.concatenate([out[b, : ln[b]] for b in range(B)]))
    if tokens.size < 8:
        bad.append("only %d distinct token ids" % tokens.size)
    return bad


@pytest.mark.parametrize("s", T.SHAPES, ids=T.shape_id)
def test_translate_cases_are_not_degenerate(oracle, s):
    """Every translate case of the grid (S > 1) meets the conditions, except the batches T.DEGENERATE names -- which do not
    (the list is exact, so it cannot grow unnoticed), and none of which is one of the shape's vouched cases."""
    om = oracle.OracleModel(T.make(s))
    listed = {c for dims, c in T.DEGENERATE if dims == s.dims}
    assert not listed & set(T.vouched_cases(s)), listed
    assert listed <= set(T.cases(s)), listed
    problems, fine = {}, []
    for B, S in T.cases(s):
        if S == 1:
            continue
        _, _, _, out, ln, _, steps = T.translate_reference(oracle, om, s, B, S)
        bad = fixture_problems(B, out, ln, steps)
        if bad and (B, S) not in listed:
            problems[(B, S)] = bad
        if not bad and (B, S) in listed:
            fine.append((B, S))
    assert not problems, (T.shape_id(s), s.eos_bias, s.seed, problems)
    assert not fine, ("listed as degenerate, but meets the conditions", T.shape_id(s), fine)


def test_the_table_covers_the_accepted_family():
    """At least 20 shapes, at least 12 of them with a D, F, H, Le or Ld no preset has; no shape twice; every class present;
    every plan combination that exists among the accepted shapes is in the table: (1, 1), (1, 0), (0, 0) and (0, 1)."""
    assert len(T.SHAPES) >= 20 and len({s.dims for s in T.SHAPES}) == len(T.SHAPES)
    unusual = [s for s in T.SHAPES if any(v not in T.PRESET_VALUES[i] for i, v in enumerate(s.dims[:5]))]
    assert len(unusual) >= 12, len(unusual)
    assert {s.cls for s in T.SHAPES} == {1, 2, 3, 4, 5}
    assert all(any(S == 70 for _, S in T.cases(s)) for s in T.SHAPES if s.cls == 3)
    assert all(any(S == 70 for _, S in T.vouched_cases(s)) for s in T.SHAPES if s.cls == 3)
    assert all(set(T.vouched_cases(s)) <= set(T.cases(s)) for s in T.SHAPES)
    assert len(T.DEGENERATE) <= 12 and all(any(d == s.dims for s in T.SHAPES) for d, _ in T.DEGENERATE)
    reached = {T.expected_plan(s, S) for s in T.SHAPES for _, S in T.cases(s)}
    assert reached == {(True, True), (True, False), (False, False), (False, True)}, reached
    assert {s.dims[5] for s in T.SHAPES} >= {517, 1003}
