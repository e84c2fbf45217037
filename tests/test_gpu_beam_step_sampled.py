"""slimt_hip_beam_step_sampled on the device against `step_sampled_host` (tests/support/beam_sampled_ref.py: every column
of every live slot perturbed, sorted and conditioned by brute force), bit for bit: parent, token, token score, totals,
perturbed values, flags. N = 1 (one column), 7 (fewer columns than k = 8), 257 (more than one pass of a slot's waves at
k = 8, ragged), 4097 (many passes and one column over); k = 1, 3, 8; with and without an ids array."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_sampled_ref as SB
from test_sampling_checker import keys_of

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(hip, logits, totals, G, flags, k, keys, step, eos, ids):
    got = hip.beam_step_sampled(logits, totals, G, flags, k, keys, step, eos, ids)
    want = SB.step_sampled_host(logits, totals, G, flags, k, keys, step, eos, ids)
    for g, w, name in zip(got, want, ("parent", "token", "token_score", "totals", "perturbed", "flags")):
        same = np.array_equal(_bits(g), _bits(w)) if g.dtype == np.float32 else np.array_equal(g, w)
        assert same, (name, g, w)
    return want


def crafted(N, k, with_ids):
    """B = 5 sources: the step-0 state; live, finished and dead slots with a finished slot whose G beats every child; a row
    with -inf columns; unusable rows (a NaN, all -inf); EOS among the winners -- as far as k and N allow"""
    r = np.random.default_rng(100 * N + k)
    B, R = 5, 5 * k
    logits = (np.round(r.normal(0, 3, size=(R, N)) * 4) / 4).astype(np.float32)
    totals = -np.round(r.uniform(0, 6, size=R) * 2).astype(np.float32) / 2
    G = (totals + np.round(r.uniform(-2, 3, size=R) * 8).astype(np.float32) / 8).astype(np.float32)
    flags = np.full(R, BC.LIVE, np.uint32)
    ids = r.permutation(N).astype(np.uint32) if with_ids else None
    eos = 0
    eos_col = 0 if ids is None else int(np.nonzero(ids == eos)[0][0])
    rows = lambda b: np.arange(b * k, (b + 1) * k)
    totals[rows(0)], G[rows(0)], flags[rows(0)] = SB.start_state(1, k)
    if k >= 3:
        flags[rows(1)[1]], G[rows(1)[1]] = BC.FINISHED, 50.0   # ahead of every child: a child's value never exceeds its parent's
        flags[rows(1)[2]], totals[rows(1)[2]], G[rows(1)[2]] = BC.DEAD, -np.inf, -np.inf
    logits[rows(2)[0], N // 2:] = -np.inf
    logits[rows(3)[0], N // 2] = np.nan
    logits[rows(3)[-1]] = -np.inf
    logits[rows(4)[0], eos_col], G[rows(4)[0]] = 40.0, 40.0  # (the slot's best column by far, and the source's best slot)
    return logits, totals, G, flags, keys_of(11 + N + k, B), eos, ids


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 7, 257, 4097])
def test_step_equals_the_brute_force_checker(hip, N, k, with_ids):
    logits, totals, G, flags, keys, eos, ids = crafted(N, k, with_ids)
    parent, token, score, tot, pert, fl = _check(hip, logits, totals, G, flags, k, keys, 3, eos, ids)
    assert np.all(parent[:k][fl[:k] != BC.DEAD] == 0)       # the step-0 state: every new slot comes from slot 0
    assert token[4 * k] == eos and fl[4 * k] == BC.FINISHED and pert[4 * k] == 40.0  # EOS among the winners
    live = fl != BC.DEAD
    assert np.all(pert[live] <= 50.0) and np.isneginf(pert[~live]).all()
    if k >= 3:
        assert token[k] == BC.NONE and parent[k] == 1 and pert[k] == 50.0  # the finished slot first
        assert 0 not in parent[3 * k:4 * k] and k - 1 not in parent[3 * k:4 * k]  # unusable rows contribute nothing


def test_the_draw_statistics_batch(hip):
    """the 8192-key batch of tests/test_beam_sampled_checker.py, whose frequencies are proven there on the restatement"""
    n, k, N = 8192, 2, 8
    totals, G, flags = SB.start_state(n, k)
    rows = np.zeros((n * k, N), np.float32)
    rows[0::k] = np.linspace(0, 2.1, N).astype(np.float32)
    _check(hip, rows, totals, G, flags, k, keys_of(7, n), 0, 99, None)
