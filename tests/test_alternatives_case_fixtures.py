"""The cases of tests/support/alternatives_cases.py are worth comparing (CPU): for every case and every k of KS the targets
built on the oracle put at least a quarter of the live rows below rank k and a quarter at or above it, one row at rank
exactly k - 1 and one at exactly k, and -- where the output layer is a shortlist: the full vocabulary has no id outside it
-- at least one row outside the layer. Also: the checker's results for k are the first k of those for 8."""
import numpy as np
import pytest

from support import alternatives_cases as AC


@pytest.mark.parametrize("name", AC.case_names())
def test_case_reaches_both_sides_of_every_k(oracle, name):
    c = AC.build(oracle, name)
    lv = AC.live(c)
    n = int(lv.sum())
    assert n >= 16 and np.all(c.alt.rank[~lv] == AC.NONE)
    rank = c.alt.rank[lv].astype(np.int64)
    inside = rank != AC.NONE
    N = c.m.V if c.sl is None else len(c.sl)
    assert np.all(rank[inside] < N)
    if c.sl is not None:
        assert (~inside).sum() >= 1, "no target outside the layer"
        assert not np.isin(c.t_ids[lv][~inside], c.sl).any()
    else:
        assert inside.all()
    for k in AC.KS:
        below = int((rank < k).sum())
        above = int((inside & (rank >= k)).sum())
        print(name, "k", k, "live rows", n, "rank < k:", below, "rank >= k:", above, "outside:", int((~inside).sum()))
        assert 4 * below >= n and 4 * above >= n, (k, below, above, n)
        assert (rank == k - 1).any() and (rank == k).any(), k
    # rank < 8 <=> the target is the alternative at that place
    for b, t in zip(*np.nonzero(lv)):
        r = int(c.alt.rank[b, t])
        if r < 8:
            assert c.alt.ids[b, t, r] == c.t_ids[b, t]
        else:
            assert c.t_ids[b, t] not in c.alt.ids[b, t]
    assert np.all(c.alt.ids[lv] != AC.NONE) and np.all(np.isfinite(c.alt.scores[lv]))  # (every layer here has >= 8 columns)


def test_alternatives_for_k_are_the_first_k_of_those_for_eight(oracle):
    from test_alternatives_checker import alternatives
    c = AC.build(oracle, "emb64")
    om = oracle.OracleModel(c.m)
    for k in (1, 5):
        a = alternatives(oracle, om, c.m, c.ids, c.lens, c.sl, c.t_ids.copy(), c.t_len, k)
        w_ids, w_sc, w_rank = AC.expected(c, k)
        assert np.array_equal(a.ids, w_ids) and np.array_equal(a.scores, w_sc, equal_nan=True) and np.array_equal(a.rank, w_rank)
