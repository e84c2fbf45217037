"""The cases of tests/support/consensus_cases.py can catch the bugs they are for: shown on the CPU with the reference alone
(tests/support/consensus_ref.py). These are conditions on the inputs, not tolerances: a case whose rows all score alike, or
whose best row is always the first, passes a selection that does nothing."""
import numpy as np
import pytest

from support import consensus_cases as CC
from support import consensus_ref as R


def _rows_of_source(c, b):
    return [r for r in range(c.row_src.size) if int(c.row_src[r]) == b]


@pytest.mark.parametrize("name", CC.names())
def test_sources_with_three_or_more_rows_have_two_distinct_utilities(name):
    c = CC.table()[name]
    if c.flat:
        assert isinstance(c.flat, str) and len(c.flat) > 10  # (exempt, with its reason)
        return
    for G, b2 in c.orders:
        util, _ = CC.reference(name, G, b2)
        for b in range(c.B):
            rows = _rows_of_source(c, b)
            if len(rows) >= 3:
                assert len({float(util[r]) for r in rows}) >= 2, (name, G, b2, b)


@pytest.mark.parametrize("name", [n for n in CC.names() if CC.table()[n].B > 1])
def test_in_multi_source_cases_some_best_row_is_not_the_sources_first(name):
    c = CC.table()[name]
    for G, b2 in c.orders:
        _, best = CC.reference(name, G, b2)
        firsts = [_rows_of_source(c, b)[:1] for b in range(c.B)]
        assert any(f and int(best[b]) not in (f[0], R.NO_ROW) for b, f in enumerate(firsts)), (name, G, b2)


def _top_two_tie(c, util):
    for b in range(c.B):
        rows = [r for r in _rows_of_source(c, b) if c.lens[r] > 0]
        top = sorted((float(util[r]) for r in rows), reverse=True)
        if len(top) >= 3 and top[0] == top[1] > top[2]:
            return True
    return False


def test_some_case_has_an_exact_tie_between_a_sources_top_two_rows():
    c = CC.table()["tie"]
    for G, b2 in c.orders:
        util, best = CC.reference("tie", G, b2)
        assert _top_two_tie(c, util), (G, b2)
        assert int(best[0]) == 1 and util[1] == util[2]  # (the lower of the two)


def test_some_case_has_tokens_that_differ_only_above_bit_16_and_would_otherwise_match():
    c = CC.table()["wide_ids"]
    assert {0, 65535, 65536, 2 ** 32 - 1} <= {int(t) for t in c.ids.ravel()}
    low = CC.Case(c.name, c.ids & 0xFFFF, c.lens, c.row_src, c.B, c.orders, c.flat)
    changed = 0
    for G, b2 in c.orders:
        want = CC.reference("wide_ids", G, b2)
        got = R.select(low.ids, low.lens, low.row_src, low.B, G, b2)  # (what a 16-bit comparison would compute)
        changed += not np.array_equal(R.bits(want[0]), R.bits(got[0]))
    assert changed == len(c.orders)


def test_the_shuffled_order_is_a_permutation_of_the_sorted_one_and_no_source_ties_at_the_top():
    """so the shuffled result must equal the sorted one mapped through the permutation, the best rows included"""
    s, sh, perm = CC.table()["order5_sorted"], CC.table()["order5_shuffled"], CC.shuffle_permutation()
    assert np.array_equal(sh.ids, s.ids[perm]) and np.array_equal(sh.row_src, s.row_src[perm])
    assert not np.array_equal(perm, np.arange(perm.size))
    util, best = CC.reference("order5_sorted")
    for b in range(s.B):
        rows = _rows_of_source(s, b)
        top = sorted((float(util[r]) for r in rows), reverse=True)
        assert top[0] > top[1], b  # (no tie: the winner does not depend on the row order)
    # rows of one source in different relative orders: the sums are added in another order, the bits may differ; the test on
    # the device compares each order with the reference computed in that order
    assert any(list(np.argsort(perm)[_rows_of_source(s, b)]) != sorted(np.argsort(perm)[_rows_of_source(s, b)]) for b in range(s.B))


def test_the_table_covers_the_shapes_the_kernel_takes_other_paths_at():
    t = CC.table()
    assert {t["T%d" % T].ids.shape[1] for T in (1, 5, 63, 64, 65, 192, 256)} == {1, 5, 63, 64, 65, 192, 256}
    for T in (63, 64, 65, 192, 256):  # a full row and a shorter one per source
        c = t["T%d" % T]
        assert int(c.lens.max()) == T and int(c.lens.min()) < T
    assert t["n1"].row_src.size == 1 and t["two_rows"].row_src.size == 2 and t["three_rows"].row_src.size == 3
    c = t["lone_none_empty"]
    counts = np.bincount(c.row_src, minlength=c.B)
    assert counts[0] == 1 and counts[1] == 0 and (c.lens[c.row_src == 2] == 0).all() and (c.lens[c.row_src == 3] == 0).any()
    assert sorted(int(n) for n in t["short_rows"].lens)[:3] == [1, 2, 2] and 3 in t["short_rows"].lens
    assert len({int(x) for x in t["alpha3"].ids.ravel()} - {0}) == 3
    assert np.bincount(t["rows64"].row_src)[0] == 64 and np.bincount(CC.rows65()[2])[0] == 65
    b300 = t["b300"]
    counts = np.bincount(b300.row_src, minlength=300)
    assert b300.B == 300 and counts.min() >= 1 and counts.max() <= 3 and {1, 2, 3} <= set(counts.tolist())
    assert sorted(CC.SWEEP) == [(g, b2) for g in (1, 2, 3, 4) for b2 in (1, 4)]
