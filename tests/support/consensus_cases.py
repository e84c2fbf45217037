"""The cases tests/test_gpu_consensus.py runs through slimt_hip_consensus_select* and compares with tests/support/
consensus_ref.py, and tests/test_consensus_case_fixtures.py proves able to catch the bugs they are for (CPU, reference only).
One table, like fanout_cases.py.

What the table is built around (slimt_amd/csrc/consensus.hip): one workgroup per source finds its rows in row_src (an ordered
compaction over 1024 rows a step), stages their tokens in LDS with a row stride of T + 3, gives each wave a row and half of
its partners (the cyclic split differs for odd and even row counts), walks a row 64 positions at a time (T = 63, 64, 65, 192,
256) and counts clipped matches by position. Rows of a source are mutations of one base sentence, so that they overlap
partly: unrelated random rows would all score 0 and any selection would pass."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

# ids [N, T] uint32, lens [N], row_src [N], B; orders: the (max_order, beta2) pairs the case runs at;
# flat: a case whose utilities are equal BY DESIGN (exempt from the fixture's "two distinct utilities", with the reason)
Case = namedtuple("Case", "name ids lens row_src B orders flat")
DEFAULT = ((4, 4),)
SWEEP = tuple((g, b2) for g in (1, 2, 3, 4) for b2 in (1, 4))


def _mutations(r, base, n, T, alphabet, keep=0.75, min_len=1):
    """n rows cut from `base`: each token kept with probability `keep`, else replaced or dropped; lengths in min_len..T"""
    rows = []
    for _ in range(n):
        row = []
        for t in base:
            u = r.random()
            if u < keep:
                row.append(int(t))
            elif u < keep + (1 - keep) / 2:
                row.append(int(r.choice(alphabet)))
        while len(row) < min_len:
            row.append(int(r.choice(alphabet)))
        rows.append(row[:T])
    return rows


def _pack(rows, T):
    ids = np.zeros((len(rows), T), np.uint32)
    lens = np.zeros(len(rows), np.uint32)
    for c, row in enumerate(rows):
        ids[c, :len(row)] = row
        lens[c] = len(row)
    return ids, lens


def _sources(seed, counts, T, alphabet_size=40, base_len=None, keep=0.75):
    """rows sorted by source: counts[b] mutations of source b's base sentence"""
    r = np.random.default_rng(seed)
    alphabet = np.arange(1, alphabet_size + 1)
    rows, src = [], []
    for b, n in enumerate(counts):
        L = base_len if base_len is not None else max(1, int(r.integers(max(1, T // 2), T + 1)))
        base = r.choice(alphabet, size=L)
        rows += _mutations(r, base, n, T, alphabet, keep)
        src += [b] * n
    ids, lens = _pack(rows, T)
    return ids, lens, np.asarray(src, np.uint32)


def _case(name, ids, lens, row_src, B, orders=DEFAULT, flat=None):
    ids = np.ascontiguousarray(ids, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint32)
    row_src = np.ascontiguousarray(row_src, np.uint32)
    assert ids.ndim == 2 and lens.shape == (ids.shape[0],) and row_src.shape == lens.shape
    assert (lens <= ids.shape[1]).all() and (row_src.size == 0 or int(row_src.max()) < B)
    return Case(name, ids, lens, row_src, B, orders, flat)


def _t_case(T, seed):
    """two sources of four and three rows at row length T: the first row of each is full length (the chunk boundary)"""
    if T == 1:  # (rows of one token: the minority token loses, and the second source's first row is the minority)
        return _case("T1", [[1], [1], [2], [1], [2], [1], [1]], np.ones(7, np.uint32), [0, 0, 0, 0, 1, 1, 1], 2)
    ids, lens, src = _sources(seed, [4, 3], T, alphabet_size=12, base_len=T, keep=0.85)
    r = np.random.default_rng(seed + 1)
    for c in (0, 4):  # a full row: its last grams end at T exactly
        ids[c] = np.where(np.arange(T) < lens[c], ids[c], r.integers(1, 13, size=T))
        lens[c] = T
    return _case("T%d" % T, ids, lens, src, 2)


def _wide():
    """ids at 0, 65535, 65536, 2^32 - 1; 5 and 65536 + 5 agree in their low 16 bits and are different tokens"""
    a, b, c, d, lo, hi = 0, 65535, 65536, 2 ** 32 - 1, 5, 65536 + 5
    rows = [[a, b, c, d, lo, a, b], [a, b, c, d, hi, a, b], [d, c, lo, a, b, c], [b, b, hi, d, a, 0, 0, c]]
    ids, lens = _pack(rows, 8)
    return _case("wide_ids", ids, lens, np.zeros(4, np.uint32), 1, SWEEP)


def _order5(seed=23):
    """five sources, 3..6 rows each: sorted, reversed and shuffled row orders of the same rows"""
    ids, lens, src = _sources(seed, [4, 6, 3, 5, 4], 20, alphabet_size=15, keep=0.7)
    perm = np.random.default_rng(seed).permutation(src.size)
    rev = np.arange(src.size)[::-1].copy()
    return (_case("order5_sorted", ids, lens, src, 5, SWEEP), _case("order5_reversed", ids[rev], lens[rev], src[rev], 5),
            _case("order5_shuffled", ids[perm], lens[perm], src[perm], 5), perm)


def _b300(seed=31):
    """300 sources of 1..3 rows in a shuffled order: more workgroups than compute units, rows found across the whole array"""
    r = np.random.default_rng(seed)
    ids, lens, src = _sources(seed, list(r.integers(1, 4, size=300)), 12, alphabet_size=9, keep=0.7)
    perm = r.permutation(src.size)
    return _case("b300", ids[perm], lens[perm], src[perm], 300)


@lru_cache(maxsize=None)
def table():
    out = []
    one = _sources(3, [1], 5)
    out.append(_case("n1", *one, 1))
    out.append(_case("two_rows", *_sources(4, [2], 9, alphabet_size=6), 1, SWEEP))
    out.append(_case("three_rows", *_sources(5, [3], 11, alphabet_size=6), 1, SWEEP))
    # source 0: one row (utility 0, best is that row); 1: none; 2: only empty rows; 3: three rows and an empty one between
    ids, lens, src = _sources(6, [1, 0, 2, 4], 7, alphabet_size=6)
    lens[1] = lens[2] = lens[4] = 0
    out.append(_case("lone_none_empty", ids, lens, src, 4))
    # rows of 1, 2 and 3 tokens beside longer ones at G = 4: orders are skipped per pair
    rows = [[3], [3, 4], [3, 4, 5], [3, 4, 5, 6], [4, 5, 6, 3, 4], [5, 3], [3, 4, 3]]
    out.append(_case("short_rows", *_pack(rows, 5), np.zeros(7, np.uint32), 1, SWEEP))
    for T, seed in ((1, 7), (5, 9), (63, 9), (64, 10), (65, 11), (192, 8), (256, 13)):  # (seeds: the fixture test's conditions hold)
        out.append(_t_case(T, seed))
    out.append(_case("alpha3", *_sources(14, [5, 4], 40, alphabet_size=3, base_len=40, keep=0.6), 2, SWEEP))
    ident = np.tile(np.array([[7, 8, 9, 7, 8, 2, 7]], np.uint32), (5, 1))
    out.append(_case("identical", ident, np.full(5, 7, np.uint32), np.zeros(5, np.uint32), 1,
                     flat="all rows are one sentence: every utility is 1 by definition"))
    out.append(_wide())
    # rows 1 and 2 are one sentence and the source's top two: an exact tie, the lower row wins
    rows = [[9, 1, 2, 3, 9, 9], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [1, 2, 3, 7, 8]]
    out.append(_case("tie", *_pack(rows, 6), np.zeros(4, np.uint32), 1, ((4, 4), (2, 1))))
    out.append(_case("rows64", *_sources(15, [64], 24, alphabet_size=10, keep=0.7), 1))
    out.extend(_order5()[:3])
    out.append(_b300())
    return {c.name: c for c in out}


def names():
    return list(table())


def runs():
    """(case name, max_order, beta2) of every run"""
    return [(c.name, g, b2) for c in table().values() for g, b2 in c.orders]


def shuffle_permutation():
    """order5_shuffled's row c is order5_sorted's row perm[c]"""
    return _order5()[3]


def rows65():
    """rows64 and one more row of the same source: refused by the host call"""
    c = table()["rows64"]
    return (np.concatenate([c.ids, c.ids[:1]]), np.concatenate([c.lens, c.lens[:1]]),
            np.concatenate([c.row_src, c.row_src[:1]]), c.B)


@lru_cache(maxsize=None)
def reference(name, max_order=4, beta2=4):
    """(utility, best) of a case by tests/support/consensus_ref.py, computed once and shared (do not write to them)"""
    from support import consensus_ref
    c = table()[name]
    u, b = consensus_ref.select(c.ids, c.lens, c.row_src, c.B, max_order, beta2)
    u.setflags(write=False)
    b.setflags(write=False)
    return u, b
