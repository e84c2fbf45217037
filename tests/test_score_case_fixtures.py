"""The cases of tests/support/score_cases.py must be worth running: this module holds them, with the oracle alone and plain
arithmetic, to conditions on the INPUTS -- nothing here is measured on a device, and nothing calls the library's predicates.

  * every instantiation of the scorer's kernels is reached by some shape of the family, every decoder depth 1 .. 5 occurs and
    at least two full vocabularies are no multiple of 16;
  * the (B, T) pairs sit on and next to every row count at which the tall path changes tiling, and the chunk cases split as
    the table says;
  * where a case draws its targets from the output layer's ids every reference score is finite, and where it places
    missing tokens on purpose the checker's -inf entries are exactly those;
  * the greedy option cases are vouched cases of their shape and meet test_model_shape_fixtures.py's conditions."""
import numpy as np
import pytest

from support import model_shapes as MS
from support import score_cases as C
from test_forced_prefix_checker import forced_translate, tmax_of
from test_model_shape_fixtures import fixture_problems


def _minus_inf(sc, t_len):
    return {(b, t) for b in range(len(t_len)) for t in range(int(t_len[b])) if np.isneginf(sc[b, t])}


def _worth_running(oracle, m, om, c):
    """the checker's -inf set is exactly the intended one, every other live score is finite, and nothing else is written"""
    sc, al, peaks = C.reference(oracle, m, om, c)
    assert _minus_inf(sc, c.t_len) == c.minus_inf
    for b in range(len(c.t_len)):
        n = int(c.t_len[b])
        live = sc[b, :n]
        assert np.all(np.isfinite(live[~np.isneginf(live)])), b
        assert np.all(live <= 0.0), b
        assert np.all(np.isnan(sc[b, n:])), b
    assert peaks.shape[0] == int(np.max(c.t_len, initial=0))
    return sc


def test_every_instantiation_depth_and_odd_width_is_in_the_family():
    """(emb / 64, head size) of every shape, by hand: score_scan_kernel and score_out_kernel are instantiated on the first
    (1, 2, 4, 8), score_attn_kernel on the second (16, 32, 64). Head size 16 at emb 512 would need 32 heads, which
    model_create refuses: eleven pairs exist."""
    pairs = {(s.dims[0] // 64, s.dims[0] // s.dims[2]) for s in MS.SHAPES}
    assert pairs == {(k, h) for k in (1, 2, 4) for h in (16, 32, 64)} | {(8, 32), (8, 64)}, sorted(pairs)
    assert {s.dims[4] for s in MS.SHAPES} == {1, 2, 3, 4, 5}
    assert len({s.dims[5] for s in MS.SHAPES if s.dims[5] % 16}) >= 2
    # the long case is above 64 source tokens and both cases' T is odd and above what the forced-prefix path takes at S = 13
    B, S, T, _ = C.SHAPE_CASES["short"]
    assert T % 2 == 1 and T > tmax_of(S)
    assert C.SHAPE_CASES["long"][1] > 64 and C.SHAPE_CASES["long"][3] is None
    # the edge models' head sizes
    assert [C.dims_of(n)[0] // C.dims_of(n)[2] for n in C.SOURCE_MODELS] == [16, 32, 64]


def test_row_counts_sit_on_every_switch():
    assert [B * T for B, T in C.ROW_CASES] == list(C.ROW_COUNTS)
    assert C.ROW_COUNTS == tuple(n + d for n in (128, 512, 1024, 2048, 4096) for d in (-1, 0, 1))
    for rows in (128, 1024, 2048):
        assert any(B * T == rows and B > 1 for B, T in C.ROW_CASES), rows
    # odd counts: sentences that are no multiple of a 16-row tile, so that they straddle tiles and 128-row blocks
    assert all(T % 16 for B, T in C.ROW_CASES if (B * T) % 2 and B > 1)
    assert sorted(B * T for B, T in C.TINY_ROW_CASES) == [1024, 1025]
    # dead tiles and blocks (T = 300): a 128-row block without a live row, a live block with dead 16-row tiles, and a
    # sentence whose last live row is not the last row of its tile
    T, n = C.DEAD_T, C.DEAD_LEN
    live = np.zeros(C.DEAD_B * T, bool)
    for b in range(C.DEAD_B):
        live[b * T: b * T + n[b]] = True
    pad = np.zeros(-(-live.size // 128) * 128, bool)
    pad[:live.size] = live
    blocks = pad.reshape(-1, 8, 16).any(axis=2)
    assert (~blocks.any(axis=1)).any()
    assert (blocks.any(axis=1) & ~blocks.all(axis=1)).any()
    assert any((b * T + n[b]) % 16 != 0 for b in range(C.DEAD_B) if n[b])


def test_chunk_cases_split_as_written():
    """chunks hold max(1, 8192 // T) whole sentences"""
    for B, T, want in C.CHUNK_CASES:
        spc = max(1, C.CHUNK_ROWS // T)
        assert [min(spc, B - b0) for b0 in range(0, B, spc)] == want, (B, T)
    assert {T for _, T, _ in C.CHUNK_CASES} >= {8191, 8192, 8193}
    assert any(len(w) > 1 and w[0] > 1 and w[0] * T <= C.CHUNK_ROWS < (w[0] + 1) * T for _, T, w in C.CHUNK_CASES)


def test_search_lists_and_width_cases_are_what_they_claim():
    assert {64, 65, 64 * 64 - 1, 64 * 64, 64 * 64 + 1} <= set(C.SEARCH_SIZES)
    for N in C.SEARCH_SIZES:
        sl = C.search_shortlist(N)
        assert len(sl) == N and np.all(np.diff(sl.astype(np.int64)) > 0)
        assert sl[0] >= C.SEARCH_EDGE and sl[-1] < C.SEARCH_V - C.SEARCH_EDGE
        toks, present = C.search_tokens(sl)
        assert np.array_equal(np.sort(toks[present]), sl)  # every entry once
        absent = toks[~present]
        assert sl[0] - 1 in absent and sl[-1] + 1 in absent
        gaps = [t for t in absent if t - 1 in sl]  # (the id above sl[N - 1] is one of them)
        assert len(gaps) >= 64, (N, len(gaps))
        assert toks.max() < C.SEARCH_V
        c = C.search_inputs(N)
        assert len(c.minus_inf) == len(absent)
        ids, ln, sl2, p_ids, p_len, ok = C.search_prefix_inputs(N, tmax_of(C.SEARCH_PREFIX_S))
        assert np.array_equal(sl2, sl) and np.array_equal(np.isin(p_ids, sl), ok) and (~ok).sum() == len(absent)
        assert np.array_equal(np.unique(p_ids[ok]), sl) and not (p_ids == 0).any()
    for name, n in C.WIDTH_CASES:
        c = C.width_inputs(name, n)
        N = C.dims_of(name)[5] if n is None else n
        assert c.t_ids.shape == (C.WIDTH_B, N) and np.all(c.t_len == N)
        cols = np.arange(N) if c.sl is None else c.sl
        assert all(np.array_equal(np.sort(row), cols) for row in c.t_ids)  # every column is some row's target
    widths = [C.dims_of(name)[5] if n is None else n for name, n in C.WIDTH_CASES]
    assert widths == [8, 16, 24, 48, 56, 64, 72, 512, 517]
    # a missing token at t = 0, on a sentence's last row, on every row of a sentence, on the row that ends a 128-row block
    at, n, T = set(C.MISSING_AT), C.MISSING_LEN, C.MISSING_T
    assert any(t == 0 for _, t in at) and any(t == n[b] - 1 for b, t in at)
    assert any(all((b, t) in at for t in range(n[b])) for b in range(C.MISSING_B) if n[b])
    assert any((b * T + t) % 128 == 127 for b, t in at)
    assert all((b, t + 1) not in at for b, t in at if b != 2 and t + 1 < n[b])  # ... and a live row follows them


@pytest.mark.parametrize("s", MS.SHAPES, ids=MS.shape_id)
def test_shape_cases_score_finite_and_option_cases_are_vouched(oracle, s):
    m = MS.make(s)
    om = oracle.OracleModel(m)
    for kind in C.SHAPE_CASES:
        c = C.shape_inputs(s, kind)
        B, S, T, _ = C.SHAPE_CASES[kind]
        assert c.lens[0] == 0 and c.lens[-1] == S
        assert sorted(c.t_len.tolist()) == C.spread(B, T) and 0 in c.t_len and T in c.t_len
        assert (c.sl is None) == (kind == "long")
        _worth_running(oracle, m, om, c)
    assert set(C.OPTION_CASES) <= set(MS.vouched_cases(s))
    for B, S in C.OPTION_CASES:
        ids, lens, sl = C.option_inputs(s, B, S)
        assert (sl is None) == (S == 32)
        r_ids, r_lens, r_sl, out, ln, _, steps = MS.translate_reference(oracle, om, s, B, S)
        assert np.array_equal(r_ids, ids) and np.array_equal(r_lens, lens)  # the batch that is vouched for
        assert not fixture_problems(B, out, ln, steps), (B, S)
        # forced: full-length targets from the layer's ids, prefix lengths 0 .. Tmax; every score finite
        Tm = tmax_of(S)
        assert steps == Tm
        p_ids, p_len = C.option_prefix(s, B, S, sl, Tm)
        assert p_len[0] == 0 and p_len[-1] == Tm and not (p_ids == 0).any()
        f_out, f_ln, _, f_sc = forced_translate(oracle, om, m, ids, lens, sl, p_ids, p_len)
        assert all(np.all(np.isfinite(f_sc[b, :f_ln[b]])) for b in range(B))
        assert all(np.array_equal(f_out[b, :p_len[b]], p_ids[b, :p_len[b]]) for b in range(B))
        assert C.option_modes(s, S) == (0, 1) + ((2,) if s.plan[2] else ())


_MODELS = {}


@pytest.mark.parametrize("case", C.EDGE_CASES, ids=C.edge_id)
def test_edge_cases_score_finite_or_minus_inf_where_intended(oracle, case):
    kind, name, arg = case
    if name not in _MODELS:
        m = C.make_model(name)
        _MODELS[name] = (m, oracle.OracleModel(m))
    m, om = _MODELS[name]
    c = C.edge_inputs(case)
    assert c.t_ids.max() < m.V and np.all(c.lens <= c.ids.shape[1]) and np.all(c.t_len <= c.t_ids.shape[1])
    if kind == "source":
        assert sorted(set(c.lens.tolist())) == sorted(set(C.source_length_lens(arg))) and len(c.lens) == C.SOURCE_B
        assert {0, 1, arg, arg - 1} <= set(c.lens.tolist()) and (arg <= 64 or {64, 65} <= set(c.lens.tolist()))
    if kind == "rows":
        assert c.t_len[-1] == c.t_ids.shape[1]  # the call's last row is live
    if kind in ("missing", "search"):
        assert c.minus_inf
    else:
        assert not c.minus_inf
    _worth_running(oracle, m, om, c)


def test_search_prefixes_score_minus_inf_exactly_at_the_absent_ids(oracle):
    """the forced-prefix form of the column search (smallest and largest list): the checker records every forced token, scores
    -inf exactly at the absent ones and runs every sentence to Tmax"""
    m = C.make_model("v8192")
    om = oracle.OracleModel(m)
    Tm = tmax_of(C.SEARCH_PREFIX_S)
    for N in (C.SEARCH_SIZES[0], C.SEARCH_SIZES[-1]):
        ids, lens, sl, p_ids, p_len, ok = C.search_prefix_inputs(N, Tm)
        out, ln, _, sc = forced_translate(oracle, om, m, ids, lens, sl, p_ids, p_len)
        assert np.all(ln == Tm) and np.array_equal(out, p_ids)
        assert np.array_equal(np.isneginf(sc), ~ok) and np.all(np.isfinite(sc[ok]))
