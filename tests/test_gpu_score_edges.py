"""GPU parity of teacher-forced scoring (slimt_hip_score) at the edges where its tall kernels switch, on the smallest models
that reach each edge (tests/support/score_cases.py; tests/test_score_case_fixtures.py proves on the CPU that the cases sit
where they claim): source lengths around the attention kernel's second key register and its limit of 128; target row counts
on and next to every change of tiling; dead 16-row tiles and 128-row blocks; more than one chunk; output layers narrower than
one column tile per wave; the 64-ary column search at the sizes where it takes another round, through the scorer and through
the forced-prefix decoders that share it; missing tokens. The reference is always the checker in the oracle's PORTABLE
order -- never another device result: alignment rows bit for bit, scores within model_values.score_bound, -inf exactly where
the checker has it, unwritten entries untouched."""
import numpy as np
import pytest

from support import score_cases as C
from support.model_values import Recording
from test_forced_prefix_checker import forced_translate, tmax_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(hip, oracle):
    """(synthetic model, device model, oracle model) per model of score_cases.MODELS, created once for the module"""
    cache = {}

    def get(name):
        if name not in cache:
            m = C.make_model(name)
            cache[name] = (m, hip.Model(m), oracle.OracleModel(m))
        return cache[name]

    try:
        yield get
    finally:
        for _, gm, _ in cache.values():
            gm.close()


def _params(kind):
    return [pytest.param(c, id=C.edge_id(c)) for c in C.edges_of(kind)]


def _run(hip, oracle, engines, case, ctx=None):
    """one case of the table against the checker, with the alignment"""
    m, gm, om = engines(case[1])
    c = C.edge_inputs(case)
    ref = C.reference(oracle, m, om, c)
    B, S = c.ids.shape
    own = ctx is None
    ctx = ctx or hip.Context(gm, B, S)
    try:
        got = ctx.score(c.ids, c.lens, c.sl, c.t_ids, c.t_len, want_align=True, fill=C.FILL)
        C.check_case(got, ref, c)
    finally:
        if own:
            ctx.close()
    return c, ref, got


@pytest.mark.parametrize("case", _params("source"))
def test_source_lengths(hip, oracle, engines, case):
    """S = 1, 2, 3, 5, 63, 64, 65, 127, 128 on head sizes 16, 32 and 64; B 6, T 5; source lengths 0, 1, S - 1, S, and 64 and 65
    where S is above 64. Alignment columns at and beyond lens[b] keep the fill (check_align)."""
    _run(hip, oracle, engines, case)


@pytest.mark.parametrize("name", C.SOURCE_MODELS)
def test_129_source_tokens_are_refused_and_128_still_scored(hip, oracle, engines, name):
    """Host-side argument checks (nothing is launched). No context can hold 129 source tokens: slimt_hip_ctx_create refuses a
    max_source_length above 128 (tests/test_gpu_engine.py holds it to that), so the scorer's own "no scoring kernels" refusal
    of S > 128 cannot be reached through the C ABI -- a batch of 129 tokens is refused one check earlier, as exceeding the
    context. Both refusals are asserted; the context of 128 tokens then scores the S = 128 batch."""
    m, gm, _ = engines(name)
    c = C.source_length_inputs(name, 128)
    with pytest.raises(hip.SlimtHipError, match="max_source_length 129 > 128"):
        hip.Context(gm, C.SOURCE_B, 129)
    ctx = hip.Context(gm, C.SOURCE_B, 128)
    try:
        ids = np.ones((C.SOURCE_B, 129), np.uint32)
        with pytest.raises(hip.SlimtHipError, match="exceeds the context workspace"):
            ctx.score(ids, np.full(C.SOURCE_B, 129, np.uint32), c.sl, c.t_ids, c.t_len, want_align=True, fill=C.FILL)
        _run(hip, oracle, engines, ("source", name, 128), ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", _params("rows"))
def test_row_counts(hip, oracle, engines, case):
    """B * T = 127 .. 4097 rows on micro and mini, 1024 and 1025 on tiny11: the 128-row GEMM tiles from 1024 rows, the row
    blocks that change at 512, 2048 and 4096, one output-layer workgroup per 128 rows"""
    _run(hip, oracle, engines, case)


@pytest.mark.parametrize("case", _params("dead"))
def test_dead_tiles_and_blocks(hip, oracle, engines, case):
    """T = 300, target lengths 300, 0, 5, 300, 130, 17: scores and alignments are the checker's, everything else the fill"""
    c, _, got = _run(hip, oracle, engines, case)
    assert int((got[0] != C.FILL).sum()) == int(c.t_len.sum())


@pytest.mark.parametrize("case", _params("chunk"))
def test_chunks(hip, oracle, engines, case):
    """more than 8192 rows: one sentence per chunk at T = 8191, 8192, 8193; 2 + 1, 2 + 2 and 3 + 1 sentences"""
    _run(hip, oracle, engines, case)


@pytest.mark.parametrize("case", _params("width"))
def test_output_layer_widths(hip, oracle, engines, case):
    """shortlists of 8 .. 72 ids and the full vocabularies of 512 and 517: every column is a target of both sentences"""
    _run(hip, oracle, engines, case)


@pytest.mark.parametrize("case", _params("search"))
def test_column_search(hip, oracle, engines, case):
    """shortlists of 64, 65, 128, 4095, 4096 and 4097 ids: every entry, the id below the first, the id above the last and
    128 ids just past a present one; -inf exactly at the absent ones (the checker's np.searchsorted)"""
    c, ref, got = _run(hip, oracle, engines, case)
    assert {(b, t) for b, t in zip(*np.nonzero(np.isneginf(got[0])))} == c.minus_inf


@pytest.mark.parametrize("N", C.SEARCH_SIZES)
def test_column_search_of_the_forced_prefix_decoders(hip, oracle, engines, N):
    """the same lists and tokens as forced prefixes of full length tmax_of(64) = 96, with scores, in decode modes 0 (the
    persistent decoder) and 1 (the per-stage kernels): tokens, lengths and alignment rows bit for bit, scores within the
    bound and -inf exactly at the absent ids"""
    m, gm, om = engines("v8192")
    S = C.SEARCH_PREFIX_S
    ids, lens, sl, p_ids, p_len, ok = C.search_prefix_inputs(N, tmax_of(S))
    rec = Recording(om)
    w_out, w_ln, w_al, w_sc = forced_translate(oracle, rec, m, ids, lens, sl, p_ids, p_len)
    assert np.array_equal(np.isneginf(w_sc), ~ok)
    ctx = hip.Context(gm, ids.shape[0], S)
    try:
        for mode in (0, 1):
            ctx.set_decode_mode(mode)
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=(p_ids, p_len))
            assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), mode
            assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), mode
            C.check_scores(sc, w_sc, ln, rec.row_peaks())
    finally:
        ctx.close()


@pytest.mark.parametrize("case", _params("missing"))
def test_missing_tokens(hip, oracle, engines, case):
    """a missing token at t = 0, on the row that ends a 128-row block, on a sentence's last row and on every row of a
    sentence: -inf there and nowhere else; the rows behind them are finite wherever the checker's are (check_scores)"""
    c, _, got = _run(hip, oracle, engines, case)
    assert {(b, t) for b, t in zip(*np.nonzero(np.isneginf(got[0])))} == c.minus_inf
