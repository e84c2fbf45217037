"""GPU checks of the scorer's alternatives (include/slimt_hip.h, slimt_hip_ctx_set_score_alternatives) against the checker
of tests/test_alternatives_checker.py on the cases of tests/support/alternatives_cases.py: ids and ranks exact, alt_scores
within TOL of tests/test_gpu_forced_prefix.py of the float64 log-softmax (the project's bound for scores), -inf and
0xFFFFFFFF exactly where the checker has them; the layer-width edges; the tie rule on a model built for it; the
identities with the unarmed call and the greedy translation; placement and chunking; what is not written; every entry
point; arming; the service and the text front end."""
import io
import random

import numpy as np
import pytest
import torch

from support import alternatives_cases as AC
from test_alternatives_checker import NONE, alternatives
from test_forced_prefix_checker import tmax_of
from test_gpu_forced_prefix import TOL

pytestmark = pytest.mark.gpu

FILL, FILL_U = AC.FILL, AC.FILL_U


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _armed(ctx, ids, lens, sl, t_ids, t_len, k, want_align=False):
    """Context.score with alternatives on fill values of this module's: (scores, align, alt_ids, alt_scores, rank)"""
    B, T = t_ids.shape
    alt = (np.full((B, T, k), FILL_U, np.uint32), np.full((B, T, k), FILL, np.float32), np.full((B, T), FILL_U, np.uint32))
    sc = np.full((B, T), FILL, np.float32)
    al = np.full((B, T, ids.shape[1]), FILL, np.float32) if want_align else None
    ctx.score_async((np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(lens, np.uint32),
                     np.ascontiguousarray(t_ids, np.uint32), np.ascontiguousarray(t_len, np.uint32), sc, al), sl,
                    alternatives=alt)
    ctx.synchronize()
    return (sc, al) + alt


def _check(got, want, t_len, k):
    """got (alt_ids, alt_scores, rank) against the checker's (ids, float64 scores, rank) for k"""
    g_ids, g_sc, g_rank = got
    w_ids, w_sc, w_rank = want
    worst = 0.0
    for b in range(len(t_len)):
        n = int(t_len[b])
        assert np.array_equal(g_ids[b, :n], w_ids[b, :n, :k]), (b, np.argwhere(g_ids[b, :n] != w_ids[b, :n, :k])[:4])
        assert np.array_equal(g_rank[b, :n], w_rank[b, :n]), (b, np.flatnonzero(g_rank[b, :n] != w_rank[b, :n])[:4])
        g, w = g_sc[b, :n].astype(np.float64), w_sc[b, :n, :k]
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), b
        assert np.array_equal(g_ids[b, :n] == NONE, np.isneginf(w) & (w_ids[b, :n, :k] == NONE)), b
        fin = np.isfinite(w)
        assert np.all(np.isfinite(g[fin])), b
        worst = max(worst, float(np.abs(g[fin] - w[fin]).max(initial=0)))
        assert np.all(g_ids[b, n:] == FILL_U) and np.all(g_sc[b, n:] == FILL) and np.all(g_rank[b, n:] == FILL_U), b  # not written
    print("alternatives: k", k, "largest score error", worst)
    assert worst <= TOL, worst


_OPEN = []


def _open(hip, gm, B, S):
    """a context that is closed when the test ends, however it ends: one left open would outlive its model"""
    _OPEN.append(hip.Context(gm, B, S))
    return _OPEN[-1]


@pytest.fixture(autouse=True)
def _close_contexts():
    yield
    while _OPEN:
        _OPEN.pop().close()


@pytest.fixture(scope="module")
def engines(hip):
    cache = {}

    def get(key, m):
        if key not in cache:
            cache[key] = hip.Model(m)
        return cache[key]

    yield get
    for gm in cache.values():
        gm.close()


@pytest.fixture(scope="module")
def tiny(hip, oracle, synth_models, engines):
    m = synth_models("tiny11", 6.0)
    return m, engines("tiny11/6", m), oracle.OracleModel(m)


# ---- parity with the checker ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", AC.KS)
@pytest.mark.parametrize("name", AC.case_names())
def test_alternatives_match_the_checker(hip, oracle, engines, name, k):
    c = AC.build(oracle, name)
    gm = engines(name, c.m)
    ctx = _open(hip, gm, c.ids.shape[0], c.ids.shape[1])
    got = _armed(ctx, c.ids, c.lens, c.sl, c.t_ids, c.t_len, k)
    _check(got[2:], AC.expected(c, k), c.t_len, k)
    ctx.close()


# ---- the layer's width ----------------------------------------------------------------------------------------------------
WIDTHS = (1, 5, 17, 1000 + 7, 4096 - 5)


@pytest.fixture(scope="module")
def negative(hip, oracle, engines):
    """tiny11 with every output bias lowered by 40: the real logits are negative, a padding column's 0 would win"""
    from slimt_amd import synth
    m = synth.make_model("tiny11", seed=1234, eos_bias=6.0)
    m.params["decoder_ff_logit_out_b"].data -= np.float32(40.0)
    return m, engines("tiny11/negative", m), oracle.OracleModel(m)


@pytest.mark.parametrize("n_sl", WIDTHS)
def test_layer_width_edges(hip, oracle, negative, n_sl):
    from slimt_amd import synth
    m, gm, om = negative
    B, S, T = 3, 8, 7
    rng = np.random.default_rng(n_sl)
    ids, lens = synth.make_batch(m.V, B, S, seed=60 + n_sl, ragged=True)
    sl = np.sort(rng.choice(np.arange(1, m.V, dtype=np.uint32), size=n_sl, replace=False))
    t_len = np.array([T, 4, T], np.uint32)
    t_ids = rng.choice(sl, size=(B, T)).astype(np.uint32)
    t_ids[0, 2] = t_ids[2, 5] = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)[3]  # outside the layer
    want = alternatives(oracle, om, m, ids, lens, sl, t_ids, t_len, 8, keep_logits=True)
    lg = np.concatenate([x.ravel() for x in want.logits])
    print("width", n_sl, "negative logits: %.4f" % np.mean(lg < 0), "largest", lg.max())
    assert np.mean(lg < 0) > 0.99  # an unmasked padding column (logit 0) would be the first alternative nearly everywhere
    ctx = _open(hip, gm, B, S)
    for k in AC.KS:
        got = _armed(ctx, ids, lens, sl, t_ids, t_len, k)
        _check(got[2:], (want.ids, want.scores, want.rank), t_len, k)
        assert np.isin(got[2][(got[2] != FILL_U) & (got[2] != NONE)], sl).all()  # ids of the layer, never a padding column's
        live = np.arange(T)[None, :] < t_len[:, None]
        assert np.all((got[2][live] != NONE).sum(axis=1) == min(k, n_sl))
        assert got[4][0, 2] == NONE and got[4][2, 5] == NONE and got[0][0, 2] == -np.inf
    ctx.close()


# ---- the tie rule -----------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_column_across_tiles_and_waves(hip, oracle):
    """ids a_0 < ... < a_8 share one embedding row and one output bias, raised so that the block wins in every row. Over the
    full vocabulary a column is its id: tiles 1, 2, 3, 4, 6, 7, 9, 12, 13 (waves 1, 2, 3, 0, 2, 3, 1, 0, 1 -- different tiles
    of one wave and different waves), lane position 5 in all of them."""
    from slimt_amd import synth
    m = synth.make_model("micro", seed=1234, eos_bias=3.0)  # V = 512: 32 column tiles
    a = np.array([16 * t + 5 for t in (1, 2, 3, 4, 6, 7, 9, 12, 13)], np.uint32)
    assert len(set(int(x) // 16 for x in a)) == 9 and len(set((int(x) // 16) % 4 for x in a)) == 4 and set(a % 16) == {5}
    emb, bias = m.params["Wemb"].data, m.params["decoder_ff_logit_out_b"].data
    emb.reshape(m.V, m.D)[a] = emb.reshape(m.V, m.D)[a[0]]
    bias.reshape(-1)[a] = np.float32(60.0)
    B, S, T, k = 4, 8, 11, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=3, ragged=True)
    rng = np.random.default_rng(1)
    t_ids = rng.integers(1, m.V, size=(B, T)).astype(np.uint32)
    t_len = np.array([T, 5, T - 1, 2], np.uint32)
    t_ids[0, 3], t_ids[2, 7] = a[8], a[8]
    t_ids[0, 6], t_ids[1, 1], t_ids[3, 0] = a[3], a[3], a[3]
    om = oracle.OracleModel(m)
    want = alternatives(oracle, om, m, ids, lens, None, t_ids, t_len, k, keep_logits=True)
    for lg in want.logits:  # the block wins, tied exactly, in every row
        assert np.all(lg[:, a] == lg[:, a[:1]]) and np.all(np.delete(lg, a, axis=1).max(axis=1) < lg[:, a[0]])
    gm = hip.Model(m)
    ctx = _open(hip, gm, B, S)
    got = _armed(ctx, ids, lens, None, t_ids, t_len, k)
    for b in range(B):
        n = int(t_len[b])
        assert np.all(got[2][b, :n] == a[None, :8]), b
    assert got[4][0, 3] == 8 and got[4][2, 7] == 8
    assert got[4][0, 6] == 3 and got[4][1, 1] == 3 and got[4][3, 0] == 3
    _check(got[2:], (want.ids, want.scores, want.rank), t_len, k)
    live = np.arange(T)[None, :] < t_len[:, None]
    assert np.all(_bits(got[3][live]) == _bits(got[3][live][:, :1]))  # one logit, one (m, s): one score
    ctx.close()
    gm.close()


# ---- identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", AC.KS)
def test_armed_scores_and_alignments_are_the_unarmed_bits(hip, oracle, engines, k):
    c = AC.build(oracle, "tiny11-S32")
    gm = engines("tiny11-S32", c.m)
    B, S = c.ids.shape
    ctx = _open(hip, gm, B, S)
    plain = ctx.score(c.ids, c.lens, c.sl, c.t_ids, c.t_len, want_align=True, fill=FILL)
    got = _armed(ctx, c.ids, c.lens, c.sl, c.t_ids, c.t_len, k, want_align=True)
    assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(_bits(got[1]), _bits(plain[1]))
    n_hit = 0
    for b, t in zip(*np.nonzero(AC.live(c))):
        r = int(got[4][b, t])
        if r < k:
            assert got[2][b, t, r] == c.t_ids[b, t]
            assert _bits(got[3][b, t, r:r + 1])[0] == _bits(got[0][b, t:t + 1])[0], (b, t)
            n_hit += 1
        else:
            assert c.t_ids[b, t] not in got[2][b, t]
    assert n_hit >= AC.live(c).sum() // 4
    ctx.close()


def test_the_engines_own_greedy_translation_has_rank_zero(hip, synth_models, engines):
    """tiny11 at EOS bias 7.5: the oracle's greedy translation of this batch ends at step 1 for four sentences and runs to
    the limit for five"""
    from slimt_amd import synth
    m = synth_models("tiny11", 7.5)
    gm = engines("tiny11/7.5", m)
    B, S = 9, 16
    ids, lens = synth.make_batch(m.V, B, S, seed=71, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    ctx = _open(hip, gm, B, S)
    out, ln, _, tsc = ctx.translate(ids, lens, sl, want_align=True, scores=True)
    assert ln.min() >= 1 and len(set(ln.tolist())) > 1, ln
    got = _armed(ctx, ids, lens, sl, out, ln, 3)
    for b in range(B):
        n = int(ln[b])
        assert np.all(got[4][b, :n] == 0) and np.array_equal(got[2][b, :n, 0], out[b, :n]), b
        assert np.all(np.abs(got[3][b, :n, 0].astype(np.float64) - tsc[b, :n]) <= 2 * TOL), b
    ctx.close()


# ---- placement and chunking -------------------------------------------------------------------------------------------------
def test_alone_permuted_and_in_two_chunks_the_same_bits(hip, tiny):
    """5 sentences of 2100 rows go as two chunks (8192 // 2100 = 3 sentences per chunk: 3 + 2), the lengths of
    tests/test_gpu_score.py's chunk test"""
    from slimt_amd import synth
    m, gm, _ = tiny
    B, S, T, k = 5, 8, 2100, 8
    rng = np.random.default_rng(8)
    ids, lens = synth.make_batch(m.V, B, S, seed=5, ragged=True)
    sl = synth.make_shortlist(m.V, 1024)
    t_ids = rng.choice(sl[sl != 0], size=(B, T)).astype(np.uint32)
    t_len = np.asarray([T, 3, T - 1, 0, 1500], np.uint32)
    ctx = _open(hip, gm, B, S)
    full = _armed(ctx, ids, lens, sl, t_ids, t_len, k)

    def same(a, rows):
        for x, y in zip(a, (full[0], full[2], full[3], full[4])):
            assert np.array_equal(_bits(x), _bits(y[rows]))

    for b in range(B):
        one = _armed(ctx, ids[b:b + 1], lens[b:b + 1], sl, t_ids[b:b + 1], t_len[b:b + 1], k)
        same((one[0], one[2], one[3], one[4]), slice(b, b + 1))
    perm = rng.permutation(B)
    shuf = _armed(ctx, ids[perm], lens[perm], sl, t_ids[perm], t_len[perm], k)
    same((shuf[0], shuf[2], shuf[3], shuf[4]), perm)
    live = np.arange(T)[None, :] < t_len[:, None]
    assert np.all(full[2][~live] == FILL_U) and np.all(full[3][~live] == FILL) and np.all(full[4][~live] == FILL_U)
    assert np.all(full[2][live] != NONE) and np.all(full[4][live] < len(sl))
    ctx.close()


# ---- what is not written ----------------------------------------------------------------------------------------------------
def test_entries_behind_a_targets_end_keep_their_fill(hip, tiny):
    from slimt_amd import synth
    m, gm, _ = tiny
    B, S, T, k = 6, 8, 20, 5
    ids, lens = synth.make_batch(m.V, B, S, seed=15, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids = np.random.default_rng(2).choice(sl, size=(B, T)).astype(np.uint32)
    t_len = np.array([0, 1, 15, 16, 17, T], np.uint32)
    ctx = _open(hip, gm, B, S)
    got = _armed(ctx, ids, lens, sl, t_ids, t_len, k)
    live = np.arange(T)[None, :] < t_len[:, None]
    assert np.all(got[2][~live] == FILL_U) and np.all(got[3][~live] == FILL) and np.all(got[4][~live] == FILL_U)
    assert np.all(got[2][live] != FILL_U) and np.all(got[3][live] != FILL) and np.all(got[4][live] != FILL_U)
    # the wrapper's own fill: 0xFFFFFFFF and `fill`
    sc, al, a_ids, a_sc, rank = ctx.score(ids, lens, sl, t_ids, t_len, fill=FILL, alternatives=k)
    assert al is None and np.all(a_ids[~live] == NONE) and np.all(a_sc[~live] == FILL) and np.all(rank[~live] == NONE)
    assert np.array_equal(a_ids[live], got[2][live]) and np.array_equal(_bits(a_sc[live]), _bits(got[3][live]))
    assert np.array_equal(rank[live], got[4][live])
    ctx.close()


# ---- entry points -----------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_entry_points_give_the_same_bits(hip, tiny):
    from slimt_amd import synth
    m, gm, _ = tiny
    B, S, k = 11, 16, 5
    T = tmax_of(S) + 3
    rng = np.random.default_rng(12)
    ids, lens = synth.make_batch(m.V, B, S, seed=31, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids = rng.choice(sl, size=(B, T)).astype(np.uint32)
    t_len = np.asarray([(b * T) // (B - 1) for b in range(B)], np.uint32)
    ctx = _open(hip, gm, B, S)
    live = np.arange(T)[None, :] < t_len[:, None]
    host = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL, alternatives=k)  # slimt_hip_score

    def same(sc, a_ids, a_sc, rank):
        assert np.array_equal(_bits(sc)[live], _bits(host[0])[live])
        assert np.array_equal(a_ids[live], host[2][live]) and np.array_equal(_bits(a_sc)[live], _bits(host[3])[live])
        assert np.array_equal(rank[live], host[4][live])
        assert np.all(a_ids[~live] == a_ids[~live][:1]) and np.all(rank[~live] == rank[~live][:1])  # (one fill value)

    # pinned, asynchronous: the context's own arrays
    bufs = ctx.score_buffers(B, S, T, want_align=True)
    for dst, src in zip(bufs[:4], (ids, lens, t_ids, t_len)):
        dst[...] = src
    bufs[4][...] = FILL
    bufs[5][...] = FILL
    alt = ctx.score_async(bufs, sl, alternatives=k)
    ctx.synchronize()
    same(bufs[4], *alt)
    assert np.all(alt[0][~live] == NONE) and np.all(np.isnan(alt[1][~live]))
    # pageable, asynchronous
    got = _armed(ctx, ids, lens, sl, t_ids, t_len, k)
    same(got[0], *got[2:])
    # alt_ids alone
    only = (np.full((B, T, k), FILL_U, np.uint32), None, None)
    sc = np.full((B, T), FILL, np.float32)
    ctx.score_async((ids, lens, t_ids, t_len, sc, None), sl, alternatives=only)
    ctx.synchronize()
    assert np.array_equal(only[0], got[2])
    # device pointers
    d = [_dev(a) for a in (ids, lens, sl, t_ids, t_len)]
    d_sc = torch.full((B, T), float(FILL), dtype=torch.float32, device="cuda")
    d_ai = torch.full((B, T, k), 7, dtype=torch.int32, device="cuda")
    d_as = torch.full((B, T, k), float(FILL), dtype=torch.float32, device="cuda")
    d_ar = torch.full((B, T), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.score_device(d[0].data_ptr(), d[1].data_ptr(), B, S, d[2].data_ptr(), sl.size, d[3].data_ptr(), d[4].data_ptr(), T,
                     d_sc.data_ptr(), 0, alternatives=(k, d_ai.data_ptr(), d_as.data_ptr(), d_ar.data_ptr()))
    ctx.synchronize()
    same(d_sc.cpu().numpy(), d_ai.cpu().numpy().view(np.uint32), d_as.cpu().numpy(), d_ar.cpu().numpy().view(np.uint32))
    # host arrays are no device memory, and pinned and pageable arrays do not mix: refused with a message
    with pytest.raises(hip.SlimtHipError, match="score alternatives: alt_ids is not memory the device can write"):
        ctx.score_device(d[0].data_ptr(), d[1].data_ptr(), B, S, d[2].data_ptr(), sl.size, d[3].data_ptr(), d[4].data_ptr(), T,
                         d_sc.data_ptr(), 0, alternatives=(k, got[2].ctypes.data, 0, 0))
    with pytest.raises(hip.SlimtHipError, match="of the kind of scores"):
        ctx.score_async(bufs, sl, alternatives=(got[2], got[3], got[4]))
    ctx.close()


def test_generated_shortlist_gives_the_same_bits(hip, tiny):
    from slimt_amd import synth
    m, gm, _ = tiny
    B, S, T, k = 7, 12, 17, 8
    rng = np.random.default_rng(13)
    ids, lens = synth.make_batch(m.V, B, S, seed=32, ragged=True)
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    sl = gen.generate(ids, lens)
    assert 0 < sl.size < m.V
    t_ids = rng.choice(sl, size=(B, T)).astype(np.uint32)
    t_len = np.asarray([(b * T) // (B - 1) for b in range(B)], np.uint32)
    ctx = _open(hip, gm, B, S)
    host = _armed(ctx, ids, lens, sl, t_ids, t_len, k)
    alt = (np.full((B, T, k), FILL_U, np.uint32), np.full((B, T, k), FILL, np.float32), np.full((B, T), FILL_U, np.uint32))
    sc = np.full((B, T), FILL, np.float32)
    ctx.score_async((ids, lens, t_ids, t_len, sc, None), generator=gen, alternatives=alt)
    ctx.synchronize()
    assert np.array_equal(_bits(sc), _bits(host[0]))
    for x, y in zip(alt, host[2:]):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.isin(alt[0][alt[0] != FILL_U], sl).all()
    ctx.close()
    gen.close()


# ---- arming -----------------------------------------------------------------------------------------------------------------
def test_the_setting_is_taken_by_one_score_call_and_by_no_translate_call(hip, tiny):
    from slimt_amd import synth
    m, gm, _ = tiny
    B, S, k = 6, 16, 5
    T = tmax_of(S)
    rng = np.random.default_rng(14)
    ids, lens = synth.make_batch(m.V, B, S, seed=33, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids = rng.choice(sl, size=(B, T)).astype(np.uint32)
    t_len = np.full(B, T, np.uint32)
    prefix = (t_ids, np.full(B, 3, np.uint32))
    ctx = _open(hip, gm, B, S)
    want = ctx.score(ids, lens, sl, t_ids, t_len, alternatives=k)
    new = lambda: (np.full((B, T, k), FILL_U, np.uint32), np.full((B, T, k), FILL, np.float32), np.full((B, T), FILL_U, np.uint32))
    # armed, a translate call in between: it neither takes nor clears the setting
    alt = new()
    ctx.set_score_alternatives(k, *alt)
    before = ctx.translate(ids, lens, sl, want_align=True)
    assert np.all(alt[0] == FILL_U) and np.all(alt[2] == FILL_U)
    first = ctx.score(ids, lens, sl, t_ids, t_len)
    assert len(first) == 2 and np.array_equal(_bits(first[0]), _bits(want[0]))
    for x, y in zip(alt, want[2:]):
        assert np.array_equal(_bits(x), _bits(y))
    # consumed: a second call writes nothing
    for x, f in zip(alt, (FILL_U, FILL, FILL_U)):
        x[...] = f
    second = ctx.score(ids, lens, sl, t_ids, t_len)
    assert np.array_equal(_bits(second[0]), _bits(want[0]))
    assert np.all(alt[0] == FILL_U) and np.all(alt[1] == FILL) and np.all(alt[2] == FILL_U)
    # a refused score call takes the setting too
    ctx.set_score_alternatives(k, *alt)
    bad = t_len.copy()
    bad[1] = T + 1
    with pytest.raises(hip.SlimtHipError, match="target length"):
        ctx.score(ids, lens, sl, t_ids, bad)
    ctx.score(ids, lens, sl, t_ids, t_len)
    assert np.all(alt[0] == FILL_U)
    # k = 0 disarms
    ctx.set_score_alternatives(k, *alt)
    ctx.set_score_alternatives(0)
    ctx.score(ids, lens, sl, t_ids, t_len)
    assert np.all(alt[0] == FILL_U)
    # what is armed for translate calls survives an armed score call
    forced = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=prefix)
    sc = np.full((B, T), np.nan, np.float32)
    ctx.set_scores([sc])
    ctx.set_target_prefix([prefix])
    mid = ctx.score(ids, lens, sl, t_ids, t_len, alternatives=k)
    assert np.array_equal(mid[2], want[2]) and np.array_equal(mid[4], want[4])
    out = ctx.translate(ids, lens, sl, want_align=True)  # (armed by hand above: forced and scored)
    assert np.array_equal(out[0], forced[0]) and np.array_equal(out[1], forced[1])
    assert np.array_equal(_bits(sc), _bits(forced[3]))
    after = ctx.translate(ids, lens, sl, want_align=True)
    for x, y in zip(before, after):
        assert np.array_equal(_bits(x), _bits(y))
    # refusals at once; the context stays usable
    L = hip.lib()
    assert L.slimt_hip_ctx_set_score_alternatives(ctx.h, 9, alt[0].ctypes.data, None, None) != 0
    assert b"exceeds SLIMT_HIP_MAX_ALTERNATIVES" in L.slimt_hip_last_error()
    assert L.slimt_hip_ctx_set_score_alternatives(ctx.h, 3, None, None, None) != 0
    assert b"alt_ids is NULL" in L.slimt_hip_last_error()
    again = ctx.score(ids, lens, sl, t_ids, t_len, alternatives=k)
    assert np.all(alt[0] == FILL_U)  # (neither refused call armed anything)
    for x, y in zip(again, want):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
    ctx.close()


def test_literal_order_models_are_refused_and_take_the_setting(hip, synth_models):
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    gm.set_kv_cache_format(3)
    ctx = _open(hip, gm, 2, 8)
    with pytest.raises(hip.SlimtHipError, match="format 3"):
        ctx.score(np.ones((2, 8), np.uint32), np.full(2, 8, np.uint32), None, np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32),
                  alternatives=3)
    ctx.close()
    gm.close()


# ---- the service and the text front end -------------------------------------------------------------------------------------
def test_batch_service_alternatives_equal_the_context_calls(hip, synth_models):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(5))
    n, k = 24, 5
    sents = [list(rnd.integers(3, m.V, int(rnd.integers(1, 20)))) + [0] for _ in range(n)]
    fixed = synth.make_shortlist(m.V, 2048)
    outside = np.setdiff1d(np.arange(1, m.V), fixed)
    tgts = []
    for i, s in enumerate(sents):
        t = [int(x) for x in rnd.choice(fixed, size=(i * 2 * len(s)) // (n - 1))]
        if len(t) > 3:
            t[1] = int(outside[i])
        tgts.append(t)
    assert any(not t for t in tgts)
    svc = hip.BatchService([gm], max_words=8 * 21, workers_per_device=1, shortlist=fixed)
    ctx = _open(hip, gm, 64, 32)
    try:
        res = svc.score(sents, tgts, alternatives=k)
        plain = svc.score(sents, tgts)
        assert np.array_equal(_bits(res.scores), _bits(plain.scores))
        with pytest.raises(hip.SlimtHipError, match="not a result of"):
            plain.alternatives(0)
        with pytest.raises(hip.SlimtHipError, match="sentence"):
            res.alternatives(n)
        plain.close()
        assert len(set(int(b) for b in res.batch)) >= 2
        for i in range(n):
            a_ids, a_sc, rank = res.alternatives(i)
            nt = len(tgts[i])
            assert a_ids.shape == (nt, k) and a_sc.shape == (nt, k) and rank.shape == (nt,)
            if not nt:
                continue
            t_ids = np.asarray([tgts[i]], np.uint32)
            w = ctx.score(np.asarray([sents[i]], np.uint32), np.asarray([len(sents[i])], np.uint32), fixed, t_ids,
                          np.asarray([nt], np.uint32), alternatives=k)
            assert np.array_equal(_bits(res.token_scores(i)), _bits(w[0][0]))
            assert np.array_equal(a_ids, w[2][0]) and np.array_equal(_bits(a_sc), _bits(w[3][0])) and np.array_equal(rank, w[4][0])
            if nt > 3:
                assert rank[1] == NONE
        res.close()
        with pytest.raises(ValueError):
            svc.score(sents, tgts, alternatives=9)
    finally:
        ctx.close()
        svc.close()
        gm.close()


def test_frontend_service_returns_pieces_and_consistent_ranks(hip):
    import sentencepiece
    from slimt_amd import frontend, synth
    rnd = random.Random(7)
    words = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 8))) for _ in range(1500)]
    corpus = []
    for _ in range(3000):
        s = " ".join(rnd.choice(words) for _ in range(rnd.randint(3, 18)))
        corpus.append(s[0].upper() + s[1:] + rnd.choice(".?!"))
    out = io.BytesIO()
    sentencepiece.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=out, vocab_size=512,
                                             model_type="unigram", pad_id=-1, unk_id=1, bos_id=-1, eos_id=0, minloglevel=2)
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    package = frontend.Package(model=synth.write_bin(m), vocabulary=out.getvalue())
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        sources, targets = corpus[:8], corpus[100:108]
        k = 3
        pairs = svc.score(model, sources, targets, alternatives=k)
        plain = svc.score(model, sources, targets)
        v = model.vocabulary
        hits = 0
        for p, q in zip(pairs, plain):
            assert q.ranks is None and q.alternatives is None
            assert np.array_equal(_bits(p.token_scores), _bits(q.token_scores))
            n = len(p.target_ids)
            assert len(p.ranks) == n and len(p.alternatives) == n
            for t in range(n):
                alts = p.alternatives[t]
                assert len(alts) == k and all(isinstance(w, str) and isinstance(s, float) for w, s in alts)
                assert [s for _, s in alts] == sorted((s for _, s in alts), reverse=True)
                r = p.ranks[t]
                assert r is not None and 0 <= r < m.V  # (the full vocabulary: every token is in the layer)
                if r < k:
                    assert alts[r][0] == v.piece(p.target_ids[t])
                    assert np.float32(alts[r][1]) == p.token_scores[t]
                    hits += 1
                else:
                    assert alts[-1][1] >= float(p.token_scores[t])
        print("frontend: targets among their own first", k, "alternatives:", hits)
    finally:
        svc.close()
        model.close()
