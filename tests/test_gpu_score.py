"""GPU parity of teacher-forced scoring (include/slimt_hip.h, slimt_hip_score*) against the checker of
tests/test_score_checker.py: alignment rows bit-equal, scores within 5e-5 of its float64 log_softmax (the project's bound
for scores against a checker, TOL of tests/test_gpu_forced_prefix.py), -inf exactly where the checker has it; targets
longer than the forced-prefix path accepts; placement independence; every entry point; what is not written; the
neighbouring translate calls; refusals."""
import numpy as np
import pytest
import torch

from test_forced_prefix_checker import tmax_of
from test_gpu_forced_prefix import TOL
from test_score_checker import teacher_forced

pytestmark = pytest.mark.gpu

FILL = np.float32(-7.25)  # what the output buffers hold before a call: entries the call does not write keep it


@pytest.fixture(scope="module")
def engines(hip, oracle, synth_models):
    cache = {}

    def get(preset, eos_bias=6.0):
        if (preset, eos_bias) not in cache:
            m = synth_models(preset, eos_bias)
            cache[(preset, eos_bias)] = (m, hip.Model(m), oracle.OracleModel(m))
        return cache[(preset, eos_bias)]

    yield get
    for _, gm, _ in cache.values():
        gm.close()


def _spread(B, hi, lo=0):
    return [lo + (b * (hi - lo)) // max(1, B - 1) for b in range(B)]


def _targets(rng, B, T, sl, V, t_len, eos=0):
    pool = sl[sl != eos] if sl is not None else np.arange(1, V, dtype=np.uint32)
    return rng.choice(pool, size=(B, T)).astype(np.uint32), np.asarray(t_len, np.uint32)


def _check(got, want, lens, t_len, align=True):
    sc, al = got
    w_sc, w_al = want
    for b in range(len(t_len)):
        n, L = int(t_len[b]), int(lens[b])
        g, w = sc[b, :n].astype(np.float64), w_sc[b, :n]
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), (b, g, w)
        fin = np.isfinite(w)
        assert np.all(np.isfinite(g[fin])), (b, g)
        err = np.abs(g[fin] - w[fin])
        print("sentence", b, "n", n, "max score error", err.max(initial=0))
        assert err.max(initial=0) <= TOL, (b, err.max())
        assert np.all(sc[b, n:] == FILL), b  # t >= n_b: not written
        if align:
            assert np.array_equal(al[b, :n, :L].view(np.uint32), w_al[b, :n, :L].view(np.uint32)), b
            assert np.all(al[b, n:] == FILL) and np.all(al[b, :, L:] == FILL), b  # ... nor columns j >= lengths[b]


def _same(a, b, lens, t_len):
    """two results of the same sentences, bit for bit where the calls write"""
    for i in range(len(t_len)):
        n, L = int(t_len[i]), int(lens[i])
        assert np.array_equal(a[0][i, :n].view(np.uint32), b[0][i, :n].view(np.uint32)), i
        if a[1] is not None:
            assert np.array_equal(a[1][i, :n, :L].view(np.uint32), b[1][i, :n, :L].view(np.uint32)), i


CASES = [  # preset, S, B, shortlist
    ("tiny11", 32, 17, 4096),
    ("tiny11", 8, 17, None),
    ("tiny11", 64, 9, 4096),
    ("tiny11", 100, 3, 4096),
    ("tiny11", 8, 33, 4096),
    ("base", 32, 9, 4096),
]


@pytest.mark.parametrize("preset,S,B,n_sl", CASES)
def test_scores_and_alignments_match_the_checker(hip, oracle, engines, preset, S, B, n_sl):
    from slimt_amd import synth
    m, gm, om = engines(preset)
    rng = np.random.default_rng(S + B)
    ids, lens = synth.make_batch(m.V, B, S, seed=43 + S + B, ragged=True)
    lens[0], lens[-1] = 0, S
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    # the first case is the issue's (T = tmax_of(32) = 48: any B gives a multiple of 16); the others take an odd T, so
    # that with their odd B the B * T rows are no multiple of 16 or 128
    T = tmax_of(S) if (S, B) == (32, 17) and preset == "tiny11" else tmax_of(S) | 1
    assert (S, B, preset) == (32, 17, "tiny11") or (B * T) % 16 != 0
    t_ids, t_len = _targets(rng, B, T, sl, m.V, _spread(B, T, 0))  # 0 .. T, both included
    want = teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len)
    ctx = hip.Context(gm, B, S)
    _check(ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL), want, lens, t_len)
    sc, al = ctx.score(ids, lens, sl, t_ids, t_len, fill=FILL)
    assert al is None
    _check((sc, None), want, lens, t_len, align=False)
    ctx.close()


@pytest.mark.parametrize("S", [8, 32])
def test_targets_three_times_the_source_length(hip, oracle, engines, S):
    """what the forced-prefix path refuses: a target longer than limit_factor * S"""
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, T = 3, 3 * S
    rng = np.random.default_rng(S)
    ids, lens = synth.make_batch(m.V, B, S, seed=S, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids, t_len = _targets(rng, B, T, sl, m.V, [T, T - 1, 2 * S + 1])
    want = teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len)
    ctx = hip.Context(gm, B, S)
    _check(ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL), want, lens, t_len)
    # the same targets as a forced prefix are still refused: rows of Tmax columns cannot hold them
    Tmax = tmax_of(S)
    ctx.set_target_prefix([(np.ascontiguousarray(t_ids[:, :Tmax]), t_len)])
    with pytest.raises(hip.SlimtHipError, match="target prefix: length"):
        ctx.translate(ids, lens, sl)
    ctx.close()


def test_eos_inside_missing_tokens_and_the_forced_prefix_call(hip, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S = 5, 16
    T = tmax_of(S)
    rng = np.random.default_rng(9)
    ids, lens = synth.make_batch(m.V, B, S, seed=19, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    missing = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)[0]
    t_ids, t_len = _targets(rng, B, T, sl, m.V, [T, T, T, T - 3, 5])
    t_ids[0, 0] = 0       # EOS first
    t_ids[1, T // 2] = 0  # EOS in the middle
    t_ids[2, 4] = missing
    t_ids[3, T - 4] = 0   # EOS last
    want = teacher_forced(oracle, om, m, ids, lens, sl, t_ids, t_len)
    assert want[0][2, 4] == -np.inf and np.all(np.isfinite(want[0][2, 5:]))
    ctx = hip.Context(gm, B, S)
    got = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    _check(got, want, lens, t_len)
    assert got[0][2, 4] == -np.inf
    # through the first EOS: the GPU's own forced-prefix call with the same prefix, alignment rows bit for bit
    fo = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=(t_ids, t_len))
    for b in range(B):
        eos = np.flatnonzero(t_ids[b, :t_len[b]] == 0)
        n = int(eos[0]) + 1 if len(eos) else int(t_len[b])
        assert fo[1][b] >= n, b
        L = int(lens[b])
        assert np.array_equal(fo[2][b, :n, :L].view(np.uint32), got[1][b, :n, :L].view(np.uint32)), b
        g, w = got[0][b, :n].astype(np.float64), fo[3][b, :n].astype(np.float64)
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), b
        assert np.abs(g[np.isfinite(w)] - w[np.isfinite(w)]).max(initial=0) <= 2 * TOL, b
    ctx.close()


def test_a_sentence_scores_the_same_bits_wherever_it_sits(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T = 21, 12, 19
    rng = np.random.default_rng(4)
    ids, lens = synth.make_batch(m.V, B, S, seed=77, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids, t_len = _targets(rng, B, T, sl, m.V, _spread(B, T, 1))
    ctx = hip.Context(gm, B, S)
    full = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    for b in (0, B // 2, B - 1):  # alone
        one = ctx.score(ids[b:b + 1], lens[b:b + 1], sl, t_ids[b:b + 1], t_len[b:b + 1], want_align=True, fill=FILL)
        _same(one, (full[0][b:b + 1], full[1][b:b + 1]), lens[b:b + 1], t_len[b:b + 1])
    perm = rng.permutation(B)
    shuf = ctx.score(ids[perm], lens[perm], sl, t_ids[perm], t_len[perm], want_align=True, fill=FILL)
    _same(shuf, (full[0][perm], full[1][perm]), lens[perm], t_len[perm])
    ctx.close()


def test_more_than_one_row_chunk_equals_the_per_sentence_calls(hip, engines):
    """chunks are whole sentences of at most max(T, 8192) rows: 5 sentences of 2100 rows go as two chunks (8192 // 2100 = 3
    sentences per chunk: 3 + 2), the second one smaller than the workspace"""
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T = 5, 8, 2100
    rng = np.random.default_rng(8)
    ids, lens = synth.make_batch(m.V, B, S, seed=5, ragged=True)
    sl = synth.make_shortlist(m.V, 1024)
    t_ids, t_len = _targets(rng, B, T, sl, m.V, [T, 3, T - 1, 0, 1500])
    ctx = hip.Context(gm, B, S)
    full = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    for b in range(B):
        one = ctx.score(ids[b:b + 1], lens[b:b + 1], sl, t_ids[b:b + 1], t_len[b:b + 1], want_align=True, fill=FILL)
        _same(one, (full[0][b:b + 1], full[1][b:b + 1]), lens[b:b + 1], t_len[b:b + 1])
        assert np.all(full[0][b, t_len[b]:] == FILL)
    ctx.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_entry_points_give_the_same_bits(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S = 11, 16
    T = tmax_of(S) + 3
    rng = np.random.default_rng(12)
    ids, lens = synth.make_batch(m.V, B, S, seed=31, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids, t_len = _targets(rng, B, T, sl, m.V, _spread(B, T, 0))
    ctx = hip.Context(gm, B, S)
    host = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    # pinned, asynchronous
    bufs = ctx.score_buffers(B, S, T, want_align=True)
    for dst, src in zip(bufs[:4], (ids, lens, t_ids, t_len)):
        dst[...] = src
    bufs[4][...] = FILL
    bufs[5][...] = FILL
    ctx.score_async(bufs, sl)
    ctx.synchronize()
    assert np.array_equal(bufs[4].view(np.uint32), host[0].view(np.uint32))
    assert np.array_equal(bufs[5].view(np.uint32), host[1].view(np.uint32))
    # pageable, asynchronous
    sc = np.full((B, T), FILL, np.float32)
    al = np.full((B, T, S), FILL, np.float32)
    ctx.score_async((ids, lens, t_ids, t_len, sc, al), sl)
    ctx.synchronize()
    assert np.array_equal(sc.view(np.uint32), host[0].view(np.uint32)) and np.array_equal(al.view(np.uint32), host[1].view(np.uint32))
    # device pointers; a device tgt_len above T behaves as T
    big = t_len.copy()
    big[t_len == T] = T + 5
    d = [_dev(a) for a in (ids, lens, sl, t_ids, big)]
    d_sc = torch.full((B, T), float(FILL), dtype=torch.float32, device="cuda")
    d_al = torch.full((B, T, S), float(FILL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.score_device(d[0].data_ptr(), d[1].data_ptr(), B, S, d[2].data_ptr(), sl.size, d[3].data_ptr(), d[4].data_ptr(), T,
                     d_sc.data_ptr(), d_al.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_sc.cpu().numpy().view(np.uint32), host[0].view(np.uint32))
    assert np.array_equal(d_al.cpu().numpy().view(np.uint32), host[1].view(np.uint32))
    ctx.close()


def test_generated_shortlist_is_the_generators(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T = 7, 12, 17
    rng = np.random.default_rng(13)
    ids, lens = synth.make_batch(m.V, B, S, seed=32, ragged=True)
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    sl = gen.generate(ids, lens)
    assert 0 < sl.size < m.V
    t_ids, t_len = _targets(rng, B, T, sl, m.V, _spread(B, T, 0))
    ctx = hip.Context(gm, B, S)
    host = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    sc = np.full((B, T), FILL, np.float32)
    al = np.full((B, T, S), FILL, np.float32)
    ctx.score_async((ids, lens, t_ids, t_len, sc, al), generator=gen)
    ctx.synchronize()
    assert np.array_equal(sc.view(np.uint32), host[0].view(np.uint32)) and np.array_equal(al.view(np.uint32), host[1].view(np.uint32))
    ctx.close()
    gen.close()


def test_neighbouring_translate_calls_and_a_growing_workspace(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S = 18, 16
    T = tmax_of(S)
    rng = np.random.default_rng(14)
    ids, lens = synth.make_batch(m.V, B, S, seed=33, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids, t_len = _targets(rng, B, T, sl, m.V, _spread(B, T, 1))
    prefix = (t_ids, np.minimum(t_len, 3).astype(np.uint32))
    ctx = hip.Context(gm, B, S)

    def translates():
        return (ctx.translate(ids, lens, sl, want_align=True), ctx.translate(ids, lens, sl, want_align=True, scores=True),
                ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=prefix))

    before = translates()
    small = ctx.score(ids[:2], lens[:2], sl, t_ids[:2, :5], np.minimum(t_len[:2], 5), want_align=True, fill=FILL)
    large = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)  # the workspace grows
    again = ctx.score(ids[:2], lens[:2], sl, t_ids[:2, :5], np.minimum(t_len[:2], 5), want_align=True, fill=FILL)
    assert np.array_equal(small[0].view(np.uint32), again[0].view(np.uint32))
    assert np.array_equal(small[1].view(np.uint32), again[1].view(np.uint32))
    after = translates()
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # options armed before a score call are still armed after it: the next translate call takes them
    sc = np.full((B, T), np.nan, np.float32)
    ctx.set_scores([sc])
    ctx.set_target_prefix([prefix])
    mid = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    assert np.array_equal(mid[0].view(np.uint32), large[0].view(np.uint32))
    out = ctx.translate(ids, lens, sl, want_align=True)  # (armed by hand above: forced and scored)
    assert np.array_equal(out[0], before[2][0]) and np.array_equal(out[1], before[2][1])
    assert np.array_equal(sc.view(np.uint32), before[2][3].view(np.uint32))
    ctx.close()


def test_refusals_leave_the_context_usable(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T = 4, 8, 9
    rng = np.random.default_rng(15)
    ids, lens = synth.make_batch(m.V, B, S, seed=34, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    t_ids, t_len = _targets(rng, B, T, sl, m.V, [T, 4, 0, 2])
    ctx = hip.Context(gm, B, S)
    good = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=FILL)
    bad_len = t_len.copy()
    bad_len[1] = T + 1
    with pytest.raises(hip.SlimtHipError, match="target length"):
        ctx.score(ids, lens, sl, t_ids, bad_len)
    bad_ids = t_ids.copy()
    bad_ids[0, 3] = m.V
    with pytest.raises(hip.SlimtHipError, match="out of range"):
        ctx.score(ids, lens, sl, bad_ids, t_len)
    with pytest.raises(hip.SlimtHipError, match="T is 0"):
        ctx.score(ids, lens, sl, np.zeros((B, 0), np.uint32), np.zeros(B, np.uint32))
    with pytest.raises(hip.SlimtHipError, match="exceeds"):
        ctx.score(np.zeros((B + 1, S), np.uint32), np.zeros(B + 1, np.uint32), sl, np.zeros((B + 1, T), np.uint32),
                  np.zeros(B + 1, np.uint32))
    bad_ids[0, 3] = t_ids[0, 3]
    bad_ids[1, 6] = m.V  # behind the target's end: not part of the target, not checked, not read into any live row
    ok = ctx.score(ids, lens, sl, bad_ids, t_len, want_align=True, fill=FILL)
    assert np.array_equal(ok[0].view(np.uint32), good[0].view(np.uint32))
    assert np.array_equal(ok[1].view(np.uint32), good[1].view(np.uint32))
    ctx.close()


def test_literal_order_models_are_refused(hip, synth_models):
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    gm.set_kv_cache_format(3)
    ctx = hip.Context(gm, 2, 8)
    with pytest.raises(hip.SlimtHipError, match="format 3"):
        ctx.score(np.ones((2, 8), np.uint32), np.full(2, 8, np.uint32), None, np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32))
    ctx.close()
    gm.close()
