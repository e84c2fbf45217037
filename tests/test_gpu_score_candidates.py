"""GPU tests of candidate scoring (slimt_hip_score_candidates*, slimt_hip_candidates_rank*): N candidate targets over B sources
encoded once (tests/support/candidate_cases.py; tests/test_candidate_case_fixtures.py proves on the CPU that the cases sit
where they claim relative to the attention's run length G and the 8192-row chunks).

The judge is always the CPU checker -- teacher_forced of tests/test_score_checker.py on the DUPLICATED sources in PORTABLE
mode: alignment rows bit for bit, scores within model_values.score_bound, -inf exactly where the checker has it, every entry
the call does not write still the fill, as many non-fill scores as target tokens. In addition every case asserts the
contract itself: scores and alignments are bitwise those of ctx.score on ids[cand_src], from a context made for the
comparison with max_batch >= N."""
import numpy as np
import pytest
import torch

from support import candidate_cases as CC
from support import score_cases as C
from test_alternatives_checker import NONE, alternatives
from test_gpu_forced_prefix import TOL
from test_score_checker import teacher_forced

pytestmark = pytest.mark.gpu
G = CC.G


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def _call(ctx, c, **kw):
    return ctx.score_candidates(c.ids, c.lens, c.sl, c.t_ids, c.t_len, c.cand_src, want_align=True, fill=C.FILL, **kw)


def _same_bits(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    assert np.array_equal(_bits(got[1]), _bits(want[1]))


def _fresh_checker(oracle, m, om, sl):
    """The oracle keeps the cross-attention K / V of its last batch and takes a later batch for the same one when the address,
    B, S and four probed values of the encoder output agree. Batches of DUPLICATED sources that differ in one candidate's
    source agree in all of them (the allocator hands the address out again), so a one-token batch goes through the checker
    before every reference: the next batch never has its B and S."""
    one = np.ones((1, 1), np.uint32)
    teacher_forced(oracle, om, m, one, one[0], sl, one if sl is None else sl[:1].reshape(1, 1), one[0])


def _run(hip, oracle, engines, c, max_batch=None):
    """case c against the checker on the duplicated sources and against ctx.score on them; returns (candidate result,
    the duplicated call's result)"""
    m, gm, om = engines(c.model)
    d = CC.duplicated(c)
    (B, S), N = c.ids.shape, len(c.t_len)
    ctx = hip.Context(gm, max_batch or B, S)
    try:
        got = _call(ctx, c)
    finally:
        ctx.close()
    _fresh_checker(oracle, m, om, d.sl)
    C.check_case(got, C.reference(oracle, m, om, d), d)
    assert int((got[0] != C.FILL).sum()) == int(c.t_len.sum())
    wide = hip.Context(gm, max(N, 1), S)
    try:
        want = wide.score(d.ids, d.lens, d.sl, d.t_ids, d.t_len, want_align=True, fill=C.FILL)
    finally:
        wide.close()
    _same_bits(got, want)
    return got, want


@pytest.fixture(scope="module")
def fan(hip, oracle, engines):
    """the fan case and its result through the blocking host call, checked once"""
    c = CC.fan()
    got, _ = _run(hip, oracle, engines, c)
    return c, got


def test_fan(fan):
    """micro, S 7, T 5: four sources of 7, 1, 4 and 6 tokens with 0, 1, 3 and G + 1 candidates, sorted; target lengths 0, 1, T"""
    c, got = fan
    assert got[0].shape == (sum(CC.FAN_COUNTS), CC.FAN_T)


@pytest.mark.parametrize("how", ["reversed", "interleaved"])
def test_order_changes_no_bit(hip, oracle, engines, fan, how):
    """the same candidates reversed, and interleaved by source: each candidate's outputs are bitwise the sorted call's"""
    c, sorted_got = fan
    perm = np.asarray(CC.order_perms(len(c.t_len))[how])
    got, _ = _run(hip, oracle, engines, CC.permuted(c, perm))
    _same_bits(got, (sorted_got[0][perm], sorted_got[1][perm]))


@pytest.mark.parametrize("name", list(CC.RUN_COUNTS))
def test_runs(hip, oracle, engines, name):
    """one source with G - 1, G, G + 1 and 2 G + 1 candidates; two with G and G (the change on the run's edge) and with G - 1
    and G + 1 (in mid-run)"""
    _run(hip, oracle, engines, CC.runs(name))


@pytest.mark.parametrize("name", list(CC.DEAD_CASES))
def test_dead_candidates(hip, oracle, engines, name):
    """empty candidates first in a run, first of a source (in mid-run and on the edge), last, as a whole run between two
    sources, as a whole source, and as the whole call"""
    _run(hip, oracle, engines, CC.dead(name))


@pytest.mark.parametrize("S", CC.KEY_S)
@pytest.mark.parametrize("model", CC.KEY_MODELS)
def test_key_registers_and_the_largest_lds(hip, oracle, engines, model, S):
    """S = 64, 65, 128 on head sizes 16, 32, 64: sources of S tokens and of one, candidates (0, 1, 0) -- restaged inside a run and back"""
    _run(hip, oracle, engines, CC.keys(model, S))


def test_rows_past_the_128_row_tiles(hip, oracle, engines):
    """mini: 25 candidates x T 41 = 1025 rows over three sources"""
    _run(hip, oracle, engines, CC.rows())


def test_chunks_split_a_source(hip, oracle, engines):
    """micro, T 2731: chunks of two candidates; source 0's three straddle the edge, the second chunk mixes both sources"""
    _run(hip, oracle, engines, CC.chunks())


def test_more_candidates_than_the_context_has_sentences(hip, oracle, engines):
    """max_batch 2, 40 candidates: N is bounded by the row limits alone"""
    c = CC.many()
    _run(hip, oracle, engines, c, max_batch=CC.MANY_B)
    _, gm, _ = engines(c.model)
    ctx = hip.Context(gm, CC.MANY_B, CC.FAN_S)
    try:
        assert _call(ctx, c._replace(t_ids=c.t_ids[:0], t_len=c.t_len[:0], cand_src=c.cand_src[:0]))[0].shape == (0, CC.FAN_T)
        with pytest.raises(hip.SlimtHipError, match="exceeds the context workspace"):  # B is still the context's
            _call(ctx, c._replace(ids=np.repeat(c.ids, 2, axis=0), lens=np.repeat(c.lens, 2)))
    finally:
        ctx.close()


def test_alternatives(hip, oracle, engines, fan):
    """the fan case armed with k = 3: ids, scores and ranks against the alternatives checker on the duplicated sources"""
    c, plain = fan
    m, gm, om = engines(c.model)
    d, k = CC.duplicated(c), 3
    _fresh_checker(oracle, m, om, d.sl)
    want = alternatives(oracle, om, m, d.ids, d.lens, d.sl, d.t_ids, d.t_len, 8)
    ctx = hip.Context(gm, *c.ids.shape)
    try:
        got = _call(ctx, c, alternatives=k)
        again = _call(ctx, c)  # disarmed by the call that took it
    finally:
        ctx.close()
    assert len(again) == 2
    _same_bits(got, plain)
    g_ids, g_sc, g_rank = got[2:]
    worst = 0.0
    for b in range(len(c.t_len)):
        n = int(c.t_len[b])
        assert np.array_equal(g_ids[b, :n], want.ids[b, :n, :k]) and np.array_equal(g_rank[b, :n], want.rank[b, :n]), b
        g, w = g_sc[b, :n].astype(np.float64), want.scores[b, :n, :k]
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), b
        fin = np.isfinite(w)
        worst = max(worst, float(np.abs(g[fin] - w[fin]).max(initial=0)))
        assert np.all(g_ids[b, n:] == NONE) and np.all(g_sc[b, n:] == C.FILL) and np.all(g_rank[b, n:] == NONE), b
    print("alternatives: largest score error", worst)
    assert worst <= TOL, worst


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_entry_points_give_the_same_bits(hip, engines, fan):
    """pinned _async (written in place), pageable _async, _device and _async_generated against the blocking host call"""
    from slimt_amd import synth
    c, host = fan
    m, gm, _ = engines(c.model)
    (B, S), (N, T) = c.ids.shape, c.t_ids.shape
    ctx = hip.Context(gm, B, S)
    try:
        # pinned: the context's own arrays, read and written in place
        bufs = ctx.score_candidates_buffers(B, S, N, T, want_align=True)
        for dst, src in zip(bufs[:5], (c.ids, c.lens, c.t_ids, c.t_len, c.cand_src)):
            dst[...] = src
        bufs[5][...] = C.FILL
        bufs[6][...] = C.FILL
        ctx.score_candidates_async(bufs, c.sl)
        ctx.synchronize()
        _same_bits(bufs[5:], host)
        # pageable
        sc, al = np.full((N, T), C.FILL, np.float32), np.full((N, T, S), C.FILL, np.float32)
        ctx.score_candidates_async((c.ids, c.lens, c.t_ids, c.t_len, c.cand_src, sc, al), c.sl)
        ctx.synchronize()
        _same_bits((sc, al), host)
        # device pointers, and the ranking behind them on the same stream
        d = [_dev(a) for a in (c.ids, c.lens, c.t_ids, c.t_len, c.cand_src)]
        d_sc = torch.full((N, T), float(C.FILL), dtype=torch.float32, device="cuda")
        d_al = torch.full((N, T, S), float(C.FILL), dtype=torch.float32, device="cuda")
        d_tot = torch.zeros(N, dtype=torch.float32, device="cuda")
        d_best = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert c.sl is None  # (micro scores over its full vocabulary)
        ctx.score_candidates_device(d[0].data_ptr(), d[1].data_ptr(), B, S, 0, 0, d[2].data_ptr(), d[3].data_ptr(), T,
                                    d[4].data_ptr(), N, d_sc.data_ptr(), d_al.data_ptr())
        for mean in (False, True):
            ctx.candidates_rank_device(d_sc.data_ptr(), d[3].data_ptr(), d[4].data_ptr(), N, T, B, d_tot.data_ptr(),
                                       d_best.data_ptr(), mean=mean)
            ctx.synchronize()
            tot, best = hip.candidates_rank(host[0], c.t_len, c.cand_src, B, mean=mean)
            assert np.array_equal(_bits(d_tot.cpu().numpy()), _bits(tot))
            assert np.array_equal(d_best.cpu().numpy().view(np.uint32), best)
            w_tot, w_best = CC.rank_reference(host[0], c.t_len, c.cand_src, B, mean)
            assert np.array_equal(_bits(tot), _bits(w_tot)) and np.array_equal(best, w_best)
            assert best[0] == CC.NONE and best[1] == 0  # no candidate; one candidate
        _same_bits((d_sc.cpu().numpy(), d_al.cpu().numpy()), host)
    finally:
        ctx.close()
    # a generated shortlist: against the blocking call with the list the generator gives for the B sources
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    ctx = hip.Context(gm, B, S)
    try:
        sl = gen.generate(c.ids, c.lens)
        assert 0 < sl.size < m.V
        want = ctx.score_candidates(c.ids, c.lens, sl, c.t_ids, c.t_len, c.cand_src, want_align=True, fill=C.FILL)
        sc, al = np.full((N, T), C.FILL, np.float32), np.full((N, T, S), C.FILL, np.float32)
        ctx.score_candidates_async((c.ids, c.lens, c.t_ids, c.t_len, c.cand_src, sc, al), generator=gen)
        ctx.synchronize()
        _same_bits((sc, al), want)
    finally:
        ctx.close()
        gen.close()


def test_device_values_out_of_range_are_clamped(hip, engines, fan):
    """device arrays cannot be checked: a cand_src >= B is taken as B - 1 and a length past T as T; every other candidate
    keeps its bits and nothing outside the arrays is touched (the fill behind them survives)"""
    c, host = fan
    _, gm, _ = engines(c.model)
    (B, S), (N, T) = c.ids.shape, c.t_ids.shape
    src, t_len = c.cand_src.copy(), c.t_len.copy()
    src[3], t_len[2] = 1000, T + 50  # (both live: lengths 5 and 1)
    ctx = hip.Context(gm, B, S)
    try:
        d = [_dev(a) for a in (c.ids, c.lens, c.t_ids, t_len, src)]
        d_sc = torch.full((N + 1, T), float(C.FILL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.score_candidates_device(d[0].data_ptr(), d[1].data_ptr(), B, S, 0, 0, d[2].data_ptr(), d[3].data_ptr(), T,
                                    d[4].data_ptr(), N, d_sc.data_ptr(), 0)
        ctx.synchronize()
        sc = d_sc.cpu().numpy()
        keep = np.ones(N, bool)
        keep[[2, 3]] = False
        assert np.array_equal(_bits(sc[:N][keep]), _bits(host[0][keep]))
        assert np.all(sc[N] == C.FILL) and np.all(sc[2] != C.FILL)
        want = ctx.score_candidates(c.ids, c.lens, c.sl, c.t_ids, np.minimum(t_len, T), np.minimum(src, B - 1), fill=C.FILL)
        assert np.array_equal(_bits(sc[:N]), _bits(want[0]))
    finally:
        ctx.close()


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("N,B", CC.RANK_SIZES)
def test_rank_equals_the_numpy_loop(hip, N, B, mean):
    """crafted scores (no model): NaN and -inf totals, exact ties, +0 against -0, empty candidates, sources without
    candidates, shuffled sources: totals and best exactly the float32 loop's"""
    sc, t_len, src = CC.rank_inputs(N, B, seed=N + B)
    tot, best = hip.candidates_rank(sc, t_len, src, B, mean=mean)
    w_tot, w_best = CC.rank_reference(sc, t_len, src, B, mean)
    assert np.array_equal(_bits(tot), _bits(w_tot))
    assert np.array_equal(best, w_best), np.flatnonzero(best != w_best)[:8]
    perm = np.random.default_rng(N).permutation(N)  # any order of the candidates: the same winners
    _, p_best = hip.candidates_rank(sc[perm], t_len[perm], src[perm], B, mean=mean)
    back = np.where(p_best == CC.NONE, CC.NONE, perm[np.minimum(p_best, N - 1)])
    keys = CC.rank_reference(sc, t_len, src, B, mean)[0]
    for b in range(B):
        if best[b] == CC.NONE:
            assert back[b] == CC.NONE
        else:  # the permuted call may pick another member of a tie: the same key
            kb, kp = (keys[x] / np.float32(t_len[x]) if mean else keys[x] for x in (best[b], back[b]))
            assert kb == kp and src[back[b]] == b


# ---- the service and the text front end -------------------------------------------------------------------------------------
def test_batch_service_candidates_equal_the_pair_scores(hip, synth_models):
    """about 40 ragged sources with 0 to 5 candidates each (empty candidates among them): per candidate bitwise what
    BatchService.score gives for the pair; totals and best equal the numpy loop's, in both modes"""
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(15))
    n = 40
    sents = [list(rnd.integers(3, m.V, int(rnd.integers(1, 20)))) + [0] for _ in range(n)]
    fixed = synth.make_shortlist(m.V, 2048)
    cands = [[[int(x) for x in rnd.choice(fixed, size=int(rnd.integers(0, 2 * len(s))))] for _ in range(i % 6)]
             for i, s in enumerate(sents)]
    cands[7][0] = []  # an empty candidate beside live ones
    cands[5] = [[], [], [], [], []]  # a source whose candidates are all empty
    assert {len(c) for c in cands} == set(range(6))
    svc = hip.BatchService([gm], max_words=8 * 21, workers_per_device=1, shortlist=fixed)
    try:
        res, c_off, totals, best = svc.score_candidates(sents, cands)
        _, _, totals_m, best_m = mean = svc.score_candidates(sents, cands, mean=True)
        flat_src = [sents[i] for i in range(n) for _ in cands[i]]
        flat_tgt = [t for cs in cands for t in cs]
        pairs = svc.score(flat_src, flat_tgt)
        assert res.n == len(flat_tgt) == int(c_off[-1]) and list(np.diff(c_off)) == [len(c) for c in cands]
        assert len(set(int(b) for b in res.batch)) >= 2
        assert np.array_equal(res.targets, pairs.targets) and np.array_equal(res.target_offsets, pairs.target_offsets)
        assert np.array_equal(_bits(res.scores), _bits(pairs.scores))
        assert np.array_equal(_bits(res.alignments), _bits(pairs.alignments))
        assert np.array_equal(_bits(mean[0].scores), _bits(res.scores))
        N, T = res.n, max(1, max(len(t) for t in flat_tgt))
        sc = np.zeros((N, T), np.float32)
        for e in range(N):
            sc[e, :len(flat_tgt[e])] = res.token_scores(e)
        t_len = np.asarray([len(t) for t in flat_tgt], np.uint32)
        src = np.repeat(np.arange(n, dtype=np.uint32), np.diff(c_off).astype(np.int64))
        for mode, (tot, bst) in ((False, (totals, best)), (True, (totals_m, best_m))):
            w_tot, w_best = CC.rank_reference(sc, t_len, src, n, mode)
            assert np.array_equal(_bits(tot), _bits(w_tot))
            local = np.where(w_best == CC.NONE, CC.NONE, w_best.astype(np.int64) - c_off[:-1].astype(np.int64)).astype(np.uint32)
            assert np.array_equal(bst, local)
        assert best[0] == CC.NONE and best[5] == CC.NONE and best[1] == 0
        with pytest.raises(hip.SlimtHipError, match="not a result of"):
            pairs.candidates(n)
        pairs.close()
        res.close()
        mean[0].close()
        with pytest.raises(ValueError):
            svc.score_candidates(sents, cands[:-1])
    finally:
        svc.close()
        gm.close()


def test_frontend_rerank(hip):
    """Service.rerank on three sentences: the candidates' PairScores are those of Service.score on the pairs, the best index
    is the argmax of their float32 totals (by the sum, and per token)"""
    import io
    import random
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
        sources = corpus[:3]
        candidates = [corpus[100:103], [], corpus[200:202]]
        for mean in (False, True):
            ranked = svc.rerank(model, sources, candidates, mean=mean)
            assert [len(p) for p, _ in ranked] == [3, 0, 2] and ranked[1][1] is None
            for i, (pairs, best) in enumerate(ranked):
                if not pairs:
                    continue
                want = svc.score(model, [sources[i]] * len(pairs), candidates[i])
                keys = []
                for p, q in zip(pairs, want):
                    assert p.source_ids == q.source_ids and p.target_ids == q.target_ids
                    assert np.array_equal(_bits(p.token_scores), _bits(q.token_scores))
                    assert np.array_equal(_bits(p.alignment), _bits(q.alignment))
                    tot = np.float32(0)
                    for x in p.token_scores:
                        tot = np.float32(tot + x)
                    keys.append(tot / np.float32(len(p.token_scores)) if mean else tot)
                assert best == int(np.argmax(keys))
        with pytest.raises(ValueError):
            svc.rerank(model, sources, candidates[:2])
    finally:
        svc.close()
        model.close()
