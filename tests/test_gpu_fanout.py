"""GPU parity of fan-out translate calls (include/slimt_hip.h, slimt_hip_translate_fanout*): N decoder rows over B sources
encoded once. A fan-out call's checker is an existing checker on the duplicated batch ids[row_src], lens[row_src]; its other
reference is slimt_hip_translate itself on that batch. For every row:
  * tokens, lengths and alignment bits equal the checker's, scores are within 5e-5 * max(1, 1 / T) of its float64;
  * tokens, lengths, alignment bits AND score bits equal the duplicated call's in decode mode 1 (the same decoder kernels);
  * tokens, lengths and alignment bits equal the duplicated call's in decode mode 0.
The cases and what they are for: tests/support/fanout_cases.py (tests/test_fanout_case_fixtures.py proves them on the CPU)."""
import numpy as np
import pytest
import torch

from support import fanout_cases as FC
from test_forced_prefix_checker import forced_translate, tmax_of
from test_sampling_checker import keys_of, sampled_translate
from test_truncation_checker import truncated_translate

pytestmark = pytest.mark.gpu

TOL = 5e-5


@pytest.fixture(scope="module")
def engines(hip, oracle, synth_models):
    cache = {}

    def get(c):
        key = (c.preset, c.dims, c.eos_bias, c.model_seed)
        if key not in cache:
            m = FC.model_of(c, synth_models)
            cache[key] = (m, hip.Model(m), oracle.OracleModel(m))
        return cache[key]

    yield get
    for _, gm, _ in cache.values():
        gm.close()


_INPUTS = {}


def _inputs(c, m):
    """(ids, lens, shortlist, keys, duplicated ids, duplicated lens, prefix ids, prefix lens) of a case, made once"""
    if c.name not in _INPUTS:
        ids, lens, sl, keys = FC.inputs(c, m.V)
        _INPUTS[c.name] = (ids, lens, sl, keys) + FC.duplicated(ids, lens, c.row_src) + FC.prefixes(c, m.V, sl, tmax_of(c.S))
    return _INPUTS[c.name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, scores, what):
    """tokens, lengths, alignment bits (and score bits) of two device results"""
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what
    if scores:  # (of the recorded tokens: a translate call leaves the rest of a row as it finds it)
        live = np.arange(got[0].shape[1])[None, :] < got[1][:, None]
        assert np.array_equal(_bits(got[3])[live], _bits(want[3])[live]), what


def _against_checker(got, want, T, scores):
    out, ln, al = got[:3]
    w_out, w_ln, w_al, w_sc = want
    assert np.array_equal(ln, w_ln), (ln, w_ln)
    assert np.array_equal(out, w_out)
    assert np.array_equal(_bits(al), _bits(w_al))
    if scores:
        tol = TOL * max(1.0, 1.0 / T)
        worst = 0.0
        for b in range(len(ln)):
            n = int(ln[b])
            g, w = got[3][b, :n].astype(np.float64), w_sc[b, :n]
            assert np.array_equal(np.isneginf(g), np.isneginf(w)), (b, g, w)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (b, g, w)
            fin = np.isfinite(w)
            worst = max(worst, np.abs(g[fin] - w[fin]).max(initial=0))
        print("scores: max |gpu - float64| = %.3g (bound %.3g)" % (worst, tol))
        assert worst <= tol, worst


# kind -> (keyword arguments of the translate wrappers, the checker on the duplicated batch, temperature of the score bound)
def _kind(kind, oracle, om, m, inp):
    ids, lens, sl, keys, d_ids, d_lens, p_ids, p_len = inp
    none = np.zeros_like(p_len)
    if kind == "greedy":
        return dict(), lambda: forced_translate(oracle, om, m, d_ids, d_lens, sl, p_ids, none), 1.0
    if kind == "scored":
        return dict(scores=True), lambda: forced_translate(oracle, om, m, d_ids, d_lens, sl, p_ids, none), 1.0
    if kind in ("sampled0.7", "sampled1.0"):
        T = float(kind[7:])
        return dict(scores=True, sampling=(T, keys)), lambda: sampled_translate(oracle, om, m, d_ids, d_lens, sl, keys, T), T
    if kind == "truncated":
        return (dict(scores=True, sampling=(1.0, keys), truncation=(FC.TOP_K, FC.TOP_P)),
                lambda: truncated_translate(oracle, om, m, d_ids, d_lens, sl, keys, 1.0, FC.TOP_K, FC.TOP_P), 1.0)
    if kind == "forced":
        return dict(scores=True, prefix=(p_ids, p_len)), lambda: forced_translate(oracle, om, m, d_ids, d_lens, sl, p_ids, p_len), 1.0
    assert kind == "sampled+forced"
    return (dict(scores=True, sampling=(1.0, keys), prefix=(p_ids, p_len)),
            lambda: sampled_translate(oracle, om, m, d_ids, d_lens, sl, keys, 1.0, p_ids, p_len), 1.0)


KINDS = ["greedy", "scored", "sampled0.7", "sampled1.0", "truncated", "forced", "sampled+forced"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [c.name for c in FC.PARITY])
def test_fanout_equals_the_checker_and_the_duplicated_call(hip, oracle, engines, name, kind):
    c = FC.parity(name)
    m, gm, om = engines(c)
    inp = _inputs(c, m)
    ids, lens, sl, keys, d_ids, d_lens = inp[:6]
    kw, checker, T = _kind(kind, oracle, om, m, inp)
    scores = "scores" in kw
    N = c.row_src.size
    ctx = hip.Context(gm, max(N, c.B), c.S)
    try:
        got = ctx.translate_fanout(ids, lens, c.row_src, sl, want_align=True, **kw)
        assert got[0].shape == (N, tmax_of(c.S)) and got[2].shape == (N, tmax_of(c.S), c.S)
        _against_checker(got, checker(), T, scores)
        ctx.set_decode_mode(1)
        _same_bits(got, ctx.translate(d_ids, d_lens, sl, want_align=True, **kw), scores, "duplicated, mode 1")
        ctx.set_decode_mode(0)
        _same_bits(got, ctx.translate(d_ids, d_lens, sl, want_align=True, **kw), False, "duplicated, mode 0")
    finally:
        ctx.close()


def _sampled(ctx, ids, lens, row_src, sl, keys, T=1.0):
    return ctx.translate_fanout(ids, lens, row_src, sl, want_align=True, scores=True, sampling=(T, keys))


def _duplicated_mode1(ctx, ids, lens, row_src, sl, **kw):
    d_ids, d_lens = FC.duplicated(ids, lens, row_src)
    ctx.set_decode_mode(1)
    try:
        return ctx.translate(d_ids, d_lens, sl, want_align=True, **kw)
    finally:
        ctx.set_decode_mode(0)


@pytest.mark.parametrize("name", sorted(FC.edges()))
def test_tiling_edges_equal_the_duplicated_call(hip, engines, name):
    """runs that cross the 16-row workgroup boundary, dead waves, sources without rows, one staging per row: sampled, scored
    and aligned, bit for bit the step-wise translate of the duplicated batch"""
    c = FC.edge_case(name)
    m, gm, _ = engines(c)
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    ctx = hip.Context(gm, max(N, c.B), c.S)
    try:
        got = _sampled(ctx, ids, lens, c.row_src, sl, keys)
        _same_bits(got, _duplicated_mode1(ctx, ids, lens, c.row_src, sl, scores=True, sampling=(1.0, keys)), True, name)
        greedy = ctx.translate_fanout(ids, lens, c.row_src, sl, want_align=True, scores=True)
        _same_bits(greedy, _duplicated_mode1(ctx, ids, lens, c.row_src, sl, scores=True), True, name + ", greedy")
        if name == "arange":  # plain translate, with 16 stagings per workgroup
            ctx.set_decode_mode(1)
            _same_bits(greedy, ctx.translate(ids, lens, sl, want_align=True, scores=True), True, "plain translate")
    finally:
        ctx.close()


def test_shuffled_rows_keep_their_bits(hip, engines):
    c = FC.edge_case("n33")
    m, gm, _ = engines(c)
    ids, lens, sl, keys = FC.inputs(c, m.V)
    perm = np.random.default_rng(9).permutation(c.row_src.size)
    ctx = hip.Context(gm, c.row_src.size, c.S)
    try:
        want = _sampled(ctx, ids, lens, c.row_src, sl, keys)
        got = _sampled(ctx, ids, lens, c.row_src[perm], sl, np.ascontiguousarray(keys[perm]))
        _same_bits(got, tuple(np.ascontiguousarray(a[perm]) for a in want), True, "shuffled")
    finally:
        ctx.close()


def test_one_source_with_seventeen_rows_and_one_token_sources(hip, engines):
    for c in (FC.single_source(), FC.one_token()):
        m, gm, _ = engines(c)
        ids, lens, sl, keys = FC.inputs(c, m.V)
        ctx = hip.Context(gm, c.row_src.size, c.S)
        try:
            got = _sampled(ctx, ids, lens, c.row_src, sl, keys)
            _same_bits(got, _duplicated_mode1(ctx, ids, lens, c.row_src, sl, scores=True, sampling=(1.0, keys)), True, c.name)
        finally:
            ctx.close()


def test_greedy_rows_of_a_source_are_that_sources_plain_translation(hip, engines):
    c = FC.parity("s32")
    m, gm, _ = engines(c)
    ids, lens, sl, _ = FC.inputs(c, m.V)
    ctx = hip.Context(gm, c.row_src.size, c.S)
    try:
        got = ctx.translate_fanout(ids, lens, c.row_src, sl, want_align=True, scores=True)
        ctx.set_decode_mode(1)
        plain = ctx.translate(ids, lens, sl, want_align=True, scores=True)
        _same_bits(got, tuple(a[c.row_src] for a in plain), True, "plain rows")
        assert len({tuple(plain[0][b, :plain[1][b]]) for b in range(c.B)}) == c.B  # (the sources do differ)
    finally:
        ctx.close()


def test_literal_kv_format_and_every_decode_mode(hip, engines, synth_models):
    """K/V cache format 3 decodes with the same kernels; the context's mode set beforehand changes nothing, and neither the
    plan nor the last decoder plan changes with a fan-out call"""
    c = FC.parity("s8")
    m, gm, _ = engines(c)
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    ctx = hip.Context(gm, N, c.S)
    try:
        ctx.translate(ids, lens, sl)  # (a persistent decoder launch: its plan is what must stay)
        want = None
        for mode in (0, 1, 3):
            ctx.set_decode_mode(mode)
            plan, dplan = ctx.plan(c.S), ctx.debug_decoder_plan()
            got = _sampled(ctx, ids, lens, c.row_src, sl, keys)
            assert ctx.plan(c.S) == plan and ctx.debug_decoder_plan() == dplan, mode
            want = want or got
            _same_bits(got, want, True, "mode %d" % mode)
    finally:
        ctx.close()
    lit = hip.Model(m)
    lit.set_kv_cache_format(3)
    ctx = hip.Context(lit, N, c.S)
    try:
        got = _sampled(ctx, ids, lens, c.row_src, sl, keys)
        d_ids, d_lens = FC.duplicated(ids, lens, c.row_src)
        _same_bits(got, ctx.translate(d_ids, d_lens, sl, want_align=True, scores=True, sampling=(1.0, keys)), True, "format 3")
    finally:
        ctx.close()
        lit.close()


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).cuda()


def test_every_entry_point_writes_the_same_bits_and_nothing_leaks(hip, oracle, engines):
    from slimt_amd import synth
    c = FC.parity("s8")
    m, gm, _ = engines(c)
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N, B, S, Tm = c.row_src.size, c.B, c.S, tmax_of(c.S)
    p_ids, p_len = FC.prefixes(c, m.V, sl, Tm)
    kw = dict(scores=True, sampling=(1.0, keys), prefix=(p_ids, p_len))
    ctx = hip.Context(gm, N, S)
    try:
        before = ctx.translate(ids, lens, sl, want_align=True, scores=True)
        want = ctx.translate_fanout(ids, lens, c.row_src, sl, want_align=True, **kw)  # pageable
        _same_bits(ctx.translate(ids, lens, sl, want_align=True, scores=True), before, True, "plain translate afterwards")
        _same_bits(ctx.translate_fanout_pinned(ids, lens, c.row_src, sl, want_align=True, **kw), want, True, "pinned, async")
        no_sc = ctx.translate_fanout_pinned(ids, lens, c.row_src, sl, want_align=True, sampling=(1.0, keys), prefix=(p_ids, p_len))
        _same_bits(no_sc, want, False, "no destination armed")
        # keys = None: the row indices
        rows = ctx.translate_fanout(ids, lens, c.row_src, sl, want_align=True, scores=True, sampling=(1.0, None))
        _same_bits(rows, _sampled(ctx, ids, lens, c.row_src, sl, np.arange(N, dtype=np.uint64)), True, "row-index keys")
        # device arrays, device keys, device prefix; a row_src out of range is clamped and disturbs no other row
        bad = c.row_src.copy()
        bad[3] = B + 7
        d_ids, d_len, d_sl, d_keys, d_pi, d_pl = _dev(ids), _dev(lens), _dev(sl), _dev(keys), _dev(p_ids), _dev(p_len)
        d_out = torch.zeros((N, Tm), dtype=torch.int32, device="cuda")
        d_ol = torch.zeros((N,), dtype=torch.int32, device="cuda")
        d_sc = torch.zeros((N, Tm), dtype=torch.float32, device="cuda")
        d_al = torch.zeros((N, Tm, S), dtype=torch.float32, device="cuda")
        for src, rows_checked in ((c.row_src, np.arange(N)), (bad, np.delete(np.arange(N), 3))):
            d_src = _dev(src)
            ctx.translate_fanout_device(d_ids.data_ptr(), d_len.data_ptr(), B, S, d_src.data_ptr(), N, d_sl.data_ptr(), sl.size,
                                        1.5, 0, d_out.data_ptr(), d_ol.data_ptr(), d_al.data_ptr(), steps_hint=Tm,
                                        scores=d_sc.data_ptr(), sampling=(1.0, d_keys.data_ptr()),
                                        prefix=(d_pi.data_ptr(), d_pl.data_ptr()))
            ctx.synchronize()
            got = (d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), d_al.cpu().numpy(), d_sc.cpu().numpy())
            n = got[1]
            for r in rows_checked:  # (the device call writes scores of recorded tokens only)
                assert n[r] == want[1][r] and np.array_equal(got[0][r], want[0][r]), r
                assert np.array_equal(_bits(got[2][r]), _bits(want[2][r])), r
                assert np.array_equal(_bits(got[3][r, :n[r]]), _bits(want[3][r, :n[r]])), r
        clamped = ctx.translate_fanout(ids, lens, np.where(bad >= B, B - 1, bad).astype(np.uint32), sl, want_align=True, **kw)
        assert np.array_equal(got[0][3], clamped[0][3]) and got[1][3] == clamped[1][3]  # (B + 7 read source B - 1)
        # a generated lexical shortlist: from the B sources given, rows or not
        blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
        gen = hip.ShortlistGenerator(blob, m.V, m.V)
        try:
            osl = oracle.OracleShortlist(blob, m.V, m.V).generate(ids, lens)
            gp = FC.prefixes(c, m.V, osl, Tm)
            gkw = dict(scores=True, sampling=(1.0, keys), prefix=gp)
            few = FC.sorted_src([0, 5, 4, 4, 4])  # (source 0 has no row and still contributes its words)
            fk = np.ascontiguousarray(keys[: few.size])
            fkw = dict(scores=True, sampling=(1.0, fk), prefix=(gp[0][: few.size], gp[1][: few.size]))
            _same_bits(ctx.translate_fanout_pinned(ids, lens, c.row_src, generator=gen, want_align=True, **gkw),
                       ctx.translate_fanout(ids, lens, c.row_src, osl, want_align=True, **gkw), True, "generated")
            _same_bits(ctx.translate_fanout_pinned(ids, lens, few, generator=gen, want_align=True, **fkw),
                       ctx.translate_fanout(ids, lens, few, osl, want_align=True, **fkw), True, "generated, a source without rows")
        finally:
            gen.close()
        _same_bits(ctx.translate(ids, lens, sl, want_align=True, scores=True), before, True, "plain translate at the end")
    finally:
        ctx.close()


def test_refusals_consume_what_was_armed(hip, engines):
    c = FC.parity("s8")
    m, gm, _ = engines(c)
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    ctx = hip.Context(gm, N, c.S)
    try:
        bad = c.row_src.copy()
        bad[-1] = c.B
        with pytest.raises(hip.SlimtHipError, match="names source"):
            _sampled(ctx, ids, lens, bad, sl, keys)
        with pytest.raises(hip.SlimtHipError, match="max_batch"):
            ctx.translate_fanout(ids, lens, np.zeros(N + 1, np.uint32), sl, sampling=(1.0, None))
        # (the sampling armed by the refused calls is gone: a plain call is greedy again)
        plain = ctx.translate(ids, lens, sl, want_align=True, scores=True)
        _same_bits(ctx.translate(ids, lens, sl, want_align=True, scores=True), plain, True, "greedy twice")
        again = ctx.translate_fanout(ids, lens, np.arange(c.B, dtype=np.uint32), sl, want_align=True, scores=True)
        _same_bits(again, plain, False, "fan-out of every source once is greedy too")
    finally:
        ctx.close()


# ---- the service and the text front end -------------------------------------------------------------------------------------
def test_batch_service_samples_equal_the_per_sentence_fanout_whatever_the_batches(hip, synth_models):
    """sample j of sentence i is row j of a fan-out call on that sentence alone under sampling_key(seed, i * n + j): with
    every sentence in one batch, in batches of four, and with a batch split because n * its sentences exceed max_words"""
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(15))
    L, count, n, seed = 9, 12, 3, 5
    sents = [list(rnd.integers(3, m.V, L - 1)) + [0] for _ in range(count)]  # (one length: the padding is the sentence's own)
    fixed = synth.make_shortlist(m.V, 2048)
    Tm = tmax_of(L)
    ctx = hip.Context(gm, 20, L)
    lens = np.full(1, L, np.uint32)

    def alone(i, n):
        keys = np.asarray([hip.sampling_key(seed, i * n + j) for j in range(n)], np.uint64)
        return ctx.translate_fanout(np.asarray([sents[i]], np.uint32), lens, np.zeros(n, np.uint32), fixed, want_align=True,
                                    scores=True, sampling=(1.0, keys))

    def check(res, which, n):
        assert res.n == len(which) * n
        for k, i in enumerate(which):
            out, ln, al, sc = alone(i, n)
            for j in range(n):
                e, t = k * n + j, int(ln[j])
                assert np.array_equal(res.target(e), out[j, :t]), (i, j)
                assert np.array_equal(_bits(res.token_scores(e)), _bits(sc[j, :t])), (i, j)
                assert np.array_equal(_bits(res.alignment(e)), _bits(al[j, :t, :L])), (i, j)

    try:
        batches = []
        for max_words in (40, 200):  # B * 9 <= max_words: batches of four sentences, and all twelve in one
            svc = hip.BatchService([gm], max_words=max_words, wrap_length=16, workers_per_device=1, shortlist=fixed, temperature=1.0)
            try:
                res = svc.translate_samples(sents, n, seed=seed)
                batches.append(len(set(int(b) for b in res.batch)))
                check(res, range(count), n)
                res.close()
                if max_words == 40:  # 20 rows each: two sentences per call, so the batch of three goes as two calls
                    res = svc.translate_samples(sents[:3], 20, seed=seed)
                    assert len(set(int(b) for b in res.batch)) == 2
                    check(res, range(3), 20)
                    res.close()
                    with pytest.raises(hip.SlimtHipError, match="samples per sentence"):
                        svc.translate_samples(sents[:3], 41, seed=seed)
                    with pytest.raises(hip.SlimtHipError, match="samples per sentence"):
                        svc.translate_samples(sents[:3], 0, seed=seed)
            finally:
                svc.close()
        assert batches == [3, 1]
        greedy = hip.BatchService([gm], max_words=200, wrap_length=16, workers_per_device=1, shortlist=fixed)
        try:
            with pytest.raises(hip.SlimtHipError, match="does not sample"):
                greedy.translate_samples(sents, n)
        finally:
            greedy.close()
    finally:
        ctx.close()
        gm.close()


def test_frontend_samples_and_sample_and_rerank(hip):
    """translate(samples=n): n alternatives per text, reproducible for a seed, alternative 0 the Response itself;
    sample_and_rerank is that call followed by rerank of the alternatives' texts"""
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
        sources, n, sampling = corpus[:3], 4, (1.0, 11)
        got = svc.translate(model, sources, sampling=sampling, samples=n)
        again = svc.translate(model, sources, sampling=sampling, samples=n)
        assert len(got) == 3
        for r, q in zip(got, again):
            assert len(r.samples) == n and r.samples[0] is r
            assert [a.target.text for a in r.samples] == [a.target.text for a in q.samples]
            # (every alternative covers the text's segments, each with its scores and alignment)
            assert all(len(a.token_scores) == len(a.alignments) == len(r.alignments) >= 1 for a in r.samples)
        assert any(len({a.target.text for a in r.samples}) > 1 for r in got)  # (the alternatives are draws of their own)
        responses, ranked = svc.sample_and_rerank(model, sources, n, sampling)
        texts = [[a.target.text for a in r.samples] for r in got]
        assert [[a.target.text for a in r.samples] for r in responses] == texts
        want = svc.rerank(model, sources, texts)
        for (pairs, best), (w_pairs, w_best) in zip(ranked, want):
            assert best == w_best and len(pairs) == n
            for p, q in zip(pairs, w_pairs):
                assert p.target_ids == q.target_ids and np.array_equal(_bits(p.token_scores), _bits(q.token_scores))
        with pytest.raises(ValueError):
            svc.translate(model, sources, samples=n)
    finally:
        svc.close()
        model.close()
