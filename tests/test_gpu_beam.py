"""GPU parity of beam search (include/slimt_hip.h, slimt_hip_translate_beam*): every output -- ids, lengths, order, totals,
token scores, alignment rows -- bit for bit against `beam_translate` (tests/support/beam_cases.py: the contract over the
oracle's decode_step), the entry points against each other, and cross-checks that need no new checker: beam 1 against
slimt_hip_translate in decode mode 1, every hypothesis rescored by slimt_hip_score_candidates, slimt_hip_candidates_rank
over the token scores. The cases and what they are for: tests/support/beam_cases.py (tests/test_beam_case_fixtures.py
proves them on the CPU)."""
import numpy as np
import pytest
import torch

from support import beam_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(hip, oracle, synth_models):
    cache = {}

    def get(c):
        key = (c.preset, c.dims, c.eos_bias, c.model_seed, c.kv_format)
        if key not in cache:
            m = BC.model_of(c, synth_models)
            gm = hip.Model(m)
            if c.kv_format is not None:
                gm.set_kv_cache_format(c.kv_format)
            cache[key] = (m, gm, oracle.OracleModel(m))
        return cache[key]

    yield get
    for _, gm, _ in cache.values():
        gm.close()


_WANT = {}


def _case(c, oracle, engines):
    """(model, device model, inputs, the checker's result) of a case; the reference is computed once and left unchanged"""
    m, gm, om = engines(c)
    if c.name not in _WANT:
        ids, lens, sl = BC.inputs(c, m.V)
        want = BC.beam_translate(oracle, om, m, ids, lens, sl, c.k, c.mode)
        for a in want:
            a.setflags(write=False)
        _WANT[c.name] = (ids, lens, sl, want)
    return (m, gm) + _WANT[c.name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """ids, lengths, totals, token scores, alignment rows of two results: the recorded entries bit for bit"""
    out, ln, tot, sc, al = got
    w_out, w_ln, w_tot, w_sc, w_al = want
    assert np.array_equal(ln, w_ln), (what, ln, w_ln)
    assert np.array_equal(_bits(tot), _bits(w_tot)), (what, tot, w_tot)
    live = np.arange(out.shape[2])[None, None, :] < ln[:, :, None]
    assert np.array_equal(out[live], w_out[live]), what
    if sc is not None and w_sc is not None:
        assert np.array_equal(_bits(sc)[live], _bits(w_sc)[live]), what
    if al is not None and w_al is not None:
        assert np.array_equal(_bits(al)[live], _bits(w_al)[live]), what


def _ctx(hip, gm, c):
    return hip.Context(gm, c.max_batch or c.B * c.k + 3, c.S)


@pytest.mark.parametrize("name", [c.name for c in BC.PARITY])
def test_beam_equals_the_checker(hip, oracle, engines, name):
    c = BC.parity(name)
    m, gm, ids, lens, sl, want = _case(c, oracle, engines)
    ctx = _ctx(hip, gm, c)
    try:
        got = ctx.translate_beam(ids, lens, c.k, sl, mean=c.mode == 1, want_align=True)
        T = BC.tmax_of(c.S)
        assert got[0].shape == (c.B, c.k, T) and got[4].shape == (c.B, c.k, T, c.S)
        _same(got, want, name)
        # what the search does not write stays as the call zeroed it
        dead = ~(np.arange(T)[None, None, :] < got[1][:, :, None])
        assert not got[0][dead].any() and not _bits(got[4])[dead].any() and not _bits(got[3])[dead].any()
    finally:
        ctx.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()


def test_entry_points_give_the_same_bits(hip, oracle, engines):
    c = BC.parity("k6")
    m, gm, ids, lens, sl, want = _case(c, oracle, engines)
    B, S, k, T = c.B, c.S, c.k, BC.tmax_of(c.S)
    ctx = _ctx(hip, gm, c)
    try:
        _same(ctx.translate_beam_pinned(ids, lens, k, sl, want_align=True), want, "_async, pinned")
        bufs = (ids, lens, np.zeros((B, k, T), np.uint32), np.zeros((B, k), np.uint32), np.zeros((B, k), np.float32),
                np.zeros((B, k, T), np.float32), np.zeros((B, k, T, S), np.float32))
        ctx.translate_beam_async(bufs, sl)
        ctx.synchronize()
        _same(bufs[2:], want, "_async, pageable")
        d_ids, d_len, d_sl = _dev(ids), _dev(lens), _dev(sl)
        for hint in (0, T):
            d_out = torch.zeros((B, k, T), dtype=torch.int32, device="cuda")
            d_ol = torch.zeros((B, k), dtype=torch.int32, device="cuda")
            d_tot = torch.zeros((B, k), dtype=torch.float32, device="cuda")
            d_sc = torch.zeros((B, k, T), dtype=torch.float32, device="cuda")
            d_al = torch.zeros((B, k, T, S), dtype=torch.float32, device="cuda")
            ctx.translate_beam_device(d_ids.data_ptr(), d_len.data_ptr(), B, S, k, d_sl.data_ptr(), sl.size, 1.5, 0,
                                      d_out.data_ptr(), d_ol.data_ptr(), d_tot.data_ptr(), d_sc.data_ptr(), d_al.data_ptr(),
                                      steps_hint=hint)
            ctx.synchronize()
            got = (d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), d_tot.cpu().numpy(),
                   d_sc.cpu().numpy(), d_al.cpu().numpy())
            _same(got, want, "_device, steps_hint %d" % hint)
    finally:
        ctx.close()


def test_generated_shortlist_variant_equals_the_listed_call(hip, oracle, engines):
    from slimt_amd import synth
    c = BC.parity("k6")
    m, gm, ids, lens, _, _ = _case(c, oracle, engines)
    blob = synth.make_lexical_shortlist(m.V, m.V, frequent=64, best=8, seed=5)
    gen = hip.ShortlistGenerator(blob, m.V, m.V, shared=False, check=False)
    ctx = _ctx(hip, gm, c)
    try:
        sl = gen.generate(ids, lens)
        want = ctx.translate_beam(ids, lens, c.k, sl, want_align=True)
        _same(ctx.translate_beam_generated(gen, ids, lens, c.k, want_align=True), want, "_async_generated")
        _same(ctx.translate_beam_pinned(ids, lens, c.k, generator=gen, want_align=True), want, "_async_generated, pinned")
    finally:
        ctx.close()
        gen.close()


# ---- cross-checks against what the library already has --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k6", "full"])
def test_beam_one_is_greedy_translate_in_decode_mode_1(hip, oracle, engines, name):
    c = BC.parity(name)
    m, gm, ids, lens, sl, _ = _case(c, oracle, engines)
    ctx = _ctx(hip, gm, c)
    try:
        out, ln, tot, sc, al = ctx.translate_beam(ids, lens, 1, sl, want_align=True)
        ctx.set_decode_mode(1)
        w_out, w_ln, w_al = ctx.translate(ids, lens, sl, want_align=True)
        assert np.array_equal(ln[:, 0], w_ln) and np.array_equal(out[:, 0], w_out)
        assert np.array_equal(_bits(al[:, 0]), _bits(w_al))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["k6", "mean", "base"])
def test_rescoring_and_ranking_reproduce_the_search(hip, oracle, engines, name):
    """every returned hypothesis, scored teacher-forced from its source: the alignment rows are the scorer's bit for bit
    (its contract with the step-wise decoder: a wrong state reorder or a wrong walk cannot hide), its scores are within
    1e-4 of the token scores (each side within the project's 5e-5 of float64); the ranking over the token scores
    reproduces the totals bit for bit and picks rank 0."""
    c = BC.parity(name)
    m, gm, ids, lens, sl, _ = _case(c, oracle, engines)
    ctx = _ctx(hip, gm, c)
    try:
        out, ln, tot, sc, al = ctx.translate_beam(ids, lens, c.k, sl, mean=c.mode == 1, want_align=True)
        B, k, T = out.shape
        alive = (ln > 0).reshape(-1)
        tgt, tl = out.reshape(B * k, T)[alive], ln.reshape(-1)[alive]
        src = np.repeat(np.arange(B, dtype=np.uint32), k)[alive]
        r_sc, r_al = ctx.score_candidates(ids, lens, sl, tgt, tl, src, want_align=True, fill=0.0)
        live = np.arange(T)[None, :] < tl[:, None]
        assert np.array_equal(_bits(r_al)[live], _bits(al.reshape(B * k, T, -1)[alive])[live])
        worst = np.abs(r_sc[live].astype(np.float64) - sc.reshape(B * k, T)[alive][live]).max()
        print("rescored against token scores: worst %.3g (bound 1e-4)" % worst)
        assert worst <= 1e-4
        totals, best = hip.candidates_rank(sc.reshape(B * k, T)[alive], tl, src, B, mean=c.mode == 1)
        assert np.array_equal(_bits(totals), _bits(tot.reshape(-1)[alive]))
        first = np.concatenate([[0], np.cumsum((ln > 0).sum(axis=1))[:-1]])
        assert np.array_equal(best, first.astype(np.uint32))
    finally:
        ctx.close()


def test_kv_cache_format_3(hip, oracle, engines):
    """The literal float order of the cross-attention (K/V cache format 3) is not PORTABLE's, so no oracle mode has its
    bits: the beam call on such a model is compared with the device's own step-wise translate (beam 1: tokens, lengths,
    alignment bits) and with itself (totals are the ascending sums of the token scores, which slimt_hip_candidates_rank
    reproduces bit for bit; the hypotheses are sorted and distinct; a source alone gives the same bits)."""
    c = BC.KV3
    m, gm, _ = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    ctx = _ctx(hip, gm, c)
    try:
        out, ln, tot, sc, al = ctx.translate_beam(ids, lens, 1, sl, want_align=True)
        ctx.set_decode_mode(1)
        w_out, w_ln, w_al = ctx.translate(ids, lens, sl, want_align=True)
        assert np.array_equal(ln[:, 0], w_ln) and np.array_equal(out[:, 0], w_out) and np.array_equal(_bits(al[:, 0]), _bits(w_al))
        got = ctx.translate_beam(ids, lens, c.k, sl, want_align=True)
        out, ln, tot, sc, al = got
        B, k, T = out.shape
        assert (ln > 0).all()
        totals, best = hip.candidates_rank(sc.reshape(B * k, T), ln.reshape(-1), np.repeat(np.arange(B, dtype=np.uint32), k), B)
        assert np.array_equal(_bits(totals), _bits(tot.reshape(-1))) and np.array_equal(best, np.arange(B, dtype=np.uint32) * k)
        for b in range(B):
            assert all(tot[b, j] >= tot[b, j + 1] for j in range(k - 1))
            assert len({tuple(out[b, j, :ln[b, j]]) for j in range(k)}) == k
            _same(ctx.translate_beam(ids[b:b + 1], lens[b:b + 1], c.k, sl, want_align=True), tuple(a[b:b + 1] for a in got), "alone")
    finally:
        ctx.close()


# ---- isolation and options --------------------------------------------------------------------------------------------------
def test_a_source_alone_and_inside_a_larger_batch(hip, oracle, engines):
    c = BC.parity("k6")
    m, gm, ids, lens, sl, want = _case(c, oracle, engines)
    ctx = _ctx(hip, gm, c)
    try:
        for b in range(c.B):
            alone = ctx.translate_beam(ids[b:b + 1], lens[b:b + 1], c.k, sl, want_align=True)
            _same(alone, tuple(a[b:b + 1] for a in want), "source %d alone" % b)
    finally:
        ctx.close()


def test_a_beam_call_leaves_the_next_greedy_call_unchanged(hip, oracle, engines):
    c = BC.parity("k6")
    m, gm, ids, lens, sl, want = _case(c, oracle, engines)
    ctx = _ctx(hip, gm, c)
    try:
        for mode in (0, 1):
            ctx.set_decode_mode(mode)
            before = ctx.translate(ids, lens, sl, want_align=True)
            _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True), want, "mode %d" % mode)
            after = ctx.translate(ids, lens, sl, want_align=True)
            assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
                       for a, b in zip(before, after))
    finally:
        ctx.close()


def test_an_armed_option_refuses_the_beam_call_and_is_consumed(hip, oracle, engines):
    c = BC.parity("k6")
    m, gm, ids, lens, sl, want = _case(c, oracle, engines)
    R, T = c.B * c.k, BC.tmax_of(c.S)
    ctx = _ctx(hip, gm, c)
    try:
        arms = [
            (lambda: ctx.set_scores([np.zeros((R, T), np.float32)]), "scores are armed"),
            (lambda: ctx.set_target_prefix([(np.zeros((R, T), np.uint32), np.zeros(R, np.uint32))]), "prefix is armed"),
            (lambda: ctx.set_sampling(1.0, [None]), "sampling is armed"),
            (lambda: (ctx.set_sampling(1.0, [None]), ctx.set_sampling_truncation(4, 0.9)), "sampling is armed"),
            (lambda: ctx.set_sampling_truncation(4, 0.9), "truncation"),
            (lambda: ctx.set_fanout_consensus(2, 4, np.zeros(c.B, np.uint32), np.zeros(R, np.float64)), "consensus"),
        ]
        for arm, message in arms:
            arm()
            with pytest.raises(hip.SlimtHipError, match=message):
                ctx.translate_beam(ids, lens, c.k, sl)
            _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True), want, message)  # consumed: the next call is plain
        with pytest.raises(hip.SlimtHipError, match="exceed the context's max_batch"):
            ctx.translate_beam(ids, lens, 8, sl)
    finally:
        ctx.close()


# ---- the frontend -------------------------------------------------------------------------------------------------------------
from test_text_frontend import corpus, spm_model  # noqa: E402,F401  (the text frontend tests' fixtures)


def test_frontend_beam_search(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    blob = synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5)
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model, shortlist=blob)
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        texts = [" ".join(corpus[i:i + 2]) + "\n" + corpus[i + 2] for i in range(0, 12, 3)]
        greedy = svc.translate(model, texts)
        one = svc.beam_search(model, texts, 1)
        for g, r in zip(greedy, one):
            assert len(r.nbest) == 1 and r.nbest[0] is r and r.target.text == g.target.text
        k = 4
        got = svc.beam_search(model, texts, k)
        assert len(got) == len(texts)
        for r in got:
            assert len(r.nbest) == k and r.nbest[0] is r
            n = r.source.sentence_count()
            for a in r.nbest:  # every alternative covers the text's sentences, each with its scores and alignment
                assert len(a.hypothesis_scores) == len(a.token_scores) == len(a.alignments) == n
                for s in range(n):  # the engine's totals: the ascending f32 sums of the token scores
                    tot = np.float32(0)
                    for x in a.token_scores[s]:
                        tot = np.float32(tot + x)
                    assert len(a.token_scores[s]) == 0 or np.float32(a.hypothesis_scores[s]) == tot
            for s in range(n):
                keys = [a.hypothesis_scores[s] for a in r.nbest]
                assert keys == sorted(keys, reverse=True)
        assert any(len({a.target.text for a in r.nbest}) > 1 for r in got)
        with pytest.raises(ValueError):
            svc.beam_search(model, texts, 0)
    finally:
        svc.close()
        model.close()
