"""Fan-out calls armed with slimt_hip_ctx_set_fanout_combine: bit for bit against the restatement stepping the oracle's decoder
(support/combine_ref.py), weights (1, 0) against the plain translation and a forced-prefix call, the refusals (each
consumed), and the frontend's contrast= keyword."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import combine_ref as CR
from test_gpu_beam import _bits, _ctx, engines  # noqa: F401  (the beam tests' fixtures)

pytestmark = pytest.mark.gpu

# chosen on the CPU with the oracle: under these settings the checker's tokens differ from the primaries' greedy translation
# (which ends in EOS at once under these biases: the contrast cancels a bias every source shares), and one group of cd3 reaches
# EOS at its second step while the others run to Tmax. k is the group's size m; group g reads the sources g, g + 1, ...
# (cyclic): every source is a primary once
CASES = {"cd2": (BC.case("cd2", "tiny11", 8.0, 8, 3, 2, 4096), (1.0, -0.7), -np.inf),
         "cd3": (BC.case("cd3", "tiny11", 9.0, 9, 3, 3, 1000), (1.0, 0.5, -1.0), -4.0)}


def _rows(c):
    return np.asarray([(g + j) % c.B for g in range(c.B) for j in range(c.k)], np.uint32)


def _same(got, want, what, rows=slice(None)):
    """tokens, lengths, scores and alignment rows of (out, len, align, scores) against (out, len, scores, align)"""
    out, ln, al, sc = (a[rows] for a in got)
    w_out, w_ln, w_sc, w_al = (a[rows] for a in want)
    assert np.array_equal(ln, w_ln), (what, ln, w_ln)
    live = np.arange(out.shape[1])[None, :] < ln[:, None]
    assert np.array_equal(out[live], w_out[live]), what
    assert np.array_equal(_bits(sc)[live], _bits(w_sc)[live]), (what, sc[live], w_sc[live])
    assert np.array_equal(_bits(al)[live], _bits(w_al)[live]), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_combined_fanout_equals_the_checker(hip, oracle, engines, name):
    c, w, gap = CASES[name]
    m, gm, om = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    rows = _rows(c)
    want = CR.translate(oracle, om, m, ids, lens, rows, sl, c.k, w, gap)
    greedy = CR.translate(oracle, om, m, ids, lens, rows, sl, c.k, (1.0,) + (0.0,) * (c.k - 1))
    assert not (np.array_equal(want[0], greedy[0]) and np.array_equal(want[1], greedy[1]))  # the case bites
    ctx = _ctx(hip, gm, c)
    try:
        got = ctx.translate_fanout(ids, lens, rows, sl, want_align=True, scores=True, combine=(w, gap))
        _same(got, want, name)
        for g in range(c.B):  # the rows of a group: identical tokens and lengths
            assert len({(int(got[1][r]), got[0][r].tobytes()) for r in range(g * c.k, (g + 1) * c.k)}) == 1
        _same(ctx.translate_fanout_pinned(ids, lens, rows, sl, want_align=True, scores=True, combine=(w, gap)), want, name + ", pinned")
    finally:
        ctx.close()


def test_weights_one_zero_are_greedy_and_the_contrast_rows_are_scored(hip, engines):
    c = CASES["cd2"][0]
    m, gm, _ = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    rows = _rows(c)
    ctx = _ctx(hip, gm, c)
    try:
        out, ln, al, sc = ctx.translate_fanout(ids, lens, rows, sl, want_align=True, scores=True, combine=((1.0, 0.0), None))
        ctx.set_decode_mode(1)  # (the per-stage decoder: the form a fan-out row is bit for bit)
        p_out, p_ln, p_al, p_sc = ctx.translate(ids, lens, sl, want_align=True, scores=True)
        live = np.arange(out.shape[1])[None, :] < p_ln[:, None]
        assert np.array_equal(ln[0::2], p_ln) and np.array_equal(out[0::2][live], p_out[live])
        assert np.array_equal(_bits(al[0::2])[live], _bits(p_al)[live])
        assert np.abs(sc[0::2][live] - p_sc[live]).max() <= 5e-5  # (another normaliser: scores.h's float sum)
        # the contrast rows' scores: the primaries' tokens forced under the contrast sources
        src = rows[1::2]
        f_out, f_ln, _, f_sc = ctx.translate(ids[src], lens[src], sl, scores=True, prefix=(out[0::2], ln[0::2]))
        assert np.array_equal(f_ln, ln[1::2]) and np.array_equal(f_out[live], out[1::2][live])
        assert np.abs(sc[1::2][live] - f_sc[live]).max() <= 5e-5
    finally:
        ctx.close()


def test_refusals_each_consumed(hip, engines):
    c = CASES["cd2"][0]
    m, gm, _ = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    rows, T = _rows(c), BC.tmax_of(c.S)
    ctx = _ctx(hip, gm, c)
    try:
        plain = ctx.translate_fanout(ids, lens, rows, sl, want_align=True, scores=True)
        arm = lambda: ctx.set_fanout_combine(2, (1.0, -0.7), -1.0)
        fan = lambda **kw: ctx.translate_fanout(ids, lens, rows, sl, combine=((1.0, -0.7), None), **kw)
        calls = [(lambda: ctx.translate_fanout(ids, lens, rows[:5], sl, combine=((1.0, -0.7), None)), "5 rows are no multiple of the 2 members"),
                 (lambda: (arm(), ctx.translate(ids, lens, sl)), "not a fan-out call"),
                 (lambda: (arm(), ctx.translate_beam(ids, lens, 2, sl)), "armed on a beam call"),
                 (lambda: fan(prefix=(np.zeros((6, T), np.uint32), np.zeros(6, np.uint32))), "a target prefix is armed too"),
                 (lambda: fan(sampling=(1.0, None)), "sampling is armed too"),
                 (lambda: fan(sampling=(1.0, None), truncation=(4, 1.0)), "sampling is armed too"),
                 (lambda: fan(constraints=dict(no_repeat_ngram=2)), "step constraints are armed too"),
                 (lambda: fan(consensus=(2, 4)), "consensus is armed too")]
        for call, message in calls:
            with pytest.raises(hip.SlimtHipError, match=message):
                call()
            got = ctx.translate_fanout(ids, lens, rows, sl, want_align=True, scores=True)  # consumed: the next call is plain
            assert all(np.array_equal(g.view(np.uint32), p.view(np.uint32)) for g, p in zip(got, plain)), message
        for members, w, gap in ((5, (1.0,) * 5, 0.0), (2, (1.0, 17.0), 0.0), (2, (1.0, 1.0), 0.5), (1, (1.0,), np.nan)):
            with pytest.raises(hip.SlimtHipError):  # refused at once
                ctx.set_fanout_combine(members, w, gap)
        with pytest.raises(hip.SlimtHipError, match="2\\^20 or more"):
            hip.combine_step(np.zeros((1, 1 << 20), np.float32), 1, (1.0,))
    finally:
        ctx.close()


from test_text_frontend import corpus, spm_model  # noqa: E402,F401  (the text frontend tests' fixtures)


def test_frontend_contrast_gives_a_response_per_text(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model,
                               shortlist=synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5))
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        texts = [corpus[0], corpus[1] + "\n" + corpus[2], corpus[3]]
        for kw in (dict(weight=0.5), dict(weight=0.5, gap=-2.0, texts=texts[::-1])):
            out = svc.translate(model, texts, contrast=kw)
            assert len(out) == len(texts)
            for r in out:
                n = r.source.sentence_count()
                assert r.target.sentence_count() == n and len(r.token_scores) == n and all(len(s) for s in r.token_scores)
        with pytest.raises(ValueError, match="at least two texts"):
            svc.translate(model, texts[:1], contrast=dict(weight=0.5))
    finally:
        svc.close()
        model.close()
