"""Beam calls armed with slimt_hip_ctx_set_beam_groups, bit for bit against the host search over the oracle in groups
(support/beam_grouped_ref.py): the hypotheses, their groups, totals that are the sums of the token scores; penalty 0 with
G = k as k copies of beam 1; the refusals, each consumed."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_grouped_ref as GR
from test_gpu_beam import _ctx, _same, engines  # noqa: F401  (the beam tests' fixture and comparison)

pytestmark = pytest.mark.gpu

# chosen on the CPU with the oracle: under this penalty the grouped n-best of each case below differs from the plain one, and
# on each of them two groups of a source differ in their first token
PENALTY = 1.0
GROUPS = {"sl1000": 3, "full": 2, "k8": 4}  # G divides the case's k (3, 2, 8)


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_grouped_beam_equals_the_checker(hip, oracle, engines, name):
    c, G = BC.parity(name), GROUPS[name]
    m, gm, om = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    want = GR.translate(oracle, om, m, ids, lens, sl, c.k, G, PENALTY, c.mode)
    plain = BC.beam_translate(oracle, om, m, ids, lens, sl, c.k, c.mode)
    # the case bites, on the checker's results alone
    assert not (np.array_equal(want[0], plain[0]) and np.array_equal(want[1], plain[1]))
    firsts = [{int(want[0][b, j, 0]) for j in range(c.k) if want[5][b, j] == q and want[1][b, j]} for b in range(c.B) for q in range(G)]
    assert any(x and y and x.isdisjoint(y) for b in range(c.B) for x in firsts[b * G:(b + 1) * G] for y in firsts[b * G:(b + 1) * G])
    ctx = _ctx(hip, gm, c)
    try:
        got = ctx.translate_beam(ids, lens, c.k, sl, want_align=True, groups=(G, PENALTY), want_groups=True)
        _same(got[:5], want[:5], name)
        assert np.array_equal(got[5], want[5]), (name, got[5], want[5])
        out, ln, tot, sc = got[:4]
        for b, j in np.ndindex(c.B, c.k):  # a total is the f32 sum, in order, of the token scores: the penalty is in none
            total = np.float32(0)
            for x in sc[b, j, :ln[b, j]]:
                total = np.float32(total + x)
            assert ln[b, j] == 0 or total.view(np.uint32) == tot[b, j].view(np.uint32), (name, b, j)
        _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True), plain, name + ", the next un-armed call")
    finally:
        ctx.close()


def test_zero_penalty_is_greedy_k_times_and_refusals_are_consumed(hip, engines):
    c = BC.parity("sl1000")
    m, gm, _ = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    ctx = _ctx(hip, gm, c)
    try:
        one = ctx.translate_beam(ids, lens, 1, sl, want_align=True)
        got = ctx.translate_beam(ids, lens, c.k, sl, want_align=True, groups=(c.k, 0.0), want_groups=True)
        assert np.array_equal(got[5], np.tile(np.arange(c.k, dtype=np.uint32), (c.B, 1)))  # equal totals: ties to the lower slot
        for j in range(c.k):
            _same(tuple(a[:, j:j + 1] for a in got[:5]), one, "group %d" % j)
        plain = ctx.translate_beam(ids, lens, c.k, sl, want_align=True)
        calls = [(lambda: (ctx.set_beam_groups(c.k, 0.5), ctx.translate(ids, lens, sl)), "not a beam call"),
                 (lambda: ctx.translate_beam(ids, lens, c.k, sl, groups=(2, 0.5)), "2 groups do not divide a beam of 3"),
                 (lambda: (ctx.set_beam_sampling(None, c.B), ctx.translate_beam(ids, lens, c.k, sl, groups=(c.k, 0.5))),
                  "beam sampling is armed too"),
                 (lambda: ctx.translate_beam(ids, lens, c.k, sl, groups=(c.k, 0.5), constraints=dict(no_repeat_ngram=3)),
                  "beam constraints are armed too")]
        for call, message in calls:
            with pytest.raises(hip.SlimtHipError, match=message):
                call()
            _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True), plain, message)  # consumed: the next call is plain
    finally:
        ctx.close()


from test_text_frontend import corpus, spm_model  # noqa: E402,F401  (the text frontend tests' fixtures)


def test_frontend_returns_each_hypothesis_with_its_group(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model,
                               shortlist=synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5))
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        texts, k, G = [corpus[0], corpus[1] + "\n" + corpus[2]], 4, 2
        for r in svc.beam_search(model, texts, k, groups=G, diversity=1.0):
            for s in range(r.source.sentence_count()):
                groups = [a.group[s] for a in r.nbest if a.group[s] >= 0]
                assert groups and set(groups) <= set(range(G)) and all(groups.count(q) <= k // G for q in range(G))
        with pytest.raises(ValueError, match="groups must divide the beam"):
            svc.beam_search(model, texts, k, groups=3)
    finally:
        svc.close()
        model.close()
