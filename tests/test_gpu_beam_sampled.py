"""GPU parity of a beam call sampled without replacement (slimt_hip_ctx_set_beam_sampling): tokens, lengths, totals,
perturbed values, token scores and alignment rows bit for bit against `sampled_beam_translate`
(tests/support/beam_sampled_ref.py: the oracle's decode_step in PORTABLE mode under the restatement's selection), as
tests/test_gpu_beam.py compares the un-armed call; distinct hypotheses, independence of batch position and neighbours,
dependence on the keys, and the option's consumption and refusals."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_sampled_ref as SB
from test_sampling_checker import keys_of

pytestmark = pytest.mark.gpu

# B = 3 ragged sources; the EOS bias lets some hypotheses finish early and leaves others live at Tmax (asserted below)
CASE = BC.case("sampled", "tiny11", 7.0, 8, 3, 8, 4096)
KEYS = keys_of(21, CASE.B)


@pytest.fixture(scope="module")
def setup(hip, oracle, synth_models):
    m = BC.model_of(CASE, synth_models)
    gm = hip.Model(m)
    ids, lens, sl = BC.inputs(CASE, m.V)
    yield m, gm, oracle.OracleModel(m), ids, lens, sl
    gm.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """the recorded entries of two results (ids, lengths, totals, token scores, alignment rows, perturbed) bit for bit"""
    ln = got[1]
    assert np.array_equal(ln, want[1]), (what, ln, want[1])
    assert np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(_bits(got[5]), _bits(want[5])), what
    live = np.arange(got[0].shape[2])[None, None, :] < ln[:, :, None]
    assert np.array_equal(got[0][live], want[0][live]), what
    assert np.array_equal(_bits(got[3])[live], _bits(want[3])[live]) and np.array_equal(_bits(got[4])[live], _bits(want[4])[live]), what


def _hyps(res, b):
    return [tuple(res[0][b, j, :res[1][b, j]]) for j in range(res[0].shape[1]) if res[1][b, j]]


@pytest.mark.parametrize("k", [1, 4, 8])
def test_armed_call_equals_the_checker(hip, oracle, setup, k):
    m, gm, om, ids, lens, sl = setup
    want = SB.sampled_beam_translate(oracle, om, m, ids, lens, sl, k, KEYS)
    ctx = hip.Context(gm, CASE.B * k + 3, CASE.S)
    try:
        got = ctx.translate_beam(ids, lens, k, sl, want_align=True, sampling_keys=KEYS)
        _same(got, want, "k %d" % k)
        _same(ctx.translate_beam_pinned(ids, lens, k, sl, want_align=True, sampling_keys=KEYS), want, "pinned, k %d" % k)
        T = BC.tmax_of(CASE.S)
        ended = [got[0][b, j, got[1][b, j] - 1] == 0 for b in range(CASE.B) for j in range(k) if got[1][b, j]]
        if k == 8:  # the case shows both ends: EOS before Tmax, and live at Tmax
            assert any(ended) and not all(ended) and (got[1] == T).any() and (got[1] < T).any()
        for b in range(CASE.B):
            hyps = _hyps(got, b)
            assert len(set(hyps)) == len(hyps) == k  # pairwise distinct
            assert np.all(got[5][b] <= 0) and np.all(np.diff(got[2][b]) <= 0)  # G never above the root's +0; ordered by totals
    finally:
        ctx.close()


def test_a_source_depends_on_its_key_only_and_the_keys_matter(hip, setup):
    m, gm, om, ids, lens, sl = setup
    k = 4
    ctx = hip.Context(gm, CASE.B * k + 3, CASE.S)
    try:
        whole = ctx.translate_beam(ids, lens, k, sl, want_align=True, sampling_keys=KEYS)
        for b in range(CASE.B):
            alone = ctx.translate_beam(ids[b:b + 1], lens[b:b + 1], k, sl, want_align=True, sampling_keys=KEYS[b:b + 1])
            _same(alone, tuple(a[b:b + 1] for a in whole), "source %d alone" % b)
        turned = ctx.translate_beam(ids[::-1], lens[::-1], k, sl, want_align=True, sampling_keys=KEYS[::-1].copy())
        _same(turned, tuple(a[::-1] for a in whole), "another position, other neighbours")
        other = ctx.translate_beam(ids, lens, k, sl, sampling_keys=keys_of(22, CASE.B))
        assert any(set(_hyps(other, b)) != set(_hyps(whole, b)) for b in range(CASE.B))
    finally:
        ctx.close()


def test_the_option_is_consumed_and_refused_where_it_does_not_belong(hip, setup):
    m, gm, om, ids, lens, sl = setup
    k, B = 4, CASE.B
    ctx, fresh = hip.Context(gm, B * k + 3, CASE.S), hip.Context(gm, B * k + 3, CASE.S)
    try:
        ctx.translate_beam(ids, lens, k, sl, sampling_keys=KEYS)
        plain, want = ctx.translate_beam(ids, lens, k, sl, want_align=True), fresh.translate_beam(ids, lens, k, sl, want_align=True)
        _same(plain + (np.zeros(1),), want + (np.zeros(1),), "an un-armed call behind an armed one")
        row_src = np.repeat(np.arange(B, dtype=np.uint32), 2)
        for call in (lambda: ctx.translate(ids, lens, sl), lambda: ctx.translate_fanout(ids, lens, row_src, sl),
                     lambda: ctx.translate(ids, lens, sl, scores=True)):
            ctx.set_beam_sampling(KEYS, B)
            with pytest.raises(hip.SlimtHipError, match="not a beam call"):
                call()
            call()  # consumed: the same call goes through
        ctx.set_beam_sampling(KEYS[:2].copy(), 2)
        with pytest.raises(hip.SlimtHipError, match="2 sources armed, the call has 3"):
            ctx.translate_beam(ids, lens, k, sl)
        ctx.set_sampling(1.0, [None])
        with pytest.raises(hip.SlimtHipError, match="sampling is armed"):
            ctx.translate_beam(ids, lens, k, sl, sampling_keys=KEYS)
        _same(ctx.translate_beam(ids, lens, k, sl, want_align=True) + (np.zeros(1),), want + (np.zeros(1),), "consumed")
    finally:
        ctx.close()
        fresh.close()


from test_text_frontend import corpus, spm_model  # noqa: E402,F401  (the text frontend tests' fixtures)


def test_frontend_samples_distinct_translations_and_picks_one_of_them(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model,
                               shortlist=synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5))
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        texts, k = [corpus[0], corpus[1] + "\n" + corpus[2]], 4
        got = svc.beam_search(model, texts, k, sample_seed=5)
        picks = svc.sample_and_select(model, texts, k, (1.0, 5), without_replacement=True)
        for r, p in zip(got, picks):
            for s in range(r.source.sentence_count()):
                strings = [a.target.sentence(s) for a in r.nbest]
                assert len(set(strings)) == k and p.target.sentence(s) == strings[p.sample_index[s]]
        with pytest.raises(ValueError, match="at most 8"):
            svc.sample_and_select(model, texts, 9, (1.0, 5), without_replacement=True)
    finally:
        svc.close()
        model.close()
