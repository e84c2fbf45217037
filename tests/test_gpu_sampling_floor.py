"""GPU parity of floored sampling (include/slimt_hip.h, slimt_hip_ctx_set_sampling_floor) through translate, fan-out and the
text frontend, against the checker of tests/support/floor_ref.py driven over the oracle's logits: tokens, lengths and
alignment rows exact, scores within 5e-5 of the float64 log-softmax over the kept set.

K/V cache format 3 keeps the reference's literal float order in the cross-attention, which no oracle mode has bit for bit
(tests/support/beam_cases.py treats its beam case the same way): there the alignment rows are compared
bit for bit with the device's own floored call in the other decode mode, and with the checker's within the project's 1e-4
for that order (measured here: 2.6e-6); tokens, lengths and scores are held to the checker as everywhere else."""
import numpy as np
import pytest

from support import floor_ref
from test_sampling_checker import keys_of, sampled_translate

pytestmark = pytest.mark.gpu

TOL = 5e-5
B, S, T, FLOOR = 5, 5, 1.0, (0.1, 0.02)  # Tmax 7


@pytest.fixture(scope="module")
def batch(oracle, synth_models):
    """(model, ids, lens, shortlist, keys, the checker's floored translation): computed once, shared and left unchanged"""
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    om = oracle.OracleModel(m)
    ids, lens = synth.make_batch(m.V, B, S, seed=66, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(9, B)
    sizes = []
    want = floor_ref.floored_translate(oracle, om, m, ids, lens, sl, keys, T, *FLOOR, sizes=sizes)
    plain = sampled_translate(oracle, om, m, ids, lens, sl, keys, T)
    assert any(1 < k < n for _, _, k, n in sizes)  # (the floor cuts, and not to the maximum alone)
    assert not (np.array_equal(want[0], plain[0]) and np.array_equal(want[1], plain[1]))  # ... and changes a sentence
    return m, ids, lens, sl, keys, want


def _check(got, want, what, literal=False):
    out, ln, al, sc = got
    w_out, w_ln, w_al, w_sc = want
    assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), what
    if literal:
        print("%s: alignment: max |gpu - oracle| = %.3g" % (what, np.abs(al - w_al).max()))
        assert np.abs(al - w_al).max() <= 1e-4, what
    else:
        assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), what
    worst = max(np.abs(sc[b, :n].astype(np.float64) - w_sc[b, :n]).max() for b, n in enumerate(w_ln))
    print("%s: scores: max |gpu - float64| = %.3g" % (what, worst))
    assert worst <= TOL, what


@pytest.mark.parametrize("mode,kv_format", [(0, None), (1, None), (0, 3)])
def test_a_floored_translate_equals_the_checker(hip, batch, mode, kv_format):
    m, ids, lens, sl, keys, want = batch
    gm = hip.Model(m)
    if kv_format is not None:
        gm.set_kv_cache_format(kv_format)
    ctx = hip.Context(gm, B, S)
    try:
        ctx.set_decode_mode(mode)
        plan = ctx.plan(S)
        got = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), floor=FLOOR)
        _check(got, want, (mode, kv_format), literal=kv_format == 3)
        assert ctx.plan(S) == plan  # (slimt_hip_ctx_plan keeps reporting the context's mode)
        if kv_format == 3:
            ctx.set_decode_mode(1)
            for x, y in zip(got, ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), floor=FLOOR)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    finally:
        ctx.close()
        gm.close()


def test_fanout_floors_per_row_and_both_floors_off_is_the_plain_sampled_call(hip, batch):
    m, ids, lens, sl, keys, _ = batch
    gm = hip.Model(m)
    row_src = np.array([0, 0, 0, 3, 1, 4, 4], np.uint32)
    fkeys = keys_of(21, row_src.size)
    ctx = hip.Context(gm, row_src.size, S)
    try:
        kw = dict(want_align=True, scores=True, sampling=(T, fkeys))
        fan = ctx.translate_fanout(ids, lens, row_src, sl, floor=FLOOR, **kw)
        dup = ctx.translate(ids[row_src], lens[row_src], sl, floor=FLOOR, **kw)
        off = ctx.translate(ids[row_src], lens[row_src], sl, floor=(0.0, 0.0), **kw)
        plain = ctx.translate(ids[row_src], lens[row_src], sl, **kw)
        for x, y, z, w in zip(fan, dup, off, plain):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert np.array_equal(z.view(np.uint32), w.view(np.uint32))
    finally:
        ctx.close()
        gm.close()


def test_each_refusal_is_negative_with_a_message_and_leaves_the_next_call_unarmed(hip, batch):
    from slimt_amd import capi
    m, ids, lens, sl, keys, _ = batch
    gm = hip.Model(m)
    ctx = hip.Context(gm, 2 * B, S)
    try:
        greedy = ctx.translate(ids, lens, sl)
        refusals = [
            ("without sampling", lambda: ctx.translate(ids, lens, sl, floor=FLOOR)),
            ("truncation is armed too", lambda: ctx.translate(ids, lens, sl, sampling=(T, keys), truncation=(4, 0.9), floor=FLOOR)),
            ("beam call", lambda: (ctx.set_sampling_floor(*FLOOR), ctx.translate_beam(ids, lens, 2, sl))),
            ("sampling floor", lambda: ctx.set_sampling_floor(1.5, 0.0)),
            ("sampling floor", lambda: ctx.set_sampling_floor(0.0, 1.0)),
        ]
        for message, call in refusals:
            with pytest.raises(capi.SlimtHipError, match=message):
                call()
            again = ctx.translate(ids, lens, sl)  # (greedy: neither a floor nor anything else is left armed)
            assert np.array_equal(again[0], greedy[0]) and np.array_equal(again[1], greedy[1]), message
    finally:
        ctx.close()
        gm.close()


def test_frontend_select_picks_among_the_floored_rows_and_refuses_truncation(hip):
    import io
    import random
    import sentencepiece
    from slimt_amd import frontend, synth
    rnd = random.Random(7)
    words = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 8))) for _ in range(600)]
    corpus = [" ".join(rnd.choice(words) for _ in range(rnd.randint(3, 12))).capitalize() + "." for _ in range(1500)]
    spm = io.BytesIO()
    sentencepiece.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=spm, vocab_size=512,
                                             model_type="unigram", pad_id=-1, unk_id=1, bos_id=-1, eos_id=0, minloglevel=2)
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, frontend.Package(model=synth.write_bin(m), vocabulary=spm.getvalue()), device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        sources, n, sampling = corpus[:3], 4, (1.0, 11)
        won = svc.sample_and_select(model, sources, n, sampling, floor=FLOOR)
        processed = model.processor.process_many(sources, svc.wrap_length, svc.workers)
        drawn = svc._floored_samples(model, [segs for _, segs in processed], n, sampling, FLOOR)  # [sample][text][segment]
        for t, w in enumerate(won):
            for i in range(len(processed[t][1])):
                row = drawn[w.sample_index[i]][t][i]
                assert np.array_equal(w.token_scores[i].view(np.uint32), row[2].view(np.uint32)), (t, i)
                assert np.array_equal(w.alignments[i].view(np.uint32), row[1].view(np.uint32)), (t, i)
        responses, ranked = svc.sample_and_rerank(model, sources, n, sampling, floor=FLOOR)
        assert all(len(r.samples) == n for r in responses) and len(ranked) == len(sources)
        for kind in (svc.sample_and_select, svc.sample_and_rerank):
            with pytest.raises(ValueError):
                kind(model, sources, n, sampling, truncation=(4, 0.9), floor=FLOOR)
    finally:
        svc.close()
        model.close()
