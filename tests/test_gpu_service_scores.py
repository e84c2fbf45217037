"""GPU checks of per-token scores through the batching service and the text front end: BatchService(scores=True)
(include/slimt_hip_service_scores.h) over a lexical shortlist, a fixed list, merged launches and no merging; every
sentence's scores equal those of a direct scored call on the batch it travelled in (bit for bit: the same kernels on the
same sentences), and scores=False results are unchanged. Service.translate(..., scores=True) on a SentencePiece model:
token_scores per target sentence with sentence_scores their sums, wrapped segments' pieces concatenated, pivot's the
second hop's."""
import io
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    rnd = random.Random(7)
    words = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 8))) for _ in range(1500)]
    sents = []
    for _ in range(3000):
        s = " ".join(rnd.choice(words) for _ in range(rnd.randint(3, 18)))
        sents.append(s[0].upper() + s[1:] + rnd.choice(".?!"))
    return sents


@pytest.fixture(scope="module")
def spm_model(corpus):
    import sentencepiece
    out = io.BytesIO()
    sentencepiece.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=out, vocab_size=512,
                                             model_type="unigram", pad_id=-1, unk_id=1, bos_id=-1, eos_id=0,
                                             minloglevel=2)
    return out.getvalue()


def _direct(hip, gm, sentences, shortlist=None, generator=None):
    """the scored call on ONE padded batch of `sentences` (as the service forms it): per sentence (target, scores)"""
    B, S = len(sentences), max(len(s) for s in sentences)
    ids = np.zeros((B, S), np.uint32)
    lens = np.zeros(B, np.uint32)
    for i, s in enumerate(sentences):
        ids[i, :len(s)] = s
        lens[i] = len(s)
    ctx = hip.Context(gm, B, S)
    if generator is not None:
        out, ln, _, sc = ctx.translate_generated(generator, ids, lens, scores=True)
    else:
        out, ln, _, sc = ctx.translate(ids, lens, shortlist, scores=True)
    ctx.close()
    return [(out[i, :ln[i]], sc[i, :ln[i]]) for i in range(B)]


@pytest.mark.parametrize("vocab", ["lexical", "fixed", "full"])
@pytest.mark.parametrize("merge", [0, 1])
def test_batch_service_scores_equal_the_direct_call(hip, synth_models, vocab, merge):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(3))
    S = 12  # one length: one batch per max_words budget, the service's batches are known
    sents = [list(rnd.integers(3, m.V, S - 1)) + [0] for _ in range(60)]
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, min_count=1) if vocab == "lexical" else b""
    fixed = synth.make_shortlist(m.V, 2048) if vocab == "fixed" else None
    kw = dict(max_words=(20 + 1) * S, workers_per_device=1, lexical_shortlist=blob, source_vocab=m.V, target_vocab=m.V,
              shortlist=fixed, merge_batches=merge)  # (0: the defaults, merged launches; 1: never merged)
    plain = hip.BatchService([gm], **kw)
    scored = hip.BatchService([gm], scores=True, **kw)
    try:
        r0 = plain.translate(sents)
        r1 = scored.translate(sents)
        assert r0.scores is None and r1.scores is not None
        assert np.array_equal(r0.targets, r1.targets) and np.array_equal(r0.target_offsets, r1.target_offsets)
        assert np.array_equal(r0.alignments, r1.alignments)
        # the batches the sentences travelled in (ServiceResult.batch; one length: arrival order inside a batch) -- with
        # a lexical shortlist a batch's output layer is that of ITS sentences
        gen = hip.ShortlistGenerator(blob, m.V, m.V) if blob else None
        groups = {}
        for i in range(len(sents)):
            groups.setdefault(int(r1.batch[i]), []).append(i)
        assert len(groups) >= 3
        for members in groups.values():
            want = _direct(hip, gm, [sents[i] for i in members], fixed, gen)
            for i, (tgt, sc) in zip(members, want):
                assert np.array_equal(r1.target(i), tgt)
                assert np.array_equal(r1.token_scores(i), sc), i
                assert np.all(np.isfinite(sc)) and np.all(sc <= 1e-6)
        if gen is not None:
            gen.close()
        assert hip.host_lib().slimt_hip_service_set_scores(scored.h, 0) != 0  # only before the first translate
        assert b"before the first" in hip.host_lib().slimt_hip_service_last_error()
        r1.close()
        r0.close()
    finally:
        scored.close()
        plain.close()
        gm.close()


def test_frontend_service_translate_and_pivot_with_scores(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    blob = synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5)
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model, shortlist=blob)
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=2, max_words=256, wrap_length=24)
    try:
        texts = [" ".join(corpus[i:i + 3]) + "\n" + corpus[i + 3] for i in range(0, 40, 4)]
        plain = svc.translate(model, texts, encoding=frontend.Encoding.Byte)
        scored = svc.translate(model, texts, encoding=frontend.Encoding.Byte, scores=True)
        again = svc.translate(model, texts, encoding=frontend.Encoding.Byte)
        for p, s, a in zip(plain, scored, again):
            assert p.target.text == s.target.text == a.target.text
            assert not p.token_scores and not p.sentence_scores and not a.token_scores
            n = s.target.sentence_count()
            assert len(s.token_scores) == len(s.sentence_scores) == n
            for k in range(n):
                assert len(s.token_scores[k]) == s.target.word_count(k)
                assert np.all(np.isfinite(s.token_scores[k])) and np.all(s.token_scores[k] <= 1e-6)
                assert s.sentence_scores[k] == float(np.sum(s.token_scores[k], dtype=np.float64))
        # the scores are those of the engine on the segments the service sent: the direct BatchService call
        per_request = [model.processor.process(t, 24)[1] for t in texts]
        flat = [seg for segs in per_request for seg in segs]
        eng = svc._engine(model, True)
        res = eng.translate(flat)
        n = 0
        for r, segs in zip(scored, per_request):
            for k in range(len(segs)):
                assert np.array_equal(r.token_scores[k], res.token_scores(n))
                n += 1
        res.close()
        # a segment longer than the engine takes goes in pieces: its scores are the pieces' concatenated, one per token
        long_seg = [int(x) for x in np.random.Generator(np.random.PCG64(1)).integers(3, m.V, 300)] + [0]
        hist = svc._translate_segments(model, [[long_seg]], scores=True)
        words, _, sc = hist[0][0]
        assert len(sc) == len(words) and np.all(np.isfinite(sc))
        pieces = svc._split_long(long_seg, 0)
        res = eng.translate(pieces)
        want = np.concatenate([res.token_scores(k)[:-1] if k + 1 < len(pieces) and res.target(k)[-1] == 0
                               else res.token_scores(k) for k in range(len(pieces))])
        res.close()
        assert np.array_equal(sc, want)
        # pivot: the second hop's scores, which score the final target tokens
        piv = svc.pivot(model, model, texts[:4], scores=True)
        firsts = svc.translate(model, texts[:4], encoding=frontend.Encoding.Byte)
        second_in = [model.processor.process_annotated(r.target) for r in firsts]
        direct = svc._translate_segments(model, [segs for _, segs in second_in], scores=True)
        for r, hist in zip(piv, direct):
            assert len(r.token_scores) == r.target.sentence_count() == len(hist)
            for k, (words, _, sc) in enumerate(hist):
                assert len(r.token_scores[k]) == r.target.word_count(k) == len(words)
                assert np.array_equal(r.token_scores[k], sc)
    finally:
        svc.close()
        model.close()
