"""GPU checks of teacher-forced scoring through the batching service and the text front end: BatchService.score
(include/slimt_hip_service_score.h) over a lexical shortlist, a fixed list and the full vocabulary equals the direct
Context.score call per sentence, whatever the batching -- a sentence's results do not depend on the batch around it --,
targets longer than 1.5x their source included; frontend.Service.score on text returns the token scores of its own
tokenisation."""
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


def _direct(ctx, src, tgt, shortlist):
    """Context.score on ONE sentence pair alone: (scores [n], align [n, len(src)])"""
    ids = np.asarray([src], np.uint32)
    lens = np.asarray([len(src)], np.uint32)
    T = max(1, len(tgt))
    t_ids = np.zeros((1, T), np.uint32)
    t_ids[0, :len(tgt)] = tgt
    sc, al = ctx.score(ids, lens, shortlist, t_ids, np.asarray([len(tgt)], np.uint32), want_align=True)
    return sc[0, :len(tgt)], al[0, :len(tgt), :len(src)]


@pytest.mark.parametrize("vocab", ["lexical", "fixed", "full"])
def test_batch_service_score_equals_the_direct_call_per_sentence(hip, synth_models, vocab):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(5))
    n = 40
    sents = [list(rnd.integers(3, m.V, int(rnd.integers(1, 20)))) + [0] for _ in range(n)]
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, min_count=1) if vocab == "lexical" else b""
    fixed = synth.make_shortlist(m.V, 2048) if vocab == "fixed" else None
    pool = fixed[fixed != 0] if fixed is not None else np.arange(1, m.V)
    # targets of 0 .. 3x the source length (the prefix path stops at 1.5x), some ending in EOS, some with it inside
    tgts = []
    for i, s in enumerate(sents):
        t = [int(x) for x in rnd.choice(pool, size=(i * 3 * len(s)) // (n - 1))]
        if t and i % 3 == 0:
            t[-1] = 0
        if len(t) > 4 and i % 5 == 0:
            t[2] = 0
        tgts.append(t)
    assert any(len(t) > 1.5 * len(s) + 1 for s, t in zip(sents, tgts)) and any(not t for t in tgts)
    svc = hip.BatchService([gm], max_words=8 * 21, workers_per_device=1, lexical_shortlist=blob, source_vocab=m.V,
                           target_vocab=m.V, shortlist=fixed)
    gen = hip.ShortlistGenerator(blob, m.V, m.V) if blob else None
    ctx = hip.Context(gm, 64, 32)
    try:
        res = svc.score(sents, tgts)
        assert res.n == n and len(set(int(b) for b in res.batch)) >= 3  # several batches
        groups = {}
        for i in range(n):
            groups.setdefault(int(res.batch[i]), []).append(i)
        for members in groups.values():
            # the output layer of a lexical service is the list of the BATCH's source words
            S = max(len(sents[i]) for i in members)
            assert all(int(res.padded_length[i]) == S for i in members)
            sl = fixed
            if gen is not None:
                ids = np.zeros((len(members), S), np.uint32)
                for k, i in enumerate(members):
                    ids[k, :len(sents[i])] = sents[i]
                sl = gen.generate(ids, np.asarray([len(sents[i]) for i in members], np.uint32))
            for i in members:
                assert np.array_equal(res.target(i), np.asarray(tgts[i], np.uint32)), i
                sc, al = _direct(ctx, sents[i], tgts[i], sl)
                assert np.array_equal(res.token_scores(i).view(np.uint32), sc.view(np.uint32)), i
                if tgts[i]:
                    assert np.array_equal(res.alignment(i).view(np.uint32), al.view(np.uint32)), i
                else:  # (an empty target: no rows, whatever width the view gives them)
                    assert res.alignment(i).size == 0 and al.size == 0
        # the service still translates, and scores again the same
        tr = svc.translate(sents[:5])
        assert tr.n == 5
        tr.close()
        again = svc.score(sents, tgts)
        assert np.array_equal(again.scores.view(np.uint32), res.scores.view(np.uint32))
        again.close()
        res.close()
        with pytest.raises(ValueError):
            svc.score(sents, tgts[:-1])
        with pytest.raises(hip.SlimtHipError, match="out of range"):
            svc.score(sents[:2], [[m.V], [3, 0]])
        with pytest.raises(hip.SlimtHipError, match="empty sentence"):
            svc.score([[]], [[0]])
        ok = svc.score(sents[:2], tgts[:2])  # usable after a refusal
        assert ok.n == 2
        ok.close()
    finally:
        ctx.close()
        if gen is not None:
            gen.close()
        svc.close()
        gm.close()


def test_frontend_service_score_on_text(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    blob = synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5)
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model, shortlist=blob)
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    try:
        sources = corpus[:12]
        targets = [corpus[100 + i] + " " + corpus[200 + i] + " " + corpus[300 + i] for i in range(12)]  # ~3x the source
        pairs = svc.score(model, sources, targets)
        assert len(pairs) == 12
        v = model.vocabulary
        src = [ids + [0] for ids in v.encode_ids_batch(sources)]
        tgt = [ids + [0] for ids in v.encode_ids_batch(targets)]
        assert any(len(t) > 1.5 * len(s) + 1 for s, t in zip(src, tgt))
        direct = svc._engine(model).score(src, tgt)  # its own tokenisation through the engine
        for i, p in enumerate(pairs):
            assert p.source_ids == src[i] and p.target_ids == tgt[i]
            assert p.token_scores.shape == (len(tgt[i]),) and p.alignment.shape == (len(tgt[i]), len(src[i]))
            assert np.array_equal(p.token_scores.view(np.uint32), direct.token_scores(i).view(np.uint32))
            assert np.array_equal(p.alignment.view(np.uint32), direct.alignment(i).view(np.uint32))
            fin = np.isfinite(p.token_scores)
            assert np.all(p.token_scores[fin] <= 1e-6) and not np.any(np.isnan(p.token_scores))
            assert p.score == float(np.sum(p.token_scores, dtype=np.float64))
            rows = p.alignment.sum(axis=1)
            assert np.allclose(rows, 1.0, atol=1e-4)
        direct.close()
        assert svc.score(model, [], []) == []
        with pytest.raises(ValueError):
            svc.score(model, sources, targets[:-1])
    finally:
        svc.close()
        model.close()
