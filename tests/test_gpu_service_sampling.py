"""GPU checks of sampled decoding through the batching service and the text front end
(include/slimt_hip_service_sampling.h): a request's draws depend on its sentences and its seed alone -- the same alone or
sharing merged launches with another request's sentences, and equal to the direct Context call under
slimt_hip_sampling_key(seed, i); Service.translate(..., sampling=(T, seed)) is reproducible and scored."""
import io
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _direct(hip, gm, sentences, shortlist, T, keys):
    B, S = len(sentences), max(len(s) for s in sentences)
    ids = np.zeros((B, S), np.uint32)
    lens = np.zeros(B, np.uint32)
    for i, s in enumerate(sentences):
        ids[i, :len(s)] = s
        lens[i] = len(s)
    ctx = hip.Context(gm, B, S)
    out, ln, _, sc = ctx.translate(ids, lens, shortlist, scores=True, sampling=(T, keys))
    ctx.close()
    return [(out[i, :ln[i]], sc[i, :ln[i]]) for i in range(B)]


@pytest.mark.parametrize("merge", [0, 1])
def test_a_request_draws_the_same_alone_interleaved_and_directly(hip, synth_models, merge):
    from slimt_amd import capi, synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(5))
    S, T, seed = 12, 1.0, 7
    mine = [list(rnd.integers(3, m.V, S - 1)) + [0] for _ in range(45)]
    other = [list(rnd.integers(3, m.V, S - 1)) + [0] for _ in range(50)]
    fixed = synth.make_shortlist(m.V, 2048)
    kw = dict(max_words=(10 + 1) * S, workers_per_device=1, source_vocab=m.V, target_vocab=m.V, shortlist=fixed,
              merge_batches=merge, scores=True, temperature=T)  # (batches of 10: both requests' sentences share launches)
    svc = hip.BatchService([gm], **kw)
    try:
        alone = svc.translate(mine, seed=seed)
        results = {}
        gate = threading.Barrier(2)

        def run(name, sents, sd):
            gate.wait()
            results[name] = svc.translate(sents, seed=sd)

        threads = [threading.Thread(target=run, args=("mine", mine, seed)), threading.Thread(target=run, args=("other", other, 99))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        mixed = results["mine"]
        assert np.array_equal(alone.target_offsets, mixed.target_offsets) and np.array_equal(alone.targets, mixed.targets)
        assert np.array_equal(alone.scores.view(np.uint32), mixed.scores.view(np.uint32))
        keys = np.array([capi.sampling_key(seed, i) for i in range(len(mine))], dtype=np.uint64)
        for i, (tgt, sc) in enumerate(_direct(hip, gm, mine, fixed, T, keys)):
            assert np.array_equal(alone.target(i), tgt), i
            assert np.array_equal(alone.token_scores(i).view(np.uint32), sc.view(np.uint32)), i
            assert np.all(np.isfinite(sc)) and np.all(sc <= 1e-6)
        # the plain translate of a sampling service uses seed 0; another seed draws other translations
        plain, zero, two = svc.translate(mine), svc.translate(mine, seed=0), svc.translate(mine, seed=2)
        assert np.array_equal(plain.targets, zero.targets)
        differ = sum(1 for i in range(len(mine)) if not np.array_equal(two.target(i), alone.target(i)))
        assert differ >= len(mine) // 2, differ
        assert hip.host_lib().slimt_hip_service_set_sampling(svc.h, 0.5) != 0  # only before the first translate
        for r in (alone, mixed, results["other"], plain, zero, two):
            r.close()
    finally:
        svc.close()
    greedy = hip.BatchService([gm], max_words=(10 + 1) * S, workers_per_device=1, source_vocab=m.V, target_vocab=m.V, shortlist=fixed)
    try:
        with pytest.raises(capi.SlimtHipError):  # a service that does not sample fails loudly
            greedy.translate(mine[:2], seed=1)
    finally:
        greedy.close()
        gm.close()


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


def test_frontend_sampling_is_reproducible_and_scored(hip, spm_model, corpus):
    from slimt_amd import frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    blob = synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5)
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm_model, shortlist=blob)
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=2, max_words=256, wrap_length=24)
    try:
        texts = [" ".join(corpus[i:i + 3]) + "\n" + corpus[i + 3] for i in range(0, 40, 4)]
        a = svc.translate(model, texts, encoding=frontend.Encoding.Byte, sampling=(1.0, 7), scores=True)
        b = svc.translate(model, texts, encoding=frontend.Encoding.Byte, sampling=(1.0, 7), scores=True)
        c = svc.translate(model, texts, encoding=frontend.Encoding.Byte, sampling=(1.0, 8))
        g = svc.translate(model, texts, encoding=frontend.Encoding.Byte)
        for x, y in zip(a, b):
            assert x.target.text == y.target.text
            n = x.target.sentence_count()
            assert len(x.sentence_scores) == n and np.all(np.isfinite(x.sentence_scores))
            assert x.sentence_scores == y.sentence_scores
            for k in range(n):
                assert len(x.token_scores[k]) == x.target.word_count(k) and np.all(x.token_scores[k] <= 1e-6)
        assert any(x.target.text != y.target.text for x, y in zip(a, c))
        assert any(x.target.text != y.target.text for x, y in zip(a, g))
        assert all(not y.token_scores for y in c)
        # pivot: both hops sample (seed and seed + 1), reproducibly
        p1 = svc.pivot(model, model, texts[:4], sampling=(1.0, 3), scores=True)
        p2 = svc.pivot(model, model, texts[:4], sampling=(1.0, 3), scores=True)
        for x, y in zip(p1, p2):
            assert x.target.text == y.target.text and np.all(np.isfinite(x.sentence_scores))
    finally:
        svc.close()
        model.close()
