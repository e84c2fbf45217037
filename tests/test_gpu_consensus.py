"""GPU checks of the consensus selection (include/slimt_hip.h, slimt_hip_consensus_select*, slimt_hip_ctx_set_fanout_consensus):
utility bits (as uint64) and best against the reference of tests/support/consensus_ref.py -- integer counts and doubles in a
fixed order, so the comparison is exact. The synthetic cases and what they are for: tests/support/consensus_cases.py
(tests/test_consensus_case_fixtures.py proves them on the CPU). Armed on a fan-out call: every ordinary output has the
un-armed call's bits, and best / utility are the reference's on the rows the call returned."""
import numpy as np
import pytest
import torch

from support import consensus_cases as CC
from support import consensus_ref as R
from support import fanout_cases as FC
from test_forced_prefix_checker import tmax_of

pytestmark = pytest.mark.gpu

G, BETA2 = 4, 4
TRUNC = dict(truncation=(FC.TOP_K, FC.TOP_P))


def _same(got, want, what):
    util, best = got
    w_util, w_best = want
    assert np.array_equal(best, w_best), (what, best, w_best)
    assert np.array_equal(R.bits(util), R.bits(w_util)), (what, util, w_util)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).cuda()


# ---- the stateless call on synthetic ids ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_order,beta2", CC.runs())
def test_select_equals_the_reference(hip, name, max_order, beta2):
    c = CC.table()[name]
    got = hip.consensus_select(c.ids, c.lens, c.row_src, c.B, max_order, beta2)
    _same(got, CC.reference(name, max_order, beta2), name)
    assert not np.isnan(got[0]).any()


def test_no_rows_writes_best_only_and_65_rows_of_a_source_are_refused(hip):
    util, best = hip.consensus_select(np.zeros((0, 7), np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3)
    assert util.size == 0 and list(best) == [R.NO_ROW] * 3
    ids, lens, src, B = CC.rows65()
    with pytest.raises(hip.SlimtHipError, match="source 0 has more than 64 rows"):
        hip.consensus_select(ids, lens, src, B)


def test_shuffled_rows_give_the_sorted_result_through_the_permutation(hip):
    """the best rows map exactly (no source ties at the top: the fixture test); a utility is a sum in ascending row order, so
    under another order its last bits may differ, while against the reference computed in the same order it is exact
    (test_select_equals_the_reference). The bound: a source has at most 6 rows, so a sum has at most 5 terms <= 1 and stays
    under 8, where an addition errs by at most 2^-51; two orders of 5 additions differ by at most 10 * 2^-51, halved or more
    by the division by >= 2 references, whose own rounding adds 2^-53 each: under 2^-48"""
    ORDER_BOUND = 2.0 ** -48
    s, sh, perm = CC.table()["order5_sorted"], CC.table()["order5_shuffled"], CC.shuffle_permutation()
    u_s, b_s = hip.consensus_select(s.ids, s.lens, s.row_src, s.B, G, BETA2)
    u_h, b_h = hip.consensus_select(sh.ids, sh.lens, sh.row_src, sh.B, G, BETA2)
    assert np.array_equal(perm[b_h], b_s)
    assert np.abs(u_h - u_s[perm]).max() <= ORDER_BOUND
    rev = CC.table()["order5_reversed"]
    u_r, b_r = hip.consensus_select(rev.ids, rev.lens, rev.row_src, rev.B, G, BETA2)
    n = s.row_src.size
    assert np.array_equal(n - 1 - b_r, b_s) and np.abs(u_r[::-1] - u_s).max() <= ORDER_BOUND


@pytest.fixture(scope="module")
def micro(hip, synth_models):
    gm = hip.Model(synth_models("micro", 3.0))
    ctx = hip.Context(gm, 4, 8)
    yield ctx
    ctx.close()
    gm.close()


def _select_device(ctx, ids, lens, src, B, max_order=G, beta2=BETA2):
    N, T = ids.shape
    d_ids, d_len, d_src = _dev(ids), _dev(lens), _dev(src)
    d_util = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    d_best = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
    ctx.consensus_select_device(d_ids.data_ptr(), d_len.data_ptr(), d_src.data_ptr(), N, T, B, max_order, beta2,
                                d_util.data_ptr(), d_best.data_ptr())
    ctx.synchronize()
    return d_util.cpu().numpy(), d_best.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", ["three_rows", "lone_none_empty", "T65", "T256", "wide_ids", "rows64", "order5_shuffled", "b300"])
def test_the_device_variant_gives_the_same_bits(micro, name):
    c = CC.table()[name]
    _same(_select_device(micro, c.ids, c.lens, c.row_src, c.B), CC.reference(name), name)


def test_the_device_variant_clamps_what_it_cannot_check(micro):
    """a row_src >= B reads as B - 1 and a len > T as T; a source with 65 rows gets no selection and utility 0, the other
    sources are not disturbed; nothing else is written"""
    c = CC.table()["order5_shuffled"]
    src, lens = c.row_src.copy(), c.lens.copy()
    src[3], lens[5] = c.B + 9, c.ids.shape[1] + 40
    want = R.select(c.ids, np.minimum(lens, c.ids.shape[1]), np.minimum(src, c.B - 1), c.B, G, BETA2)
    _same(_select_device(micro, c.ids, lens, src, c.B), want, "clamped")
    ids, lens, src, _ = CC.rows65()
    three = CC.table()["three_rows"]
    T = max(ids.shape[1], three.ids.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, T - a.shape[1])))
    both = (np.concatenate([pad(three.ids), pad(ids)]), np.concatenate([three.lens, lens]),
            np.concatenate([three.row_src, src + 1]))
    util, best = _select_device(micro, *both, 2)
    w_util, w_best = R.select(pad(three.ids), three.lens, three.row_src, 1, G, BETA2)
    assert list(best) == [int(w_best[0]), R.NO_ROW]
    assert np.array_equal(R.bits(util[:3]), R.bits(w_util)) and np.array_equal(R.bits(util[3:]), R.bits(np.zeros(65)))


# ---- armed on a fan-out call ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(hip, synth_models):
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    yield m, gm
    gm.close()


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ordinary_outputs_equal(got, want, what):
    """tokens, lengths, alignment bits and the recorded tokens' score bits"""
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(_bits32(got[2]), _bits32(want[2])), what
    live = np.arange(got[0].shape[1])[None, :] < got[1][:, None]
    assert np.array_equal(_bits32(got[3])[live], _bits32(want[3])[live]), what


def _check_armed(got, want, row_src, B, what):
    _ordinary_outputs_equal(got, want, what)
    best, util = got[-2], got[-1]
    _same((util, best), R.select(got[0], got[1], row_src, B, G, BETA2), what)
    assert len({float(u) for u in util}) > 2, what  # (the draws do differ: a selection that does nothing would not pass)


def _fan_cases():
    return [FC.parity("s8"), FC.parity("s32"), FC.edge_case("shuffled")]


@pytest.mark.parametrize("c", _fan_cases(), ids=lambda c: c.name)
def test_armed_host_calls_keep_every_output_and_select_as_the_reference(hip, tiny, c):
    m, gm = tiny
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    kw = dict(scores=True, sampling=(1.0, keys), want_align=True, **TRUNC)
    ctx = hip.Context(gm, max(N, c.B), c.S)
    try:
        want = ctx.translate_fanout(ids, lens, c.row_src, sl, **kw)
        got = ctx.translate_fanout(ids, lens, c.row_src, sl, consensus=(G, BETA2), **kw)
        assert len(got) == len(want) + 2 and got[-2].shape == (c.B,) and got[-1].shape == (N,)
        _check_armed(got, want, c.row_src, c.B, "translate_fanout")
        _check_armed(ctx.translate_fanout_pinned(ids, lens, c.row_src, sl, consensus=(G, BETA2), **kw), want, c.row_src, c.B,
                     "translate_fanout_async")
        _ordinary_outputs_equal(ctx.translate_fanout(ids, lens, c.row_src, sl, **kw), want, "un-armed again")
    finally:
        ctx.close()


@pytest.mark.parametrize("c", _fan_cases(), ids=lambda c: c.name)
def test_armed_generated_call_keeps_every_output_and_selects_as_the_reference(hip, tiny, c):
    from slimt_amd import synth
    m, gm = tiny
    ids, lens, _, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    kw = dict(generator=gen, scores=True, sampling=(1.0, keys), want_align=True, **TRUNC)
    ctx = hip.Context(gm, max(N, c.B), c.S)
    try:
        want = ctx.translate_fanout_pinned(ids, lens, c.row_src, **kw)
        _check_armed(ctx.translate_fanout_pinned(ids, lens, c.row_src, consensus=(G, BETA2), **kw), want, c.row_src, c.B,
                     "translate_fanout_async_generated")
    finally:
        ctx.close()
        gen.close()


@pytest.mark.parametrize("c", _fan_cases(), ids=lambda c: c.name)
def test_armed_device_call_keeps_every_output_and_selects_as_the_reference(hip, tiny, c):
    m, gm = tiny
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N, B, S, Tm = c.row_src.size, c.B, c.S, tmax_of(c.S)
    ctx = hip.Context(gm, max(N, B), S)
    try:
        want = ctx.translate_fanout(ids, lens, c.row_src, sl, scores=True, sampling=(1.0, keys), want_align=True, **TRUNC)
        d_ids, d_len, d_sl, d_keys, d_src = _dev(ids), _dev(lens), _dev(sl), _dev(keys), _dev(c.row_src)
        d_out = torch.zeros((N, Tm), dtype=torch.int32, device="cuda")
        d_ol = torch.zeros((N,), dtype=torch.int32, device="cuda")
        d_sc = torch.zeros((N, Tm), dtype=torch.float32, device="cuda")
        d_al = torch.zeros((N, Tm, S), dtype=torch.float32, device="cuda")
        d_best = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
        d_util = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
        ctx.translate_fanout_device(d_ids.data_ptr(), d_len.data_ptr(), B, S, d_src.data_ptr(), N, d_sl.data_ptr(), sl.size, 1.5, 0,
                                    d_out.data_ptr(), d_ol.data_ptr(), d_al.data_ptr(), steps_hint=Tm, scores=d_sc.data_ptr(),
                                    sampling=(1.0, d_keys.data_ptr()), consensus=(G, BETA2, d_best.data_ptr(), d_util.data_ptr()),
                                    **TRUNC)
        ctx.synchronize()
        got = (d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), d_al.cpu().numpy(), d_sc.cpu().numpy(),
               d_best.cpu().numpy().view(np.uint32), d_util.cpu().numpy())
        _check_armed(got, want, c.row_src, B, "translate_fanout_device")
    finally:
        ctx.close()


def test_the_option_is_consumed_by_the_next_translate_call_whatever_its_outcome(hip, tiny):
    m, gm = tiny
    c = FC.parity("s8")
    ids, lens, sl, keys = FC.inputs(c, m.V)
    N = c.row_src.size
    kw = dict(scores=True, sampling=(1.0, keys), want_align=True, **TRUNC)
    ctx = hip.Context(gm, max(N, c.B), c.S)
    try:
        want = ctx.translate_fanout(ids, lens, c.row_src, sl, **kw)
        best, util = np.full(c.B, 12345, np.uint32), np.full(N, -7.0)
        # a plain translate finds it armed: refused, and consumed -- the next fan-out call runs un-armed
        ctx.set_fanout_consensus(G, BETA2, best, util)
        with pytest.raises(hip.SlimtHipError, match="not a fan-out call"):
            ctx.translate(ids, lens, sl)
        _ordinary_outputs_equal(ctx.translate_fanout(ids, lens, c.row_src, sl, **kw), want, "after the refused translate")
        assert (best == 12345).all() and (util == -7.0).all()
        # a fan-out call that fails (no rows) consumes it too
        ctx.set_fanout_consensus(G, BETA2, best, util)
        with pytest.raises(hip.SlimtHipError, match="no rows"):
            ctx.translate_fanout(ids, lens, np.zeros(0, np.uint32), sl)
        _ordinary_outputs_equal(ctx.translate_fanout(ids, lens, c.row_src, sl, **kw), want, "after the failed fan-out call")
        assert (best == 12345).all() and (util == -7.0).all()
        # max_order = 0 disarms
        ctx.set_fanout_consensus(G, BETA2, best, util)
        ctx.set_fanout_consensus(0, 0, None, None)
        ctx.translate(ids, lens, sl)
        assert (best == 12345).all() and (util == -7.0).all()
        # armed and taken: written
        ctx.set_fanout_consensus(G, BETA2, best, util)
        got = ctx.translate_fanout(ids, lens, c.row_src, sl, **kw)
        _check_armed(got + (best, util), want, c.row_src, c.B, "armed by hand")
    finally:
        ctx.close()


# ---- the service and the text front end -------------------------------------------------------------------------------------
def test_batch_service_consensus_is_the_selected_entry_of_translate_samples(hip, tiny):
    from slimt_amd import synth
    m, gm = tiny
    rnd = np.random.Generator(np.random.PCG64(15))
    count, n, seed = 9, 5, 5
    sents = [list(rnd.integers(3, m.V, int(rnd.integers(4, 12)))) + [0] for _ in range(count)]
    fixed = synth.make_shortlist(m.V, 2048)
    svc = hip.BatchService([gm], max_words=80, wrap_length=16, workers_per_device=1, shortlist=fixed, temperature=1.0,
                           truncation=(FC.TOP_K, FC.TOP_P))
    try:
        samples = svc.translate_samples(sents, n, seed=seed)
        res, util, index = svc.translate_consensus(sents, n, seed=seed, max_order=G, beta2=BETA2)
        assert res.n == count and util.shape == index.shape == (count,)
        picked_other = 0
        for i in range(count):
            rows = [samples.target(i * n + j) for j in range(n)]
            T = max(len(r) for r in rows)
            ids = np.zeros((n, T), np.uint32)
            for j, r in enumerate(rows):
                ids[j, :len(r)] = r
            w_util, w_best = R.select(ids, [len(r) for r in rows], np.zeros(n, np.uint32), 1, G, BETA2)
            j = int(index[i])
            assert j == int(w_best[0]) and R.bits(util[i:i + 1])[0] == R.bits(w_util[j:j + 1])[0], i
            e = i * n + j
            assert np.array_equal(res.target(i), samples.target(e)), i
            assert np.array_equal(_bits32(res.token_scores(i)), _bits32(samples.token_scores(e))), i
            assert np.array_equal(_bits32(res.alignment(i)), _bits32(samples.alignment(e))), i
            picked_other += j != 0
        assert picked_other > 0  # (the pick is not always the first sample)
        res.close()
        # n = 1: the lone sample, utility 0
        res, util, index = svc.translate_consensus(sents, 1, seed=seed)
        lone = svc.translate_samples(sents, 1, seed=seed)
        for i in range(count):
            assert np.array_equal(res.target(i), lone.target(i)) and util[i] == 0.0 and index[i] == 0
        res.close()
        lone.close()
        samples.close()
        with pytest.raises(hip.SlimtHipError, match="at most 64"):
            svc.translate_consensus(sents, 65, seed=seed)
    finally:
        svc.close()


def test_frontend_sample_and_select_against_samples_and_the_reference(hip):
    """text -> text: the winner of every text is the alternative of translate(samples=n) that the reference picks among the
    alternatives' token ids"""
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
        sources, n, sampling = corpus[:3], 5, (1.0, 11)
        alts = svc.translate(model, sources, sampling=sampling, samples=n)
        won = svc.sample_and_select(model, sources, n, sampling)
        # the samples' token ids, as the service under translate(samples=n) returns them: [sample][text][segment]
        processed = model.processor.process_many(sources, svc.wrap_length, svc.workers)
        drawn = svc._translate_samples(model, [segs for _, segs in processed], n, sampling)
        assert len(won) == 3
        segments = 0
        for t, (r, w) in enumerate(zip(alts, won)):
            n_seg = len(processed[t][1])  # (a source longer than wrap_length goes as several segments, each picked on its own)
            assert len(w.utility) == len(w.sample_index) == len(w.token_scores) == len(w.alignments) == n_seg >= 1
            for i in range(n_seg):
                rows = [drawn[j][t][i][0] for j in range(n)]
                ids = np.zeros((n, max(len(x) for x in rows)), np.uint32)
                for j, x in enumerate(rows):
                    ids[j, :len(x)] = x
                w_util, w_best = R.select(ids, [len(x) for x in rows], np.zeros(n, np.uint32), 1, 4, 4)
                j = int(w_best[0])
                assert w.sample_index[i] == j and R.bits([w.utility[i]])[0] == R.bits(w_util[j:j + 1])[0], (t, i)
                assert np.array_equal(_bits32(w.token_scores[i]), _bits32(r.samples[j].token_scores[i])), (t, i)
                assert np.array_equal(_bits32(w.alignments[i]), _bits32(r.samples[j].alignments[i])), (t, i)
                segments += 1
            if n_seg == 1:
                assert w.target.text == r.samples[w.sample_index[0]].target.text
        assert segments >= 3
        with pytest.raises(ValueError):
            svc.sample_and_select(model, sources, n, None)
    finally:
        svc.close()
        model.close()
