"""GPU parity of per-token scores (include/slimt_hip.h, slimt_hip_ctx_set_scores): the log-softmax probability of every
recorded token over that step's output layer, from the persistent decoder's scored 16-sentence kernels and from the
step-wise launches (decode mode 1). The reference is the checker, teacher-forced along the recorded tokens (embed ->
encode -> decode_step), with log_softmax taken in float64. Scoring only observes: tokens, lengths and alignment rows
are bit-identical to the unscored call (and the checker's); merged launches score every batch bit-identically to the
batch's own scored call; poisoned logits score NaN and still sample class 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-5


@pytest.fixture(scope="module")
def engines(hip, oracle, synth_models):
    cache = {}

    def get(preset, eos_bias):
        key = (preset, eos_bias)
        if key not in cache:
            m = synth_models(preset, eos_bias)
            cache[key] = (m, hip.Model(m), oracle.OracleModel(m))
        return cache[key]

    yield get
    for _, gm, _ in cache.values():
        gm.close()


def _teacher_forced(oracle, om, m, ids, lens, sl, out, ln):
    """float64 log_softmax of the checker's logits at the recorded tokens, step by step along them."""
    oracle.set_mode(oracle.PORTABLE)
    try:
        B, S = ids.shape
        mask = oracle.make_mask(lens, S)
        enc = om.encode(om.embed(ids), mask)
        states = np.zeros((m.dec_layers, B, m.D), np.float32)
        ref = np.full(out.shape, np.nan)
        prev = None
        for t in range(int(ln.max())):
            logits, _ = om.decode_step(enc, mask, states, prev, sl)
            lg = logits.astype(np.float64)
            mx = lg.max(axis=1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(axis=1))
            col = out[:, t].astype(np.int64) if sl is None else np.searchsorted(sl, out[:, t])
            col = np.minimum(col, lg.shape[1] - 1)
            ref[:, t] = lg[np.arange(B), col] - lse
            prev = out[:, t].astype(np.uint32)
        return ref
    finally:
        oracle.set_mode(oracle.FAITHFUL)


def _check_scores(sc, ref, ln):
    for b in range(len(ln)):
        n = int(ln[b])
        got, want = sc[b, :n].astype(np.float64), ref[b, :n]
        assert np.all(np.isfinite(got)), (b, got)
        assert np.all(got <= 1e-6), (b, got)
        err = np.abs(got - want)
        assert err.max(initial=0) <= TOL, (b, int(err.argmax()), got[err.argmax()], want[err.argmax()])
        assert abs(got.sum() - want.sum()) <= TOL * n, b


def _want(oracle, om, ids, lens, sl, eos=0):
    oracle.set_mode(oracle.PORTABLE)
    out = om.translate(ids, lens, sl, 1.5, eos, want_align=True)[:3]
    oracle.set_mode(oracle.FAITHFUL)
    return out


CASES = [  # preset, S, B, output layer, decode modes
    ("tiny11", 32, 17, 4096, (0, 1, 3, 6)),
    ("tiny11", 8, 256, 4096, (0,)),
    ("tiny11", 64, 17, 4096, (0, 1)),
    ("tiny11", 100, 1, 4096, (0, 1)),
    ("tiny11", 8, 17, None, (0, 1, 3)),  # the full vocabulary: 32,000 columns
    ("base", 32, 17, 4096, (0, 1)),
    ("base", 8, 1, None, (0,)),
]


@pytest.mark.parametrize("preset,S,B,n_sl,modes", CASES)
def test_scores_match_teacher_forced_log_softmax(hip, oracle, engines, preset, S, B, n_sl, modes):
    from slimt_amd import synth
    m, gm, om = engines(preset, 6.0)
    ids, lens = synth.make_batch(m.V, B, S, seed=31 + S + B, ragged=True)
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    w_out, w_ln, w_al = _want(oracle, om, ids, lens, sl)
    ref = _teacher_forced(oracle, om, m, ids, lens, sl, w_out, w_ln)
    ctx = hip.Context(gm, B, S)
    for mode in modes:
        ctx.set_decode_mode(mode)
        out, ln, al = ctx.translate(ids, lens, sl, want_align=True)
        s_out, s_ln, s_al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True)
        assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out) and np.array_equal(al, w_al), mode
        assert np.array_equal(s_ln, ln) and np.array_equal(s_out, out) and np.array_equal(s_al, al), mode
        _check_scores(sc, ref, ln)
        # the pinned asynchronous form: the kernels write the scores in host memory themselves
        p_out, p_ln, _, p_sc = ctx.translate_pinned(ids, lens, sl, scores=True)
        assert np.array_equal(p_out, out) and np.array_equal(p_ln, ln)
        for b in range(B):
            assert np.array_equal(p_sc[b, :ln[b]], sc[b, :ln[b]]), (mode, b)
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_scores_over_a_generated_lexical_shortlist(hip, oracle, engines, mode):
    from slimt_amd import synth
    m, gm, om = engines("tiny11", 6.0)
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    B, S = 17, 16
    ids, lens = synth.make_batch(m.V, B, S, seed=5, ragged=True)
    sl = osl.generate(ids, lens)
    w_out, w_ln, _ = _want(oracle, om, ids, lens, sl)
    ref = _teacher_forced(oracle, om, m, ids, lens, sl, w_out, w_ln)
    ctx = hip.Context(gm, B, S)
    ctx.set_decode_mode(mode)
    out, ln, _ = ctx.translate_generated(gen, ids, lens)
    s_out, s_ln, _, sc = ctx.translate_generated(gen, ids, lens, scores=True)
    assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out)
    assert np.array_equal(s_ln, ln) and np.array_equal(s_out, out)
    _check_scores(sc, ref, ln)
    ctx.close()
    gen.close()


def test_ragged_eos_rows_keep_their_scores(hip, oracle, engines):
    """Sentences end at different steps (EOS bias): every defined entry matches the reference -- the steps the tile still
    runs after a sentence has ended do not disturb it."""
    from slimt_amd import synth
    m, gm, om = engines("tiny11", 8.0)
    B, S = 40, 24
    ids, lens = synth.make_batch(m.V, B, S, seed=9, ragged=True)
    sl = synth.make_shortlist(m.V, 2048)
    w_out, w_ln, _ = _want(oracle, om, ids, lens, sl)
    assert len(set(w_ln.tolist())) >= 4
    ref = _teacher_forced(oracle, om, m, ids, lens, sl, w_out, w_ln)
    ctx = hip.Context(gm, B, S)
    for mode in (0, 1):
        ctx.set_decode_mode(mode)
        sc = np.full(w_out.shape, 7.5, np.float32)
        ctx.set_scores([sc])  # (armed by hand: the next call takes it)
        out, ln, _ = ctx.translate(ids, lens, sl)
        assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out)
        _check_scores(sc, ref, ln)
    ctx.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_merged_async_scores_equal_each_batch_own_call(hip, oracle, engines):
    from slimt_amd import capi, synth
    m, gm, om = engines("tiny11", 6.0)
    shapes = [(40, 16), (7, 12), (33, 16)]  # sizes that leave holes, mixed padded lengths
    sl = synth.make_shortlist(m.V, 4096)
    batches = [synth.make_batch(m.V, B, Sj, seed=100 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    rows = hip.translate_many_rows([b for b, _ in shapes])
    ctx = hip.Context(gm, rows, 16)
    pins, bufs, scs = [], [], []
    for ids, lens in batches:
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        arrs = []
        for dt, shape in ((np.uint32, (B, Sj)), (np.uint32, (B,)), (np.uint32, (B, T)), (np.uint32, (B,)), (np.float32, (B, T))):
            p = capi._Pinned()
            pins.append(p)
            arrs.append(p.array(dt, shape))
        arrs[0][...] = ids
        arrs[1][...] = lens
        arrs[4][...] = 7.5
        bufs.append(tuple(arrs[:4]) + (None,))
        scs.append(arrs[4])
    ctx.translate_many_async(bufs, sl, scores=scs)
    ctx.synchronize()
    own = hip.Context(gm, rows, 16)
    for (ids, lens), b, sc in zip(batches, bufs, scs):
        o_out, o_ln, _, o_sc = own.translate(ids, lens, sl, scores=True)
        w_out, w_ln, _ = _want(oracle, om, ids, lens, sl)
        assert np.array_equal(b[3], o_ln) and np.array_equal(b[2], o_out)
        assert np.array_equal(o_ln, w_ln) and np.array_equal(o_out, w_out)
        for r in range(ids.shape[0]):
            assert np.array_equal(sc[r, :o_ln[r]], o_sc[r, :o_ln[r]]), r
        ref = _teacher_forced(oracle, om, m, ids, lens, sl, w_out, w_ln)
        _check_scores(sc, ref, w_ln)
    ctx.close()
    own.close()
    for p in pins:
        p.free()


def test_merged_device_generated_scores_equal_each_batch_own_call(hip, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11", 6.0)
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    shapes = [(64, 16), (10, 13), (17, 16)]
    S = 16
    batches = [synth.make_batch(m.V, B, Sj, seed=300 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    rows = hip.translate_many_rows([b for b, _ in shapes])
    ctx = hip.Context(gm, rows, S)
    keep, args, outs, d_scs = [], [], [], []
    for ids, lens in batches:
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        d_ids, d_len = _dev(ids), _dev(lens)
        d_out = torch.full((B, T), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_ol = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_sc = torch.full((B, T), 7.5, dtype=torch.float32, device="cuda")
        keep.append((d_ids, d_len))
        outs.append((d_out, d_ol))
        d_scs.append(d_sc)
        args.append((d_ids.data_ptr(), d_len.data_ptr(), B, 0, 0, d_out.data_ptr(), d_ol.data_ptr(), 0, Sj))
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=max(int(np.float32(1.5) * np.float32(S)), 1), generator=gen,
                              scores=[d.data_ptr() for d in d_scs])
    ctx.synchronize()
    own = hip.Context(gm, rows, S)
    for (ids, lens), (d_out, d_ol), d_sc in zip(batches, outs, d_scs):
        out, ln = d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32)
        sc = d_sc.cpu().numpy()
        o_out, o_ln, _, o_sc = own.translate_generated(gen, ids, lens, scores=True)
        assert np.array_equal(ln, o_ln) and np.array_equal(out, o_out)
        for r in range(ids.shape[0]):
            assert np.array_equal(sc[r, :ln[r]], o_sc[r, :ln[r]]), r
            assert (sc[r, ln[r]:] == 7.5).all(), r
    ctx.close()
    own.close()
    gen.close()


def test_set_scores_mismatch_fails_the_call_and_is_consumed(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11", 6.0)
    B, S = 4, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=2, ragged=True)
    ctx = hip.Context(gm, B, S)
    T = max(int(np.float32(1.5) * np.float32(S)), 1)
    a, b = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    ctx.set_scores([a, b])  # two destinations for a single-batch call
    with pytest.raises(hip.SlimtHipError) as e:
        ctx.translate(ids, lens)
    assert "scores" in str(e.value)
    out, ln, _ = ctx.translate(ids, lens)  # consumed: the next call is an ordinary one
    assert ln.min() >= 1
    ctx.set_scores([0])
    with pytest.raises(hip.SlimtHipError):
        ctx.translate(ids, lens)
    ctx.close()


@pytest.mark.parametrize("poison", ["nan", "-inf", "nan-in-column-0"])
def test_poisoned_logits_score_nan_and_sample_class_zero(hip, oracle, synth_models, poison):
    import copy
    from slimt_amd import synth
    m = copy.deepcopy(synth_models("tiny11", 6.0))
    bias = m.params["decoder_ff_logit_out_b"]
    B, S = 19, 11
    ids, lens = synth.make_batch(m.V, B, S, seed=4, ragged=True)
    shortlists = (synth.make_shortlist(m.V, 1024), None)
    if poison == "nan-in-column-0":
        bias.data.reshape(-1)[0] = np.float32(np.nan)
    else:
        bias.data[...] = np.float32(np.nan) if poison == "nan" else np.float32(-np.inf)
    gm, om = hip.Model(m), oracle.OracleModel(m)
    eos = 0 if poison != "nan-in-column-0" else 7
    for sl in shortlists:
        oracle.set_mode(oracle.PORTABLE)
        w_out, w_ln, _, _ = om.translate(ids, lens, sl, 1.5, eos)
        oracle.set_mode(oracle.FAITHFUL)
        ctx = hip.Context(gm, B, S)
        for mode in (0, 1, 2, 3, 5, 6):
            ctx.set_decode_mode(mode)
            out, ln, _, sc = ctx.translate(ids, lens, sl, eos_id=eos, scores=True)
            assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), (poison, mode, sl is None)
            for b in range(B):
                assert np.isnan(sc[b, :ln[b]]).all(), (poison, mode, b)
        ctx.close()
    gm.close()
