"""GPU parity of sampled decoding (include/slimt_hip.h, slimt_hip_ctx_set_sampling) against the checker of
tests/test_sampling_checker.py. The noise is bit-reproducible on the host and the logits already are, so tokens, lengths
and alignment rows are bit-equal to the checker's, with no allowance for near-ties; scores are within
5e-5 * max(1, 1 / T) of its float64 log_softmax(logit / T) -- the project's tolerance for scores, scaled because the
exponents are. A sentence's draw depends on its key alone: not on the decode mode, the entry point, its row or its
neighbours, or on whether the launch is merged.

Decode modes: 0 (the engine's choice), 1 (the per-stage kernels) and 3 run on every shape. Sampled calls are scored, so
modes 2-6 all take the 16-sentence tiling without clusters; every context accepts mode 6 (cluster logits), and for a
sampled call it selects the kernels mode 3 does, so it runs on the first case alone, on purpose: the shape (D = 256,
packed cache, short sentences) where an unscored call in mode 6 would take the cluster kernels."""
import numpy as np
import pytest
import torch

from test_forced_prefix_checker import tmax_of
from test_sampling_checker import keys_of, sampled_translate

pytestmark = pytest.mark.gpu

TOL = 5e-5


@pytest.fixture(scope="module")
def engines(hip, oracle, synth_models):
    cache = {}

    def get(preset, eos_bias=6.0):
        if (preset, eos_bias) not in cache:
            m = synth_models(preset, eos_bias)
            cache[(preset, eos_bias)] = (m, hip.Model(m), oracle.OracleModel(m))
        return cache[(preset, eos_bias)]

    yield get
    for _, gm, _ in cache.values():
        gm.close()


def _check(got, want, T, scores=True):
    out, ln, al = got[:3]
    w_out, w_ln, w_al, w_sc = want
    assert np.array_equal(ln, w_ln), (ln, w_ln)
    assert np.array_equal(out, w_out)
    if al is not None:
        assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32))
    if scores:
        tol = TOL * max(1.0, 1.0 / T)
        worst = 0.0
        for b in range(len(ln)):
            n = int(ln[b])
            g, w = got[3][b, :n].astype(np.float64), w_sc[b, :n]
            assert np.array_equal(np.isneginf(g), np.isneginf(w)), (b, g, w)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (b, g, w)
            fin = np.isfinite(w)
            worst = max(worst, np.abs(g[fin] - w[fin]).max(initial=0))
        print("scores: max |gpu - float64| = %.3g (bound %.3g)" % (worst, tol))
        assert worst <= tol, worst


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).cuda()


CASES = [  # preset, eos bias, S, B, shortlist, decode modes
    ("tiny11", 6.0, 32, 17, 4096, (0, 1, 3, 6)),
    ("tiny11", 7.0, 8, 17, None, (0, 1, 3)),
    ("tiny11", 8.0, 64, 17, 4096, (0, 1, 3)),
    ("tiny11", 6.0, 100, 1, 4096, (0, 1, 3)),
    ("base", 6.0, 32, 17, 4096, (0, 1, 3)),
    ("base", 7.0, 8, 1, None, (0, 1, 3)),
]


@pytest.mark.parametrize("preset,eos_bias,S,B,n_sl,modes", CASES)
def test_sampled_translations_match_the_checker_bit_for_bit(hip, oracle, engines, preset, eos_bias, S, B, n_sl, modes):
    from slimt_amd import synth
    m, gm, om = engines(preset, eos_bias)
    ids, lens = synth.make_batch(m.V, B, S, seed=61 + S + B, ragged=True)
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    keys = keys_of(S + B, B)
    ctx = hip.Context(gm, B, S)
    for T in (0.7, 1.0):
        want = sampled_translate(oracle, om, m, ids, lens, sl, keys, T)
        for mode in modes:
            ctx.set_decode_mode(mode)
            _check(ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys)), want, T)
    ctx.close()


def test_every_entry_point_draws_the_same_bits(hip, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S, T = 17, 16, 1.0
    ids, lens = synth.make_batch(m.V, B, S, seed=23, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    Tm = tmax_of(S)
    keys = keys_of(4, B)
    want = sampled_translate(oracle, om, m, ids, lens, sl, keys, T)
    ctx = hip.Context(gm, B, S)
    _check(ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys)), want, T)  # pageable
    _check(ctx.translate(ids, lens, sl, want_align=True, sampling=(T, keys)), want, T, scores=False)  # no destination armed
    _check(ctx.translate_pinned(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys)), want, T)  # pinned, async
    _check(ctx.translate_pinned(ids, lens, sl, sampling=(T, keys)), want, T, scores=False)
    # keys = None: the row indices
    rows = sampled_translate(oracle, om, m, ids, lens, sl, None, T)
    _check(ctx.translate(ids, lens, sl, scores=True, sampling=(T, None)), rows, T)
    # device arrays, device keys
    d_ids, d_len, d_sl, d_keys = _dev(ids), _dev(lens), _dev(sl), _dev(keys)
    d_out = torch.zeros((B, Tm), dtype=torch.int32, device="cuda")
    d_ol = torch.zeros((B,), dtype=torch.int32, device="cuda")
    d_sc = torch.zeros((B, Tm), dtype=torch.float32, device="cuda")
    for with_scores in (True, False):
        d_out.zero_()
        ctx.translate_device(d_ids.data_ptr(), d_len.data_ptr(), B, S, d_sl.data_ptr(), sl.size, 1.5, 0, d_out.data_ptr(),
                             d_ol.data_ptr(), scores=d_sc.data_ptr() if with_scores else 0, sampling=(T, d_keys.data_ptr()))
        ctx.synchronize()
        _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), want, T,
               scores=with_scores)
    # a generated lexical shortlist: the noise goes by vocabulary id, whatever the list's layout
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    gwant = sampled_translate(oracle, om, m, ids, lens, osl.generate(ids, lens), keys, T)
    _check(ctx.translate_generated(gen, ids, lens, scores=True, sampling=(T, keys)), gwant, T)
    _check(ctx.translate_pinned(ids, lens, generator=gen, scores=True, sampling=(T, keys)), gwant, T)
    ctx.translate_device_generated(gen, d_ids.data_ptr(), d_len.data_ptr(), B, S, 1.5, 0, d_out.data_ptr(), d_ol.data_ptr(),
                                   scores=d_sc.data_ptr(), sampling=(T, d_keys.data_ptr()))
    ctx.synchronize()
    _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), gwant, T)
    ctx.close()
    gen.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_a_sentence_draws_the_same_alone_and_in_any_row(hip, engines, mode):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T = 17, 32, 1.0
    ids, lens = synth.make_batch(m.V, B, S, seed=31, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(8, B)
    ctx = hip.Context(gm, B, S)
    ctx.set_decode_mode(mode)
    full = ctx.translate(ids, lens, sl, sampling=(T, keys))
    rev = ctx.translate(ids[::-1].copy(), lens[::-1].copy(), sl, sampling=(T, keys[::-1].copy()))
    assert np.array_equal(rev[1][::-1], full[1]) and np.array_equal(rev[0][::-1], full[0])
    for b in (0, 5, 16):
        one = ctx.translate(ids[b:b + 1], lens[b:b + 1], sl, sampling=(T, keys[b:b + 1].copy()))
        assert one[1][0] == full[1][b] and np.array_equal(one[0][0], full[0][b]), b
    ctx.close()


def test_merged_launches_equal_each_batch_own_sampled_call(hip, engines):
    from slimt_amd import capi, synth
    m, gm, _ = engines("tiny11")
    shapes = [(3, 8), (17, 16), (32, 32)]  # (B_j, S_j)
    S, T = 32, 0.7
    sl = synth.make_shortlist(m.V, 4096)
    batches = [synth.make_batch(m.V, B, Sj, seed=400 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    keys = [keys_of(50 + j, B) for j, (B, _) in enumerate(shapes)]
    rows = hip.translate_many_rows([b for b, _ in shapes])
    own = hip.Context(gm, rows, S)
    owns = [own.translate(ids, lens, sl, scores=True, sampling=(T, k)) for (ids, lens), k in zip(batches, keys)]
    ctx = hip.Context(gm, rows, S)
    pins, bufs, scs = [], [], []
    for ids, lens in batches:  # pinned host arrays, one host shortlist, pageable keys
        B, Sj = ids.shape
        Tj = tmax_of(Sj)
        arrs = []
        for dt, shape in ((np.uint32, (B, Sj)), (np.uint32, (B,)), (np.uint32, (B, Tj)), (np.uint32, (B,)), (np.float32, (B, Tj))):
            pp = capi._Pinned()
            pins.append(pp)
            arrs.append(pp.array(dt, shape))
        arrs[0][...] = ids
        arrs[1][...] = lens
        bufs.append(tuple(arrs[:4]) + (None,))
        scs.append(arrs[4])
    ctx.translate_many_async(bufs, sl, scores=scs, sampling=(T, keys))
    ctx.synchronize()
    for b, sc, o in zip(bufs, scs, owns):
        assert np.array_equal(b[3], o[1]) and np.array_equal(b[2], o[0])
        for r in range(len(o[1])):
            assert np.array_equal(sc[r, :o[1][r]].view(np.uint32), o[3][r, :o[1][r]].view(np.uint32)), r
    keep, args, outs = [], [], []
    for (ids, lens), k in zip(batches, keys):  # device arrays, device keys, no scores asked for
        B, Sj = ids.shape
        d = [_dev(ids), _dev(lens), _dev(k), _dev(sl)]
        d_out = torch.zeros((B, tmax_of(Sj)), dtype=torch.int32, device="cuda")
        d_ol = torch.zeros((B,), dtype=torch.int32, device="cuda")
        keep.append(d)
        outs.append((d_out, d_ol))
        args.append((d[0].data_ptr(), d[1].data_ptr(), B, d[3].data_ptr(), sl.size, d_out.data_ptr(), d_ol.data_ptr(), 0, Sj))
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=tmax_of(S), sampling=(T, [d[2].data_ptr() for d in keep]))
    ctx.synchronize()
    for o, (d_out, d_ol) in zip(owns, outs):
        assert np.array_equal(d_ol.cpu().numpy().view(np.uint32), o[1])
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), o[0])
    with pytest.raises(Exception):  # a mismatched count fails the call, as it does for prefixes
        ctx.translate_many_device(args, S, 1.5, 0, steps_hint=tmax_of(S), sampling=(T, [keep[0][2].data_ptr()]))
    ctx.close()
    own.close()
    for pp in pins:
        pp.free()


@pytest.mark.parametrize("mode", [0, 1])
def test_prefixes_are_forced_and_scored_at_the_temperature_then_sampled(hip, oracle, engines, mode):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S, T = 17, 16, 0.7
    ids, lens = synth.make_batch(m.V, B, S, seed=71, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    Tm = tmax_of(S)
    rng = np.random.default_rng(6)
    p_ids = rng.choice(sl[sl != 0], size=(B, Tm)).astype(np.uint32)
    p_len = np.array([(0, 1, 3, Tm)[b % 4] for b in range(B)], np.uint32)
    missing = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)
    p_ids[2, 1] = missing[0]  # absent from the output layer: still fed, scored -inf
    keys = keys_of(12, B)
    want = sampled_translate(oracle, om, m, ids, lens, sl, keys, T, p_ids, p_len)
    ctx = hip.Context(gm, B, S)
    ctx.set_decode_mode(mode)
    got = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=(p_ids, p_len), sampling=(T, keys))
    _check(got, want, T)
    for b in range(B):
        n = min(int(p_len[b]), int(got[1][b]))
        assert np.array_equal(got[0][b, :n], p_ids[b, :n]), b
    assert np.isneginf(got[3][2, 1])
    ctx.close()


def test_keys_matter_the_setting_is_consumed_and_poisoned_rows_stay_class_zero(hip, oracle, engines, synth_models):
    import copy
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S, T = 17, 32, 1.0
    ids, lens = synth.make_batch(m.V, B, S, seed=81, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    ctx = hip.Context(gm, B, S)
    a = ctx.translate(ids, lens, sl, sampling=(T, keys_of(1, B)))
    b = ctx.translate(ids, lens, sl, sampling=(T, keys_of(2, B)))
    differ = sum(1 for r in range(B) if a[1][r] != b[1][r] or not np.array_equal(a[0][r], b[0][r]))
    assert differ >= (B + 1) // 2, differ
    # the call after a sampled one is greedy again
    oracle.set_mode(oracle.PORTABLE)
    try:
        w_out, w_ln, _, _ = om.translate(ids, lens, sl, 1.5, 0)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    g = ctx.translate(ids, lens, sl)
    assert np.array_equal(g[1], w_ln) and np.array_equal(g[0], w_out)
    with pytest.raises(Exception):  # a bad temperature is refused, and arms nothing
        ctx.set_sampling(0.0, [None])
    g = ctx.translate(ids, lens, sl)
    assert np.array_equal(g[1], w_ln) and np.array_equal(g[0], w_out)
    ctx.close()
    # a NaN-poisoned output row: class 0, score NaN (the poisoning of tests/test_gpu_scores.py)
    for poison in ("nan", "nan-in-column-0"):
        pm = copy.deepcopy(synth_models("tiny11", 6.0))
        bias = pm.params["decoder_ff_logit_out_b"]
        if poison == "nan":
            bias.data[...] = np.float32(np.nan)
        else:
            bias.data.reshape(-1)[0] = np.float32(np.nan)
        eos = 0 if poison == "nan" else 7
        pg, po = hip.Model(pm), oracle.OracleModel(pm)
        Bp, Sp = 19, 11
        pids, plens = synth.make_batch(pm.V, Bp, Sp, seed=4, ragged=True)
        psl = synth.make_shortlist(pm.V, 1024)
        want = sampled_translate(oracle, po, pm, pids, plens, psl, None, T, eos=eos)
        pc = hip.Context(pg, Bp, Sp)
        for mode in (0, 1):
            pc.set_decode_mode(mode)
            out, ln, _, sc = pc.translate(pids, plens, psl, eos_id=eos, scores=True, sampling=(T, None))
            assert np.array_equal(ln, want[1]) and np.array_equal(out, want[0]), (poison, mode)
            for r in range(Bp):
                assert np.all(out[r, :ln[r]] == psl[0]) and np.isnan(sc[r, :ln[r]]).all(), (poison, mode, r)
        pc.close()
        pg.close()
