"""GPU parity of forced target prefixes (include/slimt_hip.h, slimt_hip_ctx_set_target_prefix) against the checker of
tests/test_forced_prefix_checker.py: scoring given translations (prefix = target + EOS), prefixes completed greedily,
the invariants that tie forced calls to unforced and scored ones, edge cases, every translate entry point, merged
launches and the arming rules. Tokens, lengths and alignment rows are bit-equal to the checker's; scores are within
5e-5 of its float64 log_softmax."""
import numpy as np
import pytest
import torch

from test_forced_prefix_checker import forced_translate, tmax_of

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


def _targets(rng, B, T, sl, V, lens_p, eos=0):
    """random targets from the output layer (not EOS), EOS at position P_b - 1: scoring a given translation"""
    pool = sl[sl != eos] if sl is not None else np.arange(1, V, dtype=np.uint32)
    p_ids = rng.choice(pool, size=(B, T)).astype(np.uint32)
    for b in range(B):
        if lens_p[b]:
            p_ids[b, lens_p[b] - 1] = eos
    return p_ids, np.asarray(lens_p, np.uint32)


def _no_eos(rng, B, T, sl, V, lens_p, eos=0):
    pool = sl[sl != eos] if sl is not None else np.arange(1, V, dtype=np.uint32)
    return rng.choice(pool, size=(B, T)).astype(np.uint32), np.asarray(lens_p, np.uint32)


def _check(got, want, scores=True):
    out, ln, al = got[:3]
    w_out, w_ln, w_al, w_sc = want
    assert np.array_equal(ln, w_ln), (ln, w_ln)
    assert np.array_equal(out, w_out)
    if al is not None:
        assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32))
    if scores:
        sc = got[3]
        for b in range(len(ln)):
            n = int(ln[b])
            g, w = sc[b, :n].astype(np.float64), w_sc[b, :n]
            assert np.array_equal(np.isneginf(g), np.isneginf(w)), (b, g, w)
            fin = np.isfinite(w)
            assert np.all(np.isfinite(g[fin])), (b, g)
            err = np.abs(g[fin] - w[fin])
            assert err.max(initial=0) <= TOL, (b, err.max())


def _spread(B, hi, lo=0):
    return [lo + (b * (hi - lo)) // max(1, B - 1) for b in range(B)]


CASES = [  # preset, S, B, shortlist, decode modes
    ("tiny11", 32, 17, 4096, (0, 1, 2, 3, 6)),
    ("tiny11", 8, 17, None, (0, 1)),
    ("tiny11", 64, 9, 4096, (0, 1)),
    ("tiny11", 100, 3, 4096, (0,)),
    ("tiny11", 8, 33, 4096, (0,)),
    ("base", 32, 9, 4096, (0, 1)),
]


@pytest.mark.parametrize("preset,S,B,n_sl,modes", CASES)
def test_scoring_and_completing_prefixes_match_the_checker(hip, oracle, engines, preset, S, B, n_sl, modes):
    from slimt_amd import synth
    m, gm, om = engines(preset)
    rng = np.random.default_rng(S + B)
    ids, lens = synth.make_batch(m.V, B, S, seed=41 + S + B, ragged=True)
    lens[0], lens[-1] = 0, S  # sentence lengths 0 and S
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    T = tmax_of(S)
    score_p = _targets(rng, B, T, sl, m.V, _spread(B, T, 1))
    greedy_p = _no_eos(rng, B, T, sl, m.V, _spread(B, T, 0))
    wants = [forced_translate(oracle, om, m, ids, lens, sl, *p) for p in (score_p, greedy_p)]
    ctx = hip.Context(gm, B, S)
    for mode in modes:
        ctx.set_decode_mode(mode)
        for p, want in zip((score_p, greedy_p), wants):
            got = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p)
            _check(got, want)
        # scoring: out_ids echoes the targets, out_len = P_b
        got = ctx.translate(ids, lens, sl, prefix=score_p)
        assert np.array_equal(got[1], score_p[1]), mode
        for b in range(B):
            assert np.array_equal(got[0][b, :score_p[1][b]], score_p[0][b, :score_p[1][b]]), (mode, b)
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_invariants_against_unforced_calls(hip, oracle, engines, mode):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S = 24, 24
    ids, lens = synth.make_batch(m.V, B, S, seed=7, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    T = tmax_of(S)
    ctx = hip.Context(gm, B, S)
    ctx.set_decode_mode(mode)
    u = ctx.translate(ids, lens, sl, want_align=True)
    s = ctx.translate(ids, lens, sl, want_align=True, scores=True)
    zero = (np.zeros((B, T), np.uint32), np.zeros(B, np.uint32))
    f0 = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=zero)
    own = (u[0].copy(), np.minimum(u[1], T).astype(np.uint32))
    fo = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=own)
    for f in (f0, fo):
        assert np.array_equal(f[0], u[0]) and np.array_equal(f[1], u[1]) and np.array_equal(f[2], u[2])
        for b in range(B):  # bit for bit, -0 included
            assert np.array_equal(f[3][b, :u[1][b]].view(np.uint32), s[3][b, :u[1][b]].view(np.uint32)), b
    # half the sentences forced: the other half are the unforced call's
    rng = np.random.default_rng(3)
    half = _no_eos(rng, B, T, sl, m.V, [(T // 2 if b % 2 else 0) for b in range(B)])
    h = ctx.translate(ids, lens, sl, want_align=True, prefix=half)
    for b in range(0, B, 2):
        assert np.array_equal(h[0][b], u[0][b]) and h[1][b] == u[1][b] and np.array_equal(h[2][b], u[2][b]), b
    _check(h, forced_translate(oracle, om, m, ids, lens, sl, *half), scores=False)
    # the prefix does not stick: the next call is unforced
    n = ctx.translate(ids, lens, sl, want_align=True)
    assert np.array_equal(n[0], u[0]) and np.array_equal(n[1], u[1])
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_edge_cases_eos_inside_missing_tokens_full_prefix(hip, oracle, engines, mode):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S = 6, 16
    ids, lens = synth.make_batch(m.V, B, S, seed=13, ragged=True)
    lens[1], lens[2] = 0, S
    sl = synth.make_shortlist(m.V, 4096)
    missing = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)
    T = tmax_of(S)
    rng = np.random.default_rng(5)
    p_ids, _ = _no_eos(rng, B, T, sl, m.V, [0] * B)
    p_len = np.array([5, 3, T, T, 4, 2], np.uint32)
    p_ids[0, 2] = 0           # EOS in the middle of the prefix ends sentence 0 at 3 tokens
    p_ids[1, 1] = missing[0]  # absent from the shortlist: -inf, still fed
    p_ids[3, :] = missing[1:1 + T]  # every forced token absent, P = Tmax
    p_ids[4, 0] = missing[-1]
    want = forced_translate(oracle, om, m, ids, lens, sl, p_ids, p_len)
    ctx = hip.Context(gm, B, S)
    ctx.set_decode_mode(mode)
    got = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=(p_ids, p_len))
    _check(got, want)
    assert got[1][0] == 3 and got[1][2] == T and got[1][3] == T
    assert np.isneginf(got[3][1, 1]) and np.isneginf(got[3][3, :T]).all() and np.isneginf(got[3][4, 0])
    ctx.close()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_kv_cache_formats(hip, oracle, synth_models, fmt):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm, om = hip.Model(m), oracle.OracleModel(m)
    gm.set_kv_cache_format(fmt)
    B, S = 20, 32
    ids, lens = synth.make_batch(m.V, B, S, seed=17 + fmt, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    T = tmax_of(S)
    p = _no_eos(np.random.default_rng(fmt), B, T, sl, m.V, _spread(B, T))
    ctx = hip.Context(gm, B, S)
    got = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p)
    want = forced_translate(oracle, om, m, ids, lens, sl, *p)
    if fmt != 3:
        _check(got, want)
    else:  # (the reference's literal order, not the checker's: include/slimt_hip.h) -- the prefix is recorded and scored
        for b in range(B):
            n = int(p[1][b])
            assert got[1][b] >= n and np.array_equal(got[0][b, :n], p[0][b, :n]), b
            assert np.all(got[3][b, :got[1][b]] <= 0.0), b
        # every step forced (target + EOS): the tokens are fixed, so lengths and tokens are the checker's and the scores
        # meet its float64 ones up to format 3's own float order (the same forced kernels as format 0 in decode mode 1,
        # which match within 5e-5 above): most steps within 1e-5, a rare one by a few hundredths where that order's drift
        # accumulates (tests/test_gpu_cross_attention_orders.py: it flips near-tie tokens); a wrong score is off by nats
        tp = _targets(np.random.default_rng(40), B, T, sl, m.V, _spread(B, T, 1))
        tg = ctx.translate(ids, lens, sl, scores=True, prefix=tp)
        tw = forced_translate(oracle, om, m, ids, lens, sl, *tp)
        assert np.array_equal(tg[1], tp[1]) and np.array_equal(tg[1], tw[1]) and np.array_equal(tg[0], tw[0])
        errs = np.concatenate([np.abs(tg[3][b, :tp[1][b]].astype(np.float64) - tw[3][b, :tp[1][b]]) for b in range(B)])
        assert np.all(np.isfinite(errs)) and np.median(errs) <= 1e-5 and errs.max() <= 0.1, (np.median(errs), errs.max())
        assert np.mean(errs > 1e-4) <= 0.02, np.mean(errs > 1e-4)
    # the call's own greedy output as the prefix: bit-identical to the unforced scored call in this format too
    s = ctx.translate(ids, lens, sl, want_align=True, scores=True)
    f = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=(s[0].copy(), np.minimum(s[1], T).astype(np.uint32)))
    assert np.array_equal(f[0], s[0]) and np.array_equal(f[1], s[1]) and np.array_equal(f[2], s[2])
    for b in range(B):
        assert np.array_equal(f[3][b, :s[1][b]].view(np.uint32), s[3][b, :s[1][b]].view(np.uint32)), b
    ctx.close()
    gm.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_entry_points_pinned_device_generated(hip, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S = 17, 16
    ids, lens = synth.make_batch(m.V, B, S, seed=23, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    T = tmax_of(S)
    p = _targets(np.random.default_rng(1), B, T, sl, m.V, _spread(B, T, 1))
    want = forced_translate(oracle, om, m, ids, lens, sl, *p)
    ctx = hip.Context(gm, B, S)
    _check(ctx.translate_pinned(ids, lens, sl, want_align=True, scores=True, prefix=p), want)
    # device arrays
    d_ids, d_len, d_pi, d_pl = _dev(ids), _dev(lens), _dev(p[0]), _dev(p[1])
    d_sl = _dev(sl)
    d_out = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    d_ol = torch.zeros((B,), dtype=torch.int32, device="cuda")
    d_sc = torch.zeros((B, T), dtype=torch.float32, device="cuda")
    ctx.translate_device(d_ids.data_ptr(), d_len.data_ptr(), B, S, d_sl.data_ptr(), sl.size, 1.5, 0, d_out.data_ptr(),
                         d_ol.data_ptr(), scores=d_sc.data_ptr(), prefix=(d_pi.data_ptr(), d_pl.data_ptr()))
    ctx.synchronize()
    _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), want)
    # a generated lexical shortlist: host, pinned and device forms against the checker over the oracle's list
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    gsl = osl.generate(ids, lens)
    gp = _no_eos(np.random.default_rng(2), B, T, sl, m.V, _spread(B, T))  # (tokens of the fixed list: some are missing)
    gwant = forced_translate(oracle, om, m, ids, lens, gsl, *gp)
    _check(ctx.translate_generated(gen, ids, lens, scores=True, prefix=gp), gwant)
    _check(ctx.translate_pinned(ids, lens, generator=gen, scores=True, prefix=gp), gwant)
    d_gi, d_gl = _dev(gp[0]), _dev(gp[1])
    ctx.translate_device_generated(gen, d_ids.data_ptr(), d_len.data_ptr(), B, S, 1.5, 0, d_out.data_ptr(), d_ol.data_ptr(),
                                   scores=d_sc.data_ptr(), prefix=(d_gi.data_ptr(), d_gl.data_ptr()))
    ctx.synchronize()
    _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), gwant)
    ctx.close()
    gen.close()


def test_merged_launches_equal_each_batch_own_forced_call(hip, oracle, engines):
    from slimt_amd import capi, synth
    m, gm, om = engines("tiny11")
    shapes = [(40, 16), (7, 12), (33, 16)]  # holes, padded lengths S_j < S
    S = 16
    sl = synth.make_shortlist(m.V, 4096)
    batches = [synth.make_batch(m.V, B, Sj, seed=200 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    rng = np.random.default_rng(9)
    prefixes = [(_targets if j % 2 else _no_eos)(rng, B, tmax_of(Sj), sl, m.V, _spread(B, tmax_of(Sj)))
                for j, (B, Sj) in enumerate(shapes)]
    for j, (B, _) in enumerate(shapes):  # (scoring targets end in EOS: P_b >= 1)
        if j % 2:
            prefixes[j][1][prefixes[j][1] == 0] = 1
            prefixes[j][0][prefixes[j][1] == 1, 0] = 0
    rows = hip.translate_many_rows([b for b, _ in shapes])
    own = hip.Context(gm, rows, S)
    owns = [own.translate(ids, lens, sl, scores=True, prefix=p) for (ids, lens), p in zip(batches, prefixes)]
    for (ids, lens), p, o in zip(batches, prefixes, owns):
        _check(o, forced_translate(oracle, om, m, ids, lens, sl, *p))
    # pinned host arrays, one host shortlist
    ctx = hip.Context(gm, rows, S)
    pins, bufs, scs = [], [], []
    for ids, lens in batches:
        B, Sj = ids.shape
        T = tmax_of(Sj)
        arrs = []
        for dt, shape in ((np.uint32, (B, Sj)), (np.uint32, (B,)), (np.uint32, (B, T)), (np.uint32, (B,)), (np.float32, (B, T))):
            pp = capi._Pinned()
            pins.append(pp)
            arrs.append(pp.array(dt, shape))
        arrs[0][...] = ids
        arrs[1][...] = lens
        bufs.append(tuple(arrs[:4]) + (None,))
        scs.append(arrs[4])
    ctx.translate_many_async(bufs, sl, scores=scs, prefix=prefixes)
    ctx.synchronize()
    for b, sc, o in zip(bufs, scs, owns):
        assert np.array_equal(b[3], o[1]) and np.array_equal(b[2], o[0])
        for r in range(len(o[1])):
            assert np.array_equal(sc[r, :o[1][r]].view(np.uint32), o[3][r, :o[1][r]].view(np.uint32)), r
    # device arrays, per-batch shortlists, no scores asked for
    sls = [sl, synth.make_shortlist(m.V, 2048, seed=4), sl]
    keep, args, outs = [], [], []
    for (ids, lens), p, s_j in zip(batches, prefixes, sls):
        B, Sj = ids.shape
        T = tmax_of(Sj)
        d = [_dev(ids), _dev(lens), _dev(p[0]), _dev(p[1])] + ([_dev(s_j)] if s_j is not None else [])
        d_out = torch.zeros((B, T), dtype=torch.int32, device="cuda")
        d_ol = torch.zeros((B,), dtype=torch.int32, device="cuda")
        keep.append(d)
        outs.append((d_out, d_ol))
        args.append((d[0].data_ptr(), d[1].data_ptr(), B, d[4].data_ptr() if s_j is not None else 0,
                     0 if s_j is None else s_j.size, d_out.data_ptr(), d_ol.data_ptr(), 0, Sj))
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=tmax_of(S), prefix=[(k[2].data_ptr(), k[3].data_ptr()) for k in keep])
    ctx.synchronize()
    for (ids, lens), p, s_j, (d_out, d_ol) in zip(batches, prefixes, sls, outs):
        o = own.translate(ids, lens, s_j, prefix=p)
        assert np.array_equal(d_ol.cpu().numpy().view(np.uint32), o[1])
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), o[0])
    ctx.close()
    own.close()
    for pp in pins:
        pp.free()


def test_merged_device_generated(hip, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    shapes = [(64, 16), (10, 13)]
    S = 16
    batches = [synth.make_batch(m.V, B, Sj, seed=300 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    rng = np.random.default_rng(11)
    rows = hip.translate_many_rows([b for b, _ in shapes])
    ctx = hip.Context(gm, rows, S)
    keep, args, outs, d_scs, prefixes = [], [], [], [], []
    for ids, lens in batches:
        B, Sj = ids.shape
        T = tmax_of(Sj)
        gsl = osl.generate(ids, lens)
        p = _no_eos(rng, B, T, gsl, m.V, _spread(B, T))
        prefixes.append(p)
        d = [_dev(ids), _dev(lens), _dev(p[0]), _dev(p[1])]
        d_out = torch.zeros((B, T), dtype=torch.int32, device="cuda")
        d_ol = torch.zeros((B,), dtype=torch.int32, device="cuda")
        d_sc = torch.zeros((B, T), dtype=torch.float32, device="cuda")
        keep.append(d)
        outs.append((d_out, d_ol))
        d_scs.append(d_sc)
        args.append((d[0].data_ptr(), d[1].data_ptr(), B, 0, 0, d_out.data_ptr(), d_ol.data_ptr(), 0, Sj))
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=tmax_of(S), generator=gen, scores=[d.data_ptr() for d in d_scs],
                              prefix=[(k[2].data_ptr(), k[3].data_ptr()) for k in keep])
    ctx.synchronize()
    for (ids, lens), p, (d_out, d_ol), d_sc in zip(batches, prefixes, outs, d_scs):
        want = forced_translate(oracle, om, m, ids, lens, osl.generate(ids, lens), *p)
        _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), want)
    ctx.close()
    gen.close()


def test_arming_rules(hip, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S = 4, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=2, ragged=True)
    T = tmax_of(S)
    ctx = hip.Context(gm, B, S)
    u = ctx.translate(ids, lens)
    ok = (np.ones((B, T), np.uint32), np.ones(B, np.uint32))
    bad = [
        [ok, ok],                                                  # two batches for a single-batch call
        [(ok[0], 0)],                                              # a NULL entry
        [(ok[0], np.full(B, T + 1, np.uint32))],                   # P_b > Tmax
        [(np.full((B, T), m.V, np.uint32), ok[1])],                # an id >= V
    ]
    for armed in bad:
        ctx.set_target_prefix(armed)
        with pytest.raises(hip.SlimtHipError) as e:
            ctx.translate(ids, lens)
        assert "prefix" in str(e.value)
        n = ctx.translate(ids, lens)  # consumed: the next call is unforced
        assert np.array_equal(n[0], u[0]) and np.array_equal(n[1], u[1])
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_generated_shortlists_async_merged_and_step_wise(hip, oracle, engines, mode):
    """slimt_hip_translate_many_async_generated with prefixes (pinned: read in place), and decode mode 1 (the step-wise
    path) over a generated list, against the checker over the oracle's list of each batch"""
    from slimt_amd import capi, synth
    m, gm, om = engines("tiny11")
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    shapes = [(40, 16), (9, 11)]
    S = 16
    batches = [synth.make_batch(m.V, B, Sj, seed=500 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    rng = np.random.default_rng(12)
    rows = hip.translate_many_rows([b for b, _ in shapes])
    ctx = hip.Context(gm, rows, S)
    ctx.set_decode_mode(mode)
    pins, bufs, scs, prefixes, wants = [], [], [], [], []
    for j, (ids, lens) in enumerate(batches):
        B, Sj = ids.shape
        T = tmax_of(Sj)
        gsl = osl.generate(ids, lens)
        p = (_targets if j else _no_eos)(rng, B, T, gsl, m.V, _spread(B, T, 1))
        arrs = []
        for dt, shape in ((np.uint32, (B, Sj)), (np.uint32, (B,)), (np.uint32, (B, T)), (np.uint32, (B,)), (np.float32, (B, T)),
                          (np.uint32, (B, T)), (np.uint32, (B,))):
            pp = capi._Pinned()
            pins.append(pp)
            arrs.append(pp.array(dt, shape))
        arrs[0][...], arrs[1][...], arrs[5][...], arrs[6][...] = ids, lens, p[0], p[1]
        bufs.append(tuple(arrs[:4]) + (None,))
        scs.append(arrs[4])
        prefixes.append((arrs[5], arrs[6]))
        wants.append(forced_translate(oracle, om, m, ids, lens, gsl, *p))
        # the blocking form of the same batch, on its own
        _check(ctx.translate_generated(gen, ids, lens, scores=True, prefix=p), wants[-1])
    ctx.translate_many_async(bufs, generator=gen, scores=scs, prefix=prefixes)
    ctx.synchronize()
    for b, sc, want in zip(bufs, scs, wants):
        _check((b[2], b[3], None, sc), want)
    ctx.close()
    for pp in pins:
        pp.free()
    gen.close()


def _direct_forced(hip, gm, sentences, prefixes, generator):
    """the forced scored call on ONE padded batch of `sentences` (as the service forms it): per sentence (target, scores)"""
    B, S = len(sentences), max(len(s) for s in sentences)
    T = tmax_of(S)
    ids = np.zeros((B, S), np.uint32)
    lens = np.zeros(B, np.uint32)
    p_ids = np.zeros((B, T), np.uint32)
    p_len = np.zeros(B, np.uint32)
    for i, (s, p) in enumerate(zip(sentences, prefixes)):
        ids[i, :len(s)] = s
        lens[i] = len(s)
        p_ids[i, :len(p)] = p
        p_len[i] = len(p)
    ctx = hip.Context(gm, B, S)
    out, ln, _, sc = ctx.translate_generated(generator, ids, lens, scores=True, prefix=(p_ids, p_len))
    ctx.close()
    return [(out[i, :ln[i]], sc[i, :ln[i]]) for i in range(B)]


@pytest.mark.parametrize("merge", [0, 1])
def test_batch_service_prefixes_equal_the_direct_forced_call(hip, synth_models, merge):
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    gm = hip.Model(m)
    rnd = np.random.Generator(np.random.PCG64(8))
    S = 12  # one length: the service's batches are known (ServiceResult.batch)
    T = tmax_of(S)
    sents = [list(rnd.integers(3, m.V, S - 1)) + [0] for _ in range(60)]
    # a third not forced, a third forced targets + EOS (scored translations), a third prefixes then greedy
    prefixes = [[] if i % 3 == 0 else list(rnd.integers(3, m.V, 1 + i % T)) + ([0] if i % 3 == 1 else [])
                for i in range(len(sents))]
    prefixes = [p[:T] for p in prefixes]
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, min_count=1)
    svc = hip.BatchService([gm], max_words=(20 + 1) * S, workers_per_device=1, lexical_shortlist=blob, source_vocab=m.V,
                           target_vocab=m.V, merge_batches=merge, scores=True)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    try:
        r = svc.translate(sents, prefixes=prefixes)
        groups = {}
        for i in range(len(sents)):
            groups.setdefault(int(r.batch[i]), []).append(i)
        assert len(groups) >= 3
        for members in groups.values():
            want = _direct_forced(hip, gm, [sents[i] for i in members], [prefixes[i] for i in members], gen)
            for i, (tgt, sc) in zip(members, want):
                assert np.array_equal(r.target(i), tgt), i
                assert np.array_equal(r.token_scores(i).view(np.uint32), sc.view(np.uint32)), i
                n = len(prefixes[i])
                assert np.array_equal(tgt[:n], prefixes[i]), i
                if i % 3 == 1:
                    assert len(tgt) == n, i
        r.close()
        # sentences without prefixes in a prefixed request are the plain request's
        r0 = svc.translate(sents)
        r1 = svc.translate(sents, prefixes=[[] for _ in sents])
        assert np.array_equal(r0.targets, r1.targets) and np.array_equal(r0.scores.view(np.uint32), r1.scores.view(np.uint32))
        r0.close()
        r1.close()
        # an over-long prefix: max(1, (size_t)(limit_factor * source length)) tokens at most
        with pytest.raises(hip.SlimtHipError) as e:
            svc.translate([sents[0]], prefixes=[[5] * (tmax_of(len(sents[0])) + 1)])
        assert "prefix" in str(e.value)
        with pytest.raises(ValueError):
            svc.translate([sents[0], sents[1]], prefixes=[[5]])
    finally:
        gen.close()
        svc.close()
        gm.close()
