"""GPU parity of truncated sampling (include/slimt_hip.h, slimt_hip_ctx_set_sampling_truncation) against the checker of
tests/test_truncation_checker.py, which finds the kept set by sorting where the kernel descends a radix tree. The weights
are integers with the same bits on both sides, so the kept set -- and with it columns, tokens, lengths and alignment
rows -- is bit-equal to the checker's, with no allowance for near-ties; thresholds are equal as values; scores are within
5e-5 * max(1, 1 / T) of the float64 log-softmax over the kept set, the project's tolerance for sampled scores."""
import numpy as np
import pytest
import torch

from test_forced_prefix_checker import tmax_of
from test_sampling_checker import keys_of, row_keys
from test_truncation_checker import KeptSets, truncated_row, truncated_translate

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


@pytest.fixture
def contexts(hip):
    """hip.Context(...) that is closed when the test ends, passed or failed: before the module's models are"""
    opened = []

    def make(gm, B, S):
        opened.append(hip.Context(gm, B, S))
        return opened[-1]

    yield make
    for c in opened:
        c.close()


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


# ---- 1: the kernel alone --------------------------------------------------------------------------------------------------
KINDS = ("normal", "equal", "two-values", "ascending", "descending", "one-ulp", "signed-zeros", "some-neg-inf", "some-nan",
         "one-pos-inf", "all-neg-inf", "all-nan")


def _row(kind, N, rng):
    x = rng.normal(0.0, 3.0, N).astype(np.float32)
    if kind == "equal":
        x[:] = np.float32(1.25)
    elif kind == "two-values":
        x = rng.choice(np.array([0.5, 2.0], np.float32), N)
    elif kind == "ascending":
        x = np.sort(x)
    elif kind == "descending":
        x = np.sort(x)[::-1].copy()
    elif kind == "one-ulp":
        x = (np.uint32(0x3F800000) + rng.permutation(N).astype(np.uint32) % np.uint32(1024)).view(np.float32)
    elif kind == "signed-zeros":
        x = rng.choice(np.array([-1.5, -0.0, 0.0, 0.75, -3.0], np.float32), N)
    elif kind == "some-neg-inf":
        x[rng.random(N) < 0.3] = -np.inf
    elif kind == "some-nan":
        x[rng.random(N) < 0.1] = np.nan
        x[rng.integers(N)] = np.nan
    elif kind == "one-pos-inf":
        x[rng.integers(N)] = np.inf
    elif kind == "all-neg-inf":
        x[:] = -np.inf
    elif kind == "all-nan":
        x[:] = np.nan
    return np.ascontiguousarray(x, dtype=np.float32)


@pytest.mark.parametrize("N", [1, 7, 64, 255, 256, 257, 4096, 4100, 70001])
def test_the_selection_kernel_matches_the_sorting_checker(hip, N):
    from slimt_amd import capi
    rng = np.random.default_rng(1000 + N)
    # five rows per call: the twelve kinds in three groups, the last filled up with further normal rows
    groups = [KINDS[0:5], KINDS[5:10], KINDS[10:12] + ("normal",) * 3]
    ids_alt = ((np.arange(N, dtype=np.uint64) * 3 + 1) % (1 << 32)).astype(np.uint32)
    worst, calls = 0.0, 0
    for gi, kinds in enumerate(groups):
        logits = np.stack([_row(k, N, rng) for k in kinds])
        keys = keys_of(N + gi, 5)
        steps = np.array([0, 1, 2, 7, 40], np.uint32)
        for T in (0.7, 1.0):
            ids = ids_alt if T == 1.0 else None
            inv_T = np.float32(1.0) / np.float32(T)
            tol = TOL * max(1.0, 1.0 / T)
            z32 = (logits * inv_T).astype(np.float32)
            sets = [KeptSets(z32[r]) for r in range(5)]  # (one sort per row and temperature: the reference is computed once)
            rkeys = [row_keys(keys[r], steps[r], logits[r], ids, inv_T) for r in range(5)]
            for top_k in sorted({0, 1, 2, max(N - 1, 0), N, N + 5}):
                for top_p in (1e-6, 0.5, 0.9, 1.0):
                    cols, thr, kept, sc = capi.sample_truncated(logits, T, top_k, top_p, ids=ids, keys=keys, steps=steps)
                    calls += 1
                    for r in range(5):
                        w_col, w_none, w_kept, w_tau, w_sc = truncated_row(keys[r], steps[r], logits[r], ids, inv_T, top_k, top_p,
                                                                            sets=sets[r], rkeys=rkeys[r])
                        where = (kinds[r], T, top_k, top_p)
                        assert kept[r] == w_kept.sum(), where
                        assert thr[r] == w_tau, where  # (as values: +-0 are one threshold)
                        assert cols[r] == w_col, where
                        assert np.isnan(sc[r]) == np.isnan(w_sc), where + (sc[r], w_sc)
                        if not np.isnan(w_sc):
                            assert np.isfinite(w_sc) and abs(float(sc[r]) - w_sc) <= tol, where + (sc[r], w_sc)
                            worst = max(worst, abs(float(sc[r]) - w_sc))
    print("N = %d: %d calls, scores: max |gpu - float64| = %.3g" % (N, calls, worst))


# ---- 2: through translate -------------------------------------------------------------------------------------------------
CASES = [  # preset, eos bias, S, B, shortlist, T
    ("tiny11", 7.0, 8, 17, None, 0.7),
    ("tiny11", 6.0, 32, 17, 4096, 1.0),
    ("base", 7.0, 8, 1, None, 0.7),
]


@pytest.mark.parametrize("top_k,top_p", [(8, 1.0), (0, 0.9), (40, 0.8)])
@pytest.mark.parametrize("preset,eos_bias,S,B,n_sl,T", CASES)
def test_truncated_translations_match_the_checker_in_every_decode_mode(hip, contexts, oracle, engines, preset, eos_bias, S, B, n_sl, T,
                                                                       top_k, top_p):
    from slimt_amd import synth
    m, gm, om = engines(preset, eos_bias)
    ids, lens = synth.make_batch(m.V, B, S, seed=61 + S + B, ragged=True)
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    keys = keys_of(S + B, B)
    sizes = []
    want = truncated_translate(oracle, om, m, ids, lens, sl, keys, T, top_k, top_p, sizes=sizes)
    n_cols = m.V if sl is None else sl.size
    assert any(n < n_cols for _, _, n in sizes)  # (something is cut)
    ctx = contexts(gm, B, S)
    for mode in (0, 1, 3):
        ctx.set_decode_mode(mode)
        plan = ctx.plan(S)
        _check(ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), truncation=(top_k, top_p)), want, T)
        assert ctx.plan(S) == plan  # (slimt_hip_ctx_plan is unchanged: it reports the context's mode before and after)
    ctx.close()


# ---- 3: both off ----------------------------------------------------------------------------------------------------------
def test_both_settings_off_is_the_untruncated_sampled_call_bit_for_bit(hip, contexts, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T = 17, 32, 0.7
    ids, lens = synth.make_batch(m.V, B, S, seed=23, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(4, B)
    ctx = contexts(gm, B, S)
    for mode in (0, 1):
        ctx.set_decode_mode(mode)
        a = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys))
        b = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), truncation=(0, 1.0))
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), mode
    ctx.close()


# ---- 4: top_k = 1 ---------------------------------------------------------------------------------------------------------
def test_top_1_is_the_greedy_token_with_score_zero_wherever_one_column_is_kept(hip, contexts, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S, T = 17, 16, 0.7
    ids, lens = synth.make_batch(m.V, B, S, seed=29, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(6, B)
    sizes = []
    want = truncated_translate(oracle, om, m, ids, lens, sl, keys, T, 1, 1.0, sizes=sizes)
    ctx = contexts(gm, B, S)
    got = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), truncation=(1, 1.0))
    _check(got, want, T)
    single = [(b, t) for b, t, n in sizes if n == 1]
    assert len(single) >= len(sizes) // 2
    for b, t in single:
        assert got[3][b, t] == 0.0, (b, t)  # (+-0)
    if len(single) == len(sizes):  # no tied maxima anywhere: the whole call is the greedy one
        g = ctx.translate(ids, lens, sl)
        assert np.array_equal(g[0], got[0]) and np.array_equal(g[1], got[1])
    ctx.close()


# ---- 5: independence of position and entry point --------------------------------------------------------------------------
def test_a_sentence_draws_the_same_alone_first_and_last(hip, contexts, engines):
    from slimt_amd import synth
    m, gm, _ = engines("tiny11")
    B, S, T, trunc = 17, 32, 1.0, (40, 0.9)
    ids, lens = synth.make_batch(m.V, B, S, seed=31, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(8, B)
    ctx = contexts(gm, B, S)
    full = ctx.translate(ids, lens, sl, scores=True, sampling=(T, keys), truncation=trunc)
    rev = ctx.translate(ids[::-1].copy(), lens[::-1].copy(), sl, scores=True, sampling=(T, keys[::-1].copy()), truncation=trunc)
    assert np.array_equal(rev[1][::-1], full[1]) and np.array_equal(rev[0][::-1], full[0])
    for b in range(B):  # (first <-> last, and the recorded tokens' scores bit for bit too)
        n = int(full[1][b])
        assert np.array_equal(rev[3][B - 1 - b, :n].view(np.uint32), full[3][b, :n].view(np.uint32)), b
    for b in (0, 5, 16):
        one = ctx.translate(ids[b:b + 1], lens[b:b + 1], sl, sampling=(T, keys[b:b + 1].copy()), truncation=trunc)
        assert one[1][0] == full[1][b] and np.array_equal(one[0][0], full[0][b]), b
    ctx.close()


def test_every_entry_point_draws_the_same_truncated_bits(hip, contexts, oracle, engines):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S, T, trunc = 17, 16, 1.0, (40, 0.8)
    ids, lens = synth.make_batch(m.V, B, S, seed=23, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    Tm = tmax_of(S)
    keys = keys_of(4, B)
    want = truncated_translate(oracle, om, m, ids, lens, sl, keys, T, *trunc)
    ctx = contexts(gm, B, S)
    _check(ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), truncation=trunc), want, T)  # pageable
    _check(ctx.translate(ids, lens, sl, want_align=True, sampling=(T, keys), truncation=trunc), want, T, scores=False)
    _check(ctx.translate_pinned(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), truncation=trunc), want, T)
    d_ids, d_len, d_sl, d_keys = _dev(ids), _dev(lens), _dev(sl), _dev(keys)
    d_out = torch.zeros((B, Tm), dtype=torch.int32, device="cuda")
    d_ol = torch.zeros((B,), dtype=torch.int32, device="cuda")
    d_sc = torch.zeros((B, Tm), dtype=torch.float32, device="cuda")
    ctx.translate_device(d_ids.data_ptr(), d_len.data_ptr(), B, S, d_sl.data_ptr(), sl.size, 1.5, 0, d_out.data_ptr(),
                         d_ol.data_ptr(), scores=d_sc.data_ptr(), sampling=(T, d_keys.data_ptr()), truncation=trunc)
    ctx.synchronize()
    _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), want, T)
    # a generated lexical shortlist: the set goes by values and the noise by vocabulary id, whatever the list's layout
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    gwant = truncated_translate(oracle, om, m, ids, lens, osl.generate(ids, lens), keys, T, *trunc)
    _check(ctx.translate_generated(gen, ids, lens, scores=True, sampling=(T, keys), truncation=trunc), gwant, T)
    _check(ctx.translate_pinned(ids, lens, generator=gen, scores=True, sampling=(T, keys), truncation=trunc), gwant, T)
    d_out.zero_()
    ctx.translate_device_generated(gen, d_ids.data_ptr(), d_len.data_ptr(), B, S, 1.5, 0, d_out.data_ptr(), d_ol.data_ptr(),
                                   scores=d_sc.data_ptr(), sampling=(T, d_keys.data_ptr()), truncation=trunc)
    ctx.synchronize()
    _check((d_out.cpu().numpy().view(np.uint32), d_ol.cpu().numpy().view(np.uint32), None, d_sc.cpu().numpy()), gwant, T)
    ctx.close()
    gen.close()


def test_translate_many_gives_each_batch_its_own_single_call_result(hip, contexts, engines):
    from slimt_amd import capi, synth
    m, gm, _ = engines("tiny11")
    shapes = [(3, 8), (17, 16), (32, 32)]  # (B_j, S_j)
    S, T, trunc = 32, 0.7, (40, 0.9)
    sl = synth.make_shortlist(m.V, 4096)
    batches = [synth.make_batch(m.V, B, Sj, seed=400 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    keys = [keys_of(50 + j, B) for j, (B, _) in enumerate(shapes)]
    rows = hip.translate_many_rows([b for b, _ in shapes])
    own = contexts(gm, rows, S)
    owns = [own.translate(ids, lens, sl, scores=True, sampling=(T, k), truncation=trunc) for (ids, lens), k in zip(batches, keys)]
    plain = [own.translate(ids, lens, sl, sampling=(T, k)) for (ids, lens), k in zip(batches, keys)]
    assert any(not np.array_equal(o[0], p[0]) for o, p in zip(owns, plain))  # (the truncation is in force)
    ctx = contexts(gm, rows, S)
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
    ctx.translate_many_async(bufs, sl, scores=scs, sampling=(T, keys), truncation=trunc)
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
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=tmax_of(S), sampling=(T, [d[2].data_ptr() for d in keep]), truncation=trunc)
    ctx.synchronize()
    for o, (d_out, d_ol) in zip(owns, outs):
        assert np.array_equal(d_ol.cpu().numpy().view(np.uint32), o[1])
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), o[0])
    ctx.close()
    own.close()
    for pp in pins:
        pp.free()


# ---- 6: with a prefix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_forced_steps_are_whole_and_the_first_drawn_step_is_truncated(hip, contexts, oracle, engines, mode):
    from slimt_amd import synth
    m, gm, om = engines("tiny11")
    B, S, T, trunc = 17, 16, 0.7, (8, 0.9)
    ids, lens = synth.make_batch(m.V, B, S, seed=71, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    Tm = tmax_of(S)
    rng = np.random.default_rng(6)
    p_ids = rng.choice(sl[sl != 0], size=(B, Tm)).astype(np.uint32)
    p_len = np.array([(0, 1, 3, Tm)[b % 4] for b in range(B)], np.uint32)
    missing = np.setdiff1d(np.arange(1, m.V, dtype=np.uint32), sl)
    p_ids[2, 1] = missing[0]  # absent from the output layer: still fed, scored -inf
    keys = keys_of(12, B)
    sizes = []
    want = truncated_translate(oracle, om, m, ids, lens, sl, keys, T, *trunc, p_ids=p_ids, p_len=p_len, sizes=sizes)
    ctx = contexts(gm, B, S)
    ctx.set_decode_mode(mode)
    got = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=(p_ids, p_len), sampling=(T, keys), truncation=trunc)
    _check(got, want, T)
    assert np.isneginf(got[3][2, 1])
    # the forced steps score as in the untruncated sampled call: over the whole layer
    plain = ctx.translate(ids, lens, sl, scores=True, prefix=(p_ids, p_len), sampling=(T, keys))
    tol = TOL * max(1.0, 1.0 / T)
    for b in range(B):
        n = min(int(p_len[b]), int(got[1][b]), int(plain[1][b]))
        assert np.array_equal(got[0][b, :n], p_ids[b, :n]), b
        g, w = got[3][b, :n].astype(np.float64), plain[3][b, :n].astype(np.float64)
        assert np.array_equal(np.isneginf(g), np.isneginf(w))
        fin = np.isfinite(w)
        assert np.abs(g[fin] - w[fin]).max(initial=0) <= tol, b
    # ... and the first drawn step of every sentence that has one is cut to at most the top 8 (and ties)
    first = {}
    for b, t, n in sizes:
        first.setdefault(b, (t, n))
    assert first and all(t == int(p_len[b]) and n < 4096 for b, (t, n) in first.items())
    ctx.close()


# ---- 7: validation --------------------------------------------------------------------------------------------------------
def test_bad_settings_are_refused_and_truncation_without_sampling_fails_one_call(hip, contexts, oracle, engines):
    from slimt_amd import capi, synth
    m, gm, om = engines("tiny11")
    B, S = 5, 8
    ids, lens = synth.make_batch(m.V, B, S, seed=81, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    oracle.set_mode(oracle.PORTABLE)
    try:
        w_out, w_ln, _, _ = om.translate(ids, lens, sl, 1.5, 0)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    ctx = contexts(gm, B, S)
    for bad in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(capi.SlimtHipError, match="top_p"):
            ctx.set_sampling_truncation(4, bad)
        g = ctx.translate(ids, lens, sl)  # (refused at once: nothing was armed)
        assert np.array_equal(g[1], w_ln) and np.array_equal(g[0], w_out)
    with pytest.raises(capi.SlimtHipError, match="without sampling"):
        ctx.translate(ids, lens, sl, truncation=(4, 0.9))
    g = ctx.translate(ids, lens, sl)  # the failed call consumed the setting: the next one is clean
    assert np.array_equal(g[1], w_ln) and np.array_equal(g[0], w_out)
    # ... and a truncated call leaves nothing armed behind: the next sampled call is untruncated
    keys = keys_of(3, B)
    a = ctx.translate(ids, lens, sl, scores=True, sampling=(1.0, keys))
    ctx.translate(ids, lens, sl, sampling=(1.0, keys), truncation=(2, 0.5))
    b = ctx.translate(ids, lens, sl, scores=True, sampling=(1.0, keys))
    for x, y in zip(a, b):
        if x is not None:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    ctx.close()


# ---- 8: service and frontend ----------------------------------------------------------------------------------------------
def test_a_truncating_service_is_reproducible_and_equals_the_checker(hip, oracle, synth_models):
    from slimt_amd import capi, synth
    m = synth_models("tiny11", 6.0)
    gm, om = hip.Model(m), oracle.OracleModel(m)
    rnd = np.random.Generator(np.random.PCG64(5))
    S, T, seed, trunc = 12, 1.0, 7, (40, 0.9)
    mine = [list(rnd.integers(3, m.V, S - 1)) + [0] for _ in range(23)]
    fixed = synth.make_shortlist(m.V, 2048)
    kw = dict(max_words=(10 + 1) * S, workers_per_device=1, source_vocab=m.V, target_vocab=m.V, shortlist=fixed,
              scores=True, temperature=T)  # (batches of 10, merging at its default: a truncating service does not merge)
    svc = hip.BatchService([gm], truncation=trunc, **kw)
    try:
        a, b = svc.translate(mine, seed=seed), svc.translate(mine, seed=seed)
        assert np.array_equal(a.target_offsets, b.target_offsets) and np.array_equal(a.targets, b.targets)
        assert np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32))
        ids = np.array(mine, np.uint32)
        lens = np.full(len(mine), S, np.uint32)
        keys = np.array([capi.sampling_key(seed, i) for i in range(len(mine))], dtype=np.uint64)
        w_out, w_ln, _, w_sc = truncated_translate(oracle, om, m, ids, lens, fixed, keys, T, *trunc)
        for i in range(len(mine)):
            n = int(w_ln[i])
            assert np.array_equal(a.target(i), w_out[i, :n]), i
            assert np.abs(a.token_scores(i).astype(np.float64) - w_sc[i, :n]).max() <= TOL, i
        assert hip.host_lib().slimt_hip_service_set_sampling_truncation(svc.h, 2, 0.5) != 0  # only before the first translate
        a.close()
        b.close()
    finally:
        svc.close()
    with pytest.raises(capi.SlimtHipError):  # a service that does not sample cannot truncate
        hip.BatchService([gm], max_words=(10 + 1) * S, workers_per_device=1, source_vocab=m.V, target_vocab=m.V, shortlist=fixed,
                         truncation=trunc)
    gm.close()


def test_frontend_truncation_is_reproducible_and_scored(hip):
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
    spm = io.BytesIO()
    sentencepiece.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=spm, vocab_size=512,
                                             model_type="unigram", pad_id=-1, unk_id=1, bos_id=-1, eos_id=0, minloglevel=2)
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    blob = synth.make_lexical_shortlist(m.V, m.V, frequent=32, best=8, seed=5)
    package = frontend.Package(model=synth.write_bin(m), vocabulary=spm.getvalue(), shortlist=blob)
    cfg = frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph")
    model = frontend.Model(cfg, package, device=0)
    svc = frontend.Service(workers=2, max_words=256, wrap_length=24)
    try:
        texts = [" ".join(corpus[i:i + 3]) + "\n" + corpus[i + 3] for i in range(0, 24, 4)]
        kw = dict(encoding=frontend.Encoding.Byte, sampling=(1.0, 7), scores=True)
        a = svc.translate(model, texts, truncation=(4, 0.9), **kw)
        b = svc.translate(model, texts, truncation=(4, 0.9), **kw)
        c = svc.translate(model, texts, **kw)
        for x, y in zip(a, b):
            assert x.target.text == y.target.text and x.sentence_scores == y.sentence_scores
            assert np.all(np.isfinite(x.sentence_scores))
            for k in range(x.target.sentence_count()):
                assert len(x.token_scores[k]) == x.target.word_count(k) and np.all(x.token_scores[k] <= 1e-6)
        assert any(x.target.text != y.target.text for x, y in zip(a, c))
        with pytest.raises(ValueError):
            svc.translate(model, texts, encoding=frontend.Encoding.Byte, truncation=(4, 0.9))
        p1 = svc.pivot(model, model, texts[:3], sampling=(1.0, 3), truncation=(4, 0.9))
        p2 = svc.pivot(model, model, texts[:3], sampling=(1.0, 3), truncation=(4, 0.9))
        assert all(x.target.text == y.target.text for x, y in zip(p1, p2))
    finally:
        svc.close()
        model.close()
