"""GPU parity over the VALUES a model may hold, not only the default synthetic family: every value family of
slimt_amd.synth.FAMILIES and one ceiling model per shape (tests/support/model_values.py; tests/test_model_value_fixtures.py
holds them to be worth comparing) on the four shapes with a persistent decoder, against the oracle's PORTABLE order, bit for
bit -- encoder layer by layer, decoder steps teacher-forced, greedy translation in every decode mode and K/V cache format,
the cache form every sentence takes -- and, one case per family, through the options added since the families were last
looked at: scores, forced prefixes, sampling, the one-pass scorer and merged launches.

What a ceiling model is for: decoder layer 1's K / V accumulators sit at +254 * 127 * D and -254 * 128 * D (-2^23 + 65,536 at
D = 256) in every row. Every source position then has the SAME K row and the same V row: layer 1's attention is uniform
whatever K holds, and its context vector is that V row. So a sign lost in the 24-bit unpack of V, a quantiser that clamps to
-128, or a conversion split in two changes every context vector of that layer and with it every number compared below; a
sign lost in the unpack of K is NOT visible on a ceiling model -- that is covered by the families whose sentences take the
24-bit form with varied values (w64 and w48 at emb 512), translated in every mode with the forms checked."""
import numpy as np
import pytest

from support import model_values as T
from test_forced_prefix_checker import forced_translate, tmax_of
from test_gpu_kv_narrow import colsum_centres
from test_gpu_model_shapes import encoder_reference
from test_sampling_checker import keys_of, sampled_translate
from test_score_checker import teacher_forced

pytestmark = pytest.mark.gpu

MODELS = T.ENTRIES + T.CEILINGS
PACKED = (256, 512)  # emb sizes with the packed K/V cache (formats 0 / 2 / 1 differ there)
OPTION_ENTRIES = [e for e in T.ENTRIES if e.dims[0] in PACKED]
OPTION_CASE = T.TRANSLATE_CASES[0]  # (21, 13, shortlist 200)


def _fresh(gm):
    """start format 0's watches afresh at the real limits, so that what earlier batches of this model needed cannot switch a
    form off (tests/test_gpu_kv_narrow.py does the same)"""
    gm.debug_kv_narrow_limit(2 ** 19)
    gm.debug_kv_tight_limit(2 ** 15)


def _device_model(hip, m):
    gm = hip.Model(m)
    if m.D in PACKED:
        gm.set_kv_centres(colsum_centres(m))  # the tight form holds the signed accumulator; no calibration batch
    return gm


@pytest.fixture(scope="module")
def engines(hip, oracle):
    """(synthetic model, device model, oracle model) per table entry, created once for the module"""
    cache = {}

    def get(e):
        key = (e.family, e.dims)
        if key not in cache:
            m = T.make(e)
            cache[key] = (m, _device_model(hip, m), oracle.OracleModel(m))
        m, gm, om = cache[key]
        if m.D in PACKED:
            _fresh(gm)
        return m, gm, om

    try:
        yield get
    finally:
        for _, gm, _ in cache.values():
            gm.close()


def _modes(dims, S):
    """every decode mode: 0 automatic, 1 per-stage kernels, 2 / 3 / 4 / 5 = 16 / 32 / 8 / 4 sentences per workgroup, and 6
    (cluster logits) where the kernel has it: emb 256 with sources of up to 32 tokens"""
    return (0, 1, 2, 3, 4, 5) + ((6,) if dims[0] == 256 and S <= 32 else ())


def _check_scores(got, want, ln, peaks):
    """scores against the checker's float64 ones, row by row: within max(TOL, 8 ulps of the row's largest |logit|)
    (T.score_bound), -inf exactly where the checker has it"""
    worst = 0.0
    for b in range(len(ln)):
        n = int(ln[b])
        g, w = got[b, :n].astype(np.float64), want[b, :n]
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), (b, g, w)
        fin = np.isfinite(w)
        assert np.all(np.isfinite(g[fin])), (b, g)
        bound = np.array([T.score_bound(peaks[t, b]) for t in range(n)])
        err = np.abs(g - w)
        worst = max(worst, float((err[fin] / bound[fin]).max(initial=0)))
        assert np.all(err[fin] <= bound[fin]), (b, err[fin].max(), bound[fin].min())
    print("scores: at most %.3f of the bound; largest |logit| %.1f" % (worst, peaks.max()))


ENC_CASES = [pytest.param(e, S, id="%s-S%d" % (T.entry_id(e), S)) for e in MODELS
             for S in (13, 40) + ((70,) if e.dims[0] == 256 else ())]


@pytest.mark.parametrize("e,S", ENC_CASES)
def test_encoder_every_layer_bit_exact(hip, oracle, engines, e, S):
    """B = 5 and 21; decode mode 0 (the persistent encoder where the shape has one) and 1 (the per-stage kernels), and the
    forced 32- and 64-row tiles where mode 0 is a persistent encoder. On the ceiling model encoder layer 1's W2 has
    one-signed columns: at FFN 1536 / 2048 every accumulator of theirs is past 2^24, where float(accS) rounds."""
    m, gm, om = engines(e)
    for B in (5, 21):
        ids, lens = T.batch(e.dims, B, S)
        want, _ = encoder_reference(oracle, om, m, ids, lens, S)
        ctx = hip.Context(gm, B, S)
        try:
            assert ctx.plan(S) == T.expected_plan(e.dims, S)
            runs = [(0, 0), (1, 0)] + ([(0, 32), (0, 64)] if T.expected_plan(e.dims, S)[0] else [])
            for mode, rows in runs:
                ctx.set_decode_mode(mode)
                ctx.set_encode_rows(rows)
                enc, emb, layers = ctx.encode(ids, lens, want_embed=True, want_layers=True)
                assert np.array_equal(emb, want[0]), (B, mode, rows)
                for l in range(1, m.enc_layers + 1):
                    assert np.array_equal(layers[l - 1], want[l]), (B, mode, rows, l, np.abs(layers[l - 1] - want[l]).max())
                assert np.array_equal(enc, want[-1]), (B, mode, rows)
        finally:
            ctx.close()


@pytest.mark.parametrize("e", MODELS, ids=T.entry_id)
def test_decoder_steps_teacher_forced_bit_exact(hip, oracle, engines, e):
    """Five Decoder::step calls with random previous tokens, (B, S) = (5, 13) and (21, 40): SSRU states, last-layer attention
    and logits, over a 200-id shortlist and over the full vocabulary. The ceiling model's layer-1 K and V are at the
    accumulators' extremes and its decoder W2 has the one-signed columns."""
    m, gm, om = engines(e)
    for B, S in ((5, 13), (21, 40)):
        ids, lens = T.batch(e.dims, B, S, salt=1)
        ctx = hip.Context(gm, B, S)
        try:
            enc, _, _ = ctx.encode(ids, lens)
            want_enc, mask = encoder_reference(oracle, om, m, ids, lens, S)
            assert np.array_equal(enc, want_enc[-1])
            enc = want_enc[-1]
            for sl in (T.shortlist(e.dims, T.SHORTLIST), None):
                ctx.decode_begin(sl)
                oracle.set_mode(oracle.PORTABLE)
                states = np.zeros((m.dec_layers, B, m.D), dtype=np.float32)
                r = np.random.Generator(np.random.PCG64(5))
                prev = None
                for t in range(5):
                    want_logits, want_attn = om.decode_step(enc, mask, states, prev, sl)
                    logits, attn, st = ctx.decode_step(prev)
                    assert np.array_equal(st, states), (B, S, sl is None, t, np.abs(st - states).max())
                    assert np.array_equal(attn, want_attn), (B, S, sl is None, t)
                    assert np.array_equal(logits, want_logits), (B, S, sl is None, t, np.abs(logits - want_logits).max())
                    prev = r.choice(np.arange(m.V) if sl is None else sl, size=B).astype(np.uint32)
                oracle.set_mode(oracle.FAITHFUL)
        finally:
            oracle.set_mode(oracle.FAITHFUL)
            ctx.close()


TR_CASES = [pytest.param(e, c, id="%s-B%d-S%d" % ((T.entry_id(e),) + c[:2])) for e in T.ENTRIES for c in T.TRANSLATE_CASES]


@pytest.mark.parametrize("e,case", TR_CASES)
def test_translate_tokens_lengths_alignments(hip, oracle, engines, e, case):
    """Model::forward in every decode mode the shape has; where the K/V cache is packed, in cache formats 0, 2 and 1 on a
    device model of this test's own, centres set to 127 colsum. The CPU fixture test keeps these batches from being
    degenerate (but the two T.DEGENERATE lists). The ceiling models' greedy output IS degenerate (every sentence ends at
    step 1, or none ever does): they are compared teacher-forced above and, forced, with the cache forms below."""
    B, S, n_sl = case
    m, gm, om = engines(e)
    ids, lens, sl, w_out, w_ln, w_al, _ = T.translate_reference(oracle, om, e.dims, B, S, n_sl)
    own = _device_model(hip, m) if m.D in PACKED else None
    ctx = hip.Context(own or gm, B, S)
    try:
        for fmt in ((0, 2, 1) if own else (None,)):
            if fmt is not None:
                own.set_kv_cache_format(fmt)
            for mode in _modes(e.dims, S):
                ctx.set_decode_mode(mode)
                out, ln, al = ctx.translate(ids, lens, sl, limit_factor=1.5, eos_id=0, want_align=True)
                assert np.array_equal(ln, w_ln), (fmt, mode, ln, w_ln)
                assert np.array_equal(out, w_out), (fmt, mode)
                assert np.array_equal(al, w_al), (fmt, mode)
    finally:
        ctx.close()
        if own:
            own.close()


FORM_CASES = [pytest.param(e, c, id="%s-B%d-S%d" % ((T.entry_id(e),) + c)) for e in MODELS if e.dims[0] in PACKED
              for c in T.FORM_CASES[e.dims[0]]]


@pytest.mark.parametrize("e,case", FORM_CASES)
def test_cache_forms_follow_the_oracles_accumulators_at_the_real_limits(hip, oracle, e, case):
    """Format 0: slimt_hip_debug_kv_formats must equal expected_forms of tests/test_gpu_kv_narrow.py computed from the oracle's
    accumulators at the limits the library ships with, 2^19 and 2^15 -- with sentences on both sides of both (emb 512: a8_24 and w48 mix 16 / 20 and
    20 / 24 bits in one batch; emb 256: default and ln0.3 mix 16 / 20). No peak of the table sits ON a limit: the nearest is 238
    from 2^19 (w48, emb 512) and 33 from 2^15 (default, emb 256), so this test pins the shipped limits only to within those
    distances; the off-by-one is pinned by test_a_limit_at_a_sentences_own_peak_moves_its_form below.
    On a ceiling model every sentence of layer 1 takes the 24-bit form and every one of layer 2 a narrower one, in the same
    workgroup. Decoders without a reader for the 16-bit form (T.tight_tried) get 20 bits where 16 would do. The translation itself stays the oracle's, in every decode mode with a persistent decoder; a ceiling model is
    also run FORCED through random targets of full length with scores and alignments (its greedy output is degenerate),
    which reads the 24-bit cache at every step: a sign lost in its unpack, or a -128 where the quantiser must give -127,
    moves layer 1's context vectors and so the alignment rows (bit for bit) and the scores."""
    B, S = case
    D = e.dims[0]
    m = T.make(e)
    gm, om = _device_model(hip, m), oracle.OracleModel(m)
    ids, lens = T.batch(e.dims, B, S, salt=2)
    sl = T.shortlist(e.dims, T.SHORTLIST)
    ctx = hip.Context(gm, B, S)
    try:
        oracle.set_mode(oracle.PORTABLE)
        want = om.translate(ids, lens, sl, 1.5, 0, want_align=True)[:3]
        oracle.set_mode(oracle.FAITHFUL)
        forced = None
        if e.family == "ceiling":
            p = T.ceiling_targets(B, S, sl)
            rec = T.Recording(om)
            forced = (p, forced_translate(oracle, rec, m, ids, lens, sl, *p), rec.row_peaks())
        for rows in T.ENCODE_ROWS[D]:
            ctx.set_encode_rows(rows)
            by_tight = {t: T.forms_of(oracle, m, om, ids, lens, max(1, rows // S), tight=t)[0] for t in (True, False)}
            if e.family == "ceiling":
                assert all((f[0] == 1).all() and (f[1] != 1).all() for f in by_tight.values())
            for mode in [k for k in _modes(e.dims, S) if k != 1]:
                ctx.set_decode_mode(mode)
                forms = by_tight[T.tight_tried(mode, S)]
                _fresh(gm)
                got = ctx.translate(ids, lens, sl, want_align=True)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (rows, mode)
                seen = ctx.debug_kv_formats(m.dec_layers, B)
                if not T.forms_recorded(S, rows, mode):
                    assert seen is None, (rows, mode, seen)
                    continue
                assert seen is not None and np.array_equal(seen, forms), (rows, mode, seen, forms)
                if forced:
                    p, (w_out, w_ln, w_al, w_sc), peaks = forced
                    _fresh(gm)
                    out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p)
                    assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), (rows, mode)
                    assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), (rows, mode)
                    _check_scores(sc, w_sc, ln, peaks)
                    assert np.array_equal(ctx.debug_kv_formats(m.dec_layers, B), forms), (rows, mode)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
        ctx.close()
        gm.close()


BOUNDARY = [pytest.param(T.entry("default", 256), 64, id="default-D256"), pytest.param(T.entry("a8_24", 512), 32, id="a8_24-D512")]


def boundary_limits(values, group, cap):
    """values [Ld][2][B][S][D] (int64): the extremes (lo, hi) of the (layer, workgroup of `group` sentences) whose peak is
    the median of those below `cap`, and the limits next to them. A value v is inside [-limit, limit) iff -limit <= v < limit: hi is
    outside at limit = hi and inside at hi + 1; lo is inside at limit = -lo and outside at -lo - 1."""
    B = values.shape[2]
    ext = [(int(v[:, s0:s0 + group].min()), int(v[:, s0:s0 + group].max())) for v in values for s0 in range(0, B, group)]
    ext = sorted((e for e in ext if max(-e[0], e[1]) < cap), key=lambda e: max(-e[0], e[1]))
    lo, hi = ext[len(ext) // 2]
    return lo, hi, [v for v in (hi, hi + 1, -lo - 1, -lo) if 1 <= v <= cap]


@pytest.mark.parametrize("e,rows", BOUNDARY)
def test_a_limit_at_a_sentences_own_peak_moves_its_form(hip, oracle, e, rows):
    """The off-by-one of the form predicates on a family model per packed shape, case (21, 13): the 20-bit limit is set to one
    encoder workgroup's largest accumulator hi and to hi + 1, and to -lo - 1 and -lo for its smallest (16-bit form off);
    then the 16-bit limit likewise on the signed accumulators. Inside is -limit <= v < limit, so the workgroup's sentences
    must change form between the two limits of the pair on the side of its peak -- asserted on the oracle's forms first --
    and the device must show the oracle's forms at all four: `<=` for `<` at either end, or a limit off by one, fails."""
    from test_gpu_kv_narrow import centred, expected_forms, kv_accumulators
    B, S, n_sl = T.TRANSLATE_CASES[0]
    group = max(1, rows // S)
    m = T.make(e)
    gm, om = _device_model(hip, m), oracle.OracleModel(m)
    ids, lens, sl, w_out, w_ln, w_al, _ = T.translate_reference(oracle, om, e.dims, B, S, n_sl)
    acc = kv_accumulators(oracle, m, om, ids, lens).astype(np.int64)
    signed = centred(acc, colsum_centres(m))
    ctx = hip.Context(gm, B, S)
    try:
        ctx.set_encode_rows(rows)
        for values, cap, tight in ((acc, 2 ** 19, False), (signed, 2 ** 15, True)):
            lo, hi, limits = boundary_limits(values, group, cap)
            assert len(limits) == 4, (lo, hi)

            def want(limit):
                return expected_forms(acc, limit if not tight else 2 ** 19, group, signed, limit if tight else 0)

            pair = (hi, hi + 1) if hi >= -lo else (-lo - 1, -lo)
            assert not np.array_equal(want(pair[0]), want(pair[1])), (tight, lo, hi)
            for limit in limits:
                for mode in (2, 4):  # (16 and 8 sentences per decoder workgroup: both read every form)
                    ctx.set_decode_mode(mode)
                    gm.debug_kv_narrow_limit(2 ** 19 if tight else limit)
                    gm.debug_kv_tight_limit(limit if tight else 0)
                    out, ln, al = ctx.translate(ids, lens, sl, want_align=True)
                    assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out) and np.array_equal(al, w_al), (tight, limit, mode)
                    seen = ctx.debug_kv_formats(m.dec_layers, B)
                    assert seen is not None and np.array_equal(seen, want(limit)), (tight, limit, mode, lo, hi, seen, want(limit))
    finally:
        ctx.close()
        gm.close()


def _option_inputs(e):
    B, S, n_sl = OPTION_CASE
    ids, lens = T.batch(e.dims, B, S, salt=2)
    return B, S, ids, lens, T.shortlist(e.dims, n_sl)


def _spread(B, hi, lo=0):
    return [lo + (b * (hi - lo)) // max(1, B - 1) for b in range(B)]


@pytest.mark.parametrize("e", OPTION_ENTRIES, ids=T.entry_id)
def test_scores_of_the_greedy_translation(hip, oracle, engines, e):
    m, gm, om = engines(e)
    B, S, ids, lens, sl = _option_inputs(e)
    rec = T.Recording(om)
    w_out, w_ln, w_al, w_sc = forced_translate(oracle, rec, m, ids, lens, sl, np.zeros((B, tmax_of(S)), np.uint32), np.zeros(B, np.uint32))
    ctx = hip.Context(gm, B, S)
    try:
        for mode in (0, 1):
            ctx.set_decode_mode(mode)
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True)
            assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), mode
            assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), mode
            _check_scores(sc, w_sc, ln, rec.row_peaks())
    finally:
        ctx.close()


@pytest.mark.parametrize("e", OPTION_ENTRIES, ids=T.entry_id)
def test_a_forced_prefix_then_greedy(hip, oracle, engines, e):
    """prefixes of 0 .. Tmax random tokens (no EOS), completed greedily: tokens, lengths and alignment rows bit for bit,
    scores within the bound"""
    m, gm, om = engines(e)
    B, S, ids, lens, sl = _option_inputs(e)
    Tm = tmax_of(S)
    p = (np.random.default_rng(S + B).choice(sl[sl != 0], size=(B, Tm)).astype(np.uint32), np.asarray(_spread(B, Tm), np.uint32))
    rec = T.Recording(om)
    w_out, w_ln, w_al, w_sc = forced_translate(oracle, rec, m, ids, lens, sl, *p)
    ctx = hip.Context(gm, B, S)
    try:
        for mode in (0, 1):
            ctx.set_decode_mode(mode)
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p)
            assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), mode
            assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), mode
            _check_scores(sc, w_sc, ln, rec.row_peaks())
    finally:
        ctx.close()


@pytest.mark.parametrize("e", OPTION_ENTRIES, ids=T.entry_id)
def test_temperature_sampling(hip, oracle, engines, e):
    """decode modes 0 and 1 at temperature 0.7: the draw is bit for bit the checker's; scores are those of z = logit / T, so
    the row's peak L is that of z and the bound T.score_bound(L) as for every other score here -- the project's 5e-5 is NOT
    scaled by 1 / T as tests/test_gpu_sampling.py does (test_model_value_fixtures.py checks the bound on the scaled logits)"""
    m, gm, om = engines(e)
    B, S, ids, lens, sl = _option_inputs(e)
    temp = T.SAMPLING_TEMPERATURE
    keys = keys_of(S + B, B)
    rec = T.Recording(om)
    w_out, w_ln, w_al, w_sc = sampled_translate(oracle, rec, m, ids, lens, sl, keys, temp)
    peaks = rec.row_peaks(np.float32(1.0) / np.float32(temp))
    ctx = hip.Context(gm, B, S)
    try:
        for mode in (0, 1):
            ctx.set_decode_mode(mode)
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(temp, keys))
            assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out), mode
            assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), mode
            _check_scores(sc, w_sc, ln, peaks)
    finally:
        ctx.close()


@pytest.mark.parametrize("e", OPTION_ENTRIES, ids=T.entry_id)
def test_the_one_pass_scorer_on_targets_three_times_the_source_length(hip, oracle, engines, e):
    """slimt_hip_score with T = 3 S and alignments, target lengths 0 .. T"""
    m, gm, om = engines(e)
    B, S, ids, lens, sl = _option_inputs(e)
    Tt = 3 * S
    fill = np.float32(-7.25)
    t_ids = np.random.default_rng(B).choice(sl[sl != 0], size=(B, Tt)).astype(np.uint32)
    t_len = np.asarray(_spread(B, Tt), np.uint32)
    rec = T.Recording(om)
    w_sc, w_al = teacher_forced(oracle, rec, m, ids, lens, sl, t_ids, t_len)
    ctx = hip.Context(gm, B, S)
    try:
        sc, al = ctx.score(ids, lens, sl, t_ids, t_len, want_align=True, fill=fill)
        _check_scores(sc, w_sc, t_len, rec.row_peaks())
        for b in range(B):
            n, L = int(t_len[b]), int(lens[b])
            assert np.array_equal(al[b, :n, :L].view(np.uint32), w_al[b, :n, :L].view(np.uint32)), b
            assert np.all(sc[b, n:] == fill) and np.all(al[b, n:] == fill) and np.all(al[b, :, L:] == fill), b
    finally:
        ctx.close()


@pytest.mark.parametrize("e", OPTION_ENTRIES, ids=T.entry_id)
def test_two_merged_batches_equal_each_batch_own_call(hip, oracle, engines, e):
    """slimt_hip_translate_many_async on two batches (21 x 13 and 5 x 9, the second padded to fewer tokens) with scores: each
    batch's tokens, lengths and scores are bit for bit its own call's, and its own call's tokens are the oracle's"""
    from slimt_amd import capi
    m, gm, om = engines(e)
    S = OPTION_CASE[1]
    sl = T.shortlist(e.dims, OPTION_CASE[2])
    batches = [T.batch(e.dims, B, Sj, salt=3) for B, Sj in ((OPTION_CASE[0], S), (5, 9))]
    rows = hip.translate_many_rows([ids.shape[0] for ids, _ in batches])
    own = hip.Context(gm, rows, S)
    ctx = hip.Context(gm, rows, S)
    pins = []
    try:
        owns = [own.translate(ids, lens, sl, scores=True) for ids, lens in batches]
        oracle.set_mode(oracle.PORTABLE)
        for (ids, lens), o in zip(batches, owns):
            w_out, w_ln, _, _ = om.translate(ids, lens, sl, 1.5, 0)
            assert np.array_equal(o[1], w_ln) and np.array_equal(o[0], w_out)
        oracle.set_mode(oracle.FAITHFUL)
        bufs, scs = [], []
        for ids, lens in batches:
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
        ctx.translate_many_async(bufs, sl, scores=scs)
        ctx.synchronize()
        for b, sc, o in zip(bufs, scs, owns):
            assert np.array_equal(b[3], o[1]) and np.array_equal(b[2], o[0])
            for r in range(len(o[1])):
                assert np.array_equal(sc[r, :o[1][r]].view(np.uint32), o[3][r, :o[1][r]].view(np.uint32)), r
    finally:
        oracle.set_mode(oracle.FAITHFUL)
        ctx.close()
        own.close()
        for pp in pins:
            pp.free()
