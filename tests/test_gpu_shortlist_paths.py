"""ShortlistGenerator::generate on every path the library has for it, id for id and count for count against the oracle's list
(tests/support/shortlist_cases.py; tests/test_shortlist_case_fixtures.py proves on the CPU which edges the cases reach):

  1. slimt_hip_shortlist_generate: the two kernels with the handle's staging buffers;
  2. slimt_hip_shortlist_generate_device: the same kernels on a context's stream and scratch;
  3. shortlist_generate_block inside an encoder launch (encode_tall / encode_fused / encode_wide), read back with
     slimt_hip_debug_ctx_shortlists after slimt_hip_translate_generated;
  4. its merged form, one list per sub-batch of slimt_hip_translate_many_*_generated.

A greedy translation is a weak witness of a shortlist: a missing low-probability id, a wrong patch, a padding word's list
leave every token unchanged. Where a translation is produced it is compared too (tokens, lengths, alignment rows, bit for bit
with the PORTABLE oracle's), but every list is compared by itself. All of it is integer work: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from support import shortlist_cases as T

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _tmax(S):
    return max(int(np.float32(1.5) * np.float32(S)), 1)


@pytest.fixture(scope="module")
def engines(hip):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = hip.Model(T.model(name))
        return cache[name]

    yield get
    for gm in cache.values():
        gm.close()


@pytest.fixture(scope="module")
def scratch_ctx(hip, synth_models):
    """Path 2 needs a context for its stream and its scratch only: slimt_hip_shortlist_generate_device checks the devices, not
    the vocabularies, and sizes the scratch from the generator's own. ONE context for all cases: the bitmaps of every
    vocabulary size share its scratch, each call must leave them zeroed for the next."""
    gm = hip.Model(synth_models("micro", 3.0))
    ctx = hip.Context(gm, 4, 8)
    yield ctx
    ctx.close()
    gm.close()


def _same_list(got, count, want, V):
    assert count <= V, (count, V)
    assert count == want.size, (count, want.size, np.setxor1d(got, want)[:16])
    assert np.array_equal(got, want), np.setxor1d(got, want)[:16]


@pytest.mark.parametrize("name", T.case_names())
def test_stand_alone_generators(hip, oracle, scratch_ctx, name):
    c = T.case(name)
    want = T.reference(oracle, c)
    gen = hip.ShortlistGenerator(c.blob, c.Vs, c.Vt, shared=c.shared, check=True)
    try:
        for _ in range(2):  # the handle's scratch bitmaps are left zeroed
            got = gen.generate(c.ids, c.lens)
            _same_list(got, got.size, want, c.Vt)
        if 2 not in c.paths:
            return
        B, S = c.ids.shape
        d_ids, d_len = _dev(c.ids), _dev(c.lens)
        d_out = torch.empty((c.Vt,), dtype=torch.int32, device="cuda")
        d_n = torch.empty((1,), dtype=torch.int32, device="cuda")
        for _ in range(2):  # ... and so are the context's
            d_out.fill_(SENTINEL)
            d_n.fill_(SENTINEL)
            torch.cuda.synchronize()
            gen.generate_device(scratch_ctx, d_ids.data_ptr(), d_len.data_ptr(), B, S, d_out.data_ptr(), d_n.data_ptr())
            scratch_ctx.synchronize()
            n = int(d_n.cpu().numpy().view(np.uint32)[0])
            out = d_out.cpu().numpy().view(np.uint32)
            _same_list(out[: min(n, c.Vt)], n, want, c.Vt)
            assert np.all(out[n:] == SENTINEL)  # nothing written behind the list
    finally:
        gen.close()


def _same_translation(got, want, lens):
    out, ln, al = got
    w_out, w_ln, w_al = want
    assert np.array_equal(ln, w_ln), (ln, w_ln)
    assert np.array_equal(out, w_out)
    for b in range(len(ln)):
        n, L = int(ln[b]), int(lens[b])
        assert np.array_equal(al[b, :n, :L].view(np.uint32), w_al[b, :n, :L].view(np.uint32)), b


def _open(hip, gm, B, S, rows=0, mode=0):
    ctx = hip.Context(gm, B, S)
    ctx.set_decode_mode(mode)
    if rows:
        ctx.set_encode_rows(rows)
    return ctx


@pytest.mark.parametrize("mc", T.MODEL_CASES, ids=T.model_case_id)
def test_generator_inside_the_encoder_launch(hip, oracle, engines, mc):
    """slimt_hip_translate_generated, then the list the context holds: the one the oracle generates for the batch. Twice per
    context: the publication flag's epoch is reused. S <= 32 (and 33..64 with 64-row tiles): generated in the launch by
    the workgroup of tile 0; above, and in decode mode 1: the two kernels on the context's stream."""
    enc, what, _, _, mode = mc
    name, c = T.model_case(mc)
    rows = T.ENCODERS[enc][1]
    want_sl, w_out, w_ln, w_al = T.translation(oracle, name, c)
    B, S = c.ids.shape
    ctx = _open(hip, engines(name), B, S, rows, mode)
    gen = hip.ShortlistGenerator(c.blob, c.Vs, c.Vt)
    try:
        if mode == 0 and S <= 32:
            assert ctx.plan(S) == (True, True)  # persistent encoder and decoder: the generator runs inside the encoder launch
        for _ in range(2):
            got = ctx.translate_generated(gen, c.ids, c.lens, want_align=True)
            lists, counts = ctx.debug_shortlists(1, with_counts=True)
            _same_list(lists[0], int(counts[0]), want_sl, c.Vt)
            _same_translation(got, (w_out, w_ln, w_al), c.lens)
    finally:
        gen.close()
        ctx.close()


def test_stale_size_hint(hip, oracle, engines):
    """The host picks the decoder tiling from the PREVIOUS list's size: the smallest and the largest list the blob allows in
    turn on one context (a few dozen ids; past the 16384 columns where the tiling changes) -- every call's list and
    translation are its own batch's."""
    gm = engines(T.HINT_MODEL)
    ctx = _open(hip, gm, 40, 32, T.HINT_ENCODER_ROWS)
    blob, Vs = T.generator_blob(T.HINT_MODEL, T.HINT_GENERATOR)
    gen = hip.ShortlistGenerator(blob, Vs, T.model_V(T.HINT_MODEL))
    try:
        for B, S in T.HINT_SHAPES:
            c = T.hint_case(B, S)
            want_sl, w_out, w_ln, w_al = T.translation(oracle, T.HINT_MODEL, c)
            got = ctx.translate_generated(gen, c.ids, c.lens, want_align=True)
            lists, counts = ctx.debug_shortlists(1, with_counts=True)
            _same_list(lists[0], int(counts[0]), want_sl, c.Vt)
            _same_translation(got, (w_out, w_ln, w_al), c.lens)
    finally:
        gen.close()
        ctx.close()


def _merged_setup(hip, engines, name):
    S, cases = T.merged_batches(name)
    gm = engines(T.MERGED_MODEL)
    gen = hip.ShortlistGenerator(cases[0].blob, cases[0].Vs, cases[0].Vt)
    rows = hip.translate_many_rows([c.ids.shape[0] for c in cases])
    return S, cases, gm, gen, rows


def _check_merged(hip, oracle, ctx, gm, gen, S, cases, res):
    """res: per sub-batch (out, len, align). The lists at j * V are each sub-batch's own; the translations are the oracle's of
    each batch alone, and those of each batch's own call."""
    V = T.model_V(T.MERGED_MODEL)
    lists, counts = ctx.debug_shortlists(len(cases), with_counts=True)
    own = hip.Context(gm, max(c.ids.shape[0] for c in cases), S)
    try:
        for j, c in enumerate(cases):
            want_sl, w_out, w_ln, w_al = T.translation(oracle, T.MERGED_MODEL, c)
            _same_list(lists[j], int(counts[j]), want_sl, V)
            _same_translation(res[j], (w_out, w_ln, w_al), c.lens)
            o_out, o_ln, _ = own.translate_generated(gen, c.ids, c.lens)
            assert np.array_equal(res[j][1], o_ln) and np.array_equal(res[j][0], o_out), j
    finally:
        own.close()


def _run_many_device(ctx, gen, S, cases):
    keep, args, outs = [], [], []
    for c in cases:
        B, Sj = c.ids.shape
        d_ids, d_len = _dev(c.ids), _dev(c.lens)
        d_out = torch.full((B, _tmax(Sj)), SENTINEL, dtype=torch.int32, device="cuda")
        d_ol = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
        d_al = torch.full((B, _tmax(Sj), Sj), 7.25, dtype=torch.float32, device="cuda")
        keep.append((d_ids, d_len))
        outs.append((d_out, d_ol, d_al))
        args.append((d_ids.data_ptr(), d_len.data_ptr(), B, 0, 0, d_out.data_ptr(), d_ol.data_ptr(), d_al.data_ptr(), Sj))
    torch.cuda.synchronize()
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=_tmax(S), generator=gen)
    ctx.synchronize()
    return [(o.cpu().numpy().view(np.uint32), l.cpu().numpy().view(np.uint32), a.cpu().numpy()) for o, l, a in outs]


def _assert_merged(ctx, S, n):
    """the conditions of a merged launch (slimt_hip_translate_many_*_generated): 2..8 batches, the persistent encoder (sources
    of up to 64 tokens) and decoder; the context was made for the launch's padded rows and S. That the lists then lie V ids
    apart, one per sub-batch, is what debug_shortlists(n) reads."""
    assert 2 <= n <= 8 and ctx.plan(S) == (True, True) and S <= 64


@pytest.mark.parametrize("name", [m[0] for m in T.MERGED])
def test_merged_launch_device(hip, oracle, engines, name):
    S, cases, gm, gen, rows = _merged_setup(hip, engines, name)
    ctx = hip.Context(gm, rows, S)
    try:
        _assert_merged(ctx, S, len(cases))
        for _ in range(2):
            res = _run_many_device(ctx, gen, S, cases)
            _check_merged(hip, oracle, ctx, gm, gen, S, cases, res)
    finally:
        gen.close()
        ctx.close()


@pytest.mark.parametrize("name", ["two", "eight", "eight-one-tile"])
def test_merged_launch_async(hip, oracle, engines, name):
    """slimt_hip_translate_many_async_generated on pinned arrays, read and written in place by the one launch pair"""
    S, cases, gm, gen, rows = _merged_setup(hip, engines, name)
    ctx = hip.Context(gm, rows, S)
    pins, bufs = [], []
    try:
        _assert_merged(ctx, S, len(cases))
        for c in cases:
            B, Sj = c.ids.shape
            ps = [hip._Pinned() for _ in range(5)]
            pins += ps
            b = (ps[0].array(np.uint32, (B, Sj)), ps[1].array(np.uint32, (B,)), ps[2].array(np.uint32, (B, _tmax(Sj))),
                 ps[3].array(np.uint32, (B,)), ps[4].array(np.float32, (B, _tmax(Sj), Sj)))
            b[0][...] = c.ids
            b[1][...] = c.lens
            bufs.append(b)
        for _ in range(2):
            for b in bufs:
                b[2][...] = SENTINEL
                b[3][...] = SENTINEL
                b[4][...] = np.float32(7.25)
            ctx.translate_many_async(bufs, generator=gen)
            ctx.synchronize()
            _check_merged(hip, oracle, ctx, gm, gen, S, cases, [(b[2].copy(), b[3].copy(), b[4].copy()) for b in bufs])
    finally:
        gen.close()
        ctx.close()
        for p in pins:
            p.free()


def test_launch_that_cannot_merge_leaves_the_last_list(hip, oracle, engines):
    """A launch padded to more tokens than the context takes is translated batch by batch (every batch at its own length):
    same translations, and the context holds ONE list, the last batch's, where an unmerged call leaves it."""
    S, cases, gm, gen, rows = _merged_setup(hip, engines, "repeated-word")
    assert max(c.ids.shape[1] for c in cases) == S
    ctx = hip.Context(gm, rows, S)  # max_S = S: a launch padded to S + 1 does not fit
    try:
        res = _run_many_device(ctx, gen, S + 1, cases)
        for j, c in enumerate(cases):
            _same_translation(res[j], T.translation(oracle, T.MERGED_MODEL, c)[1:], c.lens)
        lists, counts = ctx.debug_shortlists(1, with_counts=True)
        _same_list(lists[0], int(counts[0]), T.reference(oracle, cases[-1]), cases[-1].Vt)
        with pytest.raises(hip.SlimtHipError, match="shortlists"):  # no merged launch ever reserved a second count
            ctx.debug_shortlists(2)
    finally:
        gen.close()
        ctx.close()


def test_accessor_reports_the_list_the_output_layer_was_packed_from(hip, oracle, synth_models):
    """slimt_hip_score_async_generated over targets that enumerate the whole vocabulary (V = 517 = 11 x 47): a target outside
    the output layer scores -inf, every other one is finite -- so the -inf entries are exactly the ids debug_shortlists() does
    not list, and that list is the oracle's."""
    from slimt_amd import synth
    V, B, S, Tt = 517, 11, 9, 47
    m = synth.make_model("micro", seed=1234, eos_bias=3.0, dims=(64, 128, 4, 1, 1, V))
    blob = T.lexical(V, V, 24, 4, 51)
    ids, lens = synth.make_batch(V, B, S, seed=52, ragged=True)
    ids = T.padded(blob, V, ids, lens, V)
    want = oracle.OracleShortlist(blob, V, V).generate(ids, lens)
    assert 0 < want.size < V
    t_ids = np.random.default_rng(53).permutation(V).astype(np.uint32).reshape(B, Tt)
    t_len = np.full(B, Tt, np.uint32)
    gm = hip.Model(m)
    ctx = hip.Context(gm, B, S)
    gen = hip.ShortlistGenerator(blob, V, V)
    try:
        for _ in range(2):
            sc = np.full((B, Tt), np.nan, np.float32)
            ctx.score_async((ids, lens, t_ids, t_len, sc, None), generator=gen)
            ctx.synchronize()
            lists, counts = ctx.debug_shortlists(1, with_counts=True)
            _same_list(lists[0], int(counts[0]), want, V)
            listed = np.isin(t_ids, lists[0])
            assert np.array_equal(np.isneginf(sc), ~listed)
            assert np.all(np.isfinite(sc[listed]))
    finally:
        gen.close()
        ctx.close()
        gm.close()


def test_accessor_refusals(hip, oracle, engines):
    name, c = T.model_case(("rows64", "lex", 5, 13, 0))
    want = T.reference(oracle, c)
    B, S = c.ids.shape
    ctx = _open(hip, engines(name), B, S, 64)
    gen = hip.ShortlistGenerator(c.blob, c.Vs, c.Vt)
    try:
        with pytest.raises(hip.SlimtHipError, match="no \\*_generated call yet"):  # nothing generated yet
            ctx.debug_shortlists()
        ctx.translate_generated(gen, c.ids, c.lens)
        for n in (0, 9):
            with pytest.raises(hip.SlimtHipError, match="not in 1..8"):
                ctx.debug_shortlists(n)
        with pytest.raises(hip.SlimtHipError, match="shortlists"):  # one list was generated, not two
            ctx.debug_shortlists(2)
        lists, counts = ctx.debug_shortlists(1, capacity=10, with_counts=True)  # truncated; the count is reported in full
        assert int(counts[0]) == want.size > 10 and np.array_equal(lists[0], want[:10])
        ids = np.full((1, 12), SENTINEL, np.uint32)  # ... and nothing is written behind the capacity
        cnt = np.zeros(1, np.uint32)
        assert hip.lib().slimt_hip_debug_ctx_shortlists(ctx.h, 1, ids.ctypes.data, 10, cnt.ctypes.data) == 0
        assert np.array_equal(ids[0, :10], want[:10]) and np.all(ids[0, 10:] == SENTINEL)
        assert hip.lib().slimt_hip_debug_ctx_shortlists(ctx.h, 1, None, 10, cnt.ctypes.data) != 0
    finally:
        gen.close()
        ctx.close()


# ---- the batch-by-batch fallbacks of slimt_hip_translate_many_async_generated --------------------------------------------------
# Batches of 3 and 5 sentences padded to 4 and 7 tokens (two of them, pinned, are one merged launch: _assert_merged). One
# pageable array among the pinned ones, or more than eight batches, and every batch goes through the host path of a single
# call instead -- with the options armed for the whole call handed on batch by batch.
FALLBACK_SHAPES = [(3, 4), (5, 7)]
FALLBACK_S = 7


def _fallback_inputs(hip, oracle, n, options):
    """n Cases of FALLBACK_SHAPES in turn; with options per batch a forced prefix of 0..2 words of ITS list and sampling keys"""
    from slimt_amd import synth
    blob, Vs = T.generator_blob(T.MERGED_MODEL, T.MERGED_GENERATOR)
    V = T.model_V(T.MERGED_MODEL)
    cases, prefixes, keys = [], [], []
    rng = np.random.default_rng(6)
    for j in range(n):
        B, Sj = FALLBACK_SHAPES[j % 2]
        ids, lens = synth.make_batch(V, B, Sj, seed=640 + j, ragged=True)
        c = T.Case("fallback-%d" % j, blob, Vs, V, T.padded(blob, V, ids, lens, V), lens, False, (), None)
        cases.append(c)
        words = T.reference(oracle, c)
        words = words[words != 0]
        prefixes.append((rng.choice(words, size=(B, _tmax(Sj))).astype(np.uint32), rng.integers(0, 3, size=B).astype(np.uint32)))
        keys.append(hip.sampling_keys(78, B, first=100 * j))
    return cases, (prefixes if options else None), (keys if options else None)


def _fallback_buffers(hip, cases, pageable):
    """per batch (ids, lens, out, out_len, align) and a scores array, pinned; pageable: the last batch's out_len is not"""
    pins, bufs, scs = [], [], []
    for j, c in enumerate(cases):
        B, Sj = c.ids.shape
        ps = [hip._Pinned() for _ in range(6)]
        pins += ps
        b = [ps[0].array(np.uint32, (B, Sj)), ps[1].array(np.uint32, (B,)), ps[2].array(np.uint32, (B, _tmax(Sj))),
             ps[3].array(np.uint32, (B,)), ps[4].array(np.float32, (B, _tmax(Sj), Sj))]
        if pageable and j == len(cases) - 1:
            b[3] = np.zeros((B,), np.uint32)
        b[0][...] = c.ids
        b[1][...] = c.lens
        b[2][...] = SENTINEL
        b[3][...] = SENTINEL
        b[4][...] = np.float32(7.25)
        sc = ps[5].array(np.float32, (B, _tmax(Sj)))
        sc[...] = np.float32(7.5)
        bufs.append(tuple(b))
        scs.append(sc)
    return pins, bufs, scs


def _same_scores(sc, want_sc, ln):
    for r in range(len(ln)):
        assert np.array_equal(sc[r, :ln[r]].view(np.uint32), want_sc[r, :ln[r]].view(np.uint32)), r


@pytest.mark.parametrize("n,pageable,options", [(2, True, False), (9, False, False), (2, True, True), (9, False, True)],
                         ids=["pageable-array", "nine-batches", "pageable-array-options", "nine-batches-options"])
def test_async_fallbacks_equal_the_blocking_calls(hip, oracle, engines, n, pageable, options):
    """slimt_hip_translate_many_async_generated batch by batch == slimt_hip_translate_generated of each batch on the same
    context; with scores, a forced prefix and sampling keys armed together each batch gets its own."""
    cases, prefixes, keys = _fallback_inputs(hip, oracle, n, options)
    gm = engines(T.MERGED_MODEL)
    gen = hip.ShortlistGenerator(cases[0].blob, cases[0].Vs, cases[0].Vt)
    ctx = hip.Context(gm, hip.translate_many_rows([c.ids.shape[0] for c in cases]), FALLBACK_S)
    pins, bufs, scs = _fallback_buffers(hip, cases, pageable)
    try:
        _assert_merged(ctx, FALLBACK_S, 2)
        if options:
            wants = [ctx.translate_generated(gen, c.ids, c.lens, want_align=True, scores=True, prefix=p, sampling=(0.8, k))
                     for c, p, k in zip(cases, prefixes, keys)]
            ctx.translate_many_async(bufs, generator=gen, scores=scs, prefix=prefixes, sampling=(0.8, keys))
        else:
            wants = [ctx.translate_generated(gen, c.ids, c.lens, want_align=True) for c in cases]
            ctx.translate_many_async(bufs, generator=gen)
        ctx.synchronize()
        for b, sc, c, want in zip(bufs, scs, cases, wants):
            _same_translation((b[2], b[3], b[4]), want[:3], c.lens)
            if options:
                _same_scores(sc, want[3], want[1])
    finally:
        gen.close()
        ctx.close()
        for p in pins:
            p.free()


def test_async_failed_guard_consumes_every_armed_option(hip, oracle, engines):
    """Scores armed for three batches, a prefix and sampling for two, a call of two batches: it fails at the scores, and the
    next plain call is an ordinary greedy one -- the prefix and the sampling were taken with the scores."""
    cases, prefixes, keys = _fallback_inputs(hip, oracle, 2, True)
    for _, p_len in prefixes:
        p_len[...] = 2  # (every sentence forced: a prefix left armed would show)
    gm = engines(T.MERGED_MODEL)
    gen = hip.ShortlistGenerator(cases[0].blob, cases[0].Vs, cases[0].Vt)
    ctx = hip.Context(gm, hip.translate_many_rows([c.ids.shape[0] for c in cases]), FALLBACK_S)
    pins, bufs, scs = _fallback_buffers(hip, cases, True)
    try:
        wants = [ctx.translate_generated(gen, c.ids, c.lens, want_align=True) for c in cases]
        ctx.set_scores(scs + [scs[0]])
        ctx.set_target_prefix(prefixes)
        ctx.set_sampling(0.8, keys)
        with pytest.raises(hip.SlimtHipError, match="scores: 3 destinations armed, the call has 2 batches"):
            ctx.translate_many_async(bufs, generator=gen)
        ctx.translate_many_async(bufs, generator=gen)
        ctx.synchronize()
        for b, sc, c, want in zip(bufs, scs, cases, wants):
            _same_translation((b[2], b[3], b[4]), want, c.lens)
            assert (sc == np.float32(7.5)).all()
    finally:
        gen.close()
        ctx.close()
        for p in pins:
            p.free()


def test_device_call_refuses_a_generator_of_another_target_vocabulary(hip, engines):
    """slimt_hip_translate_device_generated checks the generator against the model like the host calls do: refused with their
    message, nothing written."""
    V = T.model_V(T.MERGED_MODEL)
    Vt = V - 3
    gen = hip.ShortlistGenerator(T.lexical(V, Vt, 24, 4, 45), V, Vt)
    B, S = FALLBACK_SHAPES[0]
    ctx = hip.Context(engines(T.MERGED_MODEL), B, S)
    try:
        d_ids = torch.ones((B, S), dtype=torch.int32, device="cuda")
        d_len = torch.full((B,), S, dtype=torch.int32, device="cuda")
        d_out = torch.full((B, _tmax(S)), SENTINEL, dtype=torch.int32, device="cuda")
        d_ol = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
        with pytest.raises(hip.SlimtHipError, match="shortlist target vocabulary %d != model vocabulary %d" % (Vt, V)):
            ctx.translate_device_generated(gen, d_ids.data_ptr(), d_len.data_ptr(), B, S, 1.5, 0, d_out.data_ptr(), d_ol.data_ptr())
        ctx.synchronize()
        assert (d_out.cpu().numpy() == SENTINEL).all() and (d_ol.cpu().numpy() == SENTINEL).all()
    finally:
        gen.close()
        ctx.close()
