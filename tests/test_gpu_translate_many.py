"""GPU parity of slimt_hip_translate_many_* (include/slimt_hip.h): several batches of one padded source length in ONE
encoder and ONE decoder launch -- what `workers` concurrent Model::forward calls are in the reference
(slimt/Frontend.cc:207-227, Batcher.cc:95-120). Every batch's tokens, lengths and alignment rows must equal those of its
own unmerged call AND the CPU oracle's (PORTABLE order): bit for bit, with staggered EOS, a short last batch, batch sizes
that leave holes between the sub-batches, one shared or several distinct shortlists, the full vocabulary, every decoder
tiling and every encoder."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _want(oracle, om, ids, lens, sl):
    oracle.set_mode(oracle.PORTABLE)
    out = om.translate(ids, lens, sl, 1.5, 0, want_align=True)[:3]
    oracle.set_mode(oracle.FAITHFUL)
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _run_many_device(hip, gm, batches, S, sls, mode=0, enc_rows=0, want_align=True, max_rows=None):
    """batches: [(ids, lens)] -- each padded to its own length <= S --, sls: per batch a shortlist array or None.
    Returns per batch (out, len, align)."""
    T_launch = max(int(np.float32(1.5) * np.float32(S)), 1)
    rows = hip.translate_many_rows([b[0].shape[0] for b in batches])
    ctx = hip.Context(gm, max_rows or rows, S)
    ctx.set_decode_mode(mode)
    if enc_rows:
        ctx.set_encode_rows(enc_rows)
    keep, args, outs = [], [], []
    sl_dev = {}
    for (ids, lens), sl in zip(batches, sls):
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        d_ids, d_len = _dev(ids), _dev(lens)
        if sl is not None and id(sl) not in sl_dev:
            sl_dev[id(sl)] = _dev(sl)
        d_sl = sl_dev.get(id(sl))
        d_out = torch.full((B, T), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_ol = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_al = torch.full((B, T, Sj), 7.25, dtype=torch.float32, device="cuda") if want_align else None
        keep.append((d_ids, d_len, d_sl))
        outs.append((d_out, d_ol, d_al))
        args.append((d_ids.data_ptr(), d_len.data_ptr(), B, d_sl.data_ptr() if d_sl is not None else 0,
                     0 if sl is None else sl.size, d_out.data_ptr(), d_ol.data_ptr(), d_al.data_ptr() if want_align else 0, Sj))
    ctx.translate_many_device(args, S, 1.5, 0, steps_hint=T_launch)
    ctx.synchronize()
    res = [(o.cpu().numpy().view(np.uint32), l.cpu().numpy().view(np.uint32), None if a is None else a.cpu().numpy())
           for o, l, a in outs]
    ctx.close()
    return res


def _check(oracle, om, batches, sls, res):
    for j, ((ids, lens), sl, (out, ln, al)) in enumerate(zip(batches, sls, res)):
        w_out, w_ln, w_al = _want(oracle, om, ids, lens, sl)
        assert np.array_equal(ln, w_ln), (j, ln, w_ln)
        assert np.array_equal(out, w_out), j
        if al is not None:
            assert np.array_equal(al, w_al), j


# sizes: multiples of 32 (no holes), sizes that leave holes, a short last batch, one batch alone (k = 1: the plain call)
@pytest.mark.parametrize("preset,S,sizes,n_sl,mode,enc_rows", [
    ("tiny11", 32, [64, 64, 64, 64], 2048, 0, 0),      # BASELINE config 2's batches, four per launch
    ("tiny11", 32, [64, 64, 64, 64], 2048, 2, 64),     # 16 sentences per decoder workgroup, 64-row encoder
    ("tiny11", 32, [64, 64, 10], 1024, 0, 0),          # a short last batch
    ("tiny11", 24, [33, 5, 47, 16, 1, 20, 31, 64], 1024, 0, 0),  # eight batches, holes everywhere
    ("tiny11", 13, [19, 45], 1024, 4, 32),             # 8 sentences per workgroup, 32-row encoder
    ("tiny11", 13, [19, 45], 1024, 5, 0),              # 4 sentences per workgroup
    ("tiny11", 20, [40, 24], 0, 3, 0),                 # the full vocabulary, 32 sentences per workgroup
    ("tiny11", 40, [7, 9, 3], 1024, 0, 0),             # 33..64 tokens: one sentence per encoder workgroup
    ("tiny11", 32, [50], 1024, 0, 0),                  # k = 1
    ("base", 32, [19, 32, 6], 1024, 0, 0),             # D = 512
    ("base", 10, [6, 40], 512, 0, 0),
])
def test_merged_batches_equal_their_own_calls_and_the_oracle(hip, oracle, engines, preset, S, sizes, n_sl, mode, enc_rows):
    from slimt_amd import synth
    m, gm, om = engines(preset, 6.0)  # eos_bias 6: sentences end at different steps
    sl = synth.make_shortlist(m.V, n_sl) if n_sl else None
    batches = [synth.make_batch(m.V, B, S, seed=1000 * j + 7 * B + S, ragged=True) for j, B in enumerate(sizes)]
    sls = [sl] * len(sizes)
    res = _run_many_device(hip, gm, batches, S, sls, mode, enc_rows)
    _check(oracle, om, batches, sls, res)
    # ... and the unmerged call of each batch gives the same (the oracle check above implies it; this is the direct statement)
    ctx = hip.Context(gm, max(sizes), S)
    ctx.set_decode_mode(mode)
    for (ids, lens), (out, ln, al) in zip(batches, res):
        o1, l1, a1 = ctx.translate(ids, lens, sl, want_align=True)
        assert np.array_equal(o1, out) and np.array_equal(l1, ln) and np.array_equal(a1, al)
    ctx.close()


@pytest.mark.parametrize("preset,S,shapes,n_sl,mode", [
    ("tiny11", 32, [(40, 32), (33, 27), (64, 26), (9, 32)], 1024, 0),   # padded to fewer tokens than the launch
    ("tiny11", 24, [(20, 19), (50, 24), (31, 22)], 1024, 2),
    ("tiny11", 16, [(64, 13), (64, 16)], 0, 0),
    ("tiny11", 48, [(5, 40), (7, 48), (4, 35)], 512, 0),               # 33..64 tokens
    ("base", 32, [(19, 32), (12, 25)], 512, 0),
])
def test_merged_batches_with_their_own_padded_lengths(hip, oracle, engines, preset, S, shapes, n_sl, mode):
    """A batch padded to fewer tokens than the launch keeps the step limit and the alignment width of ITS length
    (Model.cc:159-161, 84-108): outputs == the oracle on that batch at its own padded length, and == its own call."""
    from slimt_amd import synth
    m, gm, om = engines(preset, 6.0)
    sl = synth.make_shortlist(m.V, n_sl) if n_sl else None
    batches = [synth.make_batch(m.V, B, Sj, seed=400 + 13 * j + B, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    sls = [sl] * len(shapes)
    res = _run_many_device(hip, gm, batches, S, sls, mode)
    _check(oracle, om, batches, sls, res)
    ctx = hip.Context(gm, max(b for b, _ in shapes), S)
    ctx.set_decode_mode(mode)
    for (ids, lens), (out, ln, al) in zip(batches, res):
        o1, l1, a1 = ctx.translate(ids, lens, sl, want_align=True)
        assert np.array_equal(o1, out) and np.array_equal(l1, ln) and np.array_equal(a1, al)
    ctx.close()


def test_merged_batches_with_their_own_shortlists(hip, oracle, engines):
    """Model.cc:117-120: a batch's shortlist is ITS shortlist -- three batches, three lists of different sizes (two batches
    share one: one packed output layer for both)."""
    from slimt_amd import synth
    m, gm, om = engines("tiny11", 6.0)
    S = 16
    slA, slB, slC = synth.make_shortlist(m.V, 1024, seed=1), synth.make_shortlist(m.V, 1536, seed=2), synth.make_shortlist(m.V, 520, seed=3)
    sizes = [33, 20, 64, 12]
    sls = [slA, slB, slA, slC]
    batches = [synth.make_batch(m.V, B, S, seed=50 + j, ragged=True) for j, B in enumerate(sizes)]
    for mode in (0, 2):
        res = _run_many_device(hip, gm, batches, S, sls, mode)
        _check(oracle, om, batches, sls, res)


def test_merged_launch_falls_back_batch_by_batch(hip, oracle, engines):
    """More than eight batches, sources past 64 tokens, a context too small for the merged rows: translated one by one,
    in order, on the same stream -- same results."""
    from slimt_amd import synth
    m, gm, om = engines("tiny11", 6.0)
    sl = synth.make_shortlist(m.V, 1024)
    batches = [synth.make_batch(m.V, 5 + j, 12, seed=90 + j, ragged=True) for j in range(10)]
    res = _run_many_device(hip, gm, batches, 12, [sl] * 10, max_rows=32)
    _check(oracle, om, batches, [sl] * 10, res)
    batches = [synth.make_batch(m.V, 3, 70, seed=70 + j, ragged=True) for j in range(2)]
    res = _run_many_device(hip, gm, batches, 70, [sl] * 2)
    _check(oracle, om, batches, [sl] * 2, res)
    batches = [synth.make_batch(m.V, 30, 12, seed=10 + j, ragged=True) for j in range(3)]
    res = _run_many_device(hip, gm, batches, 12, [sl] * 3, max_rows=40)  # 96 merged rows do not fit 40
    _check(oracle, om, batches, [sl] * 3, res)


@pytest.mark.parametrize("preset,S,sizes,n_sl", [("tiny11", 32, [64, 40, 64], 2048), ("tiny11", 13, [7, 33], None),
                                                   ("base", 32, [19, 19], 1024), ("tiny11", 30, [(20, 26), (33, 30), (8, 25)], 1024)])
def test_merged_pinned_async(hip, oracle, engines, preset, S, sizes, n_sl):
    """slimt_hip_translate_many_async: pinned host arrays per batch, read and written in place by the two launches;
    alignment rows staged in device memory and copied out per sentence (Model.cc:84-108)."""
    from slimt_amd import synth
    m, gm, om = engines(preset, 6.0)
    sl = None if n_sl is None else synth.make_shortlist(m.V, n_sl)
    sizes = [x if isinstance(x, tuple) else (x, S) for x in sizes]  # (B, this batch's own padded length)
    batches = [synth.make_batch(m.V, B, Sj, seed=300 + 11 * j + B, ragged=True) for j, (B, Sj) in enumerate(sizes)]
    ctx = hip.Context(gm, hip.translate_many_rows([b for b, _ in sizes]), S)
    pins, bufs = [], []
    for ids, lens in batches:
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        ps = [hip._Pinned() for _ in range(5)]
        b = (ps[0].array(np.uint32, (B, Sj)), ps[1].array(np.uint32, (B,)), ps[2].array(np.uint32, (B, T)),
             ps[3].array(np.uint32, (B,)), ps[4].array(np.float32, (B, T, Sj)))
        b[0][...] = ids
        b[1][...] = lens
        pins.append(ps)
        bufs.append(b)
    for rep in range(2):
        for b in bufs:
            b[2][...] = 0x5a5a5a5a
            b[3][...] = 0x5a5a5a5a
            b[4][...] = np.float32(7.25)
        ctx.translate_many_async(bufs, sl)
        ctx.synchronize()
        res = [(b[2].copy(), b[3].copy(), b[4].copy()) for b in bufs]
        _check(oracle, om, batches, [sl] * len(sizes), res)
    ctx.close()
    for ps in pins:
        for p in ps:
            p.free()


def test_merged_headline_shape_full_size(hip, oracle, engines):
    """BASELINE config 2 at full size: four batches of 64 sentences of 32 tokens, shortlist 4096, merged -- against the
    unmerged calls (bit for bit) with nobody emitting EOS (T = 48 for all) and with staggered endings."""
    from slimt_amd import synth
    for eos_bias in (-100.0, 6.0):
        m, gm, om = engines("tiny11", eos_bias)
        sl = synth.make_shortlist(m.V, 4096)
        batches = [synth.make_batch(m.V, 64, 32, seed=4321 + j) for j in range(4)]
        res = _run_many_device(hip, gm, batches, 32, [sl] * 4)
        ctx = hip.Context(gm, 64, 32)
        for (ids, lens), (out, ln, al) in zip(batches, res):
            o1, l1, a1 = ctx.translate(ids, lens, sl, want_align=True)
            assert np.array_equal(o1, out) and np.array_equal(l1, ln) and np.array_equal(a1, al)
        ctx.close()
        if eos_bias > 0:
            _check(oracle, om, batches[:1], [sl], res[:1])


@pytest.mark.parametrize("preset,S,shapes,mode", [
    ("tiny11", 24, [(33, 24), (20, 20), (47, 24), (5, 19)], 0),
    ("tiny11", 16, [(64, 16), (64, 16), (10, 13)], 2),
    ("base", 32, [(19, 32), (12, 27)], 0),
    ("tiny11", 2, [(3, 2)] * 8, 0),   # eight shortlists, one encoder tile: the workgroup of tile 0 generates all of them
])
def test_merged_batches_generate_their_own_lexical_shortlists(hip, oracle, engines, preset, S, shapes, mode):
    """Model.cc:117-120 per batch, merged: every batch's output vocabulary is ShortlistGenerator::generate of ITS source
    words, produced by one of the first workgroups of the ONE encoder launch; tokens, lengths and alignment rows == the
    checker's on that batch with the checker's own shortlist for it -- and the lists really differ between the batches."""
    from slimt_amd import synth
    m, gm, om = engines(preset, 6.0)
    blob = synth.make_lexical_shortlist(m.V, m.V, 100, 2, seed=21, empty_fraction=0.3, min_count=1)
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    batches = [synth.make_batch(m.V, B, Sj, seed=700 + 17 * j + B, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    sls = [osl.generate(ids, lens) for ids, lens in batches]
    assert len({tuple(s_) for s_ in sls}) > 1
    rows = hip.translate_many_rows([b for b, _ in shapes])
    ctx = hip.Context(gm, rows, S)
    ctx.set_decode_mode(mode)
    keep, args, outs = [], [], []
    for ids, lens in batches:
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        d_ids, d_len = _dev(ids), _dev(lens)
        d_out = torch.full((B, T), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_ol = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_al = torch.full((B, T, Sj), 7.25, dtype=torch.float32, device="cuda")
        keep.append((d_ids, d_len))
        outs.append((d_out, d_ol, d_al))
        args.append((d_ids.data_ptr(), d_len.data_ptr(), B, 0, 0, d_out.data_ptr(), d_ol.data_ptr(), d_al.data_ptr(), Sj))
    for rep in range(2):
        ctx.translate_many_device(args, S, 1.5, 0, steps_hint=max(int(np.float32(1.5) * np.float32(S)), 1), generator=gen)
        ctx.synchronize()
        res = [(o.cpu().numpy().view(np.uint32), l.cpu().numpy().view(np.uint32), a.cpu().numpy()) for o, l, a in outs]
        _check(oracle, om, batches, sls, res)
    ctx.close()
    gen.close()


# ---- the batch-by-batch fallbacks of slimt_hip_translate_many_async -------------------------------------------------------
# Batches of 3 and 5 sentences padded to 4 and 7 tokens (two of them, pinned, are one merged launch: the tests above). One
# pageable array among the pinned ones, or more than eight batches, and every batch goes through the host path of a single
# call instead -- with the options armed for the whole call handed on batch by batch.
FALLBACK_SHAPES = [(3, 4), (5, 7)]
FALLBACK_S = 7


def _fallback_inputs(V, n, sl, options):
    """n batches of FALLBACK_SHAPES in turn; with options per batch a forced prefix of 0..2 listed words and sampling keys"""
    from slimt_amd import capi, synth
    shapes = [FALLBACK_SHAPES[j % 2] for j in range(n)]
    batches = [synth.make_batch(V, B, Sj, seed=600 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    if not options:
        return batches, None, None
    rng = np.random.default_rng(5)
    words = sl[sl != 0]
    prefixes, keys = [], []
    for j, (B, Sj) in enumerate(shapes):
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        prefixes.append((rng.choice(words, size=(B, T)).astype(np.uint32), rng.integers(0, 3, size=B).astype(np.uint32)))
        keys.append(capi.sampling_keys(77, B, first=100 * j))
    return batches, prefixes, keys


def _fallback_buffers(hip, batches, pageable):
    """per batch (ids, lens, out, out_len, align) and a scores array, pinned; pageable: the last batch's out_len is not"""
    pins, bufs, scs = [], [], []
    for j, (ids, lens) in enumerate(batches):
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        ps = [hip._Pinned() for _ in range(6)]
        pins += ps
        b = [ps[0].array(np.uint32, (B, Sj)), ps[1].array(np.uint32, (B,)), ps[2].array(np.uint32, (B, T)),
             ps[3].array(np.uint32, (B,)), ps[4].array(np.float32, (B, T, Sj))]
        if pageable and j == len(batches) - 1:
            b[3] = np.zeros((B,), np.uint32)
        b[0][...] = ids
        b[1][...] = lens
        b[2][...] = 0x5a5a5a5a
        b[3][...] = 0x5a5a5a5a
        b[4][...] = np.float32(7.25)
        sc = ps[5].array(np.float32, (B, T))
        sc[...] = np.float32(7.5)
        bufs.append(tuple(b))
        scs.append(sc)
    return pins, bufs, scs


def _same_as_own_call(b, sc, lens, want):
    """ids and lengths, the alignment over each sentence's own columns and rows, the scores of its tokens: bit for bit"""
    assert np.array_equal(b[3], want[1]), (b[3], want[1])
    assert np.array_equal(b[2], want[0])
    for r in range(len(lens)):
        n, L = int(want[1][r]), int(lens[r])
        assert np.array_equal(b[4][r, :n, :L].view(np.uint32), want[2][r, :n, :L].view(np.uint32)), r
        if sc is not None:
            assert np.array_equal(sc[r, :n].view(np.uint32), want[3][r, :n].view(np.uint32)), r


@pytest.mark.parametrize("n,pageable,options", [(2, True, False), (9, False, False), (2, True, True), (9, False, True)],
                         ids=["pageable-array", "nine-batches", "pageable-array-options", "nine-batches-options"])
def test_async_fallbacks_equal_the_blocking_calls(hip, engines, n, pageable, options):
    """slimt_hip_translate_many_async batch by batch == slimt_hip_translate of each batch on the same context; with scores, a
    forced prefix and sampling keys armed together each batch gets its own."""
    from slimt_amd import synth
    m, gm, _ = engines("tiny11", 6.0)
    sl = synth.make_shortlist(m.V, 1024)
    batches, prefixes, keys = _fallback_inputs(m.V, n, sl, options)
    ctx = hip.Context(gm, hip.translate_many_rows([ids.shape[0] for ids, _ in batches]), FALLBACK_S)
    pins, bufs, scs = _fallback_buffers(hip, batches, pageable)
    try:
        assert ctx.plan(FALLBACK_S) == (True, True)
        if options:
            wants = [ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p, sampling=(0.8, k))
                     for (ids, lens), p, k in zip(batches, prefixes, keys)]
            ctx.translate_many_async(bufs, sl, scores=scs, prefix=prefixes, sampling=(0.8, keys))
        else:
            wants = [ctx.translate(ids, lens, sl, want_align=True) for ids, lens in batches]
            ctx.translate_many_async(bufs, sl)
        ctx.synchronize()
        for b, sc, (_, lens), want in zip(bufs, scs, batches, wants):
            _same_as_own_call(b, sc if options else None, lens, want)
    finally:
        ctx.close()
        for p in pins:
            p.free()


def _many_device_with_options(ctx, batches, sls, prefixes, keys, steps_hint, generator=None):
    """slimt_hip_translate_many_device[_generated] with scores, a forced prefix and sampling keys armed together, every
    array in device memory; per batch (None, None, out, out_len, align) as _same_as_own_call reads them, and the scores"""
    keep, args, outs, d_scs, d_pre, d_keys = [], [], [], [], [], []
    for (ids, lens), sl, (p_ids, p_len), k in zip(batches, sls, prefixes, keys):
        B, Sj = ids.shape
        T = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        d_ids, d_len, d_sl = _dev(ids), _dev(lens), None if sl is None else _dev(sl)
        d_out = torch.full((B, T), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_ol = torch.full((B,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_al = torch.full((B, T, Sj), 7.25, dtype=torch.float32, device="cuda")
        d_sc = torch.full((B, T), 7.5, dtype=torch.float32, device="cuda")
        d_pi, d_pl = _dev(p_ids), _dev(p_len)
        d_k = torch.from_numpy(np.ascontiguousarray(k).view(np.int64)).cuda()
        keep.append((d_ids, d_len, d_sl, d_pi, d_pl, d_k))
        outs.append((d_out, d_ol, d_al, d_sc))
        d_scs.append(d_sc.data_ptr())
        d_pre.append((d_pi.data_ptr(), d_pl.data_ptr()))
        d_keys.append(d_k.data_ptr())
        args.append((d_ids.data_ptr(), d_len.data_ptr(), B, 0 if d_sl is None else d_sl.data_ptr(), 0 if sl is None else sl.size,
                     d_out.data_ptr(), d_ol.data_ptr(), d_al.data_ptr(), Sj))
    ctx.translate_many_device(args, FALLBACK_S, 1.5, 0, steps_hint=steps_hint, generator=generator, scores=d_scs, prefix=d_pre,
                              sampling=(0.8, d_keys))
    ctx.synchronize()
    return [((None, None, o.cpu().numpy().view(np.uint32), l.cpu().numpy().view(np.uint32), a.cpu().numpy()), s.cpu().numpy())
            for o, l, a, s in outs]


def test_device_fallback_hands_each_batch_its_options(hip, engines):
    """slimt_hip_translate_many_device with a listed shortlist, nine batches (batch by batch): with scores, a forced prefix
    and sampling keys armed together in device memory, each batch == slimt_hip_translate of it on the same context."""
    from slimt_amd import synth
    m, gm, _ = engines("tiny11", 6.0)
    sl = synth.make_shortlist(m.V, 1024)
    batches, prefixes, keys = _fallback_inputs(m.V, 9, sl, True)
    ctx = hip.Context(gm, hip.translate_many_rows([ids.shape[0] for ids, _ in batches]), FALLBACK_S)
    try:
        assert ctx.plan(FALLBACK_S) == (True, True)
        wants = [ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p, sampling=(0.8, k))
                 for (ids, lens), p, k in zip(batches, prefixes, keys)]
        res = _many_device_with_options(ctx, batches, [sl] * 9, prefixes, keys, 0)
        for (b, sc), (_, lens), want in zip(res, batches, wants):
            _same_as_own_call(b, sc, lens, want)
    finally:
        ctx.close()


def test_device_generated_unmerged_hands_each_batch_its_options(hip, oracle, engines):
    """slimt_hip_translate_many_device_generated, nine batches (its unmerged device branch), with the same three options in
    device memory: each batch == slimt_hip_translate_generated of it on the same context. A prefix holds words of ITS list."""
    from slimt_amd import synth
    from support import shortlist_cases as T
    m, gm, _ = engines("tiny11", 6.0)
    blob = T.lexical(m.V, m.V, *T.GENERATORS[T.MERGED_GENERATOR][1:])
    osl = oracle.OracleShortlist(blob, m.V, m.V)
    gen = hip.ShortlistGenerator(blob, m.V, m.V)
    shapes = [FALLBACK_SHAPES[j % 2] for j in range(9)]
    batches = [synth.make_batch(m.V, B, Sj, seed=600 + j, ragged=True) for j, (B, Sj) in enumerate(shapes)]
    rng = np.random.default_rng(5)
    prefixes, keys = [], []
    for j, ((ids, lens), (B, Sj)) in enumerate(zip(batches, shapes)):
        words = osl.generate(ids, lens)
        words = words[words != 0]
        T_j = max(int(np.float32(1.5) * np.float32(Sj)), 1)
        prefixes.append((rng.choice(words, size=(B, T_j)).astype(np.uint32), rng.integers(0, 3, size=B).astype(np.uint32)))
        keys.append(hip.sampling_keys(77, B, first=100 * j))
    ctx = hip.Context(gm, hip.translate_many_rows([B for B, _ in shapes]), FALLBACK_S)
    try:
        assert ctx.plan(FALLBACK_S) == (True, True)
        wants = [ctx.translate_generated(gen, ids, lens, want_align=True, scores=True, prefix=p, sampling=(0.8, k))
                 for (ids, lens), p, k in zip(batches, prefixes, keys)]
        res = _many_device_with_options(ctx, batches, [None] * 9, prefixes, keys, max(int(np.float32(1.5) * np.float32(FALLBACK_S)), 1),
                                        generator=gen)
        for (b, sc), (_, lens), want in zip(res, batches, wants):
            _same_as_own_call(b, sc, lens, want)
    finally:
        gen.close()
        ctx.close()


def test_async_failed_guard_consumes_every_armed_option(hip, engines):
    """Scores armed for three batches, a prefix and sampling for two, a call of two batches: it fails at the scores, and the
    next plain call is an ordinary greedy one -- the prefix and the sampling were taken with the scores."""
    from slimt_amd import synth
    m, gm, _ = engines("tiny11", 6.0)
    sl = synth.make_shortlist(m.V, 1024)
    batches, prefixes, keys = _fallback_inputs(m.V, 2, sl, True)
    for _, p_len in prefixes:
        p_len[...] = 2  # (every sentence forced: a prefix left armed would show)
    ctx = hip.Context(gm, hip.translate_many_rows([ids.shape[0] for ids, _ in batches]), FALLBACK_S)
    pins, bufs, scs = _fallback_buffers(hip, batches, True)
    try:
        wants = [ctx.translate(ids, lens, sl, want_align=True) for ids, lens in batches]
        ctx.set_scores(scs + [scs[0]])
        ctx.set_target_prefix(prefixes)
        ctx.set_sampling(0.8, keys)
        with pytest.raises(hip.SlimtHipError, match="scores: 3 destinations armed, the call has 2 batches"):
            ctx.translate_many_async(bufs, sl)
        ctx.translate_many_async(bufs, sl)
        ctx.synchronize()
        for b, sc, (_, lens), want in zip(bufs, scs, batches, wants):
            _same_as_own_call(b, None, lens, want)
            assert (sc == np.float32(7.5)).all()
    finally:
        ctx.close()
        for p in pins:
            p.free()
