"""The 8- and 4-sentence tilings of the fused decoder (decode modes 4 / 5) at D = 256 keep the f32 rows and the SSRU cells at
the size of their live sentences plus four rows that the accumulator lanes of the MFMA rows no wave owns share, and the
attention scratch of the waves that own a sentence; in the LDS that frees they hold the output layer's epilogue constants
of the launch, up to a compile-time capacity (decode_fused.hip, TRIM; kernels.h, fused_decode_lds_bytes). The same
integers go through the same float operations, so every case here compares modes 4 and 5 with mode 2 (16 sentences, the
untouched kernels) token for token, length for length and alignment row for alignment row, and all three with the CPU
oracle (PORTABLE order, as in tests/test_gpu_queue_bound_outputs.py):

  * B in {1, 7, 9, 17}: a partly filled tile, and a second tile with one live row;
  * S in {3, 8, 32} and 33, 65 (the kernels for sentences of 33..64 and 65..128 tokens), short outputs (T <= 12);
  * shortlists of 16, 17, 33 columns (an odd tile count: the pair without a partner), the capacity, capacity + 1,
    capacity + 16 and the full vocabulary -- the resident path, the loading path and the edge between them -- and a
    list generated on the device, whose column count the kernel reads there;
  * the `base` shape (D = 512: the layout is not trimmed there);
  * alignments requested everywhere; an EOS bias of 6 and a narrow list end sentences -- and tiles -- at different steps;
  * several calls on one context with different lists and sizes: the constants are staged per launch.

Without a GPU: fused_decode_lds_bytes stays within the 160 KiB for every shape, tiling and cache form the launcher picks,
and says when the constants are resident."""
import numpy as np
import pytest

CAPACITY = 4096  # kernels.h, kFusedEpiOutTiles = 256 column tiles
EOS_BIAS = 6.0
GEN = dict(frequent=100, best=2, seed=21, empty_fraction=0.3, min_count=1)


def _list(V, n):
    """n sorted ids: EOS and the first few, the rest spread over the whole table"""
    if n >= V:
        return None
    r = np.random.default_rng(900 + n)
    rest = r.choice(np.arange(8, V, dtype=np.uint32), size=n - 8, replace=False)
    return np.sort(np.concatenate([np.arange(8, dtype=np.uint32), rest])).astype(np.uint32)


class World:
    def __init__(self, preset, hip, oracle, synth_models):
        from slimt_amd import synth
        self.hip, self.O = hip, oracle
        self.m = synth_models(preset, EOS_BIAS)
        self.V = self.m.V
        self.om = oracle.OracleModel(self.m, threads=16)
        self.gm = hip.Model(self.m)
        self.blob = self.osl = self.gen = None
        self._synth = synth

    def generator(self):
        if self.gen is None:
            self.blob = self._synth.make_lexical_shortlist(self.V, self.V, GEN["frequent"], GEN["best"], seed=GEN["seed"],
                                                           empty_fraction=GEN["empty_fraction"], min_count=GEN["min_count"])
            self.osl = self.O.OracleShortlist(self.blob, self.V, self.V)
            self.gen = self.hip.ShortlistGenerator(self.blob, self.V, self.V)
        return self.gen

    def close(self):
        if self.gen is not None:
            self.gen.close()
        self.gm.close()

    def batch(self, B, S, seed):
        return self._synth.make_batch(self.V, B, S, seed=seed, ragged=True)

    def expected(self, ids, lens, sl, lf):
        self.O.set_mode(self.O.PORTABLE)
        try:
            return self.om.translate(ids, lens, sl, lf, 0, want_align=True)[:3]
        finally:
            self.O.set_mode(self.O.FAITHFUL)


@pytest.fixture(scope="module")
def worlds(hip, oracle, synth_models):
    cache = {}

    def get(preset):
        if preset not in cache:
            cache[preset] = World(preset, hip, oracle, synth_models)
        return cache[preset]

    yield get
    for w in cache.values():
        w.close()


def _same(name, got, want):
    for what, g, w in zip(("tokens", "lengths", "alignments"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w).astype(g.dtype)
        assert g.shape == w.shape, (name, what, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "%s: %s differ in rows %s" % (
            name, what, np.unique(np.nonzero(g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1))[0])[:8])


def _translate(w, ctx, ids, lens, sl, lf, generated):
    if generated:
        return ctx.translate_generated(w.generator(), ids, lens, lf, 0, want_align=True)[:3]
    return ctx.translate(ids, lens, sl, lf, 0, want_align=True)[:3]


def _check(w, ctxs, B, S, seed, n_list, lf, generated=False):
    """modes 4 and 5 against mode 2, and each against the oracle; the tilings asked for are the ones that ran"""
    ids, lens = w.batch(B, S, seed)
    if generated:
        w.generator()
        sl = w.osl.generate(ids, lens)
    else:
        sl = _list(w.V, n_list)
    want = w.expected(ids, lens, sl, lf)
    assert want[0].shape[1] <= 12, want[0].shape  # (short outputs: the cases stay quick)
    got = {}
    for mode, rows in ((2, 16), (4, 8), (5, 4)):
        got[mode] = _translate(w, ctxs[mode], ids, lens, sl, lf, generated)
        assert ctxs[mode].debug_decoder_plan()["rows"] == rows, (mode, ctxs[mode].debug_decoder_plan())  # the tiling asked for ran
        _same("mode %d against the oracle (B %d S %d list %s)" % (mode, B, S, "generated" if generated else n_list), got[mode], want)
    for mode in (4, 5):
        _same("mode %d against mode 2" % mode, got[mode], got[2])
    return want


@pytest.fixture(scope="module")
def tiny_ctxs(hip, worlds):
    w = worlds("tiny11")
    ctxs = {}
    for mode in (2, 4, 5):
        ctxs[mode] = hip.Context(w.gm, 17, 65)
        ctxs[mode].set_decode_mode(mode)
    yield ctxs
    for c in ctxs.values():
        c.close()


def _lf(S):
    """a length factor with T <= 12"""
    return 1.5 if S <= 8 else 12.0 / S


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 9, 17])
def test_partial_tiles_and_a_tile_with_one_live_row(worlds, tiny_ctxs, B):
    _check(worlds("tiny11"), tiny_ctxs, B, 8, 9100 + B, CAPACITY, _lf(8))


@pytest.mark.gpu
def test_staggered_endings(worlds, tiny_ctxs):
    """a narrow list lets the EOS bias win at different steps: sentences -- and with them tiles -- leave at steps 1, 4, 6, or never"""
    want = _check(worlds("tiny11"), tiny_ctxs, 17, 8, 9117, 17, _lf(8))
    lens = set(want[1].tolist())
    assert len(lens) > 2 and min(lens) < 12 == max(lens), lens


@pytest.mark.gpu
@pytest.mark.parametrize("S", [3, 32, 33, 65])
def test_every_source_length_class(worlds, tiny_ctxs, S):
    _check(worlds("tiny11"), tiny_ctxs, 9, S, 9200 + S, 1024, _lf(S))


@pytest.mark.gpu
@pytest.mark.parametrize("n_list", [16, 17, 33, CAPACITY, CAPACITY + 1, CAPACITY + 16, 1 << 30])
def test_list_sizes_around_the_capacity(worlds, tiny_ctxs, n_list):
    w = worlds("tiny11")
    assert w.V > CAPACITY + 16
    _check(w, tiny_ctxs, 9, 8, 9300 + n_list % 1000, n_list, _lf(8))


@pytest.mark.gpu
def test_a_list_generated_on_the_device(worlds, tiny_ctxs):
    _check(worlds("tiny11"), tiny_ctxs, 9, 8, 9400, 0, _lf(8), generated=True)


@pytest.mark.gpu
def test_the_base_shape(hip, worlds):
    w = worlds("base")
    ctxs = {}
    try:
        for mode in (2, 4, 5):
            ctxs[mode] = hip.Context(w.gm, 9, 8)
            ctxs[mode].set_decode_mode(mode)
        _check(w, ctxs, 9, 8, 9500, 100, _lf(8))
    finally:
        for c in ctxs.values():
            c.close()


@pytest.mark.gpu
def test_two_calls_on_one_context_stage_their_own_constants(worlds, tiny_ctxs):
    """a wide list, a narrow one, the wide one again, a list past the capacity, and the narrow one again: every call's
    results are its own list's"""
    w = worlds("tiny11")
    ctx = tiny_ctxs[4]
    ids, lens = w.batch(9, 8, 9600)
    first = {}
    for n in (CAPACITY, 17, CAPACITY, CAPACITY + 16, 17, 33):
        sl = _list(w.V, n)
        got = ctx.translate(ids, lens, sl, 1.5, 0, want_align=True)[:3]
        if n not in first:
            first[n] = got
            _same("list of %d against the oracle" % n, got, w.expected(ids, lens, sl, 1.5))
        else:
            _same("list of %d, second call" % n, got, first[n])


def _trimmed(D, spw, mid, tight, merged, nt):
    """kernels.h, fused_decode_trimmed, restated: which launches of the 8- and 4-sentence tilings have the trimmed layout"""
    return D == 256 and spw < 16 and not merged and not (nt and spw == 4 and mid == 0 and tight)


def test_the_lds_carve_up_fits_every_tiling():
    """What the launcher asks for (kernels.h, fused_decode_launch_lds_bytes, through slimt_hip_debug_fused_decode_lds_bytes:
    host code) for every shape, tiling, sentence-length class, cache form and kind of launch it can pick stays within
    160 KiB wherever the 16-sentence launch of that kind does; launches without the trimmed layout -- 16 and 32 sentences,
    D = 512, merged ones, the one excluded 4-sentence kernel -- ask for exactly what a 16-sentence (32-sentence) launch
    asks for, with nothing resident; the trimmed ones are smaller before the constants and hold them where they fit; the
    headline's two layers keep everything resident."""
    from slimt_amd import capi
    q = capi.debug_fused_decode_lds_bytes
    limit = 160 * 1024
    epc = 256 // 32 * 16 * 256  # the output layer's pair constants at the capacity
    kinds = [dict(), dict(scores=True), dict(scores=True, forced=True), dict(scores=True, sampled=True),
             dict(scores=True, forced=True, sampled=True)]
    seen_trimmed = seen_excluded = 0
    for D, F in ((256, 1536), (512, 2048)):
        for Ld in (1, 2, 3, 4):
            for mid in ((0, 1, 2) if D == 256 else (0,)):
                for tight in (False, True):
                    for merged in (False, True):
                        for nt in (False, True):
                            for kind in kinds:
                                full = q(D, F, Ld, 16, True, mid, tight, merged=merged, nt=nt, **kind)
                                assert not full["epi_in_lds"]
                                if D == 256 and mid == 0:
                                    r32 = q(D, F, Ld, 32, True, 0, tight, merged=merged, nt=nt, **kind)
                                    assert not r32["epi_in_lds"] and not r32["ln_in_lds"]
                                if full["bytes"] > limit:  # (the launcher refuses the 16-sentence launch: no smaller tiling either)
                                    continue
                                for spw in (8, 4):
                                    r = q(D, F, Ld, spw, True, mid, tight, merged=merged, nt=nt, **kind)
                                    assert r["bytes"] <= limit and r["bytes"] % 16 == 0, (D, Ld, mid, tight, merged, nt, kind, spw, r)
                                    if not _trimmed(D, spw, mid, tight, merged, nt):
                                        assert r == full, (D, Ld, mid, tight, merged, nt, kind, spw, r, full)
                                        seen_excluded += 1
                                    else:
                                        assert r["bytes"] - (epc if r["epi_in_lds"] else 0) < full["bytes"]
                                        before = r["bytes"] - (epc if r["epi_in_lds"] else 0)
                                        assert r["epi_in_lds"] == (before + epc <= limit), (D, Ld, mid, tight, nt, kind, spw, r)
                                        seen_trimmed += 1
    assert seen_trimmed > 100 and seen_excluded > 100
    for spw in (8, 4):
        for mid in (0, 1, 2):
            for tight in (False, True):
                for nt in (False, True):
                    r = q(256, 1536, 2, spw, True, mid, tight, nt=nt)
                    want = _trimmed(256, spw, mid, tight, False, nt)
                    assert r["epi_in_lds"] == want and (mid != 0 or r["ln_in_lds"]), (spw, mid, tight, nt, r)
    # the 16-sentence layout is what it was (the headline's 16 rows at 152.3 KiB); the headline's 8-sentence launch
    assert q(256, 1536, 2, 16, True, 0, True)["bytes"] == 155968
    assert q(256, 1536, 2, 8, True, 0, True) == dict(bytes=159872, ln_in_lds=True, epi_in_lds=True)
    assert q(256, 1536, 2, 4, True, 0, True, nt=True) == q(256, 1536, 2, 16, True, 0, True, nt=True)  # the excluded kernel
