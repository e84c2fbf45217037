"""GPU parity over the FAMILY of model shapes slimt_hip_model_create accepts, not only the four presets: every shape of
tests/support/model_shapes.py (FFN sizes, head counts and layer counts no preset has; vocabularies that are no multiple of
8; the shapes next to the tuned ones, where a dispatch predicate one condition short would run a kernel on a shape it was
not written for) against the oracle's PORTABLE order, bit for bit -- encoder layer by layer, decoder steps teacher-forced,
greedy translation -- together with the plan (which kernels ran) the shape is documented to take, and the shapes that
model_create refuses."""
import numpy as np
import pytest

from support import model_shapes as T

pytestmark = pytest.mark.gpu

CASES = [pytest.param(s, B, S, id="%s-B%d-S%d" % (T.shape_id(s), B, S)) for s in T.SHAPES for B, S in T.cases(s)]

@pytest.fixture(scope="module")
def shape_engines(hip, oracle):
    """(synthetic model, device model, oracle model) per shape, created once for the module."""
    cache = {}

    def get(s):
        if s.dims not in cache:
            m = T.make(s)
            cache[s.dims] = (m, hip.Model(m), oracle.OracleModel(m))
        return cache[s.dims]

    try:
        yield get
    finally:
        for _, gm, _ in cache.values():
            gm.close()


def encoder_reference(oracle, om, m, ids, lens, S):
    oracle.set_mode(oracle.PORTABLE)
    try:
        mask = oracle.make_mask(lens, S)
        want = [om.embed(ids)]
        for l in range(1, m.enc_layers + 1):
            want.append(om.encoder_layer(l, want[-1], mask))
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    return want, mask


@pytest.mark.parametrize("s,B,S", CASES)
def test_plan_is_the_documented_one(hip, shape_engines, s, B, S):
    """slimt_hip_ctx_plan against the table's hand-written expectation: a predicate widened or narrowed by one condition
    fails here, on the host, before anything is launched."""
    _, gm, _ = shape_engines(s)
    ctx = hip.Context(gm, B, S)
    try:
        for mode in (0, 1, 2):
            ctx.set_decode_mode(mode)
            assert ctx.plan(S) == T.expected_plan(s, S, mode), (T.shape_id(s), S, mode)
    finally:
        ctx.close()


@pytest.mark.parametrize("s,B,S", CASES)
def test_encoder_every_layer_bit_exact(hip, oracle, shape_engines, s, B, S):
    m, gm, om = shape_engines(s)
    ids, lens = T.batch(s, B, S)
    want, _ = encoder_reference(oracle, om, m, ids, lens, S)
    ctx = hip.Context(gm, B, S)
    try:
        # decode mode 0 / 1: the persistent encoder where the shape has one / the per-stage kernels; where mode 0 is a
        # persistent encoder, its 32- and 64-row tilings as well (a shape without the 64-row one keeps the other)
        runs = [(0, 0), (1, 0)]
        if T.expected_plan(s, S)[0]:
            runs += [(0, 32), (0, 64)]
        for mode, rows in runs:
            ctx.set_decode_mode(mode)
            ctx.set_encode_rows(rows)
            enc, emb, layers = ctx.encode(ids, lens, want_embed=True, want_layers=True)
            assert np.array_equal(emb, want[0]), (mode, rows)
            for l in range(1, m.enc_layers + 1):
                assert np.array_equal(layers[l - 1], want[l]), (mode, rows, l, np.abs(layers[l - 1] - want[l]).max())
            assert np.array_equal(enc, want[-1]), (mode, rows)
    finally:
        ctx.close()


@pytest.mark.parametrize("s,B,S", CASES)
def test_decoder_steps_teacher_forced_bit_exact(hip, oracle, shape_engines, s, B, S):
    """Five Decoder::step calls with random previous tokens: SSRU states, last-layer attention and logits, over a shortlist
    whose size is no multiple of 64 and over the full vocabulary (N = 517, 1003: no multiple of 8)."""
    from slimt_amd import synth
    m, gm, om = shape_engines(s)
    ids, lens = T.batch(s, B, S, salt=1)
    ctx = hip.Context(gm, B, S)
    try:
        enc, _, _ = ctx.encode(ids, lens)
        # the oracle's steps start from the ORACLE's encoder output, which the device's must equal first
        want_enc, mask = encoder_reference(oracle, om, m, ids, lens, S)
        assert np.array_equal(enc, want_enc[-1])
        enc = want_enc[-1]
        for sl in (synth.make_shortlist(m.V, T.SHORTLIST), None):
            ctx.decode_begin(sl)
            oracle.set_mode(oracle.PORTABLE)
            states = np.zeros((m.dec_layers, B, m.D), dtype=np.float32)
            r = np.random.Generator(np.random.PCG64(5))
            prev = None
            for t in range(5):
                want_logits, want_attn = om.decode_step(enc, mask, states, prev, sl)
                logits, attn, st = ctx.decode_step(prev)
                assert np.array_equal(st, states), (sl is None, t, np.abs(st - states).max())
                assert np.array_equal(attn, want_attn), (sl is None, t)
                assert np.array_equal(logits, want_logits), (sl is None, t, np.abs(logits - want_logits).max())
                prev = r.choice(np.arange(m.V) if sl is None else sl, size=B).astype(np.uint32)
            oracle.set_mode(oracle.FAITHFUL)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
        ctx.close()


@pytest.mark.parametrize("s,B,S", CASES)
def test_translate_tokens_lengths_alignments(hip, oracle, shape_engines, s, B, S):
    """Model::forward in decode modes 0 (automatic), 1 (per-stage kernels) and 2 (persistent decoder, 16 sentences per
    workgroup, where the shape has it); a shape with the packed K/V cache in cache formats 0, 2 and 1 on a device model of
    this test's own (which form a sentence takes depends on the model's calibration state). Every case of the grid: the
    CPU fixture test keeps these batches from being degenerate, except S = 1 (one step) and the few T.DEGENERATE lists."""
    m, gm, om = shape_engines(s)
    ids, lens, sl, w_out, w_ln, w_al, _ = T.translate_reference(oracle, om, s, B, S)
    own = hip.Model(m) if s.packed else None
    ctx = hip.Context(own or gm, B, S)
    try:
        for fmt in ((0, 2, 1) if s.packed else (None,)):
            if fmt is not None:
                own.set_kv_cache_format(fmt)
            for mode in (0, 1, 2):
                ctx.set_decode_mode(mode)
                out, ln, al = ctx.translate(ids, lens, sl, limit_factor=1.5, eos_id=0, want_align=True)
                assert np.array_equal(ln, w_ln), (fmt, mode, ln, w_ln)
                assert np.array_equal(out, w_out), (fmt, mode)
                assert np.array_equal(al, w_al), (fmt, mode)
    finally:
        ctx.close()
        if own:
            own.close()


# (D, F, H) that slimt_hip_model_create refuses, and the size its message names. The first six are the edges of the documented
# limits; the others are shapes the per-stage kernels have no instantiation for (include/slimt_hip.h, slimt_hip_model_create).
REJECTED = [
    ((96, 128, 2), "embedding size 96"), ((576, 2048, 9), "embedding size 576"),
    ((512, 2048, 4), "head count 4"), ((256, 1536, 3), "head count 3"),
    ((64, 100, 4), "ffn size 100"), ((256, 4160, 8), "ffn size 4160"),
    ((192, 320, 8), "embedding size 192"), ((320, 704, 5), "embedding size 320"),
    ((384, 1024, 8), "embedding size 384"), ((448, 64, 7), "embedding size 448"),
    ((128, 256, 16), "head count 16"), ((256, 1536, 32), "head count 32"), ((512, 2048, 32), "head count 32"),
    ((256, 1536, 2), "head count 2"), ((256, 4096, 8), "ffn size 4096"), ((256, 2112, 8), "ffn size 2112"),
]


@pytest.mark.parametrize("dfh,names", REJECTED, ids=["D%d-F%d-H%d" % d for d, _ in REJECTED])
def test_model_create_refuses_unsupported_shapes(hip, dfh, names):
    """Host-side argument checks only: a parameter list goes in, an error naming the offending size comes back, nothing is
    launched -- and the library stays usable."""
    from slimt_amd import synth
    D, F, H = dfh
    bad = synth.make_model("micro", dims=(D, F, H, 1, 1, 64))
    with pytest.raises(hip.SlimtHipError, match=names):
        hip.Model(bad)
    good = synth.make_model("micro", eos_bias=3.0)
    gm = hip.Model(good)
    try:
        ctx = hip.Context(gm, 2, 4)
        try:
            ids, lens = synth.make_batch(good.V, 2, 4, seed=1)
            out, ln, _ = ctx.translate(ids, lens, None)
            assert out.shape[0] == 2 and ln.min() >= 1
        finally:
            ctx.close()
    finally:
        gm.close()
