"""The model shapes tests/test_gpu_model_shapes.py compares with the oracle, and tests/test_model_shape_fixtures.py
checks for being worth comparing (CPU). One table, so the two cannot drift.

Every plan below is written by hand from include/slimt_hip.h (slimt_hip_model_create, slimt_hip_ctx_plan) and the
kernels' documented shapes -- never computed by calling the library's predicates:

  persistent encoder:  emb 256 / 8 heads / FFN a multiple of 256 -- sources of up to 128 tokens (the row-tile kernels up to 32
                       tokens at FFN 1024, 1536 or 2048, a workgroup per sentence otherwise) --, or emb 512 / 8 heads / FFN 2048 with
                       sources of up to 32 tokens; 1..6 encoder layers, 1..4 decoder layers
  persistent decoder:  (emb, FFN, head size) = (64, 128, 16), (128, 256, 16), (256, 1536, 32), (512, 2048, 64); 1..4 decoder
                       layers, and its 16-sentence workgroup must fit 160 KiB of LDS. That rules out emb 256 with FOUR decoder
                       layers: three f32 row buffers 3 * 16 * 260 * 4 = 49,920 + SSRU cells 4 * 16 * 256 * 4 = 65,536 + two int8
                       rows 2 * 16 * 288 = 9,216 + hidden row 16 * 1568 = 25,088 + arg-max 2 * 16 * 16 * 4 = 2,048 + 64 +
                       attention scratch 16 * 256 * 4 = 16,384 = 168,256 bytes > 163,840 (three layers: 151,872). At emb 512 the
                       cells live in global memory and the size does not depend on the depth.
"""
from collections import namedtuple

# dims = (D, F, H, Le, Ld, V)
# plan = (encoder fused for S <= 32, encoder fused for 33 <= S <= 128, decoder fused) in decode mode 0
# packed = both persistent kernels run (emb 256 / head 32, or emb 512 / head 64 / FFN 2048): translate is compared in K/V
#          cache formats 0, 2 and 1. Emb 512 with four decoder layers has no room for the packed reader's tables and takes
#          the f32 cache in every format.
# long = also run at S = 70
# eos_bias / seed: chosen on the CPU so that the greedy batches are not degenerate (test_model_shape_fixtures.py has the
#          conditions; DEGENERATE below lists the batches no choice could help)
Shape = namedtuple("Shape", "cls dims plan packed long eos_bias seed")

SHAPES = [
    # 1. per-stage kernels only: FFN sizes that are no preset's (64; 320 and 704: multiples of 64 but not of 128 / 256), 1 and 7
    #    encoder layers, 1, 3, 4 and 5 decoder layers, vocabularies that are no multiple of 8
    Shape(1, (64, 64, 2, 1, 1, 517), (0, 0, 0), False, False, 2.0, 1234),
    Shape(1, (128, 320, 4, 7, 5, 517), (0, 0, 0), False, True, 3.0, 1237),
    Shape(1, (256, 704, 8, 3, 3, 1003), (0, 0, 0), False, False, 4.0, 1238),
    Shape(1, (512, 704, 16, 1, 4, 1003), (0, 0, 0), False, False, 6.0, 1235),
    Shape(1, (128, 2048, 2, 3, 1, 3000), (0, 0, 0), False, False, 1.0, 1234),
    Shape(1, (256, 1536, 8, 2, 5, 517), (0, 0, 0), False, True, 3.5, 1237),   # the flagship shape, one decoder layer too many
    Shape(1, (256, 1024, 8, 7, 2, 1003), (0, 0, 0), False, False, 5.0, 1236),  # ... a fused-encoder shape, one encoder layer too many
    # 2. a preset's emb / FFN with other head counts (head sizes 64, 32, 64, 16, 32)
    Shape(2, (64, 128, 1, 2, 2, 512), (0, 0, 0), False, False, 1.5, 1236),
    Shape(2, (128, 256, 4, 2, 2, 1003), (0, 0, 0), False, False, 3.0, 1234),
    Shape(2, (256, 1536, 4, 2, 2, 4000), (0, 0, 0), False, False, 5.5, 1234),
    Shape(2, (256, 1536, 16, 2, 2, 4000), (0, 0, 0), False, True, 6.0, 1236),
    Shape(2, (512, 2048, 16, 2, 2, 2000), (0, 0, 0), False, False, 7.0, 1234),
    # 3. persistent encoder, per-stage decoder (f32 K/V cache handed from one to the other). FFN 1024 is also the 64-row
    #    encoder's second instantiation; FFN 512 has the per-sentence encoder only, at every length
    Shape(3, (256, 1024, 8, 3, 2, 4000), (1, 1, 0), False, True, 4.0, 1235),
    Shape(3, (256, 2048, 8, 5, 1, 2000), (1, 1, 0), False, True, 1.0, 1235),
    Shape(3, (256, 512, 8, 1, 2, 4000), (1, 1, 0), False, True, 3.0, 1234),
    Shape(3, (256, 1024, 8, 1, 4, 1003), (1, 1, 0), False, True, 4.5, 1236),
    Shape(3, (256, 768, 8, 2, 1, 1003), (1, 1, 0), False, True, 2.5, 1235),   # per-sentence encoder, FFN no power of two
    Shape(3, (256, 1536, 8, 2, 4, 4000), (1, 1, 0), False, True, 5.5, 1238),   # flagship shape, four decoder layers (LDS, above)
    # 4. persistent decoder at other depths than the presets' 2 (+ 2 / 6 encoder layers)
    Shape(4, (256, 1536, 8, 1, 3, 1003), (1, 1, 1), True, True, 2.5, 1235),
    Shape(4, (256, 1536, 8, 7, 2, 1003), (0, 0, 1), False, False, 1.5, 1237),  # per-stage encoder in front of the persistent decoder
    Shape(4, (512, 2048, 8, 2, 1, 2000), (1, 0, 1), True, False, 3.0, 1236),
    Shape(4, (512, 2048, 8, 2, 3, 2000), (1, 0, 1), True, False, 3.0, 1235),
    Shape(4, (64, 128, 4, 1, 1, 517), (0, 0, 1), False, False, 2.0, 1238),
    Shape(4, (64, 128, 4, 6, 4, 512), (0, 0, 1), False, False, 3.0, 1238),
    Shape(4, (128, 256, 8, 1, 4, 2048), (0, 0, 1), False, False, 3.0, 1238),
    Shape(4, (128, 256, 8, 6, 1, 1003), (0, 0, 1), False, True, 3.0, 1234),
    # 5. emb 512 next to the tuned shape: another FFN size (nothing persistent), and the wide encoder with one layer
    Shape(5, (512, 1024, 8, 2, 2, 2000), (0, 0, 0), False, False, 6.0, 1234),
    Shape(5, (512, 2048, 8, 1, 4, 2000), (1, 0, 1), True, False, 6.0, 1234),  # (four decoder layers: f32 K/V cache)
]

# (dims, (B, S)) of cases(s) whose greedy batch does NOT meet the fixture conditions with the shape's eos_bias / seed, and did
# not with any eos_bias in {0, 0.5, ..., 5.5, 6, 7, 8, 10} and seed in 1234..1238 that serves the shape's vouched cases: nearly
# every sentence runs to the step limit, or ends at step 1. They are translated and compared on the device like the others (a
# weaker comparison, still bit for bit); the CPU test checks that this list is exact.
DEGENERATE = [
    ((128, 320, 4, 7, 5, 517), (21, 70)),
    ((128, 2048, 2, 3, 1, 3000), (5, 32)),
    ((256, 1024, 8, 7, 2, 1003), (21, 40)),
    ((256, 1536, 16, 2, 2, 4000), (5, 32)),
    ((256, 1024, 8, 3, 2, 4000), (5, 32)),
    ((256, 2048, 8, 5, 1, 2000), (5, 32)),
    ((256, 1536, 8, 2, 4, 4000), (5, 32)),
    ((256, 1536, 8, 2, 4, 4000), (21, 70)),
    ((256, 1536, 8, 7, 2, 1003), (5, 32)),
    ((256, 1536, 8, 7, 2, 1003), (21, 40)),
]

PRESET_VALUES = ({64, 128, 256, 512}, {128, 256, 1536, 2048}, {4, 8}, {2, 6}, {2})  # D, F, H, Le, Ld of synth.PRESETS

SHORTLIST = 200  # not a multiple of 64; make_shortlist rounds to a multiple of 8


def shape_id(s):
    return "D%d-F%d-H%d-Le%d-Ld%d-V%d" % s.dims


def cases(s):
    """(B, S) of one shape: a partly filled 16-row tile (5) and more than one tile (21) at S = 1, 13, 32, 40, and at 70 for the
    shapes marked long (every class-3 shape: the per-sentence and the 64-row encoder switch on S)."""
    return [(B, S) for S in (1, 13, 32, 40) + ((70,) if s.long else ()) for B in (5, 21)]


def vouched_cases(s):
    """The translate cases every shape's eos_bias / seed was CHOSEN for: they must meet the fixture conditions
    (test_model_shape_fixtures.py). The greedy translation itself is compared on the device for all of cases(s). These
    random models go from "every sentence ends at step 1" to "none ever ends" within about one unit of bias, at a point that
    moves with B, S and the shortlist, so one bias per shape cannot serve every batch of the grid: the other cases meet the
    conditions too unless DEGENERATE lists them. S = 1 is one step (floor(1.5 * 1)): every length is 1 whatever the model
    does, nothing to vouch for."""
    c = [(5, 13), (21, 13), (21, 32), (5, 40)]
    if s.long:
        c += [(5, 70)]
    if s.cls == 3:
        c += [(21, 40)]
    return c


def translate_shortlist(S):
    """Shortlist size of the translate comparison at source length S (None = the full vocabulary: N = 517 / 1003 ...)."""
    return None if S in (1, 32) else SHORTLIST


def expected_plan(s, S, decode_mode=0):
    """(encoder_fused, decoder_fused) as slimt_hip_ctx_plan reports them; decode mode 1 is the per-stage kernels throughout."""
    if decode_mode == 1:
        return (False, False)
    return (bool(s.plan[0] if S <= 32 else s.plan[1]), bool(s.plan[2]))


def make(s):
    from slimt_amd import synth
    return synth.make_model("tiny11", seed=s.seed, eos_bias=s.eos_bias, dims=s.dims)


def translate_reference(oracle, om, s, B, S):
    """The PORTABLE oracle's translation of case (B, S) of shape s: (ids, lengths, shortlist, out, len, align, Tmax)"""
    from slimt_amd import synth
    ids, lens = batch(s, B, S, salt=2)
    n_sl = translate_shortlist(S)
    sl = None if n_sl is None else synth.make_shortlist(s.dims[5], n_sl)
    oracle.set_mode(oracle.PORTABLE)
    try:
        out, ln, al, _ = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    return ids, lens, sl, out, ln, al, out.shape[1]


def batch(s, B, S, salt=0):
    from slimt_amd import synth
    return synth.make_batch(s.dims[5], B, S, seed=B * 100 + S + salt, ragged=S > 1)
