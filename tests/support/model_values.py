"""The model VALUES tests/test_gpu_model_values.py compares with the oracle, and tests/test_model_value_fixtures.py checks for
being worth comparing (CPU). One table, like model_shapes.py, so the two cannot drift.

Values, not shapes: the four shapes that have a persistent decoder (small vocabularies, two encoder layers), each with

  * every value family of slimt_amd.synth.FAMILIES -- weight spread, a heavy-tailed draw, the range of the activation
    multipliers, the spread of the LayerNorm scales --, with an eos_bias and a seed chosen on the CPU so that the greedy
    batches are not degenerate (test_model_value_fixtures.py has the conditions; DEGENERATE lists the batches no choice helped);
  * one CEILING model (`ceiling`), the default family pushed to the limits the kernels' comments claim: every K / V
    activation of decoder layer 1 saturates at +127 against weight rows of all +127 / -128 / -127, so that the shifted
    accumulator reaches 254 * 127 * D and -254 * 128 * D (the signed one 127 * 127 * D and -127 * 128 * D), and one-signed
    FFN W2 columns whose accumulators pass 2^24 where the FFN is wide enough for that.
"""
from collections import namedtuple

import numpy as np

# dims = (D, F, H, Le, Ld, V)
SHAPES = [
    (64, 128, 4, 2, 2, 512),
    (128, 256, 8, 2, 2, 2048),
    (256, 1536, 8, 2, 2, 4000),
    (512, 2048, 8, 2, 2, 2000),
]

FAMILY_NAMES = ["default", "w48", "w64", "heavy", "a2_6", "a8_24", "ln0.3", "w64_heavy_a8_24"]  # == list(synth.FAMILIES) (CPU test)

SHORTLIST = 200

# (B, S, shortlist size or None = the full vocabulary) of the greedy translations
TRANSLATE_CASES = [(21, 13, SHORTLIST), (21, 32, None), (5, 40, SHORTLIST)]

Entry = namedtuple("Entry", "family dims eos_bias seed")

# (eos_bias, seed) per (family, D), chosen on the CPU over eos_bias in {0.5, 1, ..., 10} and seed in 1234..1238: the pair
# that makes most of TRANSLATE_CASES meet the fixture conditions, a B = 21 case among them.
_CHOSEN = {
    ("default", 64): (3.0, 1234),
    ("w48", 64): (4.0, 1234),
    ("w64", 64): (3.0, 1234),
    ("heavy", 64): (2.0, 1234),
    ("a2_6", 64): (2.5, 1234),
    ("a8_24", 64): (3.0, 1234),
    ("ln0.3", 64): (3.0, 1235),
    ("w64_heavy_a8_24", 64): (3.0, 1235),
    ("default", 128): (3.5, 1237),
    ("w48", 128): (5.0, 1235),
    ("w64", 128): (1.0, 1234),
    ("heavy", 128): (2.5, 1237),
    ("a2_6", 128): (1.0, 1234),
    ("a8_24", 128): (3.5, 1235),
    ("ln0.3", 128): (1.0, 1234),
    ("w64_heavy_a8_24", 128): (3.0, 1234),
    ("default", 256): (5.0, 1234),
    ("w48", 256): (6.0, 1234),
    ("w64", 256): (7.0, 1234),
    ("heavy", 256): (4.0, 1234),
    ("a2_6", 256): (5.0, 1234),
    ("a8_24", 256): (5.0, 1234),
    ("ln0.3", 256): (6.0, 1234),
    ("w64_heavy_a8_24", 256): (10.0, 1234),
    ("default", 512): (6.0, 1234),
    ("w48", 512): (6.0, 1237),
    ("w64", 512): (10.0, 1236),
    ("heavy", 512): (3.0, 1234),
    ("a2_6", 512): (7.0, 1234),
    ("a8_24", 512): (7.0, 1234),
    ("ln0.3", 512): (6.0, 1234),
    ("w64_heavy_a8_24", 512): (7.0, 1234),
}

# (family, D, (B, S)) of the cases whose greedy batch does NOT meet the fixture conditions under the entry's eos_bias / seed,
# and did not under any pair of the scan that serves the entry's other cases. They are translated and compared on the device
# like the others (still bit for bit); the CPU test checks that this list is exact.
DEGENERATE = [
    ("a2_6", 128, (21, 13)),
    ("ln0.3", 128, (21, 13)),
]

ENTRIES = [Entry(f, dims, *_CHOSEN[(f, dims[0])]) for dims in SHAPES for f in FAMILY_NAMES if (f, dims[0]) in _CHOSEN]


def entry(family, D):
    return next(e for e in ENTRIES if e.family == family and e.dims[0] == D)


def entry_id(e):
    return "%s-D%d" % (e.family, e.dims[0])


def expected_plan(dims, S, decode_mode=0):
    """(encoder_fused, decoder_fused) as slimt_hip_ctx_plan reports them (model_shapes.py has the rules): every shape here
    has the persistent decoder; emb 256 the persistent encoder up to 128 tokens, emb 512 up to 32."""
    if decode_mode == 1:
        return (False, False)
    D = dims[0]
    return (D == 256 or (D == 512 and S <= 32), True)


def make(e):
    from slimt_amd import synth
    if e.family == "ceiling":
        return make_ceiling(e.dims)
    return synth.make_model("tiny11", seed=e.seed, eos_bias=e.eos_bias, dims=e.dims, family=e.family)


CEILING_EOS_BIAS, CEILING_SEED = 3.0, 1234


def make_ceiling(dims):
    """The default family at `dims`, pushed to the ceilings:
      * last encoder LayerNorm bias + 6: every encoder output is positive (and >= 0.5);
      * decoder layer 1's K / V activation multiplier 127 / 0.5: every activation of theirs saturates at +127;
      * in those two payloads ([N][K]) row 0 = all +127, row 1 = all -128, row 2 = all -127, last row = all +127;
      * in encoder layer 1's and decoder layer 1's W2 payload row 0 (logical column 0) = all +127, row 1 = all -128;
      * decoder layer 2 untouched: its cache keeps varied, narrow values next to layer 1's 24-bit ones."""
    from slimt_amd import synth
    m = synth.make_model("tiny11", seed=CEILING_SEED, eos_bias=CEILING_EOS_BIAS, dims=dims)
    P = m.params
    b = P["encoder_l%d_ffn_ffn_ln_bias" % m.enc_layers]
    b.data = (b.data + np.float32(6.0)).astype(np.float32)
    for t in "kv":
        a = P["decoder_l1_context_W%s_QuantMultA" % t]
        a.data = np.full_like(a.data, np.float32(127.0 / 0.5))
        W = P["decoder_l1_context_W%s" % t]
        q = np.ascontiguousarray(W.data).reshape(m.D, m.D).copy()
        q[0], q[1], q[2], q[-1] = 127, -128, -127, 127
        W.data = q.astype(np.int8)
    for L in ("encoder_l1", "decoder_l1"):
        W = P[L + "_ffn_W2"]
        q = np.ascontiguousarray(W.data).reshape(m.D, m.F).copy()  # payload [N = D][K = F]
        q[0], q[1] = 127, -128
        W.data = q.astype(np.int8)
    return m


CEILINGS = [Entry("ceiling", dims, CEILING_EOS_BIAS, CEILING_SEED) for dims in SHAPES]


class Recording:
    """an OracleModel that keeps the logits of every decode_step: step t of a checker's loop is logits[t]"""

    def __init__(self, om):
        self.om, self.logits = om, []

    def __getattr__(self, name):
        return getattr(self.om, name)

    def decode_step(self, *args):
        logits, attn = self.om.decode_step(*args)
        self.logits.append(np.array(logits, dtype=np.float32))
        return logits, attn

    def row_peaks(self, scale=1.0):
        """[steps][B]: the largest |logit * scale| of every row (scale: a sampled call's float32 1 / temperature)"""
        return np.stack([np.abs(lg.astype(np.float64) * float(scale)).max(axis=1) for lg in self.logits])


def ceiling_targets(B, S, sl):
    """(ids [B, Tmax], lengths [B] = Tmax): the random targets (no EOS) a ceiling model is forced through"""
    Tm = max(1, int(np.float32(1.5) * np.float32(S)))
    pool = sl[sl != 0]
    return np.random.default_rng(B + S).choice(pool, size=(B, Tm)).astype(np.uint32), np.full(B, Tm, np.uint32)


SAMPLING_TEMPERATURE = 0.7


def batch(dims, B, S, salt=0):
    from slimt_amd import synth
    return synth.make_batch(dims[5], B, S, seed=B * 100 + S + salt, ragged=S > 1)


def shortlist(dims, n):
    from slimt_amd import synth
    return None if n is None else synth.make_shortlist(dims[5], n)


def translate_reference(oracle, om, dims, B, S, n_sl):
    """The PORTABLE oracle's greedy translation of case (B, S, n_sl): (ids, lengths, shortlist, out, len, align, steps)"""
    ids, lens = batch(dims, B, S, salt=2)
    sl = shortlist(dims, n_sl)
    oracle.set_mode(oracle.PORTABLE)
    try:
        out, ln, al, _ = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    return ids, lens, sl, out, ln, al, out.shape[1]


def encoder_output(oracle, om, ids, lens):
    """[B * S][D] float32, PORTABLE order: what the decoder's K / V projections read"""
    B, S = ids.shape
    oracle.set_mode(oracle.PORTABLE)
    try:
        enc = om.encode(om.embed(ids), oracle.make_mask(lens, S))
    finally:
        oracle.set_mode(oracle.FAITHFUL)
    return np.ascontiguousarray(enc.reshape(B * S, -1), dtype=np.float32)


def forms_of(oracle, m, om, ids, lens, group, tight=True):
    """(expected cache forms [Ld][B] at the real limits 2^19 / 2^15 under centres 127 colsum, accumulators, signed ones);
    tight = False: a call that does not try the 16-bit form (tight_tried below)"""
    from test_gpu_kv_narrow import centred, colsum_centres, expected_forms, kv_accumulators
    acc = kv_accumulators(oracle, m, om, ids, lens)
    signed = centred(acc, colsum_centres(m))
    return expected_forms(acc, 2 ** 19, group, signed, 2 ** 15 if tight else 0), acc, signed


def forms_recorded(S, rows, mode):
    """Whether a translate call caches per-sentence forms at all (tests/test_gpu_kv_narrow.py): sentences of 33 .. 64 tokens
    take the packed cache through the 64-row encoder, one sentence per workgroup, and the tilings of 16 / 8 / 4 sentences --
    with 32-row tiles forced, or the 32-sentence tiling (decode mode 3), the batch is cached as f32 and nothing is recorded."""
    return S <= 32 or (rows != 32 and mode != 3)


def tight_tried(mode, S):
    """Which decoders read the 16-bit form (tests/test_gpu_kv_narrow.py; slimt_hip_debug_kv_tight_limit): the tilings of 16 /
    8 / 4 sentences, and of 32 up to 32 source tokens -- not the cluster kernels (decode mode 6). Elsewhere a sentence that
    would fit 16 bits is cached in 20."""
    return mode != 6 and not (mode == 3 and S > 32)


# the batches whose cache forms are compared (the packed cache: emb 256 up to 128 source tokens, emb 512 up to 32), and the
# encoder tiles forced for them: the sentences of one encoder workgroup, max(1, rows // S) of them, decide a form together
FORM_CASES = {256: [(21, 13), (21, 32), (5, 40)], 512: [(21, 13), (21, 32)]}
ENCODE_ROWS = {256: (64, 32), 512: (32,)}

TOL = 5e-5  # the project's bound for scores against a float64 checker (tests/test_gpu_forced_prefix.py), set on default-family logits


def score_bound(L):
    """For a row whose largest |logit| is L: eight float32 ulps of L -- the error of a float32 log-sum-exp dominated by a
    term of that size --, and at least TOL. Not tuned against the device (test_model_value_fixtures.py checks it on the CPU)."""
    return max(TOL, 8.0 * float(np.spacing(np.float32(L))))
