"""The comparisons of tests/test_gpu_model_values.py must not be vacuous. Conditions on the INPUTS of that test, computed by
the oracle alone (nothing measured on the device): every value family's greedy batches are worth translating, the ceiling
models do reach the ceilings the kernels' comments claim, some family does mix the cache forms in one batch, and the bound
on scores is one a plain float32 log-softmax of the same logits keeps."""
import numpy as np
import pytest

from support import model_values as T
from test_forced_prefix_checker import forced_translate
from test_gpu_kv_narrow import centred, colsum_centres, kv_accumulators
from test_model_shape_fixtures import fixture_problems


def test_the_table_covers_every_family_at_every_shape():
    """Every entry of synth.FAMILIES at each of the four shapes with a persistent decoder; at most one translate case in
    four is listed as degenerate, and no (family, shape) loses both of its B = 21 cases."""
    from slimt_amd import synth
    assert T.FAMILY_NAMES == list(synth.FAMILIES)
    assert {(e.family, e.dims) for e in T.ENTRIES} == {(f, d) for f in synth.FAMILIES for d in T.SHAPES}
    assert len(T.ENTRIES) == len(synth.FAMILIES) * len(T.SHAPES)
    cases = {(B, S) for B, S, _ in T.TRANSLATE_CASES}
    assert len(set(T.DEGENERATE)) == len(T.DEGENERATE) and all(c in cases for _, _, c in T.DEGENERATE)
    assert 4 * len(T.DEGENERATE) <= len(T.ENTRIES) * len(T.TRANSLATE_CASES)
    for e in T.ENTRIES:
        listed = {c for f, D, c in T.DEGENERATE if (f, D) == (e.family, e.dims[0])}
        assert any(B == 21 and (B, S) not in listed for B, S, _ in T.TRANSLATE_CASES), T.entry_id(e)
    # only the case without a shortlist uses the full vocabulary; sizes stay small
    assert [n for _, _, n in T.TRANSLATE_CASES].count(None) == 1
    assert max(B for B, _, _ in T.TRANSLATE_CASES) <= 37 and max(S for _, S, _ in T.TRANSLATE_CASES) <= 70
    assert max(d[5] for d in T.SHAPES) <= 4000


@pytest.mark.parametrize("e", T.ENTRIES, ids=T.entry_id)
def test_translate_cases_are_not_degenerate(oracle, e):
    """Every translate case of every (family, shape) meets fixture_problems of test_model_shape_fixtures.py, except the
    cases T.DEGENERATE names -- which do not: the list is exact, so it cannot grow unnoticed."""
    om = oracle.OracleModel(T.make(e))
    listed = {c for f, D, c in T.DEGENERATE if (f, D) == (e.family, e.dims[0])}
    problems, fine = {}, []
    for B, S, n_sl in T.TRANSLATE_CASES:
        _, _, _, out, ln, _, steps = T.translate_reference(oracle, om, e.dims, B, S, n_sl)
        bad = fixture_problems(B, out, ln, steps)
        if bad and (B, S) not in listed:
            problems[(B, S)] = bad
        if not bad and (B, S) in listed:
            fine.append((B, S))
    assert not problems, (T.entry_id(e), e.eos_bias, e.seed, problems)
    assert not fine, ("listed as degenerate, but meets the conditions", T.entry_id(e), fine)


@pytest.mark.parametrize("dims", T.SHAPES, ids=lambda d: "D%d" % d[0])
def test_ceiling_models_reach_the_ceilings(oracle, dims):
    """The oracle's own accumulators on the ceiling model of each shape, for a batch the GPU test uses:
      * decoder layer 1's K and V: the shifted accumulator's maximum is 254 * 127 * D and its minimum -254 * 128 * D (at D =
        256 the ceiling of the 24-bit form: 8,258,048 and -8,323,072, the latter 65,536 short of -2^23), the signed one's
        127 * 127 * D and -127 * 128 * D (at D = 512 what the 24-bit form holds: -8,323,072 again);
      * every sentence of layer 1 is past both limits (24-bit form), every sentence of layer 2 below 2^19;
      * the one-signed W2 columns of encoder layer 1 and decoder layer 1: the FFN's input to W2 is relu(...) >= 0, so its
        quantised value is in [0, 127] and the shifted one in [127, 254]: whatever the input, |accS| >= 127 * 127 * F
        against the +127 column and >= 127 * 128 * F against the -128 one, at most 254 * 128 * F. That passes 2^24 =
        16,777,216 from F = 1040 on: on the shapes with F = 1536 and 2048 for EVERY row of every batch, which is asserted
        here through the oracle's accumulators of the smallest input (zeros) and of a random one. With F = 128 and 256
        even 254 * 128 * F = 4,161,536 / 8,323,072 stays below 2^24 -- no model of those shapes can pass it; there the
        columns are asserted to reach their own closed forms (the floor 127 * colsum at a zero input)."""
    D, F = dims[0], dims[1]
    m = T.make_ceiling(dims)
    om = oracle.OracleModel(m)
    for B, S in ((21, 13), (5, 40)):
        ids, lens = T.batch(dims, B, S, salt=2)
        assert T.encoder_output(oracle, om, ids, lens).min() >= 0.5  # 0.5 * 254 = 127: every activation saturates
        acc = kv_accumulators(oracle, m, om, ids, lens).astype(np.int64)
        signed = centred(acc, colsum_centres(m))
        assert acc[0].max() == 254 * 127 * D and acc[0].min() == -254 * 128 * D
        assert signed[0].max() == 127 * 127 * D and signed[0].min() == -127 * 128 * D
        for t in range(2):  # K and V, every row of every sentence: the four extreme columns exactly
            assert (acc[0, t, :, :, 0] == 254 * 127 * D).all() and (acc[0, t, :, :, 1] == -254 * 128 * D).all()
            assert (acc[0, t, :, :, 2] == -254 * 127 * D).all() and (acc[0, t, :, :, -1] == 254 * 127 * D).all()
        # what the 24-bit form holds fits it: the shifted accumulator up to emb 256, the signed one at emb 512
        assert np.abs(signed if D == 512 else acc).max() < 2 ** 23 and (D < 512 or np.abs(acc).max() >= 2 ** 23)
        assert np.abs(acc[1]).max() < 2 ** 19
        forms = T.forms_of(oracle, m, om, ids, lens, 1)[0]
        assert (forms[0] == 1).all() and (forms[1] != 1).all(), forms
    # the greedy output of a ceiling model is degenerate in every translate case (every sentence ends at step 1, or none ever
    # ends): that is why the GPU test compares the ceilings teacher-forced, layer by layer and forced, not in its greedy grid
    for B, S, n_sl in T.TRANSLATE_CASES:
        _, _, _, out, ln, _, steps = T.translate_reference(oracle, om, dims, B, S, n_sl)
        assert fixture_problems(B, out, ln, steps) and (np.all(ln == 1) or np.all(ln == steps)), (B, S, ln.tolist())
    r = np.random.Generator(np.random.PCG64(F))
    x = np.zeros((8, F), np.float32)
    x[1:] = np.maximum(r.normal(0, 1.0, size=(7, F)), 0).astype(np.float32)
    for L in ("encoder_l1", "decoder_l1"):
        W = np.ascontiguousarray(m.params[L + "_ffn_W2"].data).reshape(D, F)
        assert (W[0] == 127).all() and (W[1] == -128).all()
        aq = float(np.asarray(m.params[L + "_ffn_W2_QuantMultA"].data).ravel()[0])
        acc = oracle.affine_acc(x, W, aq).astype(np.int64)
        assert acc[0, 0] == 127 * 127 * F and acc[0, 1] == -127 * 128 * F
        assert (acc[:, 0] >= 127 * 127 * F).all() and (acc[:, 1] <= -127 * 128 * F).all()
        if 127 * 127 * F > 2 ** 24:
            assert (np.abs(acc[:, :2]) > 2 ** 24).all()
            assert (acc[:, :2].astype(np.float32).astype(np.int64) != acc[:, :2]).any()  # float(accS) does round
        else:
            assert 254 * 128 * F < 2 ** 24


def _mixes(oracle, D):
    """{family: [(B, S, rows)]} of the cases at emb D whose expected forms (the predicate of test_gpu_kv_narrow.py at the real
    limits, centres 127 colsum) hold both the 16-bit and the 20-bit form in one batch"""
    found = {}
    for e in T.ENTRIES:
        if e.dims[0] != D:
            continue
        m = T.make(e)
        om = oracle.OracleModel(m)
        for B, S in T.FORM_CASES[D]:
            ids, lens = T.batch(e.dims, B, S, salt=2)
            for rows in T.ENCODE_ROWS[D]:
                forms = T.forms_of(oracle, m, om, ids, lens, max(1, rows // S))[0]
                if (forms == 2).any() and (forms == 0).any():
                    found.setdefault(e.family, []).append((B, S, rows))
    return found


def test_a_family_mixes_the_16_and_20_bit_forms_in_one_batch_at_emb_256(oracle):
    """`default` and `ln0.3` do, in every case of the table (about half of the sentence-layers each)."""
    found = _mixes(oracle, 256)
    assert {"default", "ln0.3"} <= set(found), found


def test_a_family_mixes_the_16_and_20_bit_forms_in_one_batch_at_emb_512(oracle):
    """The oracle finds one: `a8_24` (15 sentence-layers in 20 bits, 27 in 16, in both cases of the table). `w48` mixes the
    20- and the 24-bit form there (4 / 38), and `w64` takes the 24-bit form throughout."""
    found = _mixes(oracle, 512)
    assert "a8_24" in found, found


def _log_softmax_errors(z):
    """per row of float32 z: (|float32 log-softmax - float64 log-softmax| over every column, largest |z|)"""
    x = z.astype(np.float32)
    mx = x.max(axis=1, keepdims=True)
    lsm32 = (x - mx) - np.log(np.exp(x - mx).sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    assert lsm32.dtype == np.float32
    x64 = x.astype(np.float64)
    mx64 = x64.max(axis=1, keepdims=True)
    lsm64 = (x64 - mx64) - np.log(np.exp(x64 - mx64).sum(axis=1, keepdims=True))
    return np.abs(lsm32.astype(np.float64) - lsm64).max(axis=1), np.abs(x64).max(axis=1)


@pytest.mark.parametrize("D", [256, 512])
def test_a_float32_log_softmax_keeps_the_score_bound_on_every_model(oracle, D):
    """T.score_bound(L) = max(5e-5, 8 spacing(float32(L))) for a row whose largest |logit| is L: the project's 5e-5 was set
    on default-family logits, and a float32 log-sum-exp dominated by a term of size L carries a few of ITS ulps. Before the
    GPU test relies on the bound, a plain float32 numpy log-softmax of the checker's own logits must stay within it against
    the float64 one, in every column of every row the checker produces:
      * every family, greedy, case (21, 13, shortlist 200), on the logits and on z = float32(logit * float32(1 / 0.7)), what a
        sampled call at the GPU test's temperature scores (L is then the peak of z; the bound is NOT scaled by 1 / T);
      * the ceiling model, forced through the random targets of the GPU test in every case it runs them.
    Largest L seen (D = 256 / D = 512), logits: default 6.9 / 9.8, w48 10.1 / 12.0, w64 13.0 / 21.6, heavy 6.8 / 8.8, a2_6 7.5 /
    9.6, a8_24 6.9 / 9.7, ln0.3 7.7 / 11.0, w64_heavy_a8_24 13.4 / 16.0, ceiling 5.7 / 8.1; of z: at most 1 / 0.7 times
    that, 30.9. So 8 spacing(L) <= 8 spacing(31) = 1.5e-5 everywhere in this table: the bound is the project's 5e-5 on every
    row the GPU test scores (the float32 log-softmax stays within 0.08 of it), and the term in L, which decides from |logit| =
    64 on, is kept for models that reach it and is exercised here only as far as these logits go."""
    B, S, n_sl = T.TRANSLATE_CASES[0]
    inv_T = np.float32(1.0) / np.float32(T.SAMPLING_TEMPERATURE)
    runs = []
    for e in T.ENTRIES + T.CEILINGS:
        if e.dims[0] != D:
            continue
        m = T.make(e)
        om = oracle.OracleModel(m)
        if e.family != "ceiling":
            rec = T.Recording(om)
            ids, lens = T.batch(e.dims, B, S, salt=2)
            forced_translate(oracle, rec, m, ids, lens, T.shortlist(e.dims, n_sl), np.zeros((B, 1), np.uint32), np.zeros(B, np.uint32))
            runs.append((T.entry_id(e), rec.logits, (np.float32(1.0), inv_T)))
            continue
        for Bc, Sc in T.FORM_CASES[D]:
            rec = T.Recording(om)
            ids, lens = T.batch(e.dims, Bc, Sc, salt=2)
            sl = T.shortlist(e.dims, T.SHORTLIST)
            forced_translate(oracle, rec, m, ids, lens, sl, *T.ceiling_targets(Bc, Sc, sl))
            runs.append(("%s-B%d-S%d" % (T.entry_id(e), Bc, Sc), rec.logits, (np.float32(1.0),)))
    for name, logits, scales in runs:
        for scale in scales:
            worst, Lmax = 0.0, 0.0
            for lg in logits:
                err, L = _log_softmax_errors((lg * scale).astype(np.float32))
                bound = np.array([T.score_bound(v) for v in L])
                assert (err <= bound).all(), (name, float(scale), err.max(), L.max())
                worst, Lmax = max(worst, float((err / bound).max())), max(Lmax, float(L.max()))
            print("%s x %.3f: largest |z| %.1f, float32 log-softmax error at most %.2f of the bound" % (name, scale, Lmax, worst))
