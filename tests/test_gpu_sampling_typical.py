"""GPU parity of locally typical sampling (slimt_hip_ctx_set_sampling_typical) through translate and fan-out, against the
checker of tests/support/typical_ref.py over the oracle's logits, held as tests/test_gpu_sampling_floor.py holds the floors
(K/V cache format 3 included: alignments bit for bit against the device's other decode mode, 1e-4 against the checker)."""
import numpy as np
import pytest

from support import typical_ref
from test_sampling_checker import keys_of, sampled_translate

pytestmark = pytest.mark.gpu

TOL = 5e-5
B, S, T, MASS = 5, 5, 1.0, 0.5  # Tmax 7


@pytest.fixture(scope="module")
def batch(oracle, synth_models):
    """(model, ids, lens, shortlist, keys, the checker's typical translation): computed once, shared and left unchanged"""
    from slimt_amd import synth
    m = synth_models("tiny11", 6.0)
    om = oracle.OracleModel(m)
    ids, lens = synth.make_batch(m.V, B, S, seed=66, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys = keys_of(9, B)
    sizes = []
    want = typical_ref.typical_translate(oracle, om, m, ids, lens, sl, keys, T, MASS, sizes=sizes)
    plain = sampled_translate(oracle, om, m, ids, lens, sl, keys, T)
    assert any(k < n for k, n in sizes)  # (the set is cut at some step)
    assert not (np.array_equal(want[0], plain[0]) and np.array_equal(want[1], plain[1]))  # ... and changes a sentence
    return m, ids, lens, sl, keys, want


@pytest.mark.parametrize("mode,kv_format", [(0, None), (1, None), (0, 3)])
def test_a_typical_translate_equals_the_checker(hip, batch, mode, kv_format):
    m, ids, lens, sl, keys, (w_out, w_ln, w_al, w_sc) = batch
    gm = hip.Model(m)
    if kv_format is not None:
        gm.set_kv_cache_format(kv_format)
    ctx = hip.Context(gm, B, S)
    try:
        ctx.set_decode_mode(mode)
        plan = ctx.plan(S)
        got = out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), typical=MASS)
        assert ctx.plan(S) == plan  # (slimt_hip_ctx_plan keeps reporting the context's mode)
        assert np.array_equal(ln, w_ln) and np.array_equal(out, w_out)
        if kv_format == 3:
            assert np.abs(al - w_al).max() <= 1e-4
            ctx.set_decode_mode(1)
            for x, y in zip(got, ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(T, keys), typical=MASS)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        else:
            assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32))
        worst = max(np.abs(sc[b, :n].astype(np.float64) - w_sc[b, :n]).max() for b, n in enumerate(w_ln))
        print("%s: scores: max |gpu - float64| = %.3g" % ((mode, kv_format), worst))
        assert worst <= TOL
    finally:
        ctx.close()
        gm.close()


def test_fanout_cuts_per_row_and_mass_one_is_the_plain_sampled_call(hip, batch):
    m, ids, lens, sl, keys, _ = batch
    gm = hip.Model(m)
    row_src = np.array([0, 0, 0, 3, 1, 4, 4], np.uint32)
    ctx = hip.Context(gm, row_src.size, S)
    try:
        kw = dict(want_align=True, scores=True, sampling=(T, keys_of(21, row_src.size)))
        fan = ctx.translate_fanout(ids, lens, row_src, sl, typical=MASS, **kw)
        dup = ctx.translate(ids[row_src], lens[row_src], sl, typical=MASS, **kw)
        off = ctx.translate(ids[row_src], lens[row_src], sl, typical=1.0, **kw)
        plain = ctx.translate(ids[row_src], lens[row_src], sl, **kw)
        for x, y, z, w in zip(fan, dup, off, plain):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            assert np.array_equal(z.view(np.uint32), w.view(np.uint32))
    finally:
        ctx.close()
        gm.close()


@pytest.mark.parametrize("message,options", [
    ("without sampling", dict(typical=MASS)),
    ("truncation is armed too", dict(sampling=True, truncation=(4, 0.9), typical=MASS)),
    ("floor is armed too", dict(sampling=True, floor=(0.1, 0.0), typical=MASS)),
    ("typical sampling is armed too", dict(sampling=True, constraints=dict(no_repeat_ngram=2), typical=MASS)),
    ("beam call", dict(beam=2)),
    ("mass 0 is not in", dict(mass=0.0)),
    ("mass 1.5 is not in", dict(mass=1.5)),
    ("mass nan is not in", dict(mass=float("nan"))),
])
def test_each_refusal_is_negative_with_a_message_and_leaves_the_next_call_unarmed(hip, batch, message, options):
    from slimt_amd import capi
    m, ids, lens, sl, keys, _ = batch
    gm = hip.Model(m)
    ctx = hip.Context(gm, 2 * B, S)
    try:
        greedy = ctx.translate(ids, lens, sl)
        with pytest.raises(capi.SlimtHipError, match=message):
            if "beam" in options or "mass" in options:
                ctx.set_sampling_typical(options.get("mass", MASS))
                ctx.translate_beam(ids, lens, 2, sl)
            else:
                ctx.translate(ids, lens, sl, **dict(options, sampling=(T, keys)) if "sampling" in options else options)
        again = ctx.translate(ids, lens, sl)  # (greedy: nothing is left armed)
        assert np.array_equal(again[0], greedy[0]) and np.array_equal(again[1], greedy[1])
    finally:
        ctx.close()
        gm.close()
