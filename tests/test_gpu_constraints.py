"""GPU parity of step constraints: the kernel alone against the restatement of tests/support/constraints_ref.py, then translate,
fan-out and the text frontend against its checker loop over the oracle's logits -- tokens, lengths and alignment rows exact,
scores within 5e-5 of the float64 log-softmax over the candidates; K/V format 3 as in tests/test_gpu_sampling_floor.py."""
from contextlib import closing

import numpy as np
import pytest

from support import constraints_ref
from test_gpu_sampling_floor import _check
from test_sampling_checker import keys_of
from test_text_frontend import corpus, spm_model  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

TOL = 5e-5
B, S, T, EOS_BIAS = 5, 8, 0.25, 9.0  # Tmax 12; T: the sampled calls' temperature
CN = (2, 1.05, 6, (4,))  # no repeated bigram, penalty 1.05, at least 6 tokens, never id 4
KW = constraints_ref.as_dict(CN)
SHAPES = [(N, R, ids) for N in (1, 63, 64, 65, 4096, 4097, 32000) for R in (1, 5) for ids in (False, True)] + [(1 << 19, 1, False)]


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("N,R,with_ids", SHAPES)
def test_the_constraint_kernel_matches_the_restatement(hip, N, R, with_ids, sampled):
    """Column, banned count and fallback exact, the score within TOL (NaN where the row holds one). N: the 4-column groups, one wave,
    either side of the resident bound, the column bound (dynamic LDS above 64 KiB). A launch: a row and its successors, its setting."""
    from slimt_amd import capi
    T, inv_T = (0.5, np.float32(2.0)) if sampled else (1.0, np.float32(1.0))
    ids, eos = constraints_ref.layout(N, with_ids)
    cases = constraints_ref.crafted_rows(N, ids, eos, 7 * N + R)
    worst, lifted = 0.0, 0
    for at, (kind, _, _, cn) in enumerate(cases):
        part = [cases[(at + r) % len(cases)][1:3] for r in range(R)]
        logits, lens = np.stack([x for x, _ in part]), np.array([len(h) for _, h in part], np.uint32)
        hist = np.array([h + [0] * (max(1, lens.max()) - len(h)) for _, h in part], np.uint32)
        keys = keys_of(N + at, R) if sampled else None
        cols, sc, nb, fb = capi.constrained_step(logits, hist, lens, constraints_ref.as_dict(cn), eos, T, ids=ids, keys=keys, steps=lens if sampled else None)
        for r, (x, h) in enumerate(part):
            w_col, w_none, w_nb, w_fb, w_sc, _, _ = constraints_ref.constrained_row(x, h, cn, ids, eos, inv_T, keys[r] if sampled else None, lens[r])
            assert (cols[r], nb[r], fb[r]) == (0 if w_none else w_col, w_nb, w_fb), (kind, r)
            assert np.isnan(sc[r]) == np.isnan(w_sc) and not abs(float(sc[r]) - w_sc) > TOL, (kind, r, sc[r], w_sc)
            worst = max(worst, 0.0 if np.isnan(w_sc) else abs(float(sc[r]) - w_sc))
            lifted += w_fb
    assert lifted >= (1 if N <= 64 else 0)
    print("N = %d R = %d ids = %d sampled = %d: scores: max |gpu - float64| = %.3g" % (N, R, with_ids, sampled, worst))


@pytest.fixture(scope="module")
def batch(oracle, synth_models):
    """Shared, left unchanged. eos_bias and the seeds were picked on the CPU so that the reference meets the conditions asserted here
    and its two float orders (PORTABLE, FAITHFUL) agree on this batch: K/V format 3 has a third order."""
    from slimt_amd import synth
    m = synth_models("tiny11", EOS_BIAS)
    om = oracle.OracleModel(m)
    ids, lens = synth.make_batch(m.V, B, S, seed=69, ragged=True)
    sl = synth.make_shortlist(m.V, 4096)
    keys, want = keys_of(9, B), {}
    for sampled in (False, True):
        trace, t = [], T if sampled else None
        want[sampled] = constraints_ref.constrained_translate(oracle, om, m, ids, lens, sl, CN, keys, t, trace=trace)
        plain = constraints_ref.constrained_translate(oracle, om, m, ids, lens, sl, constraints_ref.OFF, keys, t)
        assert [any(hit[i] for hit in trace) for i in range(3)] == [True] * 3, sampled  # n-gram, EOS rule, penalty: each bit
        assert not (np.array_equal(want[sampled][0], plain[0]) and np.array_equal(want[sampled][1], plain[1])), sampled
    return m, ids, lens, sl, keys, want


@pytest.fixture
def context(hip, batch):
    made = []  # (a context on a model of its own, both closed behind the test)

    def make(rows, max_s, kv_format=None):
        gm = hip.Model(batch[0])
        if kv_format is not None:
            gm.set_kv_cache_format(kv_format)
        made[:0] = [hip.Context(gm, rows, max_s), gm]
        return made[0]
    yield make
    [x.close() for x in made]


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("mode,kv_format", [(0, None), (1, None), (0, 3)])
def test_a_constrained_translate_equals_the_checker(batch, context, mode, kv_format, sampled):
    m, ids, lens, sl, keys, want = batch
    ctx = context(B, S, kv_format)
    ctx.set_decode_mode(mode)
    plan = ctx.plan(S)
    kw = dict(want_align=True, scores=True, sampling=(T, keys) if sampled else None, constraints=KW)
    got = ctx.translate(ids, lens, sl, **kw)
    _check(got, want[sampled], (mode, kv_format, sampled), literal=kv_format == 3)
    assert ctx.plan(S) == plan  # (slimt_hip_ctx_plan keeps reporting the context's mode)
    if kv_format == 3:
        ctx.set_decode_mode(1)
        for x, y in zip(got, ctx.translate(ids, lens, sl, **kw)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("sampled", [False, True])
def test_fanout_a_forced_prefix_and_the_all_off_setting(oracle, batch, context, sampled):
    m, ids, lens, sl, keys, want = batch
    row_src = np.array([0, 0, 0, 3, 1, 4, 4], np.uint32)
    ctx = context(row_src.size, S)
    kw = dict(want_align=True, scores=True, sampling=(T, keys_of(21, row_src.size)) if sampled else None)
    fan = ctx.translate_fanout(ids, lens, row_src, sl, constraints=KW, **kw)
    dup = ctx.translate(ids[row_src], lens[row_src], sl, constraints=KW, **kw)
    plan = ctx.plan(S)
    off = ctx.translate(ids[row_src], lens[row_src], sl, constraints=constraints_ref.as_dict(constraints_ref.OFF), **kw)
    assert ctx.plan(S) == plan
    plain = ctx.translate(ids[row_src], lens[row_src], sl, **kw)
    for x, y, z, w in zip(fan, dup, off, plain):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(z.view(np.uint32), w.view(np.uint32))
    # a forced prefix: its steps are unconstrained (a repeated bigram, the suppressed id 4) and count as history
    kw["sampling"] = (T, keys) if sampled else None
    p_ids, p_len = np.zeros((B, 12), np.uint32), np.array([0, 4, 5, 2, 12], np.uint32)
    p_ids[:, :5] = [sl[9], sl[7], sl[9], sl[7], 4]
    w_pre = constraints_ref.constrained_translate(oracle, oracle.OracleModel(m), m, ids, lens, sl, CN, keys, T if sampled else None, p_ids, p_len)
    assert all(np.array_equal(w_pre[0][b, :n], p_ids[b, :n]) for b, n in enumerate(np.minimum(p_len, w_pre[1])))
    _check(ctx.translate(ids, lens, sl, prefix=(p_ids, p_len), constraints=KW, **kw), w_pre, ("prefix", sampled))


def test_each_refusal_is_negative_with_a_message_and_leaves_the_next_call_unarmed(batch, context):
    from slimt_amd import capi
    m, ids, lens, sl, keys, _ = batch
    ctx = context(2 * B, 128)
    greedy = ctx.translate(ids, lens, sl)
    long_ids, long_lens = np.ones((1, 128), np.uint32), np.array([128], np.uint32)  # at limit factor 9: Tmax 1152 > 1024
    refusals = [
        ("truncation is armed too", lambda: ctx.translate(ids, lens, sl, sampling=(T, keys), truncation=(4, 0.9), constraints=KW)),
        ("floor is armed too", lambda: ctx.translate(ids, lens, sl, sampling=(T, keys), floor=(0.1, 0.0), constraints=KW)),
        ("beam call", lambda: (ctx.set_step_constraints(**KW), ctx.translate_beam(ids, lens, 2, sl))),
        ("history bound", lambda: ctx.translate(long_ids, long_lens, sl, limit_factor=9.0, constraints=KW)),
        ("columns", lambda: capi.constrained_step(np.zeros((1, (1 << 19) + 1), np.float32), long_ids[:, :1], long_lens // 128, KW)),
        ("no_repeat_ngram", lambda: ctx.set_step_constraints(no_repeat_ngram=9)),
        ("repetition_penalty", lambda: ctx.set_step_constraints(repetition_penalty=-1.0)),
        ("suppressed ids", lambda: ctx.set_step_constraints(suppress=list(range(65))))]
    for message, call in refusals:
        with pytest.raises(capi.SlimtHipError, match=message):
            call()
        again = ctx.translate(ids, lens, sl)  # (greedy: neither constraints nor anything else is left armed)
        assert np.array_equal(again[0], greedy[0]) and np.array_equal(again[1], greedy[1]), message


@pytest.mark.parametrize("sampling", [None, (0.5, 11)])
def test_the_text_frontend_under_constraints_equals_the_context_call_on_the_same_segments(hip, spm_model, corpus, sampling):
    from slimt_amd import capi, frontend, synth
    m = synth.make_model("micro", eos_bias=3.0)  # V = 512 = the vocabulary's size
    model = frontend.Model(frontend.Config(encoder_layers=m.enc_layers, decoder_layers=m.dec_layers, num_heads=m.H, split_mode="paragraph"),
                           frontend.Package(model=synth.write_bin(m), vocabulary=spm_model), device=0)
    svc = frontend.Service(workers=1, max_words=256, wrap_length=24)
    with closing(model), closing(svc), closing(capi.Context(model.engine, 32, 128)) as ctx:
        sources, kw = corpus[:3], dict(no_repeat_ngram=1, min_length=4)
        segs = [seg for _, ss in model.processor.process_many(sources, svc.wrap_length, svc.workers) for seg in ss]
        ids = np.array([seg + [0] * (max(map(len, segs)) - len(seg)) for seg in segs], np.uint32)  # one batch, keyed by index
        sm = sampling and (sampling[0], np.array([capi.sampling_key(sampling[1], e) for e in range(len(segs))], np.uint64))
        out, ln, _, sc = ctx.translate(ids, [len(seg) for seg in segs], None, svc.limit_factor, model.vocabulary.eos_id(), scores=True,
                                       sampling=sm, constraints=kw)
        assert all(len(set(out[e, :n])) == n >= 4 for e, n in enumerate(ln))  # (no token twice, no early EOS)
        for got in [svc.translate(model, sources, sampling=sampling, constraints=kw)] + (
                [svc.sample_and_select(model, sources, 1, sampling, constraints=kw)] if sampling else []):  # (1 sample: the same keys)
            assert np.array_equal(np.concatenate([x for r in got for x in r.token_scores]), np.concatenate([sc[e, :n] for e, n in enumerate(ln)]))
