"""GPU parity of the per-call translate options -- per-token scores, forced target prefixes, temperature sampling -- over the
FAMILY of model shapes (tests/support/model_shapes.py), where tests/test_gpu_model_shapes.py arms none of them and the options'
own test files run tiny11 and base only. The score, force and sample epilogues of the per-stage decoder (decode mode 1) then
run at head sizes 16 and 64, at emb 64 and 128 with other head counts, at 1, 3, 4 and 5 decoder layers and over
vocabularies that are no multiple of 8; the persistent decoder's (modes 0 and 2) at depths 1, 3 and 4.

Every shape runs case (5, 13) under a 200-id shortlist and case (21, 32) over the full vocabulary
(tests/support/score_cases.py). The references are the checkers in the oracle's PORTABLE order: tokens, lengths, alignment
rows and sampled draws bit for bit, scores within model_values.score_bound of the row's largest |logit|."""
import numpy as np
import pytest

from support import model_shapes as T
from support import score_cases as C
from support.model_values import Recording
from test_forced_prefix_checker import forced_translate, tmax_of
from test_gpu_scores import _teacher_forced
from test_sampling_checker import keys_of, sampled_translate

pytestmark = pytest.mark.gpu

CASES = [pytest.param(s, B, S, id="%s-B%d-S%d" % (T.shape_id(s), B, S)) for s in T.SHAPES for B, S in C.OPTION_CASES]


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


@pytest.fixture(scope="module")
def forced_references(oracle, shape_engines):
    """(prefix, checker's forced translation, row peaks) per (shape, B, S): computed once, shared by the forced test and the
    cache-format test, never written to"""
    cache = {}

    def get(s, B, S):
        if (s.dims, B, S) not in cache:
            m, _, om = shape_engines(s)
            ids, lens, sl = C.option_inputs(s, B, S)
            p = C.option_prefix(s, B, S, sl, tmax_of(S))
            rec = Recording(om)
            want = forced_translate(oracle, rec, m, ids, lens, sl, *p)
            cache[(s.dims, B, S)] = (p, want, rec.row_peaks())
        return cache[(s.dims, B, S)]

    return get


def _same_translation(got, want, tag):
    (out, ln, al), (w_out, w_ln, w_al) = got, want
    assert np.array_equal(ln, w_ln), (tag, ln, w_ln)
    assert np.array_equal(out, w_out), tag
    assert np.array_equal(al.view(np.uint32), w_al.view(np.uint32)), tag


@pytest.mark.parametrize("s,B,S", CASES)
def test_forced_and_scored(hip, shape_engines, forced_references, s, B, S):
    """random targets of full length tmax_of(S), forced over prefixes of 0 .. Tmax tokens and completed greedily, with scores
    and alignments: the comparison stays strong where the shape's greedy output alone is short"""
    _, gm, _ = shape_engines(s)
    ids, lens, sl = C.option_inputs(s, B, S)
    p, (w_out, w_ln, w_al, w_sc), peaks = forced_references(s, B, S)
    ctx = hip.Context(gm, B, S)
    try:
        for mode in C.option_modes(s, S):
            ctx.set_decode_mode(mode)
            assert ctx.plan(S) == T.expected_plan(s, S, mode), mode
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p)
            _same_translation((out, ln, al), (w_out, w_ln, w_al), mode)
            C.check_scores(sc, w_sc, ln, peaks)
    finally:
        ctx.close()


@pytest.mark.parametrize("s,B,S", CASES)
def test_greedy_and_scored(hip, oracle, shape_engines, s, B, S):
    """the shape's vouched greedy cases (tests/test_score_case_fixtures.py holds them to the fixture conditions): scores
    against the float64 log-softmax of the oracle's logits along the oracle's own translation"""
    m, gm, om = shape_engines(s)
    ids, lens, sl, w_out, w_ln, w_al, _ = T.translate_reference(oracle, om, s, B, S)
    rec = Recording(om)
    ref = _teacher_forced(oracle, rec, m, ids, lens, sl, w_out, w_ln)
    ctx = hip.Context(gm, B, S)
    try:
        for mode in C.option_modes(s, S):
            ctx.set_decode_mode(mode)
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True)
            _same_translation((out, ln, al), (w_out, w_ln, w_al), mode)
            C.check_scores(sc, ref, ln, rec.row_peaks())
    finally:
        ctx.close()


@pytest.mark.parametrize("s,B,S", CASES)
def test_sampled_and_scored(hip, oracle, shape_engines, s, B, S):
    """temperature 0.7 under per-sentence keys: draws, lengths and alignments bit for bit the checker's. Scores are those of
    z = logit / T, so a row's peak is that of z and the bound model_values.score_bound of it, as in
    tests/test_gpu_model_values.py."""
    m, gm, om = shape_engines(s)
    ids, lens, sl = C.option_inputs(s, B, S)
    temp = C.OPTION_TEMPERATURE
    keys = keys_of(S + B, B)
    rec = Recording(om)
    w_out, w_ln, w_al, w_sc = sampled_translate(oracle, rec, m, ids, lens, sl, keys, temp)
    peaks = rec.row_peaks(np.float32(1.0) / np.float32(temp))
    ctx = hip.Context(gm, B, S)
    try:
        for mode in C.option_modes(s, S):
            ctx.set_decode_mode(mode)
            out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, sampling=(temp, keys))
            _same_translation((out, ln, al), (w_out, w_ln, w_al), mode)
            C.check_scores(sc, w_sc, ln, peaks)
    finally:
        ctx.close()


PACKED = [pytest.param(s, B, S, id="%s-B%d-S%d" % (T.shape_id(s), B, S)) for s in T.SHAPES if s.packed for B, S in C.OPTION_CASES]


@pytest.mark.parametrize("s,B,S", PACKED)
def test_forced_and_scored_in_every_cache_format(hip, shape_engines, forced_references, s, B, S):
    """shapes with the packed K/V cache: the forced case in cache formats 0, 2 and 1 on a device model of this test's own
    (which form a sentence takes depends on the model's calibration state), as
    tests/test_gpu_model_shapes.py::test_translate_tokens_lengths_alignments does without options"""
    m, _, _ = shape_engines(s)
    ids, lens, sl = C.option_inputs(s, B, S)
    p, (w_out, w_ln, w_al, w_sc), peaks = forced_references(s, B, S)
    own = hip.Model(m)
    ctx = hip.Context(own, B, S)
    try:
        for fmt in (0, 2, 1):
            own.set_kv_cache_format(fmt)
            for mode in C.option_modes(s, S):
                ctx.set_decode_mode(mode)
                out, ln, al, sc = ctx.translate(ids, lens, sl, want_align=True, scores=True, prefix=p)
                _same_translation((out, ln, al), (w_out, w_ln, w_al), (fmt, mode))
                C.check_scores(sc, w_sc, ln, peaks)
    finally:
        ctx.close()
        own.close()
