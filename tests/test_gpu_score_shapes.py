"""GPU parity of teacher-forced scoring (slimt_hip_score) over the FAMILY of model shapes, not only tiny11 and base: every
shape of tests/support/model_shapes.py -- all eleven (emb / 64, head size) pairs the tall kernels of score_tall.hip are
instantiated for, decoder depths 1 .. 5 (the K/V offset of layer l and the alignment of the last layer only), full
vocabularies of 517 and 1003 ids (an output layer whose last column tile is partly filled) -- against the checker of
tests/test_score_checker.py in the oracle's PORTABLE order: alignment rows bit for bit, scores within
model_values.score_bound of the row's largest |logit|, unwritten entries untouched. tests/support/score_cases.py holds the
cases; tests/test_score_case_fixtures.py proves on the CPU that they reach what they claim."""
import numpy as np
import pytest

from support import model_shapes as T
from support import score_cases as C

pytestmark = pytest.mark.gpu

CASES = [pytest.param(s, kind, id="%s-%s" % (T.shape_id(s), kind)) for s in T.SHAPES for kind in C.SHAPE_CASES]


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
def references(oracle, shape_engines):
    """(inputs, checker's result) per (shape, kind): computed once, shared by the tests below, never written to"""
    cache = {}

    def get(s, kind):
        if (s.dims, kind) not in cache:
            m, _, om = shape_engines(s)
            c = C.shape_inputs(s, kind)
            cache[(s.dims, kind)] = (c, C.reference(oracle, m, om, c))
        return cache[(s.dims, kind)]

    return get


def _score(ctx, c, want_align=True):
    return ctx.score(c.ids, c.lens, c.sl, c.t_ids, c.t_len, want_align=want_align, fill=C.FILL)


@pytest.mark.parametrize("s,kind", CASES)
def test_scores_and_alignments_match_the_checker(hip, shape_engines, references, s, kind):
    """short: B 5, S 13, T 27 over a 200-id shortlist; long: B 3, S 70, T 21 over the full vocabulary. Target lengths 0 .. T,
    lens[0] = 0 and lens[-1] = S; with the alignment and without it."""
    _, gm, _ = shape_engines(s)
    c, ref = references(s, kind)
    B, S = c.ids.shape
    ctx = hip.Context(gm, B, S)
    try:
        C.check_case(_score(ctx, c), ref, c)
        C.check_case(_score(ctx, c, want_align=False), ref, c, align=False)
    finally:
        ctx.close()


@pytest.mark.parametrize("s", T.SHAPES, ids=T.shape_id)
def test_scores_do_not_depend_on_which_encoder_ran(hip, shape_engines, references, s):
    """The scorer goes through the context's own encoder and attends over K / V computed from its output: decode modes 0
    and 1, and the persistent encoder's 32- and 64-row tilings where the shape has one, give the checker's result and the
    same bits as each other."""
    _, gm, _ = shape_engines(s)
    c, ref = references(s, "short")
    B, S = c.ids.shape
    runs = [(0, 0), (1, 0)] + ([(0, 32), (0, 64)] if T.expected_plan(s, S)[0] else [])
    ctx = hip.Context(gm, B, S)
    try:
        first = None
        for mode, rows in runs:
            ctx.set_decode_mode(mode)
            ctx.set_encode_rows(rows)
            got = _score(ctx, c)
            C.check_case(got, ref, c)
            if first is None:
                first = got
            assert np.array_equal(got[0].view(np.uint32), first[0].view(np.uint32)), (mode, rows)
            assert np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32)), (mode, rows)
    finally:
        ctx.close()
