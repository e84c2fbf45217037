"""Beam calls under slimt_hip_ctx_set_beam_constraints, bit for bit against the host search over the oracle under the rows
z' (support/beam_constrained_ref.py) where the setting bites; beam 1 against constrained greedy; the refusals, each consumed."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_constrained_ref as BR
from support import constraints_ref as CR
from test_gpu_beam import _ctx, _same, engines  # noqa: F401  (the beam tests' fixture and comparison)

pytestmark = pytest.mark.gpu

CN = (3, 1.2, 4, ())  # chosen on the CPU with the oracle: the plain search repeats 3-grams on each case below, no step lifts


@pytest.mark.parametrize("name", ["sl1000", "full", "k8"])  # a shortlist, the full vocabulary, k = 8
def test_constrained_beam_equals_the_checker(hip, oracle, engines, name):
    c = BC.parity(name)
    m, gm, om = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    trace = {}
    want = BR.translate(oracle, om, m, ids, lens, sl, c.k, CN, c.mode, trace)
    plain = BC.beam_translate(oracle, om, m, ids, lens, sl, c.k, c.mode)
    # the case bites, on the checker's results alone
    assert BR.violations(plain[0], plain[1], CN) > 0 and trace["lifts"] == 0 and BR.violations(want[0], want[1], CN) == 0
    ctx = _ctx(hip, gm, c)
    try:
        _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True, constraints=CR.as_dict(CN)), want, name)
        _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True), plain, name + ", the next plain call")
    finally:
        ctx.close()


def test_beam_one_is_constrained_greedy_and_refusals_are_consumed(hip, engines):
    c = BC.parity("sl1000")
    m, gm, _ = engines(c)
    ids, lens, sl = BC.inputs(c, m.V)
    cn = CR.as_dict(CN)
    ctx = _ctx(hip, gm, c)
    try:
        out, ln, _, _, _ = ctx.translate_beam(ids, lens, 1, sl, constraints=cn)
        w_out, w_ln, _ = ctx.translate(ids, lens, sl, want_align=True, constraints=cn)
        assert np.array_equal(ln[:, 0], w_ln) and np.array_equal(out[:, 0], w_out)  # beam 1: the constrained greedy call's tokens
        plain = ctx.translate_beam(ids, lens, c.k, sl, want_align=True)
        calls = [(lambda: (ctx.set_beam_constraints(**cn), ctx.translate(ids, lens, sl)), "not a beam call"),
            (lambda: (ctx.set_beam_sampling(None, c.B), ctx.translate_beam(ids, lens, c.k, sl, constraints=cn)), "beam sampling is armed too"),
            (lambda: ctx.translate_beam(ids, lens, c.k, sl, limit_factor=65.0, constraints=cn), "bounds of 512 tokens and 65536 columns")]
        for call, message in calls:
            with pytest.raises(hip.SlimtHipError, match=message):
                call()
            _same(ctx.translate_beam(ids, lens, c.k, sl, want_align=True), plain, message)  # consumed: the next call is plain
        with pytest.raises(hip.SlimtHipError, match="65536 columns and 1..512 tokens"):
            hip.beam_step_constrained(np.zeros((1, 65537), np.float32), [0.0], [1], 1, np.zeros((1, 4), np.uint32), 0, cn)
    finally:
        ctx.close()
