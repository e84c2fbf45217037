"""slimt_hip_beam_step_constrained against `beam_step_host` over the rows z' (support/beam_constrained_ref.py), bit for bit.
N = 1 (one column), 17 (an odd few), 4097 (one over the register-resident bound, more than one sweep)."""
import numpy as np
import pytest

from support import beam_cases as BC
from support import beam_constrained_ref as BR
from support import constraints_ref as CR
from test_gpu_beam_step import _bits

pytestmark = pytest.mark.gpu


def _check(hip, logits, totals, flags, hists, t, cn, ids, eos, k, Th):
    rows = lambda hs: np.array([h + [0] * (Th - len(h)) for h in hs], np.uint32)
    history = rows(hists)
    got = hip.beam_step_constrained(logits, totals, flags, k, history, t, CR.as_dict(cn), eos, ids)
    z, nb, lifted = BR.z_rows(logits, hists, flags, cn, ids, eos)
    want, new, _, _ = BR.step(logits, totals, flags, k, eos, ids, hists, cn)
    for g, w, name in zip(got, want, ("parent", "token", "token_score", "totals", "flags")):
        assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(w) if g.dtype == np.float32 else w), (name, g, w)
    assert np.array_equal(got[5], rows(new)) and np.array_equal(got[6], nb) and np.array_equal(got[7], lifted)
    return want, z, lifted


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 17, 4097])
def test_step_equals_the_checker_over_the_constrained_rows(hip, N, k, B, with_ids):
    seen = set()
    for variant in BR.VARIANTS:
        logits, totals, flags, hists, t, cn, ids, eos, roles = BR.crafted(N, k, B, with_ids, variant)
        (parent, token, score, tot, fl), z, lifted = _check(hip, logits, totals, flags, hists, t, cn, ids, eos, k, 24)
        e = int(np.flatnonzero((np.arange(N) if ids is None else ids) == eos)[0])
        other = CR.sets(hists[0], cn, N, ids, eos)[1]
        assert other[e] == (t < cn[2]) and other.sum() == int(t < cn[2])  # EOS by min_length; the suppressed id has no column
        if t == 0:
            assert fl[0] != BC.DEAD and parent[0] == 0 and (N > 1 or lifted[0])
            continue
        top = int(np.argmax(logits[0]))
        if cn[0] == 8 and N > 1:
            assert z[0, top] == -np.inf and not lifted[0] and BC.row_scores(z[0])[1] < logits[0, top]  # M excludes the banned maximum
            if "twin" in roles:
                assert np.isfinite(z[1, top]) and np.array_equal(logits[0], logits[1])  # one row, other bans
            if "seen" in roles and N >= 17:
                r = roles["seen"]
                assert z[r, 3] == np.float32(2.0) * (np.float32(1.0) / np.float32(1.3)) and z[r, 4] == np.float32(-2.0) * np.float32(1.3)
                seen.add("seen")
        if cn[0] == 1 and "lifts" in roles:
            assert lifted[roles["lifts"]]
            seen.add("lifts")
        if "finished" in roles:
            i = int(np.flatnonzero(token[roles["finished"] // k * k:][:k] == BC.NONE)[0])
            assert fl[roles["finished"] // k * k + i] == BC.FINISHED
            seen.add("finished")
        seen |= {"dead"} & set(roles)
    assert seen >= set(roles) - {"max banned", "twin"} - (set() if N >= 17 else {"seen"})  # every planted role was met ...
    assert B * k < 8 or set(roles) == {"max banned", "twin", "finished", "lifts", "seen", "dead"}  # ... and all are planted


def test_the_lds_bound(hip):  # k = 8, N = 2^16, Th = 512 under a penalty: both bitmaps of every slot, the longest histories
    N, k, Th, t = 1 << 16, 8, 512, 511
    r = np.random.default_rng(5)
    ids, eos = CR.layout(N, True)
    logits = (np.round(r.normal(0, 3, size=(k, N)) * 4) / 4).astype(np.float32)
    logits[:, np.arange(N) % 8 != 3] = -np.inf  # (the checker sorts every candidate)
    totals = (-np.round(r.uniform(0, 6, size=k) * 2) / 2).astype(np.float32)
    hists = [[int(x) for x in ids[r.integers(0, 8, t) * 8 + 3]] for _ in range(k)]  # 8 tokens: 3-grams repeat
    _, z, lifted = _check(hip, logits, totals, np.full(k, BC.LIVE, np.uint32), hists, t, (3, 1.2, 4, (2,)), ids, eos, k, Th)
    assert not lifted.any() and ((z == -np.inf) & np.isfinite(logits)).sum(axis=1).min() >= 1  # every slot bans a column

