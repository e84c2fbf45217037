"""The fused decoder takes a step's next embedding row from the tied output layer's packed tile (kernels.h,
FusedDecodeArgs::out_tied_exact): column ix of the tile holds the bytes of Wemb[shortlist[ix]] whenever re-quantising the
dequantised table gave every byte back, which the model's load proves (engine.cpp, model_build). The same integers go
through the same three float operations, so tokens, lengths and alignment rows must equal the CPU oracle's (PORTABLE
order, as in tests/test_gpu_queue_bound_outputs.py) on every path that reaches the seam:

  * shortlists of 16, 17 and 100 columns (columns in the last, partly filled tile), and the full vocabulary;
  * the 16-, 8- and 4-sentence tilings (decode modes 2 / 4 / 5);
  * a merged call of three sub-batches with their own lists, and a generated list;
  * a forced prefix whose tokens lie outside the list (those steps keep the table), and a sampled call;
  * a model whose EOS bias ends sentences at different steps (every model here);
  * a model whose Wemb holds -128 (it comes back as -127): the proof fails, the flag reads off, results still match.

The calls, their inputs, their device runs and their expected results are tests/support/call_sequences.py's (the options'
own checkers: OracleModel.translate, forced_translate, sampled_translate); scores are held against the float64 checkers
within that module's tolerance. tiny11-shaped models, B <= 24, S <= 8, T <= 12. The proof alone also runs without a GPU."""
import copy

import numpy as np
import pytest

from support import call_sequences as CS

LISTS = (16, 17, 100)
CTX_SHAPE = (64, 8)  # the merged call's 16 + 32 + 16 rows


def _list(V, n):
    """n sorted ids: EOS, the first few, and ids spread over the whole table (so the rows lie far apart in it)"""
    r = np.random.default_rng(400 + n)
    rest = r.choice(np.arange(8, V, dtype=np.uint32), size=n - 8, replace=False)
    return np.sort(np.concatenate([np.arange(8, dtype=np.uint32), rest])).astype(np.uint32)


class Env(CS.Env):
    """call_sequences' environment with this file's lists: L<n> = _list(V, n); the merged call's own lists (its names
    for them) are the three sizes too."""
    OWN = {"A": "L100", "B": "L17", "S520": "L16"}

    def shortlist(self, name):
        if name is None:
            return None
        name = self.OWN.get(name, name)
        if name not in self._sl:
            assert name[0] == "L", name
            self._sl[name] = _list(self.V, int(name[1:]))
        return self._sl[name]


def _minus_128(m):
    """a copy of the model whose table holds -128: one whole column and a scatter of single entries"""
    m2 = copy.copy(m)
    m2.params = dict(m.params)
    w = copy.copy(m.params["Wemb"])
    q = np.array(w.data, dtype=np.int8).reshape(m.V, m.D)
    q[:, 5] = -128
    r = np.random.default_rng(77)
    q[r.integers(0, m.V, 4000), r.integers(0, m.D, 4000)] = -128
    w.data = q
    m2.params["Wemb"] = w
    return m2


@pytest.fixture(scope="module")
def envs(hip, oracle, synth_models):
    cache = {}

    def get(kind):
        if kind not in cache:
            models = synth_models if kind == "tied" else (lambda preset, eos_bias: _minus_128(synth_models(preset, eos_bias)))
            cache[kind] = Env("tiny11", oracle, models, hip)
        return cache[kind]

    yield get
    for env in cache.values():
        env.close()


def _t(name, B, S, seed, **opt):
    return CS._t("seam_" + name, B, S, seed, **opt)


SINGLE = [_t("L%d" % n, 21, 8, 8100 + n, sl="L%d" % n, align=True) for n in LISTS] + [
    _t("L17_device", 24, 7, 8120, entry="device", sl="L17", align=True),
    _t("full", 5, 8, 8130, sl=None, align=True),
    _t("generated", 19, 8, 8140, entry="generated", sl="gen", align=True),
]
MERGED = CS.Call("seam_many_own", "many", 0, 8, 0, where="device", subs=((9, 8, 8201), (21, 6, 8202), (6, 5, 8203)), sls="own")
FORCED = _t("forced_off_list", 13, 8, 8300, sl="L100", align=True, scores=True, prefix=True)
SAMPLED = _t("sampled", 17, 8, 8400, sl="L100", align=True, scores=True, sampling=0.7)


def _check(hip, env, ctx, call):
    want = CS.oracle_expected(call, env)
    got = CS.run(call, hip, ctx, env)
    assert set(got) == set(want), (call.name, sorted(got), sorted(want))
    for n, v in want.items():
        if v[0] == "exact":
            w = v[1].astype(got[n].dtype)
            assert got[n].shape == w.shape and np.array_equal(got[n].view(np.uint32), w.view(np.uint32)), \
                "%s.%s differs from the oracle at rows %s" % (call.name, n, CS.differing_rows(got[n], w))
        else:  # scores: a float64 checker (NaN: not written)
            g, w = got[n].astype(np.float64), v[1]
            written = got[n].view(np.uint32) != CS.PAT
            assert np.array_equal(written, ~np.isnan(w)), "%s.%s: written entries differ from the checker's" % (call.name, n)
            assert np.array_equal(np.isneginf(g[written]), np.isneginf(w[written])), "%s.%s: -inf entries differ" % (call.name, n)
            fin = written & np.isfinite(w)
            worst = np.abs(g[fin] - w[fin]).max(initial=0.0)
            assert worst <= v[2], "%s.%s: |got - float64| = %.3g > %.3g" % (call.name, n, worst, v[2])
    return got


def _context(hip, env, mode=0):
    ctx = hip.Context(env.gm, *CTX_SHAPE)
    ctx.set_decode_mode(mode)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 4, 5])
def test_every_tiling_and_list_size_equals_the_oracle(hip, envs, mode):
    env = envs("tied")
    assert env.gm.debug_out_tied_exact() is True
    ctx = _context(hip, env, mode)
    try:
        ctx.profile_enable(hip.K_DECODE_FUSED)
        for call in SINGLE:
            _check(hip, env, ctx, call)
        assert ctx.profile_read()["launches"] >= len(SINGLE)  # every call ran the persistent decoder
        lens = set(np.concatenate([CS.oracle_expected(c, env)["out_len"][1] for c in SINGLE]).tolist())
        assert len(lens) > 2 and min(lens) < 12 == max(lens), lens  # the EOS bias ends sentences at different steps, or never
    finally:
        ctx.profile_enable(hip.K_NONE)
        ctx.close()


@pytest.mark.gpu
def test_a_merged_call_with_three_lists_equals_the_oracle(hip, envs):
    env = envs("tied")
    ctx = _context(hip, env)
    try:
        ctx.profile_enable(hip.K_DECODE_FUSED)
        _check(hip, env, ctx, MERGED)
        assert ctx.profile_read()["launches"] == 1  # one merged launch: each tile reads its own job's tile
    finally:
        ctx.profile_enable(hip.K_NONE)
        ctx.close()


@pytest.mark.gpu
def test_forced_tokens_outside_the_list_keep_the_table(hip, envs, monkeypatch):
    env = envs("tied")

    def off_list(call, env, sl, B, T):  # every sentence but the first has a prefix, none of its tokens in the list
        r = np.random.default_rng(call.seed + 1)
        pool = np.setdiff1d(np.arange(2, env.V, dtype=np.uint32), sl)
        p_len = r.integers(1, 5, size=B).astype(np.uint32)
        p_len[0] = 0
        return r.choice(pool, size=(B, T)).astype(np.uint32), p_len

    monkeypatch.setattr(CS, "_prefix", off_list)
    ctx = _context(hip, env)
    try:
        got = _check(hip, env, ctx, FORCED)
        p_ids, p_len = CS.inputs(FORCED, env)["p_ids"], CS.inputs(FORCED, env)["p_len"]
        for b in range(FORCED.B):  # the prefixes were recorded (the steps behind them come from the tile again)
            n = min(int(p_len[b]), int(got["out_len"][b]))
            assert np.array_equal(got["out_ids"][b, :n], p_ids[b, :n])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_sampled_call_equals_its_checker(hip, envs):
    env = envs("tied")
    ctx = _context(hip, env)
    try:
        _check(hip, env, ctx, SAMPLED)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_table_with_minus_128_reads_off_and_still_matches(hip, envs):
    env = envs("minus128")
    assert env.gm.debug_out_tied_exact() is False
    for mode in (2, 4):
        ctx = _context(hip, env, mode)
        try:
            for call in (SINGLE[1], SINGLE[4]):  # 17 columns; the full vocabulary
                _check(hip, env, ctx, call)
        finally:
            ctx.close()


@pytest.mark.parametrize("preset", ["micro", "mini", "tiny11", "base"])
def test_the_load_time_proof(preset):
    """slimt_hip_debug_tied_output_proof (host code: what model_build runs on Wemb): exact for the synthetic presets,
    not for a table with a -128."""
    from slimt_amd import capi, synth
    m = synth.make_model(preset, eos_bias=0.0)
    w = m.params["Wemb"]
    q = np.array(w.data, dtype=np.int8).reshape(m.V, m.D)
    assert q.min() >= -127
    assert capi.debug_tied_output_proof(q, w.mult) is True
    q[m.V // 2, m.D - 1] = -128
    assert capi.debug_tied_output_proof(q, w.mult) is False
    w2 = _minus_128(m).params["Wemb"]
    assert capi.debug_tied_output_proof(np.asarray(w2.data).reshape(m.V, m.D), w2.mult) is False
