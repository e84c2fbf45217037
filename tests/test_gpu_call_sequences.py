"""A context's call history never changes a call's results.

Every other GPU test runs its calls on a context made for the case, or repeats one kind of call on it. A service context
lives for days and sees every kind of call in every order, and the engine carries a great deal from one call to the next
(the host shortlist cache, the last batch's cache forms, the last decoder launch's column count, ticket bases paired with
device counters that are never reset, workspaces that grow lazily, per-model watches). Here the sequences of
tests/support/call_sequences.py run on ONE model and ONE context each, and every call must give, bit for bit, its expected
result -- every output pre-filled with a pattern, so that what a call must not write is compared too.

The expected result of a call is computed once per module. Tokens, lengths, alignment rows (greedy, forced, sampled,
truncated, merged, fan-out), the consensus pick and its utilities come from the CPU oracle in PORTABLE order through the
features' own checkers (OracleModel.translate, forced_translate, sampled_translate, truncated_translate,
support/consensus_ref.py); so do the step-wise API's encoder output, logits, attention and SSRU states (OracleModel.encode /
decode_step), debug_cross_attention's outputs (OracleModel.cross_attention) and the alternatives' ids and ranks
(test_alternatives_checker.alternatives, the pattern behind tgt_len). The outputs below are log-probabilities: their
checkers are float64 and none is bit-exact. For these only, the expected bits are the call on a fresh model and a fresh
context, and that fresh result is first held against the float64 checker within the project's tolerance:
  * per-token scores of translate calls (the checkers of the calls' options, 5e-5 * max(1, 1 / T));
  * scores of score / score_candidates (teacher_forced, 5e-5; their alignment rows: the checker's values, equal);
  * alt_scores of scored alternatives (alternatives, 5e-5).

Also here: the ticket and claim counters run modulo 2^32, which no launch of the suite had ever reached;
slimt_hip_debug_ctx_set_counters puts a context shortly before the wrap (and the shortlist hand-over's epoch before its
reserved value) and the launches that cross it must give the same results."""
import numpy as np
import pytest

from support import call_sequences as CS
from test_gpu_kv_narrow import colsum_centres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def envs(hip, oracle, synth_models):
    cache = {}

    def get(preset, tight=False):
        if (preset, tight) not in cache:
            env = CS.Env(preset, oracle, synth_models, hip, share=cache.get((preset, False)))  # one oracle per preset
            if tight:  # the tight K/V form is live from the first batch (tests/test_gpu_kv_narrow.py)
                env.gm.set_kv_centres(colsum_centres(env.m))
            cache[(preset, tight)] = env
        return cache[(preset, tight)]

    yield get
    for env in cache.values():
        env.close()


_EXPECTED = {}  # (preset, call name) -> {output: array}


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _hold_against(name, out, got, want, tol):
    """a fresh result against its float64 checker: NaN in the checker = not written (the pattern) or NaN"""
    g = got.astype(np.float64)
    pat = np.ascontiguousarray(got).view(np.uint32) == CS.PAT
    nan = np.isnan(want)
    assert (pat | np.isnan(g))[nan].all(), f"{name}.{out}: written where the checker has nothing"
    assert not pat[~nan].any(), f"{name}.{out}: entries the checker has were not written"
    assert np.array_equal(np.isneginf(g[~nan]), np.isneginf(want[~nan])), f"{name}.{out}: -inf entries differ"
    fin = ~nan & np.isfinite(want)
    worst = np.abs(g[fin] - want[fin]).max(initial=0.0)
    assert worst <= tol, f"{name}.{out}: |fresh - float64| = {worst:.3g} > {tol:.3g}"


def expected(hip, env, call):
    key = (env.preset, call.name)
    if key not in _EXPECTED:
        want = CS.oracle_expected(call, env)
        exp = {n: v[1] for n, v in want.items() if v is not None and v[0] == "exact"}
        if len(exp) < len(want):  # outputs without a bit-exact oracle function: a fresh model and a fresh context
            gm = hip.Model(env.m)
            ctx = hip.Context(gm, *CS.CTX_SHAPE)
            try:
                fresh = CS.run(call, hip, ctx, env)
            finally:
                ctx.close()
                gm.close()
            assert set(fresh) == set(want), (call.name, sorted(fresh), sorted(want))
            for n, v in want.items():
                if v is not None and v[0] == "exact":
                    assert _bits_equal(fresh[n], v[1].astype(fresh[n].dtype)), f"{call.name}.{n}: a fresh context differs from the oracle at rows {CS.differing_rows(fresh[n], v[1].astype(fresh[n].dtype))}"
                    continue
                if v is not None:
                    _hold_against(call.name, n, fresh[n], v[1], v[2])
                exp[n] = fresh[n]
        _EXPECTED[key] = exp
    return _EXPECTED[key]


def _compare(seq, i, names, call, got, want):
    bad = []
    if set(got) != set(want):
        bad.append("outputs %s, expected %s" % (sorted(got), sorted(want)))
    for n in sorted(set(got) & set(want)):
        w = want[n].astype(got[n].dtype) if want[n].dtype != got[n].dtype and want[n].dtype.itemsize == got[n].dtype.itemsize else want[n]
        if not _bits_equal(got[n], w):
            bad.append("%s differs at rows %s" % (n, CS.differing_rows(got[n], w)))
    assert not bad, "sequence %s, call %d (%s) after %s: %s" % (seq, i, call.name, names[max(0, i - 2):i] or "nothing", "; ".join(bad))


def run_sequence(hip, env, seq, ctx=None, items=None, at_end=None):
    """Runs the sequence on one context of env's model; every call == its expected result, and no call that returned 0 set
    slimt_hip_last_error. at_end(ctx): called behind the last call, before the context and the model are put back."""
    items = list(CS.SEQUENCES[seq] if items is None else items)
    L = hip.lib()
    own = ctx is None
    if own:
        ctx = hip.Context(env.gm, *CS.CTX_SHAPE)
    names, queued = [], None
    try:
        for item in items:
            if item[0] == "@":
                CS.apply_setter(item, ctx, env)
                continue
            if item == "<queue":
                queued = []
                continue
            if item == ">queue":
                ctx.synchronize()
                for i, call, finish in queued:
                    _compare(seq, i, names, call, finish(), expected(hip, env, call))
                queued = None
                continue
            call, i = CS.CALLS[item], len(names)
            want = expected(hip, env, call)  # (before the call: a fresh context's launches do not fall between queued ones)
            refused = call.kind.startswith("refused") or call.opt.get("refused")
            # a failure of this call's own (a poll limit no other call names): the text the last error must still hold
            assert L.slimt_hip_debug_break_shortlist_handoff(ctx.h, 0, (1 << 24) + 1 + i) != 0
            before = L.slimt_hip_last_error()
            assert str((1 << 24) + 1 + i).encode() in before, before
            finish = CS.start(call, hip, ctx, env)
            names.append(item)
            if queued is not None:
                queued.append((i, call, finish))
            else:
                ctx.synchronize()
                _compare(seq, i, names, call, finish(), want)
            assert refused or L.slimt_hip_last_error() == before, \
                "sequence %s, call %d (%s) returned 0 and set the last error: %r" % (seq, i, item, L.slimt_hip_last_error())
        if at_end is not None:
            at_end(ctx)
    finally:
        if own:
            ctx.set_decode_mode(0)
            ctx.set_encode_rows(0)
            ctx.close()
        env.gm.set_kv_cache_format(0)


TINY = [s for s in CS.SEQUENCES]
CASES = [("tiny11", s, False) for s in TINY] + [("tiny11", "output_layer", True)] + [("base", s, False) for s in CS.BASE_SEQUENCES]


def _case_id(preset, seq, tight):
    """a shuffle's id carries the sequence it drew"""
    drawn = "[%s]" % ",".join(CS.SEQUENCES[seq]) if seq.startswith("shuffle_") else ""
    return "%s-%s%s%s" % (preset, seq, "-tight" if tight else "", drawn)


@pytest.mark.parametrize("preset,seq,tight", CASES, ids=[_case_id(*c) for c in CASES])
def test_a_sequence_on_one_context_gives_every_call_its_own_result(hip, envs, preset, seq, tight):
    env = envs(preset, tight)

    def tight_was_live(ctx):  # its encoders submitted sentence-layers to the tight form (read before the watch is restarted)
        assert sum(env.gm.debug_kv_tight_watch()[2]) > 0

    run_sequence(hip, env, seq, at_end=tight_was_live if tight else None)


# launches of the persistent decoder per call: 1 = one merged launch, 3 = batch by batch
MERGED = [("many_dev", 1), ("many_own", 1), ("many_gen", 1), ("many_pinned", 1), ("many_pinned_gen", 1), ("many_fallback", 3)]


@pytest.mark.parametrize("name,launches", MERGED)
def test_the_merged_calls_merge_and_the_fallback_falls_back(hip, envs, name, launches):
    """The catalogue's merged calls reach the merged launch and `many_fallback` the batch-by-batch path (else the sequences
    would stay green while testing neither); a merged generated call leaves one list per sub-batch."""
    env = envs("tiny11")
    ctx = hip.Context(env.gm, *CS.CTX_SHAPE)
    try:
        ctx.profile_enable(hip.K_DECODE_FUSED)
        call = CS.CALLS[name]
        _compare(name, 0, [], call, CS.run(call, hip, ctx, env), expected(hip, env, call))
        assert ctx.profile_read()["launches"] == launches
        if call.opt["sls"] == "gen":
            lists = ctx.debug_shortlists(len(call.opt["subs"]))
            for got, want in zip(lists, CS.inputs(call, env)["sls"]):
                assert np.array_equal(got, want)
    finally:
        ctx.profile_enable(hip.K_NONE)
        ctx.close()


# ---- the counters' wrap-around --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("preset", ["tiny11", "base"])
def test_launches_that_cross_2_to_the_32_tickets_give_the_same_results(hip, envs, preset):
    """The decoder and encoder ticket counters (fused, tall, merged, fan-out launches; base: the wide encoder) cross 2^32
    inside these launches: every one of them takes its tiles by `counter - base` in unsigned arithmetic."""
    env = envs(preset)
    ctx = hip.Context(env.gm, *CS.CTX_SHAPE)
    try:
        run_sequence(hip, env, "before the wrap", ctx, ["probe"])
        ctx.debug_set_counters(0xFFFFFFF0)
        run_sequence(hip, env, "wrap at 0xFFFFFFF0", ctx, ["probe", "tr_gen", "probe", "many_dev", "probe", "fo_host", "probe", "enc_40", "probe"])
    finally:
        ctx.close()


def test_the_claim_word_crosses_2_to_the_32_in_both_halves(hip, envs):
    """XCD-affine claims (Model.set_xcd_affinity(1) under a decoder budget, the 16-sentence tiling): the arrivals' half of
    the claim word crosses 2^32 in the first launch, the claims' half in the fourth."""
    env = envs("tiny11")
    gm = hip.Model(env.m)
    ctx = hip.Context(gm, *CS.CTX_SHAPE)
    try:
        gm.set_xcd_affinity(1)
        gm.set_decoder_budget(64)
        ctx.set_decode_mode(2)
        ctx.debug_set_counters(0xFFFFFFF0)
        names = ["probe", "tr_A", "probe", "kv_64x8", "probe", "tr_B"]
        for i, n in enumerate(names):
            call = CS.CALLS[n]
            want = expected(hip, env, call)
            _compare("claim word at 0xFFFFFFF0", i, names, call, CS.run(call, hip, ctx, env), want)
            # the plan is recorded under a decoder budget only, and the claim branch takes the 16-sentence tiling of up to
            # 16 workgroups per home XCD: this launch went through it
            assert ctx.debug_decoder_plan()["rows"] == 16 and (call.B + 15) // 16 <= 16
    finally:
        ctx.close()
        gm.close()


def test_the_shortlist_handover_epoch_passes_its_reserved_value(hip, envs):
    """gen_epoch 0xFFFFFFFE -> 0xFFFFFFFF (used, then folded to 0) -> 1 (the flags cleared again before it is reused):
    generated calls on either side give the same results, unmerged and merged."""
    env = envs("tiny11")
    ctx = hip.Context(env.gm, *CS.CTX_SHAPE)
    try:
        run_sequence(hip, env, "before the epoch's wrap", ctx, ["tr_gen"])  # (the hand-over's flags exist from here on)
        ctx.debug_set_counters(0xFFFFFFFE)
        run_sequence(hip, env, "epoch at 0xFFFFFFFE", ctx, ["tr_gen", "tr_dev_gen", "many_gen", "tr_pinned_gen", "probe", "tr_gen"])
    finally:
        ctx.close()
