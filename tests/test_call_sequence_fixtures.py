"""CPU proof that the call sequences of tests/support/call_sequences.py can catch what they are for (the oracle only).

A stale destination, a skipped launch or a stale shortlist passes unnoticed wherever the call before had the same expected
outputs, so: in every hand-written sequence two consecutive calls whose outputs have the same shapes have different
expected outputs; the translations under the lists A, A' (A's size, another last id), B and the generated list differ
pairwise, and so do those under the full vocabulary and its 1024-entry list. Every piece of carried state named in
STATE_ITEMS is claimed by a sequence, every call of the catalogue is in one, and the shuffles are their seeds'. These are
conditions on the inputs: the seeds in the catalogue are chosen so that they hold."""
import numpy as np
import pytest

from support import call_sequences as CS

PRESETS = {"tiny11": CS.HAND_WRITTEN, "base": list(CS.BASE_SEQUENCES)}


@pytest.fixture(scope="module")
def envs(oracle, synth_models):
    cache = {}

    def get(preset):
        if preset not in cache:
            cache[preset] = CS.Env(preset, oracle, synth_models)
        return cache[preset]

    return get


def _reference(v):
    return None if v is None else np.asarray(v[1])


def _same(a, b):
    """two calls' expected outputs: None = not comparable (other outputs or shapes), else whether they are all equal"""
    if set(a) != set(b):
        return None
    known = [n for n in a if a[n] is not None and b[n] is not None]
    if any(_reference(a[n]).shape != _reference(b[n]).shape for n in known):
        return None
    return all(np.array_equal(_reference(a[n]), _reference(b[n]), equal_nan=_reference(a[n]).dtype.kind == "f") for n in known)


@pytest.mark.parametrize("preset,seq", [(p, s) for p, ss in PRESETS.items() for s in ss])
def test_consecutive_calls_of_one_shape_expect_different_outputs(envs, preset, seq):
    env = envs(preset)
    names = CS.calls_of(seq)
    for a, b in zip(names, names[1:]):
        ea, eb = CS.oracle_expected(CS.CALLS[a], env), CS.oracle_expected(CS.CALLS[b], env)
        if not ea and not eb:
            continue  # (two refused calls: nothing is written)
        same = _same(ea, eb)
        if same is None:
            continue
        if not any(v is not None for v in ea.values()):  # outputs without an oracle function: other inputs at least
            ia, ib = CS.inputs(CS.CALLS[a], env), CS.inputs(CS.CALLS[b], env)
            assert a != b and not np.array_equal(ia["ids"], ib["ids"]), (seq, a, b)
            continue
        assert not same, f"{seq}: {a} then {b} expect the same outputs: a stale result would pass"


@pytest.mark.parametrize("preset", list(PRESETS))
def test_the_shortlists_of_sequence_1_give_pairwise_different_translations(envs, preset):
    env = envs(preset)
    a, a2 = env.shortlist("A"), env.shortlist("A2")
    assert a.size == a2.size and np.array_equal(a[:-1], a2[:-1]) and a[-1] != a2[-1]
    assert a.size != env.shortlist("B").size
    names = ("tr_A", "tr_A2", "tr_B", "tr_gen", "tr_full")
    assert all(n in CS.SEQUENCES["shortlist_cache"] for n in names)
    ids = {n: CS.inputs(CS.CALLS[n], env)["ids"] for n in names}
    assert all(np.array_equal(ids[n], ids["tr_A"]) for n in names)  # one batch: only the list changes
    exp = {n: CS.oracle_expected(CS.CALLS[n], env) for n in names}
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            assert not np.array_equal(exp[x]["out_ids"][1], exp[y]["out_ids"][1]), (x, y)
    # ... and A' differs from A in a token, not only in an alignment row
    assert exp["tr_A"]["out_ids"][1].shape == exp["tr_A2"]["out_ids"][1].shape


def test_the_output_layers_of_sequence_2_give_different_translations(envs):
    env = envs("tiny11")
    full, short = (CS.oracle_expected(CS.CALLS[n], env) for n in ("out_full", "out_1024"))
    assert not np.array_equal(full["out_ids"][1], short["out_ids"][1])
    assert CS.CALLS["out_full"].S <= 32 and env.shortlist("S1024").size == 1024 and env.V > 16384
    assert np.array_equal(CS.inputs(CS.CALLS["out_full"], env)["ids"], CS.inputs(CS.CALLS["out_1024"], env)["ids"])


def test_the_probe_has_several_decoder_tiles_and_a_partly_filled_last_one():
    assert CS.PROBE["B"] > 4 * 16 and CS.PROBE["B"] % 16 and CS.PROBE["B"] % 32 and CS.PROBE["B"] % 8
    seq = CS.SEQUENCES["launch_bookkeeping"]
    assert all(seq[i + 1] == "probe" for i in range(0, len(seq), 2)) and set(seq[::2]) == set(CS.TICKETED)


def test_every_state_item_is_claimed_and_every_call_is_in_a_sequence():
    missing = [s for s in CS.STATE_ITEMS if not CS.STATE_COVERAGE.get(s)]
    assert not missing, missing
    assert all(n in CS.HAND_WRITTEN for names in CS.STATE_COVERAGE.values() for n in names)
    used = {n for s in CS.HAND_WRITTEN for n in CS.calls_of(s)}
    assert used == set(CS.CALLS), set(CS.CALLS) ^ used
    for s in CS.SEQUENCES:
        assert all(n in CS.CALLS for n in CS.calls_of(s)), s
        assert CS.SEQUENCE_DOC[s].strip()


def test_calls_stay_small_and_the_context_holds_them_all():
    long_ones = []
    for c in CS.CALLS.values():
        shapes = [(B, S) for B, S, _ in c.opt["subs"]] if c.kind == "many" else [(c.B, c.S)]
        for B, S in shapes:
            assert B <= CS.CTX_SHAPE[0] and (S <= CS.CTX_SHAPE[1] or c.opt.get("refused"))
            if S > 40:
                assert B <= 7, c.name
                long_ones.append(S)
        n = sum(c.opt["counts"]) if "counts" in c.opt else 0
        assert n <= CS.CTX_SHAPE[0], c.name
    assert {65, 128, 129} <= set(long_ones)


def test_the_shuffles_are_their_seeds_and_differ():
    for s in CS.SHUFFLE_SEEDS:
        assert CS.SEQUENCES["shuffle_%d" % s] == CS.shuffle(s) and len(CS.shuffle(s)) == CS.SHUFFLE_LENGTH
    assert len({CS.shuffle(s) for s in CS.SHUFFLE_SEEDS}) == len(CS.SHUFFLE_SEEDS) == 3
