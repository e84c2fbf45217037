"""CPU checks of the beam cases (tests/support/beam_cases.py): the table holds the shapes the search's kernels can go wrong
at, and the parity cases show -- on the oracle, with the checker the GPU test uses -- what a beam search must show or a bug
hides: a reorder of the states, a finished slot carried beside a live one, a rank 0 that is not the greedy translation, a
slot still live at Tmax, and an order that depends on the length mode."""
import numpy as np
import pytest

from support import beam_cases as BC


def test_the_issues_cases_are_in_the_table():
    rows = {c.name: c for c in BC.PARITY}
    k6 = rows["k6"]
    assert (k6.preset, k6.S, k6.B, k6.k, k6.n_sl, k6.ragged) == ("tiny11", 8, 3, 6, 4096, True)
    assert k6.B * k6.k == 18 > 16 and (16 % k6.k) != 0  # a source's rows straddle the attention's 16-row workgroup
    assert (rows["k8"].B, rows["k8"].S, rows["k8"].k) == (2, 8, 8) and rows["k8"].k == BC.MAX_BEAM
    assert (rows["full"].n_sl, rows["full"].B, rows["full"].k) == (None, 2, 2)
    assert rows["sl1000"].n_sl % 16 != 0
    assert (rows["base"].preset, rows["base"].B, rows["base"].S, rows["base"].k) == ("base", 2, 8, 3)
    assert (rows["s70"].S, rows["s70"].B, rows["s70"].k) == (70, 2, 2) and rows["s70"].S > 64  # two keys per lane
    assert rows["exact"].B * rows["exact"].k == rows["exact"].max_batch
    assert rows["mean"].mode == 1 and rows["mean"]._replace(name="k6", mode=0) == k6
    assert BC.KV3.kv_format == 3 and all(c.kv_format is None for c in BC.PARITY)
    from slimt_amd import synth
    assert synth.make_model("base", eos_bias=0.0).D == 512


@pytest.fixture(scope="module")
def searched(oracle, synth_models):
    cache = {}

    def get(name):
        if name not in cache:
            c = BC.parity(name)
            m = BC.model_of(c, synth_models)
            om = oracle.OracleModel(m)
            ids, lens, sl = BC.inputs(c, m.V)
            trace = {}
            got = BC.beam_translate(oracle, om, m, ids, lens, sl, c.k, c.mode, trace=trace)
            oracle.set_mode(oracle.PORTABLE)
            try:
                greedy = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
            finally:
                oracle.set_mode(oracle.FAITHFUL)
            cache[name] = (c, got, trace, greedy)
        return cache[name]

    return get


def test_a_case_reorders_carries_and_leaves_greedy(searched):
    c, (out, ln, tot, sc, al), trace, (g_out, g_ln, _, _) = searched("k6")
    T = BC.tmax_of(c.S)
    assert trace["reorders"] >= 10                      # steps where a live slot's parent is another slot
    assert len(trace["carried_beside_live"]) >= 1       # a finished slot carried while another is live
    assert len(trace["live_at_end"]) >= 1 and (ln == T).any() and not (out[ln == T][:, T - 1] == 0).all()  # live at Tmax: no EOS
    differs = [b for b in range(c.B) if ln[b, 0] != g_ln[b] or not np.array_equal(out[b, 0, :ln[b, 0]], g_out[b, :g_ln[b]])]
    assert differs                                      # a rank 0 that is not the greedy translation
    assert len({int(x) for x in ln.reshape(-1)}) >= 3   # hypotheses of several lengths


def test_the_mean_orders_a_case_differently(searched):
    _, by_sum, _, _ = searched("k6")
    _, by_mean, _, _ = searched("mean")
    changed = [b for b in range(by_sum[0].shape[0]) if not np.array_equal(by_sum[1][b], by_mean[1][b])]
    assert changed
    for b in changed:  # the same hypotheses, in another order
        a = sorted(tuple(by_sum[0][b, j, :by_sum[1][b, j]]) for j in range(by_sum[0].shape[1]))
        assert a == sorted(tuple(by_mean[0][b, j, :by_mean[1][b, j]]) for j in range(by_mean[0].shape[1]))


@pytest.mark.parametrize("name", ["base", "s70"])
def test_the_wide_and_the_long_case_end_some_hypotheses(searched, name):
    c, (out, ln, tot, sc, al), trace, _ = searched(name)
    assert trace["reorders"] >= 1 and len(trace["carried_beside_live"]) >= 1
    assert (ln < BC.tmax_of(c.S)).any() and (ln == BC.tmax_of(c.S)).any()


def test_crafted_rows_hold_the_edges(searched):
    logits, totals, flags, eos, ids = BC.crafted_step(4097, 8, 3)
    k = 8
    rows = np.arange(k, 2 * k)
    assert np.isnan(logits[rows[3]]).any() and np.isneginf(logits[rows[4]]).all() and np.isposinf(logits[rows[5]]).any()
    assert flags[rows[2]] == BC.FINISHED and flags[rows[6]] == BC.DEAD
    assert np.array_equal(logits[rows[0]], logits[rows[1]]) and totals[rows[0]] == totals[rows[1]]
    z = logits[rows[7]]
    assert z[3] == 0 and z[9] == 0 and np.signbit(z[9]) and not np.signbit(z[3])
    assert (flags[2 * k + 1:3 * k] == BC.DEAD).all() and np.isfinite(logits[2 * k]).sum() == 2
    t0, f0 = BC.start_state(1, k)
    assert np.array_equal(totals[:k].view(np.uint32), t0.view(np.uint32)) and np.array_equal(flags[:k], f0)
    assert ids is not None and sorted(ids.tolist()) == list(range(4097))
    assert BC.crafted_step(1, 3, 1)[4] is None
