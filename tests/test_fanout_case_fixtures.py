"""CPU checks of the fan-out cases (tests/support/fanout_cases.py) and of the fan-out API's surface: each parity case can
catch the bugs it is for -- shown on the oracle, with the checkers the GPU test uses --, the tiling edges sit where their names
say, the symbols are declared, exported and wrapped, and the host entry points refuse bad arguments without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from support import fanout_cases as FC
from test_sampling_checker import keys_of, sampled_translate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_issues_three_cases_are_in_the_table():
    rows = {c.name: (c.preset, c.eos_bias, c.S, c.B, c.row_src.tolist(), c.n_sl, c.seed, c.key_seed) for c in FC.PARITY}
    assert rows["s8"] == ("tiny11", 6.0, 8, 5, np.repeat(np.arange(5), 4).tolist(), 4096, 61 + 8 + 5, 8 + 5)
    assert rows["s32"] == ("tiny11", 6.0, 32, 5, np.repeat(np.arange(5), 7).tolist(), 4096, 61 + 32 + 5, 32 + 5)
    assert rows["full"] == ("tiny11", 7.0, 8, 3, np.repeat(np.arange(3), 6).tolist(), None, 61 + 8 + 3, 8 + 3)
    assert FC.TEMPERATURES == (0.7, 1.0)
    # what the other cases are in the table for
    assert FC.parity("s64").S == 64 and FC.parity("s100").S == 100 and FC.parity("s100").row_src.size == 3
    assert FC.parity("base32").preset == "base" and FC.parity("base32").S == 32
    D, _, H = FC.parity("dh16").dims[:3]
    assert D // H == 16 and 2 in set(range(FC.parity("dh16").B)) - set(FC.parity("dh16").row_src.tolist())


@pytest.fixture(scope="module")
def greedy(oracle, synth_models):
    cache = {}

    def get(c):
        if c.name not in cache:
            m = FC.model_of(c, synth_models)
            om = oracle.OracleModel(m)
            ids, lens, sl, keys = FC.inputs(c, m.V)
            oracle.set_mode(oracle.PORTABLE)
            try:
                out, ln, _, _ = om.translate(ids, lens, sl, 1.5, 0, want_align=True)
            finally:
                oracle.set_mode(oracle.FAITHFUL)
            cache[c.name] = (m, om, ids, lens, sl, keys, [tuple(out[b, :ln[b]]) for b in range(c.B)])
        return cache[c.name]

    return get


def _sequences(out, ln):
    return [tuple(out[r, :ln[r]]) for r in range(len(ln))]


@pytest.mark.parametrize("T", FC.TEMPERATURES)
@pytest.mark.parametrize("name", [c.name for c in FC.PARITY])
def test_a_sampled_case_shows_wrong_keys_wrong_sources_and_wrong_lengths(oracle, greedy, name, T):
    c = FC.parity(name)
    m, om, ids, lens, sl, keys, greedy_seqs = greedy(c)
    # (b) under greedy no two sources translate alike: a wrong row_src lookup cannot hide
    assert len(set(greedy_seqs)) == c.B
    d_ids, d_lens = FC.duplicated(ids, lens, c.row_src)
    out, ln, al, _ = sampled_translate(oracle, om, m, d_ids, d_lens, sl, keys, T)
    seqs = _sequences(out, ln)
    # (a) every source with two rows or more has two rows that differ: a wrong key or row index cannot hide
    for b in range(c.B):
        rows = np.nonzero(c.row_src == b)[0]
        if rows.size >= 2:
            assert len({seqs[r] for r in rows}) >= 2, (b, rows)
    # (c) three different lengths or more at S = 32: a wrong per-row length or finished flag cannot hide
    if c.S == 32:
        assert name not in FC.EXEMPT_FROM_C and len(set(ln.tolist())) >= 3, sorted(set(ln.tolist()))
    # ... and the bugs themselves, on the checker: the row index for the key, and the next source for the row's own
    by_row = sampled_translate(oracle, om, m, d_ids, d_lens, sl, None, T)
    assert _sequences(by_row[0], by_row[1]) != seqs
    used = np.unique(c.row_src)
    if used.size >= 2:
        nxt = used[(np.searchsorted(used, c.row_src) + 1) % used.size]
        w_ids, w_lens = FC.duplicated(ids, lens, nxt)
        wrong = sampled_translate(oracle, om, m, w_ids, w_lens, sl, keys, T)
        differs = [seqs[r] != s or not np.array_equal(al[r], wrong[2][r]) for r, s in enumerate(_sequences(wrong[0], wrong[1]))]
        assert all(differs), differs


def test_the_exempt_cases_are_the_issues_two_at_eight_tokens():
    assert FC.EXEMPT_FROM_C == {"s8", "full"} and all(FC.parity(n).S == 8 for n in FC.EXEMPT_FROM_C)


def test_edges_sit_where_their_names_say():
    e = FC.edges()
    assert all(int(v.max()) < FC.EDGE_B for v in e.values())
    assert [e[k].size for k in ("n1", "n16", "n17", "n33")] == [1, 16, 17, 33]
    runs = {k: FC.runs_of(v) for k, v in e.items()}
    # n17: source 4's run of four starts at row 13 and is cut at the workgroup boundary: rows 13-15, then row 16 alone
    assert runs["n17"][-2:] == [(13, 3, 4), (16, 1, 4)]
    # n33: runs cut at rows 16 and 32; the last workgroup holds one row and fifteen dead waves
    assert [r for r in runs["n33"] if r[0] in (16, 32)] == [(16, 4, 2), (32, 1, 4)] and runs["n33"][-1] == (32, 1, 4)
    # run20: source 1 owns rows 2 .. 21: staged in workgroup 0 for 14 rows and again in workgroup 1 for 6
    assert (2, 14, 1) in runs["run20"] and (16, 6, 1) in runs["run20"] and (e["run20"] == 1).sum() == 20
    assert runs["arange"] == [(i, 1, i) for i in range(FC.EDGE_B)]
    assert len(runs["shuffled"]) > len(runs["n33"]) and sorted(e["shuffled"].tolist()) == e["n33"].tolist()
    for k, missing in (("none_first", 0), ("none_middle", 2), ("none_last", FC.EDGE_B - 1)):
        assert set(range(FC.EDGE_B)) - set(e[k].tolist()) == {missing}
    assert np.all(np.diff(e["reversed"].astype(np.int64)) <= 0)
    one = FC.single_source()
    assert one.B == 1 and one.row_src.size == 17 and FC.runs_of(one.row_src) == [(0, 16, 0), (16, 1, 0)]
    assert FC.one_token().S == 1


# ---- the API's surface (no device needed) ----------------------------------------------------------------------------------
FANOUT = ["slimt_hip_translate_fanout", "slimt_hip_translate_fanout_async", "slimt_hip_translate_fanout_device",
          "slimt_hip_translate_fanout_async_generated"]


def test_fanout_symbols_are_declared_exported_and_wrapped():
    from slimt_amd import capi, frontend
    header = open(os.path.join(ROOT, "include", "slimt_hip.h")).read()
    L = capi.lib()
    for name in FANOUT:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(L, name).argtypes is not None, name
    assert "a source without rows still contributes" in header and "THE CONTRACT" in header
    for name in ("translate_fanout", "translate_fanout_async", "translate_fanout_pinned", "translate_fanout_device"):
        params = inspect.signature(getattr(capi.Context, name)).parameters
        for option in ("scores", "prefix", "sampling", "truncation"):
            assert option in params, (name, option)
    assert "samples" in inspect.signature(frontend.Service.translate).parameters
    assert inspect.signature(frontend.Service.sample_and_rerank).parameters["n"]
    assert inspect.signature(capi.BatchService.translate_samples).parameters["seed"].default == 0


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_host_entry_points_fail_loudly_on_bad_arguments():
    from slimt_amd import capi
    L = capi.lib()
    ids, lens = np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32)
    out, ol = np.zeros((3, 6), np.uint32), np.zeros(3, np.uint32)
    src = np.asarray([0, 1, 1], np.uint32)

    def call(fn, ctx, row_src, N, generated=False):
        mid = () if generated else (None, 0)
        head = (ctx, None) if generated else (ctx,)
        return fn(*head, _p(ids), _p(lens), 2, 4, _p(row_src), N, *mid, 1.5, 0, _p(out), _p(ol), None)

    for fn, generated in ((L.slimt_hip_translate_fanout, False), (L.slimt_hip_translate_fanout_async, False),
                          (L.slimt_hip_translate_fanout_async_generated, True)):
        assert call(fn, None, src, 3, generated) != 0
        assert b"null argument" in L.slimt_hip_last_error()
    for fn in (L.slimt_hip_translate_fanout, L.slimt_hip_translate_fanout_async):
        assert call(fn, None, src, 0) != 0
        assert b"N = 0" in L.slimt_hip_last_error()
        bad = np.asarray([0, 1, 2], np.uint32)
        assert call(fn, None, bad, 3) != 0
        assert b"row 2 names source 2" in L.slimt_hip_last_error()
        assert call(fn, None, None, 3) != 0
        assert b"null argument" in L.slimt_hip_last_error()
    assert L.slimt_hip_translate_fanout_device(None, _p(ids), _p(lens), 2, 4, _p(src), 3, None, 0, 1.5, 0, _p(out), _p(ol), None, 0) != 0
    assert b"null argument" in L.slimt_hip_last_error()


def test_wrappers_check_shapes():
    from slimt_amd import capi
    ctx = capi.Context.__new__(capi.Context)  # (no device: the checks come before the library is called)
    ctx.h = None
    with pytest.raises(ValueError, match="row_src"):
        ctx.translate_fanout(np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32), np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError, match="keys of shape"):
        ctx.translate_fanout(np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32), np.zeros(3, np.uint32),
                             sampling=(1.0, np.zeros(2, np.uint64)))
    with pytest.raises(ValueError, match="prefix"):
        ctx.translate_fanout(np.ones((2, 4), np.uint32), np.full(2, 4, np.uint32), np.zeros(3, np.uint32),
                             prefix=(np.zeros((2, 6), np.uint32), np.zeros(2, np.uint32)))


def test_service_samples_header_is_exported_and_refuses_null_arguments():
    from slimt_amd import capi
    header = open(os.path.join(ROOT, "include", "slimt_hip_service_samples.h")).read()
    H = capi.host_lib()
    names = re.findall(r"\bint (slimt_hip_\w+)\(", header)
    assert names == ["slimt_hip_service_translate_samples", "slimt_hip_result_samples"]
    for name in names:
        assert getattr(H, name).argtypes is not None, name
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_translate_samples(None, None, None, 0, 2, 0, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert H.slimt_hip_result_samples(None, None) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
