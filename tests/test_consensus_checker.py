"""The consensus selection (include/slimt_hip.h, slimt_hip_consensus_select*) on the CPU: the reference of
tests/support/consensus_ref.py on hand-made rows with known answers, and the new entry points -- declared, exported and
wrapped; values the host can check are refused before anything reaches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from support import consensus_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["slimt_hip_consensus_select", "slimt_hip_consensus_select_device", "slimt_hip_ctx_set_fanout_consensus"]
A, B, C, D, E, F = 11, 12, 13, 14, 15, 16


def _pack(rows, T=None):
    T = T or max(1, max(len(r) for r in rows))
    ids = np.zeros((len(rows), T), np.uint32)
    for c, r in enumerate(rows):
        ids[c, :len(r)] = r
    return ids, np.asarray([len(r) for r in rows], np.uint32)


# ---- the reference on rows with known answers -----------------------------------------------------------------------------
@pytest.mark.parametrize("beta2", [1, 4, 16])
@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_identical_rows_score_one_at_every_counted_order(G, beta2):
    row = [A, B, A, C, D]
    u, scores = R.pair_utility(row, list(row), G, beta2)
    assert scores == [1.0] * G and u == 1.0
    util, best = R.select(*_pack([row, row, row]), np.zeros(3, np.uint32), 1, G, beta2)
    assert list(util) == [1.0, 1.0, 1.0] and list(best) == [0]


def test_rows_with_no_common_token_score_zero():
    u, scores = R.pair_utility([A, B, C], [D, E, F, D], 4, 4)
    assert u == 0.0 and scores == [0.0, 0.0, 0.0, 0.0]


def test_counts_are_clipped():
    assert R.match_count([A, A, A], [A, A], 1) == 2
    assert R.match_count([A, A, A], [A, A], 2) == 1
    assert R.match_count([A, A, A], [A, A], 3) == 0
    # F_1 = (1 + 4) * 2 / (4 * 2 + 3), F_2 = 5 * 1 / (4 * 1 + 2), order 3 counts (c_3(h) = 1) and scores 0
    u, scores = R.pair_utility([A, A, A], [A, A], 4, 4)
    assert scores == [10.0 / 11.0, 5.0 / 6.0, 0.0] and u == ((10.0 / 11.0 + 5.0 / 6.0) + 0.0) / 3.0


def test_match_counts_are_symmetric_and_beta2_one_makes_the_utility_symmetric():
    rnd = np.random.default_rng(2)
    for _ in range(50):
        h = [int(t) for t in rnd.integers(1, 4, size=rnd.integers(1, 12))]
        r = [int(t) for t in rnd.integers(1, 4, size=rnd.integers(1, 12))]
        for g in (1, 2, 3, 4):
            assert R.match_count(h, r, g) == R.match_count(r, h, g)
        assert R.pair_utility(h, r, 4, 1) == R.pair_utility(r, h, 4, 1)


def test_beta2_four_is_not_symmetric_on_rows_of_unequal_length():
    h, r = [A, B, C], [A, B, C, D, E, F]
    uh, ur = R.pair_utility(h, r, 2, 4)[0], R.pair_utility(r, h, 2, 4)[0]
    # M_1 = 3, M_2 = 2: F(h, r) = 15 / (24 + 3), 10 / (20 + 2); F(r, h) = 15 / (12 + 6), 10 / (8 + 5)
    assert uh == (15.0 / 27.0 + 10.0 / 22.0) / 2.0 and ur == (15.0 / 18.0 + 10.0 / 13.0) / 2.0 and uh != ur


def test_orders_longer_than_both_rows_are_skipped():
    u, scores = R.pair_utility([A, B], [A], 4, 1)
    assert scores == [2.0 / 3.0, 0.0] and u == (2.0 / 3.0 + 0.0) / 2.0  # order 2 counts: h has one bigram; 3 and 4 do not
    u, scores = R.pair_utility([A], [A], 4, 4)
    assert scores == [1.0] and u == 1.0
    assert R.pair_utility([], [], 4, 4) == (0.0, [])


def test_a_tie_goes_to_the_lower_row_and_empty_rows_do_not_compete():
    rows = [[D, E], [], [A, B, C], [A, B, C], [A, B, F]]
    src = np.array([1, 1, 1, 1, 1], np.uint32)
    util, best = R.select(*_pack(rows), src, 3, 4, 4)
    assert util[2] == util[3] > util[4] > util[0] == 0.0 and util[1] == 0.0
    assert list(best) == [R.NO_ROW, 2, R.NO_ROW]
    # a lone competing row: utility 0 and the best; a source of empty rows: none
    util, best = R.select(*_pack([[A], [], []]), np.array([0, 0, 1], np.uint32), 2)
    assert list(util) == [0.0, 0.0, 0.0] and list(best) == [0, R.NO_ROW]
    assert not np.isnan(util).any()


def test_lengths_are_clamped_to_the_row_and_ids_compared_in_full():
    ids = np.array([[5, 7], [65536 + 5, 7]], np.uint32)
    util, _ = R.select(ids, np.array([9, 2], np.uint32), np.zeros(2, np.uint32), 1, 1, 1)
    assert list(util) == [0.5, 0.5]  # (one of two unigrams matches: 5 and 65541 are different tokens)


# ---- the entry points --------------------------------------------------------------------------------------------------------
def test_declared_exported_and_wrapped():
    from slimt_amd import build, capi, frontend
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slimt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(slimt_hip_[a-z0-9_]+)\s*\(", text))
    dll = ctypes.CDLL(build.build())
    for n in NAMES:
        assert n in declared and n in capi.SYMBOLS and hasattr(dll, n), n
    for w in ("consensus_select_device", "set_fanout_consensus", "translate_fanout", "translate_fanout_async",
              "translate_fanout_pinned", "translate_fanout_device"):
        assert callable(getattr(capi.Context, w)), w
    assert callable(capi.consensus_select)
    assert (capi.CONSENSUS_MAX_ORDER, capi.CONSENSUS_MAX_BETA2, capi.CONSENSUS_MAX_ROWS, capi.CONSENSUS_MAX_T) == (4, 16, 64, 256)
    for macro, value in (("MAX_ORDER", 4), ("MAX_BETA2", 16), ("MAX_ROWS", 64), ("MAX_T", 256)):
        assert re.search(r"#define SLIMT_HIP_CONSENSUS_%s %d\b" % (macro, value), text), macro
    assert capi.lib().slimt_hip_abi_version() == 3
    assert callable(capi.BatchService.translate_consensus) and callable(capi.ServiceResult.consensus)
    assert callable(frontend.Service.sample_and_select) and callable(frontend.Service.sample_and_rerank)


def test_service_header_declares_its_two_and_the_host_library_exports_them():
    from slimt_amd import build, capi
    build.build_host_lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slimt_hip_service_consensus.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(slimt_hip_(?:service|result)_[a-z0-9_]+)\s*\(", text)))
    assert names == ["slimt_hip_result_consensus", "slimt_hip_service_translate_consensus"]
    H = capi.host_lib()
    for n in names:
        assert hasattr(H, n), n
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_translate_consensus(None, None, None, 0, 2, 0, 4, 4, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert H.slimt_hip_result_consensus(None, None, None) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()


def test_arming_refuses_bad_values_at_once():
    """the values are checked before the context: these refusals hold without a GPU, and say what is wrong"""
    from slimt_amd import capi
    L = capi.lib()
    best, util = np.zeros(2, np.uint32), np.zeros(4, np.float64)
    pb, pu = best.ctypes.data_as(ctypes.c_void_p), util.ctypes.data_as(ctypes.c_void_p)
    for args, message in (((0, 4, pb, pu), b"max_order 0 disarms and takes no arrays"),
                          ((5, 4, pb, pu), b"max_order 5 is not in 1..4"),
                          ((-1, 4, pb, pu), b"max_order -1 is not in 1..4"),
                          ((4, 0, pb, pu), b"beta2 0 is not in 1..16"),
                          ((4, 17, pb, pu), b"beta2 17 is not in 1..16"),
                          ((4, 4, None, pu), b"best or utility is NULL"),
                          ((4, 4, pb, None), b"best or utility is NULL"),
                          ((4, 4, pb, pu), b"null argument"),      # (good values: only the context is missing)
                          ((0, 0, None, None), b"null argument")):  # (disarming: the same)
        assert L.slimt_hip_ctx_set_fanout_consensus(None, *args) != 0, args
        assert message in L.slimt_hip_last_error(), (args, L.slimt_hip_last_error())


def test_select_refuses_what_the_host_can_check():
    """slimt_hip_consensus_select is stateless: its checks come before its first device call, so they hold without a GPU"""
    from slimt_amd import capi
    ids, lens = _pack([[A, B, C], [A, B], [A]], 4)
    src = np.array([0, 1, 1], np.uint32)
    with pytest.raises(capi.SlimtHipError, match="row 2 names source 2 of 2"):
        capi.consensus_select(ids, lens, np.array([0, 1, 2], np.uint32), 2)
    with pytest.raises(capi.SlimtHipError, match="length 5 of row 0 > T 4"):
        capi.consensus_select(ids, np.array([5, 2, 1], np.uint32), src, 2)
    for G in (0, 5):
        with pytest.raises(capi.SlimtHipError, match="max_order %d is not in 1..4" % G):
            capi.consensus_select(ids, lens, src, 2, max_order=G)
    for b2 in (0, 17):
        with pytest.raises(capi.SlimtHipError, match="beta2 %d is not in 1..16" % b2):
            capi.consensus_select(ids, lens, src, 2, beta2=b2)
    with pytest.raises(capi.SlimtHipError, match="0 sources"):
        capi.consensus_select(ids, lens, src, 0)
    with pytest.raises(capi.SlimtHipError, match="exceed the limits"):
        capi.consensus_select(np.zeros((1, 257), np.uint32), np.ones(1, np.uint32), np.zeros(1, np.uint32), 1)
    many = np.zeros((65, 2), np.uint32)
    with pytest.raises(capi.SlimtHipError, match="source 1 has more than 64 rows"):
        capi.consensus_select(many, np.ones(65, np.uint32), np.ones(65, np.uint32), 2)
    with pytest.raises(ValueError, match="ids .N, T., lengths .N. and row_src .N. expected"):
        capi.consensus_select(ids, lens[:2], src, 2)


def test_without_a_device_the_entry_points_fail_with_an_error_code():
    from slimt_amd import capi
    L = capi.lib()
    n = None
    assert L.slimt_hip_consensus_select(n, n, n, 1, 1, 1, 4, 4, n, n) != 0
    assert b"null argument" in L.slimt_hip_last_error()
    assert L.slimt_hip_consensus_select_device(n, n, n, n, 1, 1, 1, 4, 4, n, n) != 0
    assert b"null argument" in L.slimt_hip_last_error()
    if capi.device_count() == 0:
        ids, lens = _pack([[A, B, C], [A, B]], 4)
        with pytest.raises(capi.SlimtHipError):
            capi.consensus_select(ids, lens, np.zeros(2, np.uint32), 1)
