"""CPU-side checks of the candidate entry points (include/slimt_hip.h, slimt_hip_score_candidates* and
slimt_hip_candidates_rank*): declared, exported and wrapped; NULL arguments, mismatched shapes and values the host can check
are refused before anything reaches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["slimt_hip_score_candidates", "slimt_hip_score_candidates_async", "slimt_hip_score_candidates_device",
         "slimt_hip_score_candidates_async_generated", "slimt_hip_candidates_rank", "slimt_hip_candidates_rank_device"]


def test_declared_exported_and_wrapped():
    from slimt_amd import build, capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slimt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(slimt_hip_[a-z0-9_]+)\s*\(", text))
    dll = ctypes.CDLL(build.build())
    for n in NAMES:
        assert n in declared and n in capi.SYMBOLS and hasattr(dll, n), n
    for w in ("score_candidates", "score_candidates_async", "score_candidates_device", "candidates_rank_device"):
        assert callable(getattr(capi.Context, w)), w
    assert callable(capi.candidates_rank) and capi.CANDIDATE_RUN >= 2
    assert capi.lib().slimt_hip_abi_version() == 3


def test_every_entry_point_refuses_null():
    from slimt_amd import capi
    L = capi.lib()
    n = None
    calls = [lambda: L.slimt_hip_score_candidates(n, n, n, 1, 1, n, 0, n, n, 1, n, 1, n, n),
             lambda: L.slimt_hip_score_candidates_async(n, n, n, 1, 1, n, 0, n, n, 1, n, 1, n, n),
             lambda: L.slimt_hip_score_candidates_device(n, n, n, 1, 1, n, 0, n, n, 1, n, 1, n, n),
             lambda: L.slimt_hip_score_candidates_async_generated(n, n, n, n, 1, 1, n, n, 1, n, 1, n, n),
             lambda: L.slimt_hip_candidates_rank(n, n, n, 1, 1, 1, 0, n, n),
             lambda: L.slimt_hip_candidates_rank_device(n, n, n, n, 1, 1, 1, 0, n, n)]
    for call in calls:
        assert call() != 0
        assert b"null argument" in L.slimt_hip_last_error()


def test_rank_refuses_what_the_host_can_check():
    """slimt_hip_candidates_rank is stateless: its checks come before its first device call, so they hold without a GPU"""
    from slimt_amd import capi
    sc = np.zeros((3, 4), np.float32)
    ok_len, ok_src = np.array([4, 0, 2], np.uint32), np.array([0, 1, 1], np.uint32)
    with pytest.raises(capi.SlimtHipError, match="candidate 2 names source 2 of 2"):
        capi.candidates_rank(sc, ok_len, np.array([0, 1, 2], np.uint32), 2)
    with pytest.raises(capi.SlimtHipError, match="length 5 of candidate 0 > T 4"):
        capi.candidates_rank(sc, np.array([5, 0, 2], np.uint32), ok_src, 2)
    for mode in (2, -1):
        with pytest.raises(capi.SlimtHipError, match="neither 0 .sum. nor 1"):
            capi.candidates_rank(sc, ok_len, ok_src, 2, mode=mode)
    with pytest.raises(capi.SlimtHipError, match="0 sources"):
        capi.candidates_rank(sc, ok_len, ok_src, 0)
    with pytest.raises(ValueError, match="scores .N, T., tgt_len .N. and cand_src .N. expected"):
        capi.candidates_rank(sc, ok_len[:2], ok_src, 2)
    with pytest.raises(ValueError):
        capi.candidates_rank(sc[0], ok_len, ok_src, 2)


class _NoContext:
    """the wrappers' own checks come before the handle is used"""
    h = None
    _candidates_host = staticmethod(__import__("slimt_amd.capi", fromlist=["Context"]).Context._candidates_host)


def test_wrappers_refuse_mismatched_shapes():
    from slimt_amd import capi
    ids, lens = np.ones((2, 5), np.uint32), np.array([5, 3], np.uint32)
    t_ids, t_len, src = np.ones((3, 4), np.uint32), np.array([4, 0, 2], np.uint32), np.array([0, 1, 1], np.uint32)
    for bad in ((ids, lens, t_ids, t_len[:2], src), (ids, lens, t_ids, t_len, src[:2]), (ids, lens[:1], t_ids, t_len, src),
                (ids[0], lens, t_ids, t_len, src), (ids, lens, t_ids[0], t_len, src)):
        with pytest.raises(ValueError, match="score_candidates"):
            capi.Context.score_candidates(_NoContext(), bad[0], bad[1], None, bad[2], bad[3], bad[4])
    sc = np.zeros((3, 4), np.float32)
    for bufs in ((ids, lens, t_ids, t_len, src[:2], sc, None), (ids, lens, t_ids, t_len, src, sc[:2], None),
                 (ids, lens, t_ids, t_len, src.astype(np.int64), sc, None),
                 (ids, lens, t_ids, t_len, src, sc, np.zeros((3, 4, 4), np.float32))):
        with pytest.raises(ValueError, match="score_candidates_async"):
            capi.Context.score_candidates_async(_NoContext(), bufs)


def test_host_check_of_cand_src_comes_before_the_device():
    """with a GPU the refusal is the engine's message; without one no context exists, and the call is refused as a null
    context before anything else -- either way nothing reaches a device"""
    from slimt_amd import capi, synth
    ids, lens = np.ones((2, 5), np.uint32), np.array([5, 3], np.uint32)
    t_ids, t_len, src = np.ones((3, 4), np.uint32), np.array([4, 0, 2], np.uint32), np.array([0, 1, 2], np.uint32)
    if capi.device_count() == 0:
        with pytest.raises(capi.SlimtHipError, match="null argument"):
            capi.Context.score_candidates(_NoContext(), ids, lens, None, t_ids, t_len, src)
        return
    gm = capi.Model(synth.make_model("micro"))
    ctx = capi.Context(gm, 2, 5)
    try:
        with pytest.raises(capi.SlimtHipError, match="candidate 2 names source 2, the batch has 2"):
            ctx.score_candidates(ids, lens, None, t_ids, t_len, src)
        with pytest.raises(capi.SlimtHipError, match="target length 9 of sentence 0 > T 4"):
            ctx.score_candidates(ids, lens, None, t_ids, np.array([9, 0, 2], np.uint32), np.array([0, 1, 1], np.uint32))
    finally:
        ctx.close()
        gm.close()


def test_service_header_declares_its_two_and_the_host_library_exports_them():
    """include/slimt_hip_service_candidates.h against libslimt_hip_host.so; slimt_hip_service.h keeps its six (test_capi_symbols)"""
    from slimt_amd import build, capi
    build.build_host_lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slimt_hip_service_candidates.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(slimt_hip_(?:service|result)_[a-z0-9_]+)\s*\(", text)))
    assert names == ["slimt_hip_result_candidates", "slimt_hip_service_score_candidates"]
    H = capi.host_lib()
    for n in names:
        assert hasattr(H, n), n
    out = ctypes.c_void_p()
    assert H.slimt_hip_service_score_candidates(None, None, None, 0, None, None, None, 0, ctypes.byref(out)) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert H.slimt_hip_result_candidates(None, None, None) != 0
    assert b"null argument" in H.slimt_hip_service_last_error()
    assert callable(capi.BatchService.score_candidates) and callable(capi.ServiceResult.candidates)
    from slimt_amd import frontend
    assert callable(frontend.Service.rerank)
