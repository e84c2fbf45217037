"""CPU-side checks of the fused decoder's concurrency plan (slimt_amd/csrc/decoder_plan.h), compiled here for the host
from the same header the engine includes: decoders in flight are min(pending contexts, hardware queues); with four
queues the headline takes the 8-sentence tiling without admission waits and keeps its K/V caches temporal; with as many
queues as contexts the plan is exactly the one the engine made before the queue count was known."""
import ctypes
import itertools
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include "decoder_plan.h"
using namespace slimt_hip;
// in: B, S, Ld, rows, adaptive, narrow_ok, contexts, queues, budget, kv_policy, kv_grain, by_launch
// din: kv_bytes, pending_kv, rows_oversub, kv_budget, launch_budget
// out: rows, wgs, in_flight, queue_bound, n, wait, eighths, by_launch, k
extern "C" void plan(const long long *in, const double *din, long long *out) {
  DecoderPlanIn p;
  p.B = (int)in[0]; p.S = (int)in[1]; p.Ld = (int)in[2]; p.rows = (int)in[3];
  p.adaptive = in[4] != 0; p.narrow_ok = in[5] != 0; p.contexts = (size_t)in[6]; p.queues = (int)in[7];
  p.budget = (int)in[8]; p.kv_policy = (int)in[9]; p.kv_grain = (int)in[10]; p.by_launch = (int)in[11];
  p.kv_bytes = din[0]; p.pending_kv = din[1]; p.rows_oversub = din[2]; p.kv_budget = din[3]; p.launch_budget = din[4];
  const DecoderPlan r = decoder_plan(p);
  out[0] = r.rows; out[1] = r.wgs; out[2] = (long long)r.in_flight; out[3] = r.queue_bound; out[4] = (long long)r.n;
  out[5] = r.wait; out[6] = r.eighths; out[7] = r.by_launch; out[8] = r.k;
}
"""

KEYS = ["rows", "wgs", "in_flight", "queue_bound", "n", "wait", "eighths", "by_launch", "k"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("decoder_plan")
    src = d / "h.cc"
    src.write_text(_HARNESS)
    so = d / "h.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "slimt_amd", "csrc"), str(src), "-o", str(so)])
    h = ctypes.CDLL(str(so))
    h.plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    h.plan.restype = None
    return h


def plan(h, B=256, S=32, Ld=2, rows=16, adaptive=True, narrow_ok=True, contexts=20, queues=4, budget=224,
         kv_policy=0, kv_grain=8, by_launch=-1, kv_bytes=None, pending_kv=None, rows_oversub=1.0, kv_budget=300e6,
         launch_budget=300e6):
    if kv_bytes is None:
        kv_bytes = Ld * 2.0 * B * S * 256 * 2.0  # the tight form (2 bytes per value), D = 256
    if pending_kv is None:
        pending_kv = kv_bytes * contexts
    i = (ctypes.c_longlong * 12)(B, S, Ld, rows, int(adaptive), int(narrow_ok), contexts, queues, budget,
                                 kv_policy, kv_grain, by_launch)
    d = (ctypes.c_double * 5)(kv_bytes, pending_kv, rows_oversub, kv_budget, launch_budget)
    o = (ctypes.c_longlong * 9)()
    h.plan(i, d, o)
    return dict(zip(KEYS, list(o)))


def previous_plan(B, S, Ld, rows, adaptive, narrow_ok, contexts, budget, kv_policy, kv_bytes, pending_kv,
                  rows_oversub=1.0, kv_budget=300e6, kv_grain=8, by_launch=-1, launch_budget=300e6):
    """What engine.cpp computed before the queue count was known (every pending context a decoder in flight)."""
    if adaptive and narrow_ok and rows == 16:
        for spw in (4, 8):
            if contexts * -(-B // spw) <= rows_oversub * budget:
                rows = spw
                break
    wgs = -(-B // rows)
    n = min(max(1, budget // wgs), 64)
    active = pending_kv / contexts * min(contexts, n)
    al = 8 * Ld
    e = al if kv_policy == 1 else 0 if kv_policy == 2 else int(min(al, math.floor(al * kv_budget / active)))
    if kv_policy == 0:
        e = e // kv_grain * kv_grain
    bl, k = False, 8
    if kv_policy == 0 and by_launch != 0 and e < al and S <= 32 and 4.0 * kv_bytes <= launch_budget:
        bl = True
        k = min(by_launch, 8) if by_launch > 0 else int(min(8.0, math.floor(8.0 * launch_budget / active)))
    return dict(rows=rows, wgs=wgs, n=n, eighths=e, by_launch=int(bl), k=k)


def test_headline_at_four_queues_takes_the_narrow_tiling(harness):
    """20 contexts x B = 256, S = 32 (tight K/V form) at the runtime's default four queues: four decoders in flight,
    8 sentences per workgroup (4 x 32 workgroups within the 224 of the budget), no admission waits, every cache
    temporal."""
    p = plan(harness, contexts=20, queues=4)
    assert p == dict(rows=8, wgs=32, in_flight=4, queue_bound=1, n=7, wait=0, eighths=16, by_launch=0, k=8)
    # the narrow (20-bit) and 24-bit forms: four batches' caches still fit, the same plan
    for bpv in (2.5, 3.0):
        q = plan(harness, contexts=20, queues=4, kv_bytes=2 * 2.0 * 256 * 32 * 256 * bpv)
        assert q == p
    # more room (a larger budget, or oversubscription asked for): four launches of 4 sentences, still no waits
    p = plan(harness, contexts=20, queues=4, budget=256)
    assert (p["rows"], p["wgs"], p["n"], p["wait"]) == (4, 64, 4, 0)


def test_headline_at_32_queues_keeps_the_previous_plan(harness):
    """GPU_MAX_HW_QUEUES = 32: twenty decoders in flight, 16 sentences per workgroup, n = 14 with waits; the 24-bit
    form's 352 MB in flight are kept by launch (k = 6 of 8)."""
    p = plan(harness, contexts=20, queues=32)
    assert p == dict(rows=16, wgs=16, in_flight=20, queue_bound=0, n=14, wait=1, eighths=16, by_launch=0, k=8)
    kv24 = 2 * 2.0 * 256 * 32 * 256 * 3.0
    p = plan(harness, contexts=20, queues=32, kv_bytes=kv24)
    assert p == dict(rows=16, wgs=16, in_flight=20, queue_bound=0, n=14, wait=1, eighths=8, by_launch=1, k=6)
    # the same 24-bit batches at four queues: four in flight hold 101 MB, nothing is streamed
    assert plan(harness, contexts=20, queues=4, kv_bytes=kv24)["by_launch"] == 0


def test_fewer_contexts_than_queues_behaves_as_before(harness):
    """Contexts <= queues: every pending context is a decoder in flight, the budget is the admission's 7/8."""
    p = plan(harness, contexts=3, queues=4)
    assert p == dict(rows=4, wgs=64, in_flight=3, queue_bound=0, n=3, wait=1, eighths=16, by_launch=0, k=8)
    p = plan(harness, contexts=4, queues=4)  # 4 x 64 > 224: the 8-sentence tiling, as before (waits on)
    assert (p["rows"], p["n"], p["wait"], p["queue_bound"]) == (8, 7, 1, 0)


@pytest.mark.parametrize("queues", [4, 8, 32])
def test_plan_equals_the_previous_one_when_queues_do_not_bind(harness, queues):
    shapes = [(256, 32, 2), (64, 32, 2), (512, 32, 2), (128, 64, 2), (4096, 32, 2), (20, 12, 2), (256, 128, 4)]
    for (B, S, Ld), contexts, rows, adaptive, narrow_ok, kv_policy, bpv, budget in itertools.product(
            shapes, range(1, queues + 1), (16, 32, 8), (True, False), (True, False), (0, 1, 2), (2.0, 3.0, 4.0),
            (224, 64, 1000)):
        kv = Ld * 2.0 * B * S * 256 * bpv
        pend = kv * contexts * 1.25  # other contexts' shapes may differ
        got = plan(harness, B=B, S=S, Ld=Ld, rows=rows, adaptive=adaptive, narrow_ok=narrow_ok, contexts=contexts,
                   queues=queues, budget=budget, kv_policy=kv_policy, kv_bytes=kv, pending_kv=pend)
        want = previous_plan(B, S, Ld, rows, adaptive, narrow_ok, contexts, budget, kv_policy, kv, pend)
        assert got["in_flight"] == contexts and got["queue_bound"] == 0 and got["wait"] == 1
        assert {k: got[k] for k in want} == want, (B, S, Ld, contexts, rows, adaptive, narrow_ok, kv_policy, bpv, budget)


def test_queue_bound_waits_only_where_the_chip_would_be_oversubscribed(harness):
    """A batch of 4096 at 16 sentences is 256 workgroups, the whole chip: four of them must still be admitted one by
    one (n = 1, waits on), whatever the queues allow."""
    p = plan(harness, B=4096, contexts=20, queues=4, adaptive=False)
    assert (p["rows"], p["wgs"], p["n"], p["wait"], p["in_flight"]) == (16, 256, 1, 1, 4)
    # B = 512 at 16: 32 workgroups, seven fit the budget -> no waits
    p = plan(harness, B=512, contexts=20, queues=4, adaptive=False)
    assert (p["n"], p["wait"]) == (7, 0)
    # B = 1024 at 16: 64 workgroups, three fit -> launch k waits for k - 3
    p = plan(harness, B=1024, contexts=20, queues=4, adaptive=False)
    assert (p["n"], p["wait"]) == (3, 1)
    # a smaller budget is kept
    p = plan(harness, contexts=20, queues=4, budget=64)
    assert (p["rows"], p["n"], p["wait"]) == (16, 4, 0)
    p = plan(harness, contexts=20, queues=4, budget=48)
    assert (p["rows"], p["n"], p["wait"]) == (16, 3, 1)
