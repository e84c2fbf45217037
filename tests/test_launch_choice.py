"""CPU-side checks of the engine's launch decisions (slimt_amd/csrc/launch_choice.h), compiled here for the host from the
same header the engine includes, the way test_decoder_plan.py compiles decoder_plan.h. Every function is compared with a
NumPy transcription of the expression it replaced -- quoted from engine.cpp as it stood before the header existed
(translate_device, encode_device, kv_tight_shape) -- over the full grid of its inputs: nothing sampled, nothing left out. The kernels' *_supported()
predicates enter the header as booleans, so here they are free variables: every combination."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Each entry point walks the C-ordered product of the axes it is given (dims[a] values of axis a, concatenated in vals) and
# writes one byte / int / double per point.
_HARNESS = r"""
#include "launch_choice.h"
using namespace slimt_hip;
typedef long long i64;
static void point(size_t i, int nd, const i64 *dims, const i64 *vals, i64 *v) {
  size_t off[32], o = 0;
  for (int a = 0; a < nd; ++a) { off[a] = o; o += (size_t)dims[a]; }
  for (int a = nd - 1; a >= 0; --a) { v[a] = vals[off[a] + i % (size_t)dims[a]]; i /= (size_t)dims[a]; }
}
#define WALK(nd_) i64 v[nd_]; for (size_t i = 0; i < n; ++i) if (point(i, nd_, dims, vals, v), true)
extern "C" {
// D F H fmt S enc_rows mode lean fe te le dp dm dl -> mid, long24, packed
void kv_form(const i64 *dims, const i64 *vals, size_t n, unsigned char *mid, unsigned char *lng, unsigned char *packed) {
  WALK(14) {
    KvFormIn in;
    in.D = (int)v[0]; in.F = (int)v[1]; in.H = (int)v[2]; in.kv_format = (int)v[3]; in.S = (size_t)v[4];
    in.encode_rows = (int)v[5]; in.decode_mode = (int)v[6]; in.lean = v[7] != 0;
    in.fused_encode_ok = v[8] != 0; in.tall_encode_ok = v[9] != 0; in.long_encode_ok = v[10] != 0;
    in.decode_packed_ok = v[11] != 0; in.decode_mid_ok = v[12] != 0; in.decode_long24_ok = v[13] != 0;
    const KvForm f = kv_cache_form(in);
    mid[i] = f.mid; lng[i] = f.long24; packed[i] = f.packed;
  }
}
// S -> 24-bit slot, 20-bit slot
void slots(const i64 *dims, const i64 *vals, size_t n, unsigned char *s24, unsigned char *s20) {
  WALK(1) { s24[i] = kv24_slot_fits((size_t)v[0]); s20[i] = kv20_slot_fits((int)v[0]); }
}
// D S long_encoder
void narrow_shape(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(3) out[i] = kv_narrow_shape((int)v[0], (int)v[1], v[2] != 0);
}
// B S
void calibration_rows(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(2) out[i] = kv_calibration_rows((size_t)v[0], (size_t)v[1]);
}
// enabled writer limit fmt D S mode large mid_ok rows32_ok tight_ok
void tight_shape(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(11) {
    KvTightIn in;
    in.enabled = v[0] != 0; in.writer = v[1] != 0; in.tight_limit = (int)v[2]; in.kv_format = (int)v[3]; in.D = (int)v[4];
    in.S = (int)v[5]; in.decode_mode = (int)v[6]; in.expect_large_output = v[7] != 0;
    in.mid_ok = v[8] != 0; in.rows32_ok = v[9] != 0; in.tight_ok = v[10] != 0;
    out[i] = kv_tight_shape(in);
  }
}
// kv24 enc_tight fmt_valid fmt_B B
void tight_launch(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(5) out[i] = kv_tight_launch(v[0] != 0, v[1] != 0, v[2] != 0, (int)v[3], (int)v[4]);
}
// kv24 D F S budget
void cluster_allowed(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(5) out[i] = cluster_ok(v[0] != 0, (int)v[1], (int)v[2], (size_t)v[3], (int)v[4]);
}
// ok mode tight merged scored
void clusters(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(5) out[i] = clusters_chosen(v[0] != 0, (int)v[1], v[2] != 0, v[3] != 0, v[4] != 0);
}
// clusters scored mode n_expected tight S rows32_ok merged
void rows_requested(const i64 *dims, const i64 *vals, size_t n, int *out) {
  WALK(8) out[i] = fused_rows_requested(v[0] != 0, v[1] != 0, (int)v[2], (size_t)v[3], v[4] != 0, (size_t)v[5], v[6] != 0, v[7] != 0);
}
// tight fmt kv24
void bytes_per_value(const i64 *dims, const i64 *vals, size_t n, double *out) {
  WALK(3) out[i] = kv_bytes_per_value(v[0] != 0, v[1] != 0, v[2] != 0);
}
// by_launch plan_eighths plan_k call_slot call_k store_nt all
void launch_eighths(const i64 *dims, const i64 *vals, size_t n, int *out) {
  WALK(7) out[i] = kv_launch_eighths(v[0] != 0, (int)v[1], (int)v[2], (unsigned long long)v[3], (int)v[4], v[5] != 0, (int)v[6]);
}
// store_nt kv24 call_slot call_k
void store_streamed(const i64 *dims, const i64 *vals, size_t n, unsigned char *out) {
  WALK(4) out[i] = kv_store_streamed(v[0] != 0, v[1] != 0, (unsigned long long)v[2], (int)v[3]);
}
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_choice")
    src = d / "h.cc"
    src.write_text(_HARNESS)
    so = d / "h.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "slimt_amd", "csrc"), str(src), "-o", str(so)])
    return ctypes.CDLL(str(so))


def walk(h, name, axes, *dtypes):
    """fn over the product of the axes: the outputs shaped like the grid, and the axes as arrays that broadcast over it."""
    axes = [np.asarray(a, dtype=np.int64) for a in axes]
    dims = np.array([len(a) for a in axes], dtype=np.int64)
    vals = np.concatenate(axes)
    n = int(np.prod(dims))
    outs = [np.empty(n, dtype=t) for t in dtypes]
    fn = getattr(h, name)
    fn.restype = None
    fn(dims.ctypes.data_as(ctypes.c_void_p), vals.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n),
       *[o.ctypes.data_as(ctypes.c_void_p) for o in outs])
    grid = np.meshgrid(*axes, indexing="ij", sparse=True)
    return [o.reshape(tuple(dims)) for o in outs], grid


BOOL = [0, 1]
S_ALL = list(range(1, 130))
MODES = list(range(7))
# (D, F, H, Le, Ld) of the four presets (slimt_amd/synth.py), and one shape no persistent kernel supports
SHAPES = [(256, 1536, 8, 6, 2), (512, 2048, 8, 6, 2), (64, 128, 4, 2, 2), (128, 256, 8, 2, 2), (256, 1024, 4, 3, 3)]


def per_shape(fn):
    """The shape is one axis of the issue's grid; D, F and H move together, so the grid is walked shape by shape."""
    for D, F, H, _Le, _Ld in SHAPES:
        fn(D, F, H)


def test_kv_cache_form_over_the_full_grid(harness):
    def one(D, F, H):
        (mid, lng, packed), g = walk(harness, "kv_form", [[D], [F], [H], range(4), S_ALL, [0, 32, 64], MODES, BOOL] + [BOOL] * 6,
                                     np.uint8, np.uint8, np.uint8)
        _, _, _, fmt, S, enc_rows, mode, lean, fe, te, le, dp, dm, dl = [a.astype(np.int64) for a in g]
        lean, fe, te, le, dp, dm, dl = [a != 0 for a in (lean, fe, te, le, dp, dm, dl)]
        # const bool kv24_mid = S > 32 && S <= 64 && c->encode_rows != 32 && c->decode_mode != 3 &&
        #                       fused_decode_mid_supported(m->D, m->F, m->H, m->Ld) &&
        #                       tall_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S);
        kv24_mid = (S > 32) & (S <= 64) & (enc_rows != 32) & (mode != 3) & dm & te
        # const bool kv24_long = S > 64 && S <= 128 && c->decode_mode != 3 && fused_decode_long24_supported(m->D, m->F, m->H, m->Ld) &&
        #                        long_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S);
        kv24_long = (S > 64) & (S <= 128) & (mode != 3) & dl & le
        # const bool kv_packed = lean && (m->kv_format == 0 || m->kv_format == 2) &&
        #                   ((m->D == 256 && m->D / m->H == 32) || (m->D == 512 && m->D / m->H == 64 && m->F == 2048)) &&
        #                   ((S <= 32 && ((S + 3) & ~(size_t)3) * 3 <= S * 4 &&
        #                     fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S) &&
        #                     fused_decode_packed_supported(m->D, m->F, m->H, m->Ld)) || kv24_mid || kv24_long);
        shape = (D == 256 and D // H == 32) or (D == 512 and D // H == 64 and F == 2048)
        kv_packed = lean & ((fmt == 0) | (fmt == 2)) & shape & (
            ((S <= 32) & (((S + 3) & ~3) * 3 <= S * 4) & fe & dp) | kv24_mid | kv24_long)
        assert np.array_equal(mid != 0, np.broadcast_to(kv24_mid, mid.shape))
        assert np.array_equal(lng != 0, np.broadcast_to(kv24_long, lng.shape))
        assert np.array_equal(packed != 0, np.broadcast_to(kv_packed, packed.shape))
    per_shape(one)


def test_slot_predicates(harness):
    (s24, s20), (S,) = walk(harness, "slots", [S_ALL], np.uint8, np.uint8)
    # ((S + 3) & ~(size_t)3) * 3 <= S * 4
    assert np.array_equal(s24 != 0, ((S + 3) & ~3) * 3 <= S * 4)
    # ((S + 7) / 8) * 5120 <= ((S + 3) / 4) * 3072
    assert np.array_equal(s20 != 0, ((S + 7) // 8) * 5120 <= ((S + 3) // 4) * 3072)
    # what the comments beside them say: the 24-bit slot misses S = 1, 2, 5; the 20-bit one S = 1..4, 9..12
    assert [s for s, ok in zip(S_ALL, s24) if not ok] == [1, 2, 5]
    assert [s for s, ok in zip(S_ALL, s20) if not ok] == [1, 2, 3, 4, 9, 10, 11, 12]


def test_narrow_form_shape(harness):
    (got,), (D, S, long_enc) = walk(harness, "narrow_shape", [sorted({s[0] for s in SHAPES}), S_ALL, BOOL], np.uint8)
    slot = ((S + 7) // 8) * 5120 <= ((S + 3) // 4) * 3072
    # encode_device, the fused / tall branch:
    #   kv24 && ((D == 256 && S <= 64) || (D == 512 && S <= 32)) && ((S + 7) / 8) * 5120 <= ((S + 3) / 4) * 3072 && ...
    fused = (((D == 256) & (S <= 64)) | ((D == 512) & (S <= 32))) & slot
    # ... the long branch:  kv24 && D == 256 && ((S + 7) / 8) * 5120 <= ((S + 3) / 4) * 3072 && ...
    long_ = (D == 256) & slot
    assert np.array_equal(got != 0, np.where(long_enc != 0, long_, fused))


def test_calibration_rows(harness):
    Bs = [1, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 128, 256, 341, 342, 512, 1023, 1024, 4096]
    (got,), (B, S) = walk(harness, "calibration_rows", [Bs, S_ALL], np.uint8)
    assert np.array_equal(got != 0, B * S >= 1024)  # ... && B * S >= 1024 && ...


def test_kv_tight_shape_over_the_full_grid(harness):
    (got,), g = walk(harness, "tight_shape", [BOOL, BOOL, [0, 1, 1 << 15], range(4), sorted({s[0] for s in SHAPES}), S_ALL, MODES, BOOL,
                                              BOOL, BOOL, BOOL], np.uint8)
    enabled, writer, limit, fmt, D, S, mode, large, mid_ok, rows32_ok, tight_ok = g
    enabled, writer, large, mid_ok, rows32_ok, tight_ok = [a != 0 for a in (enabled, writer, large, mid_ok, rows32_ok, tight_ok)]
    # if (!kv_tight_enabled() || !writer || m->kv_tight_limit <= 0 || m->kv_format != 0) return false;
    gate = enabled & writer & (limit > 0) & (fmt == 0)
    # if (S > 32)
    #   return S <= 128 && m->D == 256 && c->decode_mode != 3 && c->decode_mode != 6 && c->decode_mode != 1 &&
    #          fused_decode_tight_mid_supported(m->D, m->F, m->H, m->Ld, S > 64 ? 2 : 1);
    longer = (S <= 128) & (D == 256) & (mode != 3) & (mode != 6) & (mode != 1) & mid_ok
    # const bool rows32 = m->D == 256 && (c->decode_mode == 3 || (c->decode_mode == 0 && c->expect_large_output));
    rows32 = (D == 256) & ((mode == 3) | ((mode == 0) & large))
    # if (rows32) return fused_decode_tight_rows32_supported(m->D, m->F, m->H, m->Ld);
    # if (!(c->decode_mode == 0 || c->decode_mode == 2 || c->decode_mode == 3 || c->decode_mode == 4 || c->decode_mode == 5)) return false;
    # return fused_decode_tight_supported(m->D, m->F, m->H, m->Ld);
    short = np.where(rows32, rows32_ok, ((mode == 0) | (mode == 2) | (mode == 3) | (mode == 4) | (mode == 5)) & tight_ok)
    want = gate & np.where(S > 32, longer, short)
    assert np.array_equal(got != 0, np.broadcast_to(want, got.shape))


def test_tight_rule_of_the_decoder_launch(harness):
    (got,), (kv24, enc_tight, valid, fmt_B, B) = walk(harness, "tight_launch", [BOOL, BOOL, BOOL, [0, 1, 17, 64], [1, 17, 64]], np.uint8)
    # const bool tight = kv24 && c->kv_tight && c->kv_fmt_valid && c->kv_fmt_B == (int)B;
    assert np.array_equal(got != 0, (kv24 != 0) & (enc_tight != 0) & (valid != 0) & (fmt_B == B))


def test_clusters(harness):
    DF = sorted({(s[0], s[1]) for s in SHAPES})
    for D, F in DF:
        (got,), (kv24, _, _, S, budget) = walk(harness, "cluster_allowed", [BOOL, [D], [F], S_ALL, [0, 224]], np.uint8)
        # const bool cluster_ok = kv24 && m->D == 256 && m->F == 1536 && S <= 32 && c->model->decoder_budget > 0;
        want = (kv24 != 0) & (D == 256 and F == 1536) & (S <= 32) & (budget > 0)
        assert np.array_equal(got != 0, np.broadcast_to(want, got.shape))
    (got,), (ok, mode, tight, merged, scored) = walk(harness, "clusters", [BOOL, MODES, BOOL, BOOL, BOOL], np.uint8)
    # const bool clusters = cluster_ok && c->decode_mode == 6 && !tight && !mp && !scored;
    assert np.array_equal(got != 0, (ok != 0) & (mode == 6) & (tight == 0) & (merged == 0) & (scored == 0))


def test_requested_tiling_over_the_full_grid(harness):
    (got,), g = walk(harness, "rows_requested", [BOOL, BOOL, MODES, [0, 16384, 16385, 32000], BOOL, S_ALL, BOOL, BOOL], np.int32)
    clusters, scored, mode, n_expected, tight, S, rows32_ok, merged = g
    clusters, scored, tight, rows32_ok, merged = [a != 0 for a in (clusters, scored, tight, rows32_ok, merged)]
    # f.rows_per_wg = clusters || scored ? 16 : c->decode_mode == 2 ? 16 : c->decode_mode == 3 ? 32 : c->decode_mode == 4 ? 8
    #                 : c->decode_mode == 5 ? 4 : (n_expected > 16384 ? 32 : 0);
    rows = np.where(clusters | scored, 16, np.where(mode == 2, 16, np.where(mode == 3, 32, np.where(mode == 4, 8, np.where(
        mode == 5, 4, np.where(n_expected > 16384, 32, 0))))))
    rows = np.broadcast_to(rows, got.shape).copy()
    # if (tight && f.rows_per_wg == 32 && !(S <= 32 && fused_decode_tight_rows32_supported(m->D, m->F, m->H, m->Ld))) f.rows_per_wg = 16;
    rows[np.broadcast_to(tight & ~((S <= 32) & rows32_ok), got.shape) & (rows == 32)] = 16
    # if (mp && f.rows_per_wg == 32) f.rows_per_wg = 16;
    rows[np.broadcast_to(merged, got.shape) & (rows == 32)] = 16
    assert np.array_equal(got, rows)


def test_kv_bytes_per_value(harness):
    (got,), (tight, fmt, kv24) = walk(harness, "bytes_per_value", [BOOL, BOOL, BOOL], np.float64)
    # (f.kv_tight ? 2.0 : f.kv_fmt ? 2.5 : kv24 ? 3.0 : 4.0)
    assert np.array_equal(got, np.where(tight != 0, 2.0, np.where(fmt != 0, 2.5, np.where(kv24 != 0, 3.0, 4.0))))


def test_by_launch_eighths(harness):
    (got,), g = walk(harness, "launch_eighths", [BOOL, [0, 8, 16], range(9), range(16), range(9), BOOL, [16]], np.int32)
    by_launch, plan_eighths, plan_k, call_slot, call_k, store_nt, al = g
    # int eighths = plan.eighths;
    # if (plan.by_launch) eighths = (int)(call_slot % 8) < (store_nt_rule ? call_k : plan.k) ? all : 0;
    kept = np.where(call_slot % 8 < np.where(store_nt != 0, call_k, plan_k), al, 0)
    assert np.array_equal(got, np.broadcast_to(np.where(by_launch != 0, kept, plan_eighths), got.shape))
    (got,), (store_nt, kv24, call_slot, call_k) = walk(harness, "store_streamed", [BOOL, BOOL, range(16), range(9)], np.uint8)
    # store_nt && kv24 && call_k < 8 && (int)(call_slot % 8) >= call_k
    assert np.array_equal(got != 0, (store_nt != 0) & (kv24 != 0) & (call_k < 8) & (call_slot % 8 >= call_k))
