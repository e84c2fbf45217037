// What the two selection kernels of a beam call share (beam_select.hip, beam_sampled.hip): the order-preserving key of a
// float, a slot's sorted list of 64-bit keys in LDS, the wave-wide round that takes the best candidate in lane order,
// and the tail of a step -- the start state, the step's records and new slots, the done count, the SSRU states gathered by
// parent from one block into the other and the next token's embedding. THREADS is the workgroup's size.
//
// Device code only; every helper is __forceinline__ (no out-of-line device function, no dynamic stack).
#pragma once

#include <hip/hip_runtime.h>

#include "beam.h"
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {

// a float's order as an unsigned word: -inf < ... < -0 == +0 < ... < +inf (not for NaN); never 0
__device__ __forceinline__ uint32_t bm_ordered(float v) {
  const uint32_t b = __float_as_uint(v + 0.0f);  // (-0 + 0 = +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ... and back (a -0 comes back as +0)
__device__ __forceinline__ float bm_unordered(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// The wave's shuffles, the workgroup's barrier and the relaxed atomic add as builtins: the HIP headers' __shfl*, __syncthreads
// and atomicAdd are plain inline functions, which a kernel with a target attribute of its own (beam_sampled.hip) would call
// out of line.
__device__ __forceinline__ int bm_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int bm_shfl(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
__device__ __forceinline__ float bm_shfl(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ int bm_shfl_xor(int v, int m) { return bm_shfl(v, bm_lane() ^ m); }
__device__ __forceinline__ float bm_shfl_xor(float v, int m) { return bm_shfl(v, bm_lane() ^ m); }
__device__ __forceinline__ unsigned long long bm_shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = (uint32_t)bm_shfl_xor((int)(uint32_t)v, m);
  const uint32_t hi = (uint32_t)bm_shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ void bm_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
template <class T>
__device__ __forceinline__ void bm_atomic_add(T *p, T v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The key (ov << 32) | ~c into the sorted list L[0..k) of a slot (0 = empty) whose k-th value word is *thr: 64-bit atomic
// maxima, the displaced key carried down (score_alternatives.hip's technique). The caller has seen ov >= *thr; a stale
// threshold is a lower one.
__device__ __forceinline__ void bm_list_insert(unsigned long long *L, uint32_t *thr, int k, uint32_t ov, uint32_t c) {
  unsigned long long carry = ((unsigned long long)ov << 32) | (uint32_t)~c;
  int i = k;  // the first slot the key beats (slots only rise: those before it stay above the key)
  for (int j = k - 1; j >= 0; --j) i = L[j] < carry ? j : i;
  for (; i < k && carry != 0ull; ++i) {
    const unsigned long long old = __hip_atomic_fetch_max(L + i, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned long long top = old > carry ? old : carry;
    carry = old > carry ? carry : old;
    if (i == k - 1) __hip_atomic_fetch_max(thr, (uint32_t)(top >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// The start state of source b (BeamSelectArgs::init): slot 0 live with total +0, the others dead with -inf, the zero
// embedding, step word 0, done 0.
template <int THREADS>
__device__ __forceinline__ void bm_start_state(const BeamSelectArgs &a, int b, int tid) {
  const int k = a.k, r0 = b * k, D = a.emb.D;
  const float ninf = -__builtin_inff();
  if (tid < k) {
    a.totals_out[r0 + tid] = tid == 0 ? 0.0f : ninf;
    a.flags_out[r0 + tid] = tid == 0 ? kBeamLive : kBeamDead;
    if (a.len_out) a.len_out[r0 + tid] = 0u;
    if (a.step_word) a.step_word[r0 + tid] = 0u;
  }
  if (tid == 0 && a.done) a.done[b] = 0u;
  if (a.dx) {
    for (int u = tid; u < k * D; u += THREADS) {
      const float z = 0.0f * a.emb.sqrt_d;
      a.dx[(size_t)r0 * D + u] = z + a.emb.pos[u % D];
    }
  }
}

// One round of the wave-wide "largest cand, lowest lane": a lane's place in the order, `ord`, is its lane while its candidate
// is still to be taken and 64 + lane otherwise, so the lane order is the contract's tie order. Returns the winner's ord on
// every lane (64 or more: no candidate is left); the caller takes it and retires it with ord = 64 + lane.
__device__ __forceinline__ uint32_t bm_best_lane(float cand, uint32_t ord) {
  float bc = cand;
  uint32_t bo = ord;
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    const float oc = bm_shfl_xor(bc, x);
    const uint32_t oo = (uint32_t)bm_shfl_xor((int)bo, x);
    const bool ov = oo < 64u, bv = bo < 64u;
    const bool better = ov != bv ? ov : (ov ? (oc > bc || (oc == bc && oo < bo)) : oo < bo);
    bc = better ? oc : bc;
    bo = better ? oo : bo;
  }
  return bo;
}

// a new slot as the rounds left it in lane `lane` < k
struct BmNewSlot {
  uint32_t flag, parent, tok, len;
  float lp, C;
};
// ... a dead one: what a lane keeps when no round gives it a candidate
__device__ __forceinline__ BmNewSlot bm_dead_slot() { return BmNewSlot{kBeamDead, kBeamNone, kBeamNone, 0u, 0.0f, -__builtin_inff()}; }

// round i's winner of slot ws becomes lane i's new slot: carried (a finished slot: itself, with the length it had), else
// extended by column wcol with score wlp; its total is wC
__device__ __forceinline__ void bm_fill_slot(const BeamSelectArgs &a, BmNewSlot &n, int ws, bool carried, uint32_t wcol, float wlp,
                                             float wC, const uint32_t *old_len) {
  n.parent = (uint32_t)ws;
  n.C = wC;
  if (carried) {
    n.flag = kBeamFinished;
    n.len = old_len[ws];
  } else {
    n.tok = a.ids ? a.ids[wcol] : wcol;
    n.lp = wlp;
    n.flag = n.tok == a.eos ? kBeamFinished : kBeamLive;
    n.len = (uint32_t)a.t + 1u;
  }
}

// lane < k writes the step's records and its new slot, to memory and to the workgroup's arrays
__device__ __forceinline__ void bm_store_slot(const BeamSelectArgs &a, int r, int lane, const BmNewSlot &n, uint32_t *n_flag,
                                              uint32_t *n_parent, uint32_t *n_tok) {
  a.parent[r] = n.parent;
  a.token[r] = n.tok;
  a.token_score[r] = n.lp;
  a.totals_out[r] = n.C;
  a.flags_out[r] = n.flag;
  if (a.len_out) a.len_out[r] = n.len;
  if (a.step_word) a.step_word[r] = (uint32_t)a.t + 1u;
  n_flag[lane] = n.flag;
  n_parent[lane] = n.parent;
  n_tok[lane] = n.tok;
}

// The engine's part of a step, behind a barrier after bm_store_slot: the done count, the SSRU states of every layer by
// parent from one block into the other (a dead slot: zeros), the next step's input rows (embed1's expression, position 0).
template <int THREADS>
__device__ __forceinline__ void bm_step_tail(const BeamSelectArgs &a, int b, int tid, const uint32_t *n_flag, const uint32_t *n_parent,
                                             const uint32_t *n_tok) {
  const int k = a.k, r0 = b * k, D = a.emb.D;
  if (tid == 0) {  // a source is done when no slot is live: counted once
    bool live = false;
    for (int i = 0; i < k; ++i) live = live || n_flag[i] == kBeamLive;
    if (!live && a.done[b] == 0u) {
      a.done[b] = 1u;
      bm_atomic_add(a.n_finished, 1);
    }
  }
  const size_t R = (size_t)a.B * k;
  const int D4 = D >> 2;
  for (int u = tid; u < a.Ld * k * D4; u += THREADS) {
    const int l = u / (k * D4), rem = u - l * (k * D4);
    const int i = rem / D4, d4 = rem - i * D4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (n_flag[i] != kBeamDead)
      v = reinterpret_cast<const float4 *>(a.state_src + ((size_t)l * R + (size_t)(r0 + (int)n_parent[i])) * D)[d4];
    reinterpret_cast<float4 *>(a.state_dst + ((size_t)l * R + (size_t)(r0 + i)) * D)[d4] = v;
  }
  for (int u = tid; u < k * D; u += THREADS) {
    const int i = u / D, d = u - i * D;
    float x;
    if (n_flag[i] == kBeamLive) {
      const float v = (float)a.emb.wemb[(size_t)embed_row(a.emb, n_tok[i]) * D + d] * a.emb.inv_mult;
      x = v * a.emb.sqrt_d;
    } else {
      x = 0.0f * a.emb.sqrt_d;
    }
    a.dx[(size_t)r0 * D + u] = x + a.emb.pos[d];
  }
}

}  // namespace slimt_hip
