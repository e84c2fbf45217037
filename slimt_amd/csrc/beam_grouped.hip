// Diverse beam search (slimt_hip_ctx_set_beam_groups, slimt_hip_beam_step_grouped): one selection per step over G groups
// of g = k / G slots, a later group pushed away from the columns the earlier groups took at this step.
//
// beam_select_grouped_kernel: one 512-thread workgroup per source, eight waves.
//   sweep      a WAVE PER SLOT: wave w < k owns row w of the step's f32 logits from its first load to its finished list --
//              the NaN test and the maximum M, then the uint64 sum Q of the integer weights (beam.h: exact in any order)
//              and the slot's k best (logit, column) keys in its own LDS list (beam_tail.h: 64-bit atomic maxima behind a
//              threshold word, a set of maxima, so no order of work changes it). M, the NaN bit and Q are reduced with wave
//              shuffles; the list and its threshold are touched by this wave alone. No workgroup barrier until every wave's
//              (M, Q, list) is in LDS. A row of N <= 4096 columns, N a multiple of 4, stays in registers between the two
//              passes (16 float4 loads per lane) and is read from memory once; any other row is read twice, column by
//              column. The waves k .. 7 idle through the sweep and work in the tail.
//   selection  wave 0, G group rounds one after the other. In group j's round lane 8 i + q holds the q-th best column of
//              slot j g + i (a finished slot: itself, in lane 8 i): g * 8 <= 64 lanes in the contract's tie order. A lane
//              forms cand from the logit's own bits, counts its column among the columns the earlier groups extended with
//              (at most k - g, kept in every lane's registers) and forms aug = cand - penalty * n; g rounds of the
//              wave-wide "largest aug, lowest lane" take the group's new slots, whose totals are cand. k keys per slot are
//              enough: at most k - g columns are penalised, so a slot's g best by aug lie among its k best by plain order.
//   then       beam_tail.h's records, new slots and step tail, as behind the plain selection.
// init: the start state has one live slot per group (slot j g).
//
// Every barrier is reached by every thread; no workgroup waits for another. No out-of-line device functions, no dynamic
// stack, no scratch: helpers are __forceinline__ and every register array is indexed by unrolled constants.
#include <hip/hip_runtime.h>

#include "beam.h"
#include "beam_tail.h"
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {
namespace {

constexpr int kBgThreads = 512;
constexpr int kBgQuads = kBeamGroupedResidentN / 256;  // float4 loads per lane of a resident row

struct BgShared {
  unsigned long long lists[kBeamMax][kBeamMax];  // per slot: its best keys, sorted, 0 = empty
  unsigned long long Q[kBeamMax];
  uint32_t thr[kBeamMax];     // the value part of the slot's k-th key
  float M[kBeamMax];          // a live slot's maximum (bm_max)
  uint32_t usable[kBeamMax];  // ... and whether its row is usable
  uint32_t flag[kBeamMax], len[kBeamMax];  // the slots as the step found them
  float C[kBeamMax];
  uint32_t n_flag[kBeamMax], n_parent[kBeamMax], n_tok[kBeamMax];  // the new slots
};

// one column of a usable row in pass 2: its weight, and its key where it may belong to the slot's k best
__device__ __forceinline__ void bg_column(float v, uint32_t c, float M, int k, unsigned long long *L, uint32_t *thr,
                                          unsigned long long &q) {
  q += bm_weight(v, M);
  const uint32_t ov = bm_ordered(v);
  const uint32_t th = __hip_atomic_load(thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (v > -__builtin_inff() && ov >= th) bm_list_insert(L, thr, k, ov, c);  // (rare once the list is full)
}

// the wave's maximum and NaN bit on every lane
__device__ __forceinline__ void bg_reduce_max(float &m, uint32_t &nan) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) {
    m = fmaxf(m, bm_shfl_xor(m, x));
    nan |= (uint32_t)bm_shfl_xor((int)nan, x);
  }
}

// The start state of source b: slot j g of every group live with total +0, the others dead with -inf, the zero embedding,
// step word 0, done 0 (bm_start_state with one live slot per group).
__device__ __forceinline__ void bg_start_state(const BeamSelectArgs &a, int g, int b, int tid) {
  const int k = a.k, r0 = b * k, D = a.emb.D;
  if (tid < k) {
    const bool first = tid % g == 0;
    a.totals_out[r0 + tid] = first ? 0.0f : -__builtin_inff();
    a.flags_out[r0 + tid] = first ? kBeamLive : kBeamDead;
    if (a.len_out) a.len_out[r0 + tid] = 0u;
    if (a.step_word) a.step_word[r0 + tid] = 0u;
  }
  if (tid == 0 && a.done) a.done[b] = 0u;
  if (a.dx) {
    for (int u = tid; u < k * D; u += kBgThreads) {
      const float z = 0.0f * a.emb.sqrt_d;
      a.dx[(size_t)r0 * D + u] = z + a.emb.pos[u % D];
    }
  }
}

__global__ __launch_bounds__(kBgThreads) void beam_select_grouped_kernel(BeamGroupedArgs ga) {
  __shared__ BgShared sh;
  const BeamSelectArgs &a = ga.step;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k, N = a.N, r0 = b * k, G = ga.groups, g = k / G;
  const float ninf = -__builtin_inff();
  if (a.init) {  // (the whole grid: no barrier below is skipped by part of a workgroup)
    bg_start_state(a, g, b, tid);
    return;
  }

  // the sweep: wave w < k and slot w, nobody else
  if (wave < k) {
    const int s = wave;
    const uint32_t f = a.flags_in[r0 + s];
    if (lane < kBeamMax) sh.lists[s][lane] = 0ull;
    if (lane == 0) {
      sh.flag[s] = f;
      sh.C[s] = a.totals_in[r0 + s];
      sh.len[s] = a.len_in ? a.len_in[r0 + s] : 0u;
      sh.thr[s] = 0u;
    }
    // (the wave's own LDS words: its lanes run in step and LDS serves a wave in order; the fence keeps the compiler's order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float M = ninf;
    bool usable = false;
    unsigned long long q = 0ull;
    if (f == kBeamLive) {  // (uniform in the wave)
      const float *__restrict__ row = a.logits + (size_t)(r0 + s) * N;
      unsigned long long *L = sh.lists[s];
      uint32_t nan = 0u;
      float m = ninf;
      if (N <= kBeamGroupedResidentN && (N & 3) == 0) {
        // resident: lane holds the float4 i * 64 + lane of the row for i < 16, -inf beyond the row (no weight, no key)
        float v[4 * kBgQuads];
        const int n4 = N >> 2;
#pragma unroll
        for (int i = 0; i < kBgQuads; ++i) {
          const int idx = i * 64 + lane;
          float4 x = make_float4(ninf, ninf, ninf, ninf);
          if (idx < n4) x = reinterpret_cast<const float4 *>(row)[idx];
          v[4 * i + 0] = x.x;
          v[4 * i + 1] = x.y;
          v[4 * i + 2] = x.z;
          v[4 * i + 3] = x.w;
        }
#pragma unroll
        for (int i = 0; i < 4 * kBgQuads; ++i) {
          nan |= v[i] != v[i] ? 1u : 0u;
          m = fmaxf(m, v[i]);
        }
        bg_reduce_max(m, nan);
        M = bm_max(m);
        usable = bm_usable(nan != 0u, M);
        if (usable) {
#pragma unroll
          for (int i = 0; i < kBgQuads; ++i) {
            if (i * 64 < n4) {  // (uniform)
              const uint32_t c = 4u * (uint32_t)(i * 64 + lane);
#pragma unroll
              for (int e = 0; e < 4; ++e) bg_column(v[4 * i + e], c + (uint32_t)e, M, k, L, &sh.thr[s], q);
            }
          }
        }
      } else {
        for (int c = lane; c < N; c += 64) {
          const float x = row[c];
          nan |= x != x ? 1u : 0u;
          m = fmaxf(m, x);
        }
        bg_reduce_max(m, nan);
        M = bm_max(m);
        usable = bm_usable(nan != 0u, M);
        if (usable) {
          for (int c = lane; c < N; c += 64) bg_column(row[c], (uint32_t)c, M, k, L, &sh.thr[s], q);
        }
      }
#pragma unroll
      for (int x = 1; x < 64; x <<= 1) q += bm_shfl_xor_u64(q, x);
    }
    if (lane == 0) {
      sh.M[s] = M;
      sh.usable[s] = usable ? 1u : 0u;
      sh.Q[s] = q;
    }
  }
  __syncthreads();

  // selection: wave 0, group after group; lane 8 i + q = slot j g + i's q-th candidate
  if (wave == 0) {
    const int i = lane >> 3, qq = lane & 7;
    uint32_t chosen[kBeamMax];  // the columns the groups before this one extended with, kBeamNone = none (no column is)
#pragma unroll
    for (int x = 0; x < kBeamMax; ++x) chosen[x] = kBeamNone;
    int n_chosen = 0;
    BmNewSlot mine = bm_dead_slot();
    for (int j = 0; j < G; ++j) {
      const int s = j * g + i;
      bool valid = false, carried = false;
      float cand = ninf, aug = ninf, lp = 0.0f;
      uint32_t col = 0u;
      if (i < g && qq < k) {
        const uint32_t f = sh.flag[s];
        if (f == kBeamFinished) {
          valid = qq == 0;
          carried = true;
          cand = aug = sh.C[s];
        } else if (f == kBeamLive) {
          const unsigned long long key = sh.lists[s][qq];
          if (sh.usable[s] != 0u && key != 0ull) {
            col = ~(uint32_t)key;
            const float l = a.logits[(size_t)(r0 + s) * N + col];  // (the logit's own bits: the key folds -0 into +0)
            lp = bm_logprob(l, sh.M[s], bm_normaliser(sh.Q[s]));
            cand = sh.C[s] + lp;
            valid = !(cand == ninf);
            int n = 0;
#pragma unroll
            for (int x = 0; x < kBeamMax; ++x) n += chosen[x] == col ? 1 : 0;
            // (the product rounded to f32, then one subtraction: never contracted into an fma)
            aug = n == 0 ? cand : __fsub_rn(cand, __fmul_rn(ga.penalty, (float)n));
          }
        }
      }
      uint32_t ord = valid ? (uint32_t)lane : 64u + (uint32_t)lane;
      for (int round = 0; round < g; ++round) {
        const uint32_t bo = bm_best_lane(aug, ord);
        if (bo >= 64u) break;  // (uniform) fewer than g candidates: the group's other slots stay dead
        const int w = (int)bo;
        const uint32_t wcol = (uint32_t)bm_shfl((int)col, w);
        const float wlp = bm_shfl(lp, w);
        const float wcand = bm_shfl(cand, w);
        const int wcar = bm_shfl((int)carried, w);
        if (lane == w) ord = 64u + (uint32_t)lane;
        if (lane == j * g + round) bm_fill_slot(a, mine, j * g + (w >> 3), wcar != 0, wcol, wlp, wcand, sh.len);
        if (wcar == 0) {  // (uniform) an extension, into EOS too, counts against the later groups
#pragma unroll
          for (int x = 0; x < kBeamMax; ++x) chosen[x] = x == n_chosen ? wcol : chosen[x];
          ++n_chosen;
        }
      }
    }
    if (lane < k) bm_store_slot(a, r0 + lane, lane, mine, sh.n_flag, sh.n_parent, sh.n_tok);
  }
  __syncthreads();
  if (!a.state_dst) return;  // (the whole grid) the op-level call ends here

  bm_step_tail<kBgThreads>(a, b, tid, sh.n_flag, sh.n_parent, sh.n_tok);
}

}  // namespace

hipError_t launch_beam_select_grouped(const BeamGroupedArgs &ga, hipStream_t st) {
  const BeamSelectArgs &a = ga.step;
  if (a.B < 1 || a.k < 1 || a.k > kBeamMax || !a.totals_out || !a.flags_out) return hipErrorInvalidValue;
  if (ga.groups < 1 || ga.groups > a.k || a.k % ga.groups || !(ga.penalty >= 0.0f && ga.penalty <= kBeamGroupedMaxPenalty))
    return hipErrorInvalidValue;
  if ((a.len_in != nullptr) != (a.len_out != nullptr) && !a.init) return hipErrorInvalidValue;
  if (!a.init) {
    if (!a.logits || a.N < 1 || (uint32_t)a.N >= kBeamMaxN || !a.totals_in || !a.flags_in || !a.parent || !a.token || !a.token_score)
      return hipErrorInvalidValue;
  }
  if (a.state_dst) {
    if (!a.state_src || a.state_src == a.state_dst || a.Ld < 1 || !a.dx || !a.done || !a.n_finished || !a.emb.wemb || !a.emb.pos ||
        a.emb.D < 4 || a.emb.D % 4)
      return hipErrorInvalidValue;
  } else if (a.init && a.dx && (!a.emb.pos || a.emb.D < 1)) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(beam_select_grouped_kernel, dim3(a.B), dim3(kBgThreads), 0, st, ga);
  return hipGetLastError();
}

}  // namespace slimt_hip
