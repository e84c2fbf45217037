// Sampling without replacement on a beam call (slimt_hip_ctx_set_beam_sampling, slimt_hip_beam_step_sampled): the selection
// of stochastic beam search, beam_sampled.h's contract.
//
// Under per-column noise the beam's pruning (a slot's k best LOGIT columns) is wrong: every column of every live slot is
// perturbed and compared, k N evaluations of two logarithms and a hash per source and step. So the work is split the other
// way round from beam_select_kernel: one 1024-thread workgroup per source whose 16 waves are dealt to the LIVE slots,
// floor(16 / live) waves each, and a source's rows are swept at once (at step 0 all 16 waves sweep slot 0's row). A wave
// of slot s strides the row by 64 x (waves of the slot); the row is re-read by each sweep (L2-resident: 128 KiB per source
// at k = 8, N = 4096), so N is arbitrary and no sweep holds more than one column per lane in registers.
//   sweep 1    NaN test and maximum, per wave into LDS
//   sweep 2    M from the slot's waves; the uint64 sum Q of bm_weight(l, M): shuffles, then one 64-bit LDS add per wave
//              (integers: the order is free)
//   sweep 3    lp, phi = C + lp, the column's Gumbel noise from (key, slot, step, vocabulary id) and psi, into the slot's
//              sorted LDS list of 64-bit keys (ordered(psi) << 32) | ~column behind a threshold word (beam_tail.h): the
//              list's order is the contract's (psi descending, then column ascending), its first k entries the slot's
//              candidates, its head Z
//   selection  wave 0, lane 8 s + j = candidate j of slot s: sb_condition there (k^2 <= 64 evaluations), a finished slot
//              itself in lane 8 s with its G; then k rounds of "largest cand, lowest lane" (beam_tail.h, bm_best_lane)
//   tail       the beam's (beam_tail.h), and the new slots' G
//
// Every barrier is reached by every thread (a wave without a slot skips the sweeps, not the barriers); no workgroup waits
// for another. No out-of-line device function, no dynamic stack; plain loops. The kernel carries a target attribute, so it
// uses beam_tail.h's builtin shuffles, barrier and atomic add, not the HIP headers' inline functions.
#include <hip/hip_runtime.h>

#include "beam_sampled.h"
#include "beam_tail.h"
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {
namespace {

constexpr int kSbThreads = 1024, kSbWaves = kSbThreads / 64;

// compiled without the packed f32 instructions (v_pk_*_f32), whichever build compiles it: the attribute travels with the source
#if defined(__HIP_DEVICE_COMPILE__)
#define SLIMT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else  // (the host pass only needs the kernel's stub, and its target does not know the feature)
#define SLIMT_NO_PACKED_F32
#endif

struct SbShared {
  unsigned long long lists[kBeamMax][kBeamMax];  // per slot: its best keys, sorted, 0 = empty
  unsigned long long Q[kBeamMax];
  uint32_t thr[kBeamMax];                        // the value part of the slot's k-th key
  float wm[kBeamMax][kSbWaves];                  // sweep 1 per wave of the slot (-inf / 0 where the slot has fewer)
  uint32_t wn[kBeamMax][kSbWaves];
  float M[kBeamMax];                             // sweep 2: the row's maximum, and whether the row is usable
  uint32_t ok[kBeamMax];
  uint32_t flag[kBeamMax], len[kBeamMax];        // the slots as the step found them
  float C[kBeamMax], G[kBeamMax];
  uint32_t n_flag[kBeamMax], n_parent[kBeamMax], n_tok[kBeamMax];  // the new slots
};

__global__ SLIMT_NO_PACKED_F32 __launch_bounds__(kSbThreads) void beam_select_sampled_kernel(BeamSampledArgs sa) {
  __shared__ SbShared sh;
  const BeamSelectArgs &a = sa.step;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k, N = a.N, r0 = b * k;
  const float ninf = -__builtin_inff();
  if (a.init) {  // (the whole grid: no barrier below is skipped by part of a workgroup)
    bm_start_state<kSbThreads>(a, b, tid);
    if (tid < k) sa.perturbed_out[r0 + tid] = tid == 0 ? 0.0f : ninf;
    return;
  }
  if (tid < kBeamMax) {
    const bool in = tid < k;
    sh.flag[tid] = in ? a.flags_in[r0 + tid] : kBeamDead;
    sh.C[tid] = in ? a.totals_in[r0 + tid] : ninf;
    sh.G[tid] = in ? sa.perturbed_in[r0 + tid] : ninf;
    sh.len[tid] = in && a.len_in ? a.len_in[r0 + tid] : 0u;
    sh.Q[tid] = 0ull;
    sh.thr[tid] = 0u;
    sh.M[tid] = ninf;
    sh.ok[tid] = 0u;
  }
  if (tid < kBeamMax * kBeamMax) sh.lists[tid >> 3][tid & 7] = 0ull;
  if (tid < kBeamMax * kSbWaves) {
    sh.wm[tid / kSbWaves][tid % kSbWaves] = ninf;
    sh.wn[tid / kSbWaves][tid % kSbWaves] = 0u;
  }
  // the deal: this wave's slot (the g-th live one, g = wave / waves per live slot), its place among the slot's waves
  int n_live = 0;
  for (int s = 0; s < k; ++s) n_live += a.flags_in[r0 + s] == kBeamLive ? 1 : 0;
  const int per = n_live ? kSbWaves / n_live : 0;  // (k <= 8: at least two)
  const int g = per ? wave / per : kSbWaves;
  const int wi = per ? wave - g * per : 0;
  int slot = -1;
  for (int s = 0, seen = 0; s < k; ++s) {
    if (a.flags_in[r0 + s] != kBeamLive) continue;
    if (seen == g) slot = s;
    ++seen;
  }
  const int stride = per * 64;
  const float *__restrict__ row = a.logits + (size_t)(r0 + (slot < 0 ? 0 : slot)) * N;
  bm_barrier();

  // sweep 1: NaN test and maximum
  if (slot >= 0) {
    float m = ninf;
    uint32_t nan = 0u;
    for (int c = wi * 64 + lane; c < N; c += stride) {
      const float v = row[c];
      nan |= v != v ? 1u : 0u;
      m = fmaxf(m, v);
    }
    for (int x = 1; x < 64; x <<= 1) {
      m = fmaxf(m, bm_shfl_xor(m, x));
      nan |= (uint32_t)bm_shfl_xor((int)nan, x);
    }
    if (lane == 0) {
      sh.wm[slot][wi] = m;
      sh.wn[slot][wi] = nan;
    }
  }
  bm_barrier();

  // sweep 2: the maximum of the slot's waves, and the weight sum of a usable row
  float M = ninf;
  bool usable = false;
  if (slot >= 0) {
    float m = sh.wm[slot][lane & (kSbWaves - 1)];
    uint32_t nan = sh.wn[slot][lane & (kSbWaves - 1)];
    for (int x = 1; x < kSbWaves; x <<= 1) {
      m = fmaxf(m, bm_shfl_xor(m, x));
      nan |= (uint32_t)bm_shfl_xor((int)nan, x);
    }
    M = bm_max(m);
    usable = bm_usable(nan != 0u, M);
    if (usable) {
      unsigned long long q = 0ull;
      for (int c = wi * 64 + lane; c < N; c += stride) q += bm_weight(row[c], M);
      for (int x = 1; x < 64; x <<= 1) q += bm_shfl_xor_u64(q, x);
      if (lane == 0) bm_atomic_add(&sh.Q[slot], q);
    }
    if (wi == 0 && lane == 0) {
      sh.M[slot] = M;
      sh.ok[slot] = usable ? 1u : 0u;
    }
  }
  bm_barrier();

  // sweep 3: every column's perturbed score into the slot's list
  if (usable) {
    const float L = bm_normaliser(sh.Q[slot]), C = sh.C[slot];
    const uint64_t K = sa.keys ? sa.keys[b] : sm_sentence_key(0ull, (uint64_t)b);
    const uint64_t words = sm_step_words(sm_sentence_key(K, (uint64_t)slot), (uint32_t)a.t);
    const uint32_t s0 = (uint32_t)words, s1 = (uint32_t)(words >> 32);
    unsigned long long *list = sh.lists[slot];
    for (int c = wi * 64 + lane; c < N; c += stride) {
      const float lp = bm_logprob(row[c], M, L);
      if (!(lp > ninf)) continue;
      const uint32_t id = a.ids ? a.ids[c] : (uint32_t)c;
      const float phi = C + lp;
      const uint32_t ov = bm_ordered(sb_perturb(phi, sm_gumbel(s0, s1, id)));
      const uint32_t th = __hip_atomic_load(&sh.thr[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (ov >= th) bm_list_insert(list, &sh.thr[slot], k, ov, (uint32_t)c);  // (rare once the list is full)
    }
  }
  bm_barrier();

  // selection: wave 0, lane 8 s + j = candidate j of slot s
  if (wave == 0) {
    const int s = lane >> 3, j = lane & 7;
    bool valid = false, carried = false;
    float cand = ninf, phi = ninf, lp = 0.0f;
    uint32_t col = 0u;
    if (s < k && j < k) {
      const uint32_t f = sh.flag[s];
      if (f == kBeamFinished) {
        valid = j == 0;
        carried = true;
        cand = sh.G[s];
        phi = sh.C[s];
      } else if (f == kBeamLive) {
        const unsigned long long key = sh.lists[s][j];
        if (sh.ok[s] != 0u && key != 0ull) {
          col = ~(uint32_t)key;
          const float l = a.logits[(size_t)(r0 + s) * N + col];
          lp = bm_logprob(l, sh.M[s], bm_normaliser(sh.Q[s]));
          phi = sh.C[s] + lp;
          const float psi = bm_unordered((uint32_t)(key >> 32)), Z = bm_unordered((uint32_t)(sh.lists[s][0] >> 32));
          cand = sb_condition(sh.G[s], Z, psi);
          valid = true;
        }
      }
    }
    uint32_t ord = valid ? (uint32_t)lane : 64u + (uint32_t)lane;
    BmNewSlot mine = bm_dead_slot();
    float my_G = ninf;
    for (int i = 0; i < k; ++i) {
      const uint32_t bo = bm_best_lane(cand, ord);
      if (bo >= 64u) break;  // (uniform: every lane holds the same winner) fewer than k candidates: the rest stay dead
      const int w = (int)bo;
      const uint32_t wcol = (uint32_t)bm_shfl((int)col, w);
      const float wlp = bm_shfl(lp, w);
      const float wcand = bm_shfl(cand, w);
      const float wphi = bm_shfl(phi, w);
      const int wcar = bm_shfl((int)carried, w);
      if (lane == w) ord = 64u + (uint32_t)lane;
      if (lane == i) {
        bm_fill_slot(a, mine, w >> 3, wcar != 0, wcol, wlp, wphi, sh.len);
        my_G = wcand;
      }
    }
    if (lane < k) {
      bm_store_slot(a, r0 + lane, lane, mine, sh.n_flag, sh.n_parent, sh.n_tok);
      sa.perturbed_out[r0 + lane] = my_G;
    }
  }
  bm_barrier();
  if (!a.state_dst) return;  // (the whole grid) the op-level call ends here

  bm_step_tail<kSbThreads>(a, b, tid, sh.n_flag, sh.n_parent, sh.n_tok);
}

}  // namespace

hipError_t launch_beam_select_sampled(const BeamSampledArgs &sa, hipStream_t st) {
  const BeamSelectArgs &a = sa.step;
  if (a.B < 1 || a.k < 1 || a.k > kBeamMax || !a.totals_out || !a.flags_out || !sa.perturbed_out) return hipErrorInvalidValue;
  if ((a.len_in != nullptr) != (a.len_out != nullptr) && !a.init) return hipErrorInvalidValue;
  if (!a.init) {
    if (!a.logits || a.N < 1 || (uint32_t)a.N >= kBeamMaxN || a.t < 0 || !a.totals_in || !a.flags_in || !sa.perturbed_in || !a.parent ||
        !a.token || !a.token_score)
      return hipErrorInvalidValue;
  }
  if (a.state_dst) {
    if (!a.state_src || a.state_src == a.state_dst || a.Ld < 1 || !a.dx || !a.done || !a.n_finished || !a.emb.wemb || !a.emb.pos ||
        a.emb.D < 4 || a.emb.D % 4)
      return hipErrorInvalidValue;
  } else if (a.init && a.dx && (!a.emb.pos || a.emb.D < 1)) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(beam_select_sampled_kernel, dim3(a.B), dim3(kSbThreads), 0, st, sa);
  return hipGetLastError();
}

}  // namespace slimt_hip
