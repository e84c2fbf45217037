// Beam search under step constraints (slimt_hip_ctx_set_beam_constraints, slimt_hip_beam_step_constrained): one selection
// per step over the rows z' -- each live slot's logits under the slot's own bans and penalty (constraints.h), the sets read
// from the slot's own history. The contract is one sentence: the plain beam step of beam.h over z'.
//
// One 1024-thread workgroup per source, one launch per step, in the place of beam_select_kernel. z' never goes to memory.
//   phase H   histories are rows: the k slots' history rows [Th] go to LDS (a live slot: the t tokens its chain emitted; a
//             finished one: its whole length, to be carried). The (slot, position) pairs are spread over all threads: a
//             pair marks its token as seen (theta != 1 only) and tests its window of n - 1 tokens against the slot's suffix;
//             k x n_suppress threads take one suppressed id each, the last k threads a slot's EOS rule. A marked id becomes a
//             column (cn_column) and a bit, set with an LDS atomic OR in the slot's banned or seen bitmap over the N columns:
//             dynamic LDS, k x (2 | 1) x ceil(N / 32) words before the k x Th words of history.
//   phase R   the 16 waves are dealt to the slots, per = floor(16 / k) waves each; a wave of slot s owns the columns
//             (i per + wi) 64 + lane. For N <= kBeamConstrainedResidentN = 4096 a lane's (at most 32) penalised logits and their ban
//             bits stay in registers from here on: the row is read once. Above it the same columns are walked in the same
//             order and re-read (from L2) by each pass.
//     reduction   NaN, the counts of valid, candidate and banned columns, the maxima of z over the candidates and over the valid
//                 columns, per wave into LDS; every wave of a slot merges the slot's partials alike, so the lift (no
//                 candidate while a valid column exists) and M are uniform over the slot's waves
//     pass 2      over the columns with z' > -inf: the uint64 sum Q of bm_weight(z', M) and the slot's k best keys
//                 (ordered(z') << 32) | ~column in its sorted LDS list (beam_tail.h)
//   selection by wave 0, lane 8 s + j = slot s's j-th candidate, as in beam_select.hip: lp from z' at the column (the penalty
//             applied again to the logit's own bits), k rounds of "largest cand, lowest lane"
//   tail      the new slots' history rows from LDS into the other block -- the parent's row and the new token; a carried
//             finished slot's row unchanged -- then the beam's tail (beam_tail.h): the SSRU states by parent, the embeddings
//
// Every barrier is reached by every thread (a wave without a live slot skips the passes, not the barriers); no workgroup
// waits for another. No out-of-line device functions, no dynamic stack, no scratch: helpers are __forceinline__.
#include <hip/hip_runtime.h>

#include "beam.h"
#include "beam_tail.h"
#include "constraints.h"
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {
namespace {

constexpr int kBcThreads = 1024, kBcWaves = kBcThreads / 64;
constexpr int kBcCols = 32;  // columns a lane holds
static_assert((kBcWaves / kBeamMax) * 64 * kBcCols == kBeamConstrainedResidentN, "the resident bound is the narrowest deal's columns");

struct BcShared {
  unsigned long long lists[kBeamMax][kBeamMax];  // per slot: its best keys, sorted, 0 = empty
  unsigned long long Q[kBeamMax];
  uint32_t thr[kBeamMax];                        // the value part of the slot's k-th key
  float w_mc[kBeamMax][kBcWaves], w_mv[kBeamMax][kBcWaves];  // the reduction per wave of the slot
  uint32_t w_nv[kBeamMax][kBcWaves], w_nc[kBeamMax][kBcWaves], w_nb[kBeamMax][kBcWaves], w_nan[kBeamMax][kBcWaves];
  float M[kBeamMax];                             // the maximum of z', and whether the row is usable
  uint32_t ok[kBeamMax];
  uint32_t flag[kBeamMax], len[kBeamMax], hl[kBeamMax];  // the slots as the step found them; hl: the history row's length
  float C[kBeamMax];
  uint32_t n_flag[kBeamMax], n_parent[kBeamMax], n_tok[kBeamMax];  // the new slots
};

__device__ __forceinline__ bool bc_bit(const uint32_t *bits, int c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

__device__ __forceinline__ void bc_mark(uint32_t *bits, const uint32_t *sl, int N, uint32_t id) {
  const int col = cn_column(sl, N, id);
  if (col >= 0) (void)__hip_atomic_fetch_or(&bits[col >> 5], 1u << (col & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a column's logit under the slot's penalty
__device__ __forceinline__ float bc_logit(const uint32_t *seen, bool penalised, int c, float l, float theta, float inv_theta) {
  return penalised && bc_bit(seen, c) ? cn_penalise(l, theta, inv_theta) : l;
}

// f(column, penalised logit, banned) over the lane's columns first, first + stride, ..., ascending
template <bool RESIDENT, class F>
__device__ __forceinline__ void bc_each(const float (&l)[kBcCols], uint32_t ban, const float *__restrict__ row, int N, int first, int stride,
                                        const uint32_t *banned, const uint32_t *seen, bool penalised, float theta, float inv_theta,
                                        F &&f) {
  if constexpr (RESIDENT) {
#pragma unroll
    for (int i = 0; i < kBcCols; ++i) {
      const int c = first + i * stride;
      if (c < N) f(c, l[i], ((ban >> i) & 1u) != 0);
    }
  } else {
    for (int c = first; c < N; c += stride)  // (N <= kBeamConstrainedMaxN: c stays an int)
      f(c, bc_logit(seen, penalised, c, row[c], theta, inv_theta), bc_bit(banned, c));
  }
}

template <bool RESIDENT>
__global__ __launch_bounds__(kBcThreads) void beam_constrained_kernel(BeamConstrainedArgs ca) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bc_dyn[];  // bitmaps [k][nbm][W], then histories [k][Th]
  __shared__ BcShared sh;
  const BeamSelectArgs &a = ca.step;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k, N = a.N, r0 = b * k, Th = ca.Th, W = (N + 31) >> 5;
  const float theta = ca.c.theta, inv_theta = ca.c.inv_theta;
  const bool penalised = theta != 1.0f;
  const int nbm = penalised ? 2 : 1;  // (no seen bitmap without a penalty)
  uint32_t *const hist = bc_dyn + (size_t)k * nbm * W;
  const float ninf = -__builtin_inff();
  const uint32_t L = (uint32_t)(a.t < Th ? a.t : Th);  // a live slot's history length

  if (tid < kBeamMax) {
    const bool in = tid < k;
    const uint32_t f = in ? a.flags_in[r0 + tid] : kBeamDead;
    const uint32_t ln = in && a.len_in ? a.len_in[r0 + tid] : (uint32_t)Th;  // (without lengths a finished row is carried whole)
    sh.flag[tid] = f;
    sh.C[tid] = in ? a.totals_in[r0 + tid] : ninf;
    sh.len[tid] = in && a.len_in ? ln : 0u;
    sh.hl[tid] = f == kBeamLive ? L : (f == kBeamFinished ? (ln < (uint32_t)Th ? ln : (uint32_t)Th) : 0u);
    sh.Q[tid] = 0ull;
    sh.thr[tid] = 0u;
    sh.M[tid] = ninf;
    sh.ok[tid] = 0u;
  }
  if (tid < kBeamMax * kBeamMax) sh.lists[tid >> 3][tid & 7] = 0ull;
  for (int w = tid; w < k * nbm * W; w += kBcThreads) bc_dyn[w] = 0u;
  bm_barrier();

  // phase H: the history rows, then the slots' sets
  for (int u = tid; u < k * Th; u += kBcThreads) {
    const int s = u / Th, q = u - s * Th;
    if ((uint32_t)q < sh.hl[s]) hist[u] = ca.hist_src[(size_t)(r0 + s) * Th + q];
  }
  bm_barrier();
  {
    const uint32_t n = ca.c.no_repeat_ngram;
    for (uint32_t u = tid; u < (uint32_t)k * L; u += kBcThreads) {  // (slot, position)
      const uint32_t s = u / L, q = u - s * L;
      if (sh.flag[s] != kBeamLive) continue;
      const uint32_t *h = hist + s * Th;
      uint32_t *bits = bc_dyn + (size_t)s * nbm * W;
      if (penalised) bc_mark(bits + W, a.ids, N, h[q]);
      if (n != 0 && cn_window_bans(h, L, n, q)) bc_mark(bits, a.ids, N, h[q + n - 1]);
    }
    const uint32_t ns = ca.c.n_suppress;  // (at most 64: k ns <= 512 threads)
    if ((uint32_t)tid < (uint32_t)k * ns) {
      const uint32_t s = (uint32_t)tid / ns, i = (uint32_t)tid - s * ns;
      if (sh.flag[s] == kBeamLive) bc_mark(bc_dyn + (size_t)s * nbm * W, a.ids, N, ca.c.suppress[i]);
    }
    const int es = tid - (kBcThreads - kBeamMax);
    if (es >= 0 && es < k && sh.flag[es] == kBeamLive && cn_eos_banned(L, ca.c.min_length))
      bc_mark(bc_dyn + (size_t)es * nbm * W, a.ids, N, a.eos);
  }
  bm_barrier();

  // phase R: the deal -- slot = wave / per, its wi-th wave; the one global read (RESIDENT), penalised, and the ban bits
  const int per = kBcWaves / k;
  const int slot_of = wave / per, wi = wave - slot_of * per;
  const bool mine = slot_of < k && sh.flag[slot_of < k ? slot_of : 0] == kBeamLive;  // (uniform over the wave)
  const int slot = mine ? slot_of : 0;
  const int first = wi * 64 + lane, stride = per * 64;
  const float *__restrict__ row = a.logits + (size_t)(r0 + slot) * N;
  const uint32_t *const banned = bc_dyn + (size_t)slot * nbm * W, *const seen = banned + W;
  float l[kBcCols];
  uint32_t ban = 0;
#pragma unroll
  for (int i = 0; i < kBcCols; ++i) l[i] = 0.0f;
  if constexpr (RESIDENT) {
    if (mine) {
#pragma unroll
      for (int i = 0; i < kBcCols; ++i) {
        const int c = first + i * stride;
        if (c < N) {
          l[i] = bc_logit(seen, penalised, c, row[c], theta, inv_theta);
          ban |= bc_bit(banned, c) ? 1u << i : 0u;
        }
      }
    }
  }

  // the reduction: NaN (bit 0: anywhere, bit 1: in an unbanned column), the counts, the two maxima
  if (mine) {
    uint32_t nv = 0, nc = 0, nb = 0, nan = 0;
    float mc = ninf, mv = ninf;
    bc_each<RESIDENT>(l, ban, row, N, first, stride, banned, seen, penalised, theta, inv_theta, [&](int, float z, bool bn) {
      const bool valid = z == z, cand = cn_candidate(z, bn, false);
      nv += valid ? 1u : 0u;
      nc += cand ? 1u : 0u;
      nb += bn ? 1u : 0u;
      nan |= valid ? 0u : (bn ? 1u : 3u);
      mv = valid ? fmaxf(mv, z) : mv;
      mc = cand ? fmaxf(mc, z) : mc;
    });
    for (int x = 1; x < 64; x <<= 1) {
      nv += (uint32_t)bm_shfl_xor((int)nv, x);
      nc += (uint32_t)bm_shfl_xor((int)nc, x);
      nb += (uint32_t)bm_shfl_xor((int)nb, x);
      nan |= (uint32_t)bm_shfl_xor((int)nan, x);
      mv = fmaxf(mv, bm_shfl_xor(mv, x));
      mc = fmaxf(mc, bm_shfl_xor(mc, x));
    }
    if (lane == 0) {
      sh.w_nv[slot][wi] = nv;
      sh.w_nc[slot][wi] = nc;
      sh.w_nb[slot][wi] = nb;
      sh.w_nan[slot][wi] = nan;
      sh.w_mv[slot][wi] = mv;
      sh.w_mc[slot][wi] = mc;
    }
  }
  bm_barrier();

  // the slot's lift and maximum, alike on each of its waves; pass 2: the weight sum and the k best columns of a usable slot
  if (mine) {
    uint32_t nv = 0, nc = 0, nb = 0, nan = 0;
    float mc = ninf, mv = ninf;
    for (int w = 0; w < per; ++w) {
      nv += sh.w_nv[slot][w];
      nc += sh.w_nc[slot][w];
      nb += sh.w_nb[slot][w];
      nan |= sh.w_nan[slot][w];
      mv = fmaxf(mv, sh.w_mv[slot][w]);
      mc = fmaxf(mc, sh.w_mc[slot][w]);
    }
    const bool lift = cn_lift(nc, nv);  // every valid column is banned: the bans are lifted, the penalty stays
    const float M = bm_max(lift ? mv : mc);
    const bool any_nan = (nan & (lift ? 1u : 2u)) != 0u;  // (a NaN in a banned column is -inf in z')
    const bool usable = bm_usable(any_nan, M);
    if (wi == 0 && lane == 0) {
      sh.M[slot] = M;
      sh.ok[slot] = usable ? 1u : 0u;
      if (ca.n_banned) ca.n_banned[r0 + slot] = nb | (lift ? kConstraintFallback : 0u);
    }
    if (usable) {
      unsigned long long *list = sh.lists[slot];
      unsigned long long q = 0ull;
      bc_each<RESIDENT>(l, ban, row, N, first, stride, banned, seen, penalised, theta, inv_theta, [&](int c, float z, bool bn) {
        if ((bn && !lift) || !(z > ninf)) return;  // z' = -inf: no weight, no candidate
        q += bm_weight(z, M);
        const uint32_t ov = bm_ordered(z);
        const uint32_t th = __hip_atomic_load(&sh.thr[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (ov >= th) bm_list_insert(list, &sh.thr[slot], k, ov, (uint32_t)c);  // (rare once the list is full)
      });
      for (int x = 1; x < 64; x <<= 1) q += bm_shfl_xor_u64(q, x);
      if (lane == 0) (void)__hip_atomic_fetch_add(&sh.Q[slot], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  } else if (ca.n_banned && slot_of < k && wi == 0 && lane == 0) {
    ca.n_banned[r0 + slot_of] = 0u;  // (a finished or dead slot is not constrained)
  }
  bm_barrier();

  // selection: wave 0, lane 8 s + j = slot s's j-th candidate
  if (wave == 0) {
    const int s = lane >> 3, j = lane & 7;
    bool valid = false, carried = false;
    float cand = ninf, lp = 0.0f;
    uint32_t col = 0u;
    if (s < k && j < k) {
      const uint32_t f = sh.flag[s];
      if (f == kBeamFinished) {
        valid = j == 0;
        carried = true;
        cand = sh.C[s];
      } else if (f == kBeamLive) {
        const unsigned long long key = sh.lists[s][j];
        if (sh.ok[s] != 0u && key != 0ull) {
          col = ~(uint32_t)key;
          // (the logit's own bits under the penalty: the key folds -0 into +0)
          const float z = bc_logit(bc_dyn + ((size_t)s * nbm + 1) * W, penalised, (int)col, a.logits[(size_t)(r0 + s) * N + col], theta, inv_theta);
          lp = bm_logprob(z, sh.M[s], bm_normaliser(sh.Q[s]));
          cand = sh.C[s] + lp;
          valid = !(cand == ninf);
        }
      }
    }
    uint32_t ord = valid ? (uint32_t)lane : 64u + (uint32_t)lane;
    BmNewSlot slot_new = bm_dead_slot();
    for (int i = 0; i < k; ++i) {
      const uint32_t bo = bm_best_lane(cand, ord);
      if (bo >= 64u) break;  // (uniform: every lane holds the same winner) fewer than k candidates: the rest stay dead
      const int w = (int)bo;
      const uint32_t wcol = (uint32_t)bm_shfl((int)col, w);
      const float wlp = bm_shfl(lp, w);
      const float wcand = bm_shfl(cand, w);
      const int wcar = bm_shfl((int)carried, w);
      if (lane == w) ord = 64u + (uint32_t)lane;
      if (lane == i) bm_fill_slot(a, slot_new, w >> 3, wcar != 0, wcol, wlp, wcand, sh.len);
    }
    if (lane < k) bm_store_slot(a, r0 + lane, lane, slot_new, sh.n_flag, sh.n_parent, sh.n_tok);
  }
  bm_barrier();

  // the new slots' history rows: the parent's row, then the token the slot took (a carried slot: the row alone)
  if (ca.hist_dst) {
    for (int u = tid; u < k * Th; u += kBcThreads) {
      const int i = u / Th, q = u - i * Th;
      if (sh.n_flag[i] == kBeamDead) continue;
      const uint32_t p = sh.n_parent[i], pl = sh.hl[p];
      if ((uint32_t)q < pl) ca.hist_dst[(size_t)(r0 + i) * Th + q] = hist[p * Th + q];
      else if ((uint32_t)q == pl && sh.n_tok[i] != kBeamNone) ca.hist_dst[(size_t)(r0 + i) * Th + q] = sh.n_tok[i];
    }
  }
  if (!a.state_dst) return;  // (the whole grid) the op-level call ends here

  bm_step_tail<kBcThreads>(a, b, tid, sh.n_flag, sh.n_parent, sh.n_tok);
}

}  // namespace

size_t beam_constrained_lds_bytes(int k, int N, int Th, bool penalised) {
  return ((size_t)k * (penalised ? 2 : 1) * (size_t)((N + 31) >> 5) + (size_t)k * Th) * sizeof(uint32_t);
}

hipError_t launch_beam_constrained(const BeamConstrainedArgs &ca, hipStream_t st) {
  const BeamSelectArgs &a = ca.step;
  if (a.init) return hipErrorInvalidValue;  // (the start state is launch_beam_select's)
  if (a.B < 1 || a.k < 1 || a.k > kBeamMax || !a.totals_out || !a.flags_out) return hipErrorInvalidValue;
  if ((a.len_in != nullptr) != (a.len_out != nullptr)) return hipErrorInvalidValue;
  if (!a.logits || a.N < 1 || a.N > kBeamConstrainedMaxN || a.t < 0 || !a.totals_in || !a.flags_in || !a.parent || !a.token || !a.token_score)
    return hipErrorInvalidValue;
  if (!ca.hist_src || ca.hist_src == ca.hist_dst || ca.Th < 1 || ca.Th > kBeamConstrainedMaxHistory || a.t > ca.Th) return hipErrorInvalidValue;
  if (!cn_valid(ca.c.no_repeat_ngram, ca.c.theta, ca.c.n_suppress)) return hipErrorInvalidValue;
  if (a.state_dst) {
    if (!a.state_src || a.state_src == a.state_dst || a.Ld < 1 || !a.dx || !a.done || !a.n_finished || !a.emb.wemb || !a.emb.pos ||
        a.emb.D < 4 || a.emb.D % 4)
      return hipErrorInvalidValue;
  }
  auto kernel = a.N <= kBeamConstrainedResidentN ? beam_constrained_kernel<true> : beam_constrained_kernel<false>;
  const size_t lds = beam_constrained_lds_bytes(a.k, a.N, ca.Th, ca.c.theta != 1.0f);
  const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(a.B), dim3(kBcThreads), lds, st, ca);
  return hipGetLastError();
}

}  // namespace slimt_hip
