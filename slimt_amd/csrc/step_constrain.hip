// Step constraints (slimt_hip_ctx_set_step_constraints): one step's selection over stored logits, conditioned on the row's
// history -- no-repeat n-grams, a repetition penalty, a minimum length and a suppressed-token list (constraints.h).
//
// One 256-thread workgroup per decoder row, two phases.
//   phase H   history to sets. The row's history (at most kConstraintMaxHistory = 1024 tokens, 4 KB) goes to LDS; thread q
//             (q, q + 256, ...) marks h[q] as seen and tests its window of n - 1 tokens against the suffix, threads
//             0 .. n_suppress - 1 take one suppressed id each, the last thread the EOS rule. Every marked id is turned into
//             its column (cn_column: a binary search of the sorted shortlist, per thread) and the column's bit is set
//             with an LDS atomic OR in one of two bitmaps over the N columns, banned and seen: dynamic LDS, 2 x N / 8
//             bytes (2 x 512 B at N = 4096, 128 KiB at kConstraintMaxN = 2^19). Integer ORs: every schedule gives the
//             same sets. A forced step (fcol[b] >= 0) marks nothing.
//   phase R   the row, read from memory once, with sample_floor.hip's ownership: thread t owns the 4-column groups t,
//             t + 256, ... (one 128-bit load each where the row is 16-byte aligned, four scalar loads where not) and
//             keeps 16 penalised logits and their ban bits in registers for N <= kConstrainResidentN = 4096; above it
//             the streaming variant walks the same groups in the same order and re-reads them (from L2) in each pass.
//     reduction A   valid, candidate and banned counts, the maxima of z over the candidates and over the valid columns;
//                   candidates == 0 < valid lifts the bans for the step, uniformly over the workgroup
//     selection     first maximum of z (greedy) or of the Gumbel key (sampled) over the candidates, the float sum of
//                   exp(z - M) over them and z at the forced column, merged with the arg-max's tie rule
// The result is one partial per row: EPI_ARGMAX_SC's format for a greedy step, EPI_ARGMAX_SM's for a sampled one.
// Every barrier is reached by all 256 threads. No out-of-line device functions, no dynamic stack, no scratch.
#include <hip/hip_runtime.h>

#include "constraints.h"
#include "device_common.h"

namespace slimt_hip {
namespace {

constexpr int kCnThreads = 256;
constexpr int kCnCols = 16;  // columns a thread holds: four groups of four
static_assert(kCnThreads * kCnCols == kConstrainResidentN, "the register-resident bound is threads x columns per thread");

struct CnShared {
  uint32_t hist[kConstraintMaxHistory];
  uint32_t n_valid[4], n_cand[4], n_ban[4];
  float m_cand[4], m_valid[4];
  float r_key[4], r_sum[4], r_zw[4], r_y[4];
  int r_col[4];
};

__device__ __forceinline__ bool cn_bit(const uint32_t *bits, int c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

__device__ __forceinline__ void cn_mark(uint32_t *bits, const uint32_t *sl, int N, uint32_t id) {
  const int col = cn_column(sl, N, id);
  if (col >= 0) atomicOr(&bits[col >> 5], 1u << (col & 31));
}

// the four columns from c0 (a multiple of 4, c0 < N); VEC: N is a multiple of 4 and the row 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void cn_load4(const float *__restrict__ row, int N, int c0, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4 *>(row + c0);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c0 + e < N ? row[c0 + e] : 0.0f;
  }
}

// a column's logit under the penalty
__device__ __forceinline__ float cn_logit(const uint32_t *seen, int c, float l, float theta, float inv_theta) {
  return cn_bit(seen, c) ? cn_penalise(l, theta, inv_theta) : l;
}

// f(column, penalised logit, banned) over the thread's columns, ascending
template <bool RESIDENT, bool VEC, class F>
__device__ __forceinline__ void cn_each(const float (&l)[kCnCols], uint32_t ban, const float *__restrict__ row, int N, int tid,
                                        const uint32_t *banned, const uint32_t *seen, float theta, float inv_theta, F &&f) {
  if constexpr (RESIDENT) {
#pragma unroll
    for (int i = 0; i < kCnCols; ++i) {
      const int c = 4 * ((i >> 2) * kCnThreads + tid) + (i & 3);
      if (c < N) f(c, l[i], ((ban >> i) & 1u) != 0);
    }
  } else {
    for (int c0 = 4 * tid; c0 < N; c0 += 4 * kCnThreads) {  // (N <= kConstraintMaxN: c0 stays an int)
      float v[4];
      cn_load4<VEC>(row, N, c0, v);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < N) f(c0 + e, cn_logit(seen, c0 + e, v[e], theta, inv_theta), cn_bit(banned, c0 + e));
    }
  }
}

template <bool SAMPLED, bool RESIDENT, bool VEC>
__global__ __launch_bounds__(kCnThreads) void step_constrain_kernel(StepConstrainArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cn_bits[];  // banned [W], seen [W]
  __shared__ CnShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, W = (N + 31) >> 5;
  uint32_t *const banned = cn_bits, *const seen = cn_bits + W;
  const float *__restrict__ row = a.logits + (size_t)b * N;
  const float inv_T = a.inv_T, theta = a.c.theta, inv_theta = a.c.inv_theta;
  const float ninf = -__builtin_inff();
  const int fc = a.fcol ? a.fcol[b] : -1;
  const bool constrained = fc < 0;  // (a forced step marks nothing: every valid column, no penalty)

  // phase H: the history, then the two sets
  uint32_t L = 0;
  if (constrained) {
    L = a.hist_len[b];
    L = L < (uint32_t)a.ld_hist ? L : (uint32_t)a.ld_hist;
  }
  for (int w = tid; w < 2 * W; w += kCnThreads) cn_bits[w] = 0u;
  for (uint32_t q = tid; q < L; q += kCnThreads) sh.hist[q] = a.history[(size_t)b * a.ld_hist + q];
  __syncthreads();
  if (constrained) {  // (uniform over the workgroup)
    const uint32_t n = a.c.no_repeat_ngram;
    const bool penalised = theta != 1.0f;
    for (uint32_t q = tid; q < L; q += kCnThreads) {
      if (penalised) cn_mark(seen, a.shortlist, N, sh.hist[q]);
      if (n != 0 && cn_window_bans(sh.hist, L, n, q)) cn_mark(banned, a.shortlist, N, sh.hist[q + n - 1]);
    }
    if ((uint32_t)tid < a.c.n_suppress) cn_mark(banned, a.shortlist, N, a.c.suppress[tid]);
    if (tid == kCnThreads - 1 && cn_eos_banned(L, a.c.min_length)) cn_mark(banned, a.shortlist, N, a.eos);
  }
  __syncthreads();

  // phase R: the one global read (RESIDENT), penalised, and the columns' ban bits
  float l[kCnCols];
  uint32_t ban = 0;
#pragma unroll
  for (int i = 0; i < kCnCols; ++i) l[i] = 0.0f;
  if constexpr (RESIDENT) {
#pragma unroll
    for (int j = 0; j < kCnCols / 4; ++j) {
      const int c0 = 4 * (j * kCnThreads + tid);
      if (c0 < N) {
        float v[4];
        cn_load4<VEC>(row, N, c0, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in_row = c0 + e < N;
          l[4 * j + e] = in_row ? cn_logit(seen, c0 + e, v[e], theta, inv_theta) : 0.0f;
          ban |= in_row && cn_bit(banned, c0 + e) ? 1u << (4 * j + e) : 0u;
        }
      }
    }
  }

  // reduction A: the counts and the two maxima
  uint32_t nv = 0, nc = 0, nb = 0;
  float mc = ninf, mv = ninf;
  cn_each<RESIDENT, VEC>(l, ban, row, N, tid, banned, seen, theta, inv_theta, [&](int, float lp, bool bn) {
    const float z = lp * inv_T;
    const bool valid = z == z, cand = cn_candidate(z, bn, false);
    nv += valid ? 1u : 0u;
    nc += cand ? 1u : 0u;
    nb += bn ? 1u : 0u;
    mv = valid ? fmaxf(mv, z) : mv;
    mc = cand ? fmaxf(mc, z) : mc;
  });
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    nv += (uint32_t)__shfl_xor((int)nv, m, 64);
    nc += (uint32_t)__shfl_xor((int)nc, m, 64);
    nb += (uint32_t)__shfl_xor((int)nb, m, 64);
    mv = fmaxf(mv, __shfl_xor(mv, m, 64));
    mc = fmaxf(mc, __shfl_xor(mc, m, 64));
  }
  if (lane == 0) {
    sh.n_valid[wave] = nv;
    sh.n_cand[wave] = nc;
    sh.n_ban[wave] = nb;
    sh.m_valid[wave] = mv;
    sh.m_cand[wave] = mc;
  }
  __syncthreads();
  const uint32_t n_valid = sh.n_valid[0] + sh.n_valid[1] + sh.n_valid[2] + sh.n_valid[3];
  const uint32_t n_cand = sh.n_cand[0] + sh.n_cand[1] + sh.n_cand[2] + sh.n_cand[3];
  const uint32_t n_ban = sh.n_ban[0] + sh.n_ban[1] + sh.n_ban[2] + sh.n_ban[3];
  const bool lift = cn_lift(n_cand, n_valid);  // every valid column is banned: the bans are lifted, the penalty stays
  const float M = lift ? fmaxf(fmaxf(sh.m_valid[0], sh.m_valid[1]), fmaxf(sh.m_valid[2], sh.m_valid[3]))
                       : fmaxf(fmaxf(sh.m_cand[0], sh.m_cand[1]), fmaxf(sh.m_cand[2], sh.m_cand[3]));

  // the selection over the candidates
  uint32_t s0 = 0, s1 = 0;
  if constexpr (SAMPLED) {
    s0 = a.seeds[b];
    s1 = a.seeds[a.B + b];
  }
  float bv = -3.402823466e+38f, zw = 0.0f, sum = 0.0f, by = ninf;
  int bi = 0x7fffffff;
  cn_each<RESIDENT, VEC>(l, ban, row, N, tid, banned, seen, theta, inv_theta, [&](int c, float lp, bool bn) {
    const float z = lp * inv_T;
    const bool in = cn_candidate(z, bn, lift);
    float e = in ? lse_exp(z - M) : 0.0f;
    e = z == z ? e : z;  // (a NaN anywhere in the row makes the sum NaN)
    sum += e;
    by = c == fc ? z : by;
    if (in) {
      float key = z;
      if constexpr (SAMPLED) key = sm_key(lp, inv_T, s0, s1, a.shortlist ? a.shortlist[c] : (uint32_t)c);
      if (key > bv) {  // (columns ascend: the first maximum)
        bv = key;
        bi = c;
        zw = z;
      }
    }
  });
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const float ov = __shfl_xor(bv, m, 64);
    const int oi = __shfl_xor(bi, m, 64);
    const float oz = __shfl_xor(zw, m, 64);
    sum = sum + __shfl_xor(sum, m, 64);  // (commutative: both partners get the same bits)
    by = fmaxf(by, __shfl_xor(by, m, 64));
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
      zw = oz;
    }
  }
  if (lane == 0) {
    sh.r_key[wave] = bv;
    sh.r_col[wave] = bi;
    sh.r_zw[wave] = zw;
    sh.r_sum[wave] = sum;
    sh.r_y[wave] = by;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      const float ov = sh.r_key[w];
      const int oi = sh.r_col[w];
      sum = sum + sh.r_sum[w];
      by = fmaxf(by, sh.r_y[w]);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
        zw = sh.r_zw[w];
      }
    }
    a.part_val[b] = bv;
    a.part_idx[b] = bi;
    if (a.part_sum) a.part_sum[b] = sum;
    if constexpr (SAMPLED) {
      a.part_mz[b] = M;
      a.part_zw[b] = zw;
    }
    if (a.part_y) a.part_y[b] = by;
    if (a.n_banned) a.n_banned[b] = n_ban | (lift ? kConstraintFallback : 0u);
  }
}

template <bool SAMPLED>
hipError_t cn_launch(const StepConstrainArgs &a, hipStream_t st) {
  // 128-bit loads: every row starts 16-byte aligned
  const bool vec = (a.N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15u) == 0;
  const bool resident = a.N <= kConstrainResidentN;
  auto kernel = resident ? (vec ? step_constrain_kernel<SAMPLED, true, true> : step_constrain_kernel<SAMPLED, true, false>)
                         : (vec ? step_constrain_kernel<SAMPLED, false, true> : step_constrain_kernel<SAMPLED, false, false>);
  const size_t lds = 2 * (size_t)((a.N + 31) >> 5) * sizeof(uint32_t);  // the two bitmaps
  const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(a.B), dim3(kCnThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_step_constrain(const StepConstrainArgs &a, hipStream_t st) {
  if (!a.logits || a.B < 1 || a.N < 1 || a.N > kConstraintMaxN || !a.part_val || !a.part_idx) return hipErrorInvalidValue;
  if (!a.history || !a.hist_len || a.ld_hist < 1 || a.ld_hist > kConstraintMaxHistory) return hipErrorInvalidValue;
  if (!(a.inv_T > 0.0f) || !cn_valid(a.c.no_repeat_ngram, a.c.theta, a.c.n_suppress)) return hipErrorInvalidValue;
  if ((a.fcol != nullptr) != (a.part_y != nullptr)) return hipErrorInvalidValue;
  if (a.seeds) {
    if (!a.part_sum || !a.part_mz || !a.part_zw) return hipErrorInvalidValue;
    return cn_launch<true>(a, st);
  }
  if (a.inv_T != 1.0f) return hipErrorInvalidValue;  // (a greedy step has no temperature)
  return cn_launch<false>(a, st);
}

}  // namespace slimt_hip
