// Locally typical sampling (slimt_hip_ctx_set_sampling_typical): the kept set of one sampled step (typical.h) and the draw
// over it.
//
// One 256-thread workgroup per row, with sample_floor.hip's ownership: thread t owns the 4-column groups t, t + 256, t + 512,
// t + 768 (one 128-bit load each where the row is 16-byte aligned) and keeps their 16 logits in registers.
//   A  valid (non-NaN) count and maximum M of z = logit * inv_T: wave shuffles, one LDS word each per wave
//   B  Q = sum w and A = sum w G in ONE sweep, w = tr_weight(z, M) and G = ty_gap(z, M): both uint64, shuffled as two halves,
//      one 64-bit LDS add each per wave. Every thread then forms Ebar = A / Q from the two LDS words: a lane that divides
//      alone costs the wave the same instructions and a barrier more for the broadcast
//   C  key = |G - Ebar| beside w, both in registers (RESIDENT): tr_exp has run once per column and does not run again
//   D  kappa by an ascending radix descent on the 21-bit key: three passes of 7-bit digits from the top, a 128-bin histogram
//      of uint64 weights per wave in LDS (4 KiB), merged once per pass; a prefix scan over the bins (two waves of shuffles)
//      finds the bin in which the mass reaches the double target mass * Q
//   E  the draw over w > 0 && key <= kappa: Gumbel key, first-maximum quintuple, float sum of exp(z - M) and z at the forced
//      column, merged with the arg-max's tie rule (key, then lower column), exactly as sample_floor.hip merges them
// Integer sums alone decide the set, so every order of accumulation gives the same bits. The register-resident variant covers
// N <= kTypicalResidentN = 4096 (the shortlist case). Above it the streaming variant walks the same groups in the same order
// and recomputes w and key from the row (L2) in each phase: the same arithmetic on the same columns of the same thread, so
// the same bits; N <= kTypicalMaxN. Every branch around a barrier is uniform over the workgroup.
// The result is one partial per row in EPI_ARGMAX_SM's format, like sample_truncate.hip's and sample_floor.hip's.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "typical.h"

namespace slimt_hip {
namespace {

constexpr int kTyThreads = 256;
constexpr int kTyCols = 16;   // columns a thread holds: four groups of four
constexpr int kTyDigit = 7;   // bits per pass of the descent
constexpr int kTyBins = 1 << kTyDigit;
static_assert(kTyThreads * kTyCols == kTypicalResidentN, "the register-resident bound is threads x columns per thread");
static_assert(kTypicalKeyBits % kTyDigit == 0 && kTyBins <= kTyThreads, "whole digits, and a thread per bin in the scan");

struct TyShared {
  unsigned long long hist[4][kTyBins];  // per-wave digit histograms of weights
  unsigned long long wave_tot[4];
  unsigned long long q, a;              // Q and A
  unsigned long long sel_below;         // the weight strictly below the selected bin
  uint32_t sel_bin;
  uint32_t n_valid[4];
  float mx[4];
  float r_key[4], r_sum[4], r_zw[4], r_y[4];
  int r_col[4];
  uint32_t r_kept[4];
};

__device__ __forceinline__ unsigned long long ty_shfl_xor(unsigned long long v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long ty_shfl_up(unsigned long long v, int off) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, off, 64);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// the four columns from c0 (a multiple of 4, c0 < N); VEC: N is a multiple of 4 and the row 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void ty_load4(const float *__restrict__ row, int N, int c0, float (&v)[4]) {
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

// f(slot, column, logit) over the thread's columns, ascending; slot: the column's register (RESIDENT), else 0
template <bool RESIDENT, bool VEC, class F>
__device__ __forceinline__ void ty_each(const float (&l)[kTyCols], const float *__restrict__ row, int N, int tid, F &&f) {
  if constexpr (RESIDENT) {
#pragma unroll
    for (int i = 0; i < kTyCols; ++i) {
      const int c = 4 * ((i >> 2) * kTyThreads + tid) + (i & 3);
      if (c < N) f(i, c, l[i]);
    }
  } else {
    for (int c0 = 4 * tid; c0 < N; c0 += 4 * kTyThreads) {  // (N <= kTypicalMaxN: c0 stays an int)
      float v[4];
      ty_load4<VEC>(row, N, c0, v);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < N) f(0, c0 + e, v[e]);
    }
  }
}

// a column's weight (0 where z is NaN) and, where that is above 0, its gap
__device__ __forceinline__ void ty_weigh(float z, float M, uint32_t &w, uint32_t &G) {
  w = z == z ? tr_weight(z, M) : 0u;
  G = w ? ty_gap(z, M) : 0u;
}

template <bool RESIDENT, bool VEC>
__global__ __launch_bounds__(kTyThreads) void sample_typical_kernel(SampleTypicalArgs a) {
  __shared__ TyShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const float *__restrict__ row = a.logits + (size_t)b * N;
  const float inv_T = a.inv_T;
  const float ninf = -__builtin_inff();

  // the one global read (RESIDENT)
  float l[kTyCols];
#pragma unroll
  for (int i = 0; i < kTyCols; ++i) l[i] = 0.0f;
  if constexpr (RESIDENT) {
#pragma unroll
    for (int j = 0; j < kTyCols / 4; ++j) {
      const int c0 = 4 * (j * kTyThreads + tid);
      if (c0 < N) {
        float v[4];
        ty_load4<VEC>(row, N, c0, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) l[4 * j + e] = v[e];
      }
    }
  }

  // A: the valid columns and their maximum
  uint32_t nv = 0;
  float M = ninf;
  ty_each<RESIDENT, VEC>(l, row, N, tid, [&](int, int, float lc) {
    const float z = lc * inv_T;
    const bool valid = z == z;
    nv += valid ? 1u : 0u;
    M = valid ? fmaxf(M, z) : M;
  });
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    nv += (uint32_t)__shfl_xor((int)nv, m, 64);
    M = fmaxf(M, __shfl_xor(M, m, 64));
  }
  if (lane == 0) {
    sh.n_valid[wave] = nv;
    sh.mx[wave] = M;
  }
  if (tid == 0) {
    sh.q = 0;
    sh.a = 0;
  }
  __syncthreads();
  const uint32_t n_valid = sh.n_valid[0] + sh.n_valid[1] + sh.n_valid[2] + sh.n_valid[3];
  M = fmaxf(fmaxf(sh.mx[0], sh.mx[1]), fmaxf(sh.mx[2], sh.mx[3]));

  const int fc = a.fcol ? a.fcol[b] : -1;
  const bool cut = fc < 0 && n_valid > 0;  // (a forced step draws nothing: every valid column stays)

  uint32_t key[kTyCols], w[kTyCols];  // (RESIDENT) the columns' keys and weights from phase C on
#pragma unroll
  for (int i = 0; i < kTyCols; ++i) key[i] = w[i] = 0u;
  uint32_t ebar = 0, kappa = 0;
  // a column's weight and key in phases D and E: from the registers, or formed again
  auto col = [&](int i, float lc, uint32_t &wc, uint32_t &kc) {
    if constexpr (RESIDENT) {
      wc = w[i];
      kc = key[i];
    } else {
      uint32_t G;
      ty_weigh(lc * inv_T, M, wc, G);
      kc = ty_key(G, ebar);
    }
  };
  if (cut) {  // (uniform over the workgroup, like everything around the barriers inside)
    // B: Q and A
    unsigned long long q = 0, ag = 0;
    ty_each<RESIDENT, VEC>(l, row, N, tid, [&](int i, int, float lc) {
      uint32_t wc, G;
      ty_weigh(lc * inv_T, M, wc, G);
      q += wc;
      ag += (unsigned long long)wc * G;
      if constexpr (RESIDENT) {
        w[i] = wc;
        key[i] = G;
      }
    });
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      q += ty_shfl_xor(q, m);
      ag += ty_shfl_xor(ag, m);
    }
    if (lane == 0) {
      atomicAdd(&sh.q, q);
      atomicAdd(&sh.a, ag);
    }
    __syncthreads();
    const unsigned long long Q = sh.q;
    ebar = ty_mean(sh.a, Q);
    // C: the gaps become keys
    if constexpr (RESIDENT) {
#pragma unroll
      for (int i = 0; i < kTyCols; ++i) key[i] = ty_key(key[i], ebar);
    }
    // D: kappa, digit by digit from the top
    const double target = ty_target(a.mass, Q);
    uint32_t mask = 0;
    unsigned long long below = 0;
    for (int shift = kTypicalKeyBits - kTyDigit; shift >= 0; shift -= kTyDigit) {
      for (int i = tid; i < 4 * kTyBins; i += kTyThreads) (&sh.hist[0][0])[i] = 0;
      __syncthreads();
      ty_each<RESIDENT, VEC>(l, row, N, tid, [&](int i, int, float lc) {
        uint32_t wc, kc;
        col(i, lc, wc, kc);
        if (wc != 0 && (kc & mask) == kappa) atomicAdd(&sh.hist[wave][(kc >> shift) & (kTyBins - 1)], (unsigned long long)wc);
      });
      __syncthreads();
      const unsigned long long cnt = tid < kTyBins ? sh.hist[0][tid] + sh.hist[1][tid] + sh.hist[2][tid] + sh.hist[3][tid] : 0ull;
      unsigned long long s = cnt;  // -> the sum over the bins <= tid
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = ty_shfl_up(s, off);
        s += lane >= off ? o : 0ull;
      }
      if (lane == 63) sh.wave_tot[wave] = s;
      __syncthreads();
      for (int v = 0; v < wave; ++v) s += sh.wave_tot[v];
      const unsigned long long incl = below + s, excl = incl - cnt;
      // (one bin: the sums rise with the bin, none is reached at weight 0, and the sum over all bins reaches)
      if ((double)incl >= target && !((double)excl >= target)) {
        sh.sel_bin = (uint32_t)tid;
        sh.sel_below = excl;
      }
      __syncthreads();
      kappa |= sh.sel_bin << shift;
      mask |= (uint32_t)(kTyBins - 1) << shift;
      below = sh.sel_below;
    }
  }

  // E: the draw over the kept set
  const uint32_t s0 = a.seeds[b], s1 = a.seeds[a.B + b];
  float bv = -3.402823466e+38f, zw = 0.0f, sum = 0.0f, by = ninf;
  int bi = 0x7fffffff;
  uint32_t kept = 0;
  ty_each<RESIDENT, VEC>(l, row, N, tid, [&](int i, int c, float lc) {
    const float z = lc * inv_T;
    bool in = z == z;
    if (cut && in) {
      uint32_t wc, kc;
      col(i, lc, wc, kc);
      in = wc != 0 && kc <= kappa;
    }
    float e = in ? lse_exp(z - M) : 0.0f;
    e = z == z ? e : z;  // (a NaN anywhere in the row makes the sum NaN)
    sum += e;
    by = c == fc ? z : by;
    kept += in ? 1u : 0u;
    if (in) {
      const uint32_t id = a.shortlist ? a.shortlist[c] : (uint32_t)c;
      const float gk = sm_key(lc, inv_T, s0, s1, id);
      if (gk > bv) {  // (columns ascend: the first maximum)
        bv = gk;
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
    kept += (uint32_t)__shfl_xor((int)kept, m, 64);
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
    sh.r_kept[wave] = kept;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < 4; ++v) {
      const float ov = sh.r_key[v];
      const int oi = sh.r_col[v];
      sum = sum + sh.r_sum[v];
      by = fmaxf(by, sh.r_y[v]);
      kept += sh.r_kept[v];
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
        zw = sh.r_zw[v];
      }
    }
    a.part_val[b] = bv;
    a.part_idx[b] = bi;
    a.part_sum[b] = sum;
    a.part_mz[b] = M;
    a.part_zw[b] = zw;
    if (a.part_y) a.part_y[b] = by;
    if (a.kept) a.kept[b] = kept;
    if (a.mean_gap) a.mean_gap[b] = ebar;
  }
}

}  // namespace

hipError_t launch_sample_typical(const SampleTypicalArgs &a, hipStream_t st) {
  if (!a.logits || a.B < 1 || a.N < 1 || a.N > kTypicalMaxN || !a.seeds || !a.part_val || !a.part_idx || !a.part_sum || !a.part_mz || !a.part_zw)
    return hipErrorInvalidValue;
  if (!(a.inv_T > 0.0f) || !ty_valid(a.mass)) return hipErrorInvalidValue;
  if ((a.fcol != nullptr) != (a.part_y != nullptr)) return hipErrorInvalidValue;
  // 128-bit loads: every row starts 16-byte aligned
  const bool vec = (a.N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15u) == 0;
  const bool resident = a.N <= kTypicalResidentN;
  auto kernel = resident ? (vec ? sample_typical_kernel<true, true> : sample_typical_kernel<true, false>)
                         : (vec ? sample_typical_kernel<false, true> : sample_typical_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(a.B), dim3(kTyThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace slimt_hip
