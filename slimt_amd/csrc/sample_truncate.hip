// Truncated sampling (slimt_hip_ctx_set_sampling_truncation): the kept set of one sampled step and the draw over it.
//
// One 256-thread workgroup per row over the row's N f32 logits, which the logits gemm has just written (L2-resident:
// 16 KiB at N = 4096); every pass re-reads them, so N is arbitrary.
//   pass 0     counts the valid (non-NaN) z = logit * inv_T and finds their maximum M
//   top-k      a radix select on tr_ord(z): four passes of 8-bit digits from the top, a 256-bin histogram per wave in LDS
//              (one shared histogram serialises on a hot bin), merged once per pass; a suffix scan over the bins finds the
//              digit of the k-th largest
//   top-p      the same descent with each bin holding the uint64 sum of the integer weights tr_weight(z, M) of the columns
//              with z >= tau_k, against the double target top_p * Q. Integer sums: every order of accumulation gives the
//              same bits, so the set is the host checker's, exactly
//   last pass  over z >= max(tau_k, tau_p): the sampled step's quintuple (best key, its column, M, sum of exp(z - M), z of
//              the key's column) and z at the row's forced column, merged with the arg-max's tie rule (key, then lower column)
// The result is one partial per row in EPI_ARGMAX_SM's format.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "truncation.h"

namespace slimt_hip {
namespace {

constexpr int kTrThreads = 256;

struct TrShared {
  unsigned long long hist[4][256];  // per-wave digit histograms: counts (top-k) or weights (top-p)
  unsigned long long wave_tot[4];
  unsigned long long sel_above;     // the sum strictly above the selected bin
  unsigned long long total;         // the sum over the first pass's bins (top-p: Q)
  uint32_t sel_bin;
  uint32_t n_valid[4];
  float mx[4];
  float r_key[4], r_sum[4], r_zw[4], r_y[4];
  int r_col[4];
  uint32_t r_kept[4];
};

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, int off) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, off, 64);
  const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// The largest word o among the selected columns' tr_ord(z) with reach(sum of val over the selected columns with
// tr_ord(z) >= o), where val is 1 (W = false: reach(x) is x >= k, so o is the k-th largest) or the column's weight
// (W = true: reach(x) is (double)x >= top_p * (double)Q, Q the sum over all selected columns). Selected: valid, and for
// W also z >= tau_k. The caller guarantees that the sum over all selected columns reaches. Every thread returns o.
template <bool W>
__device__ __forceinline__ uint32_t tr_select(const float *__restrict__ row, int N, float inv_T, float M, float tau_k,
                                              uint32_t k, float top_p, TrShared &sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t prefix = 0, mask = 0;
  unsigned long long above = 0;
  double target = 0.0;
  for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
    for (int w = 0; w < 4; ++w) sh.hist[w][tid] = 0;
    __syncthreads();
    for (int c = tid; c < N; c += kTrThreads) {
      const float z = row[c] * inv_T;
      const uint32_t o = tr_ord(z);
      bool in = z == z && (o & mask) == prefix;
      unsigned long long val = 1;
      if constexpr (W) {
        in = in && z >= tau_k;
        val = in ? tr_weight(z, M) : 0u;
        in = in && val != 0;
      }
      if (in) atomicAdd(&sh.hist[wave][(o >> shift) & 255u], val);
    }
    __syncthreads();
    const unsigned long long cnt = sh.hist[0][tid] + sh.hist[1][tid] + sh.hist[2][tid] + sh.hist[3][tid];
    unsigned long long s = cnt;  // -> the sum over the bins >= tid
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long o = shfl_down_u64(s, off);
      s += lane + off < 64 ? o : 0ull;
    }
    if (lane == 0) sh.wave_tot[wave] = s;
    __syncthreads();
    for (int w = wave + 1; w < 4; ++w) s += sh.wave_tot[w];
    if constexpr (W) {
      if (shift == 24) {
        if (tid == 0) sh.total = s;
        __syncthreads();
        target = (double)top_p * (double)sh.total;
      }
    }
    const unsigned long long incl = above + s, excl = incl - cnt;
    bool hit;
    if constexpr (W)
      hit = (double)incl >= target && !((double)excl >= target);
    else
      hit = incl >= k && excl < k;
    if (hit) {  // (one bin: the sums fall as the bin rises, and the one over all bins reaches)
      sh.sel_bin = (uint32_t)tid;
      sh.sel_above = excl;
    }
    __syncthreads();
    prefix |= sh.sel_bin << shift;
    mask |= 255u << shift;
    above = sh.sel_above;
  }
  return prefix;
}

__global__ __launch_bounds__(kTrThreads) void sample_truncated_kernel(SampleTruncArgs a) {
  __shared__ TrShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const float *__restrict__ row = a.logits + (size_t)b * N;
  const float inv_T = a.inv_T;
  const float ninf = -__builtin_inff();

  // pass 0: the valid columns and their maximum
  uint32_t nv = 0;
  float M = ninf;
  for (int c = tid; c < N; c += kTrThreads) {
    const float z = row[c] * inv_T;
    const bool valid = z == z;
    nv += valid ? 1u : 0u;
    M = valid ? fmaxf(M, z) : M;
  }
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
    sh.sel_bin = 0;
    sh.sel_above = 0;
  }
  __syncthreads();
  const uint32_t n_valid = sh.n_valid[0] + sh.n_valid[1] + sh.n_valid[2] + sh.n_valid[3];
  M = fmaxf(fmaxf(sh.mx[0], sh.mx[1]), fmaxf(sh.mx[2], sh.mx[3]));

  const int fc = a.fcol ? a.fcol[b] : -1;
  const bool cut = fc < 0 && n_valid > 0;  // (a forced step draws nothing: every valid column stays)
  float tau_k = ninf, tau_p = ninf;
  if (cut && a.top_k != 0 && a.top_k < n_valid) tau_k = tr_unord(tr_select<false>(row, N, inv_T, M, ninf, a.top_k, 1.0f, sh));
  if (cut && a.top_p < 1.0f) tau_p = tr_unord(tr_select<true>(row, N, inv_T, M, tau_k, 0, a.top_p, sh));
  const float tau = fmaxf(tau_k, tau_p);

  // last pass: the draw over the kept set
  const uint32_t s0 = a.seeds[b], s1 = a.seeds[a.B + b];
  float bv = -3.402823466e+38f, zw = 0.0f, sum = 0.0f, by = ninf;
  int bi = 0x7fffffff;
  uint32_t kept = 0;
  for (int c = tid; c < N; c += kTrThreads) {
    const float l = row[c];
    const float z = l * inv_T;
    const bool in = z == z && z >= tau;
    float e = in ? lse_exp(z - M) : 0.0f;
    e = z == z ? e : z;  // (a NaN anywhere in the row makes the sum NaN)
    sum += e;
    by = c == fc ? z : by;
    kept += in ? 1u : 0u;
    if (in) {
      const uint32_t id = a.shortlist ? a.shortlist[c] : (uint32_t)c;
      const float key = sm_key(l, inv_T, s0, s1, id);
      if (key > bv) {  // (columns ascend: the first maximum)
        bv = key;
        bi = c;
        zw = z;
      }
    }
  }
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
    for (int w = 1; w < 4; ++w) {
      const float ov = sh.r_key[w];
      const int oi = sh.r_col[w];
      sum = sum + sh.r_sum[w];
      by = fmaxf(by, sh.r_y[w]);
      kept += sh.r_kept[w];
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
        zw = sh.r_zw[w];
      }
    }
    a.part_val[b] = bv;
    a.part_idx[b] = bi;
    a.part_sum[b] = sum;
    a.part_mz[b] = M;
    a.part_zw[b] = zw;
    if (a.part_y) a.part_y[b] = by;
    if (a.thresholds) a.thresholds[b] = tau;
    if (a.kept) a.kept[b] = kept;
  }
}

}  // namespace

hipError_t launch_sample_truncated(const SampleTruncArgs &a, hipStream_t st) {
  if (!a.logits || a.B < 1 || a.N < 1 || a.N > kSampleTruncMaxN || !a.seeds || !a.part_val || !a.part_idx || !a.part_sum || !a.part_mz || !a.part_zw)
    return hipErrorInvalidValue;
  if (!(a.inv_T > 0.0f) || !(a.top_p > 0.0f && a.top_p <= 1.0f)) return hipErrorInvalidValue;
  if ((a.fcol != nullptr) != (a.part_y != nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_truncated_kernel, dim3(a.B), dim3(kTrThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace slimt_hip
