// Floored sampling (slimt_hip_ctx_set_sampling_floor): min-p / epsilon truncation of one sampled step and the draw over it.
//
// A floor needs two plain reductions of the row -- the maximum M and, for epsilon, the integer total Q (floor.h) -- where
// top-k / top-p need a radix select. So the row is read from memory ONCE: one 256-thread workgroup per row, thread t owns
// the 4-column groups t, t + 256, t + 512, t + 768 (columns 4 g .. 4 g + 3: one 128-bit load each where the row is 16-byte
// aligned, four scalar loads where it is not -- the same ownership either way) and keeps their 16 logits in registers.
//   reduction A   valid (non-NaN) count and maximum M of z = logit * inv_T: wave shuffles, one LDS word each per wave
//   reduction B   Q, the uint64 sum of tr_weight(z, M): shuffles and one 64-bit LDS add per wave. Integers: every order
//                 gives the same bits. Skipped when epsilon is off (min-p reads no Q) and on a forced step
//   draw          keep test (fl_keep), Gumbel key, first-maximum quintuple, float sum of exp(z - M) and z at the forced
//                 column from the same registers, merged with the arg-max's tie rule (key, then lower column)
// The register-resident variant covers N <= kFloorResidentN = 4096 (16 columns x 256 threads: the shortlist case). Above
// it the streaming variant walks the same groups in the same order, g = t, t + 256, ... while 4 g < N, and re-reads them
// (from L2) in each of the three phases: the same arithmetic on the same columns of the same thread, so the same bits; N is
// bounded by floor.h's kFloorMaxN alone. Every branch around a barrier is uniform over the workgroup.
// The result is one partial per row in EPI_ARGMAX_SM's format, like sample_truncate.hip's.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "floor.h"

namespace slimt_hip {
namespace {

constexpr int kFlThreads = 256;
constexpr int kFlCols = 16;  // columns a thread holds: four groups of four
static_assert(kFlThreads * kFlCols == kFloorResidentN, "the register-resident bound is threads x columns per thread");

struct FlShared {
  unsigned long long total;  // Q
  uint32_t n_valid[4];
  float mx[4];
  float r_key[4], r_sum[4], r_zw[4], r_y[4];
  int r_col[4];
  uint32_t r_kept[4];
};

// the four columns from c0 (a multiple of 4, c0 < N); VEC: N is a multiple of 4 and the row 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void fl_load4(const float *__restrict__ row, int N, int c0, float (&v)[4]) {
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

// f(column, logit) over the thread's columns, ascending
template <bool RESIDENT, bool VEC, class F>
__device__ __forceinline__ void fl_each(const float (&l)[kFlCols], const float *__restrict__ row, int N, int tid, F &&f) {
  if constexpr (RESIDENT) {
#pragma unroll
    for (int i = 0; i < kFlCols; ++i) {
      const int c = 4 * ((i >> 2) * kFlThreads + tid) + (i & 3);
      if (c < N) f(c, l[i]);
    }
  } else {
    for (int c0 = 4 * tid; c0 < N; c0 += 4 * kFlThreads) {  // (N <= kFloorMaxN: c0 stays an int)
      float v[4];
      fl_load4<VEC>(row, N, c0, v);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < N) f(c0 + e, v[e]);
    }
  }
}

template <bool RESIDENT, bool VEC>
__global__ __launch_bounds__(kFlThreads) void sample_floor_kernel(SampleFloorArgs a) {
  __shared__ FlShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const float *__restrict__ row = a.logits + (size_t)b * N;
  const float inv_T = a.inv_T;
  const float ninf = -__builtin_inff();

  // the one global read (RESIDENT)
  float l[kFlCols];
#pragma unroll
  for (int i = 0; i < kFlCols; ++i) l[i] = 0.0f;
  if constexpr (RESIDENT) {
#pragma unroll
    for (int j = 0; j < kFlCols / 4; ++j) {
      const int c0 = 4 * (j * kFlThreads + tid);
      if (c0 < N) {
        float v[4];
        fl_load4<VEC>(row, N, c0, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) l[4 * j + e] = v[e];
      }
    }
  }

  // reduction A: the valid columns and their maximum
  uint32_t nv = 0;
  float M = ninf;
  fl_each<RESIDENT, VEC>(l, row, N, tid, [&](int, float lc) {
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
  if (tid == 0) sh.total = 0;
  __syncthreads();
  const uint32_t n_valid = sh.n_valid[0] + sh.n_valid[1] + sh.n_valid[2] + sh.n_valid[3];
  M = fmaxf(fmaxf(sh.mx[0], sh.mx[1]), fmaxf(sh.mx[2], sh.mx[3]));

  const int fc = a.fcol ? a.fcol[b] : -1;
  const bool cut = fc < 0 && n_valid > 0;  // (a forced step draws nothing: every valid column stays)

  // reduction B: Q, where epsilon reads it
  double floor_eps = 0.0;
  if (cut && fl_needs_total(a.epsilon)) {  // (uniform over the workgroup)
    unsigned long long q = 0;
    fl_each<RESIDENT, VEC>(l, row, N, tid, [&](int, float lc) {
      const float z = lc * inv_T;
      q += z == z ? tr_weight(z, M) : 0u;
    });
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)q, m, 64);
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(q >> 32), m, 64);
      q += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) atomicAdd(&sh.total, q);
    __syncthreads();
    floor_eps = fl_eps(a.epsilon, sh.total);
  }
  const double floor_min = fl_min(a.min_p);

  // the draw over the kept set
  const uint32_t s0 = a.seeds[b], s1 = a.seeds[a.B + b];
  float bv = -3.402823466e+38f, zw = 0.0f, sum = 0.0f, by = ninf;
  int bi = 0x7fffffff;
  uint32_t kept = 0;
  fl_each<RESIDENT, VEC>(l, row, N, tid, [&](int c, float lc) {
    const float z = lc * inv_T;
    bool in = z == z;
    if (cut && in) in = fl_keep(z, M, tr_weight(z, M), floor_min, floor_eps);
    float e = in ? lse_exp(z - M) : 0.0f;
    e = z == z ? e : z;  // (a NaN anywhere in the row makes the sum NaN)
    sum += e;
    by = c == fc ? z : by;
    kept += in ? 1u : 0u;
    if (in) {
      const uint32_t id = a.shortlist ? a.shortlist[c] : (uint32_t)c;
      const float key = sm_key(lc, inv_T, s0, s1, id);
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
    if (a.kept) a.kept[b] = kept;
  }
}

}  // namespace

hipError_t launch_sample_floor(const SampleFloorArgs &a, hipStream_t st) {
  if (!a.logits || a.B < 1 || a.N < 1 || a.N > kFloorMaxN || !a.seeds || !a.part_val || !a.part_idx || !a.part_sum || !a.part_mz || !a.part_zw)
    return hipErrorInvalidValue;
  if (!(a.inv_T > 0.0f) || !fl_valid(a.min_p, a.epsilon)) return hipErrorInvalidValue;
  if ((a.fcol != nullptr) != (a.part_y != nullptr)) return hipErrorInvalidValue;
  // 128-bit loads: every row starts 16-byte aligned
  const bool vec = (a.N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15u) == 0;
  const bool resident = a.N <= kFloorResidentN;
  auto kernel = resident ? (vec ? sample_floor_kernel<true, true> : sample_floor_kernel<true, false>)
                         : (vec ? sample_floor_kernel<false, true> : sample_floor_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(a.B), dim3(kFlThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace slimt_hip
