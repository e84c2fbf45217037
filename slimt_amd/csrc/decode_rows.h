// The row and weight-fragment helpers of the decode-step kernels (decode_kernels.hip, decode_fanout.hip): 16 f32 rows in
// registers, their canonical LayerNorm and quantisation, and the prefetched B operands of the 16 x 16 x 64 int8 MFMA.
#pragma once

#include "device_common.h"

namespace slimt_hip {

constexpr int MAXDPL = 8;  // D <= 512: elements per lane of one f32 row

// ---- 16 f32 rows -> (optional LayerNorm) -> registers ---------------------
// Each wave owns rows [w*RPW, w*RPW + RPW). Lane l holds elements l + 64 i.

template <int RPW>
struct Rows {
  float v[RPW][MAXDPL];
};

template <int RPW>
__device__ __forceinline__ void rows_load(Rows<RPW> &r, const float *x, int B, int D, int row0,
                                          int lane) {
  const int dpl = D >> 6;
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int row = row0 + k;
#pragma unroll
    for (int i = 0; i < MAXDPL; ++i) {
      float t = 0.0f;
      if (i < dpl && row < B) t = x[(size_t)row * D + lane + 64 * i];
      r.v[k][i] = t;
    }
  }
}

// canonical LayerNorm (device_common.h: wave_layer_norm_row) on registers
template <int RPW>
__device__ __forceinline__ void rows_layer_norm(Rows<RPW> &r, const float *scale,
                                                const float *bias, float eps, int D, int lane) {
  const int dpl = D >> 6;
  float sc[MAXDPL], bi[MAXDPL];
#pragma unroll
  for (int i = 0; i < MAXDPL; ++i) {
    sc[i] = i < dpl ? scale[lane + 64 * i] : 0.0f;
    bi[i] = i < dpl ? bias[lane + 64 * i] : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < MAXDPL; ++i)
      if (i < dpl) s += r.v[k][i];
    s = wave_sum(s);
    const float mean = s / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < MAXDPL; ++i)
      if (i < dpl) {
        const float d = r.v[k][i] - mean;
        q += d * d;
      }
    q = wave_sum(q);
    const float sigma = __builtin_sqrtf(q / (float)D + eps);
#pragma unroll
    for (int i = 0; i < MAXDPL; ++i)
      if (i < dpl) {
        const float t = (r.v[k][i] - mean) / sigma;
        const float m = sc[i] * t;
        r.v[k][i] = m + bi[i];
      }
  }
}

template <int RPW>
__device__ __forceinline__ void rows_quantize_to_lds(const Rows<RPW> &r, float aq, char *A_lds,
                                                     int lda, int rl0, int D, int lane) {
  const int dpl = D >> 6;
#pragma unroll
  for (int k = 0; k < RPW; ++k)
#pragma unroll
    for (int i = 0; i < MAXDPL; ++i)
      if (i < dpl) A_lds[(rl0 + k) * lda + lane + 64 * i] = (char)quantize1(r.v[k][i], aq);
}

template <int RPW>
__device__ __forceinline__ void rows_store_lds(const Rows<RPW> &r, float *buf, int ldr, int rl0,
                                               int D, int lane) {
  const int dpl = D >> 6;
#pragma unroll
  for (int k = 0; k < RPW; ++k)
#pragma unroll
    for (int i = 0; i < MAXDPL; ++i)
      if (i < dpl) buf[(rl0 + k) * ldr + lane + 64 * i] = r.v[k][i];
}

// ---- weight fragment prefetch ---------------------------------------------

template <int PF, int NT>
struct BFrag {
  v4i f[PF][NT];
};

template <int PF, int NT>
__device__ __forceinline__ void bfrag_load(BFrag<PF, NT> &b, const v4i *Wp, int KS, int chunk,
                                           int nt0, int n_tiles, int lane) {
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    const int ks = chunk * PF + p;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int ntile = nt0 + nt;
      v4i t = {0, 0, 0, 0};
      if (ks < KS && ntile < n_tiles) t = Wp[((size_t)ntile * KS + ks) * 64 + lane];
      b.f[p][nt] = t;
    }
  }
}

template <int PF, int NT>
__device__ __forceinline__ void bfrag_mma(const BFrag<PF, NT> &b, const char *A_lds, int lda,
                                          int KS, int chunk, int lr, int lg, v4i (&acc)[NT]) {
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    const int ks = chunk * PF + p;
    if (ks < KS) {
      const v4i af = *reinterpret_cast<const v4i *>(A_lds + lr * lda + ks * 64 + lg * 16);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, b.f[p][nt], acc[nt], 0, 0, 0);
    }
  }
}

}  // namespace slimt_hip
