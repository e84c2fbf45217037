// Fan-out translate calls (slimt_hip_translate_fanout*): N decoder rows over B encoded sources.
//
// A fan-out call is a step-wise translate call (decode_kernels.hip) whose row r attends over the K / V of source
// row_src[r] instead of source r. Everything of a decode step but the cross-attention is row-wise and runs unchanged with
// "sentence" read as "row"; this file adds the attention that knows the source:
//   dqattn_fanout_kernel   dqattn_kernel's LayerNorm + Q projection for 16 rows of one head, then the workgroup walks its
//                          rows as RUNS of consecutive rows that name one source: the source's head slice of K and V is
//                          staged in LDS once per run and the run's waves attend over it, one wave per row
// Each row's float sequence is dqattn_kernel's line for line (the hoisted and the literal order), so a row's joined heads
// and alignment rows are the bits the step-wise slimt_hip_translate writes for that row of the duplicated batch
// src_ids[row_src]. Only the addresses the K / V operands and the length come from differ: LDS and lengths[source].
//
// Barriers: every __syncthreads() below is reached by all 1024 threads. The run boundaries depend on values that every
// thread loads from the same read-only addresses (row_src[m0 ..]) and passes through readfirstlane: the decision is the
// workgroup's. The waves of rows past the call's last (and those outside the current run) stage with the others and wait
// at the next barrier; no wave leaves before the last run.
//
// LDS: the 16 quantised rows and their Q slice as in dqattn_kernel, then K [DH/4][S][4] + V [S][DH] of ONE source,
// 8 S DH bytes: 64 KiB at S = 128, DH = 64, 78,080 bytes with the Q operands at D = 512 -- above the 64 KiB a kernel gets
// without asking (set_dynamic_lds_once), under half the 160 KiB of a gfx950 CU. Lane j reads the 16 bytes of key j in
// plane i: consecutive lanes, consecutive 16-byte slots -- no bank conflict in a 16-lane group of the 128-bit reads; V is
// read one dword per lane at consecutive addresses (lanes past the head broadcast its last column).
//
// No out-of-line device functions, no dynamic stack.
#include "device_common.h"
#include "decode_rows.h"
#include "kernels.h"

namespace slimt_hip {

namespace {

template <int PF, int DH>
__global__ __launch_bounds__(1024) void dqattn_fanout_kernel(DQAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int QT = DH / 16;  // 16-column tiles of this head's Q slice
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * 16, h = blockIdx.y;
  const int D = a.D, KS = D >> 6, lda = D + 16, S = a.S;
  char *A_lds = smem;
  float *qbuf = reinterpret_cast<float *>(smem + 16 * lda);  // [16][DH]
  float *Ks = qbuf + 16 * DH;                                // [DH/4][S][4]
  float *Vs = Ks + (size_t)DH * S;                           // [S][DH]
  const int b = m0 + wave;  // this wave's row

  // 1. this row's normalised decoder state (A row of the Q GEMM)
  Rows<1> x;
  rows_load<1>(x, a.x.x, a.rows, D, b, lane);
  // 2. Q weight fragments (only the waves that run the MFMA)
  BFrag<PF, 1> bq;
  if (wave < QT)
    bfrag_load<PF, 1>(bq, reinterpret_cast<const v4i *>(a.wq.Wp), KS, 0, h * QT + wave, D / 16, lane);
  if (a.x.ln_scale) rows_layer_norm<1>(x, a.x.ln_scale, a.x.ln_bias, a.eps, D, lane);
  rows_quantize_to_lds<1>(x, a.wq.a_quant, A_lds, lda, wave, D, lane);
  __syncthreads();
  // 3. the 16 rows' Q slice
  if (wave < QT) {
    v4i acc[1] = {v4i{0, 0, 0, 0}};
    bfrag_mma<PF, 1>(bq, A_lds, lda, KS, 0, lr, lg, acc);
    const int col = (h * QT + wave) * 16 + lr;
    const int cs = a.wq.colsum[col];
    const float pb = a.wq.pb[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = (float)(acc[0][r] + 127 * cs) * a.wq.u;
      v = v + pb;
      qbuf[(lg * 4 + r) * DH + wave * 16 + lr] = v;
    }
  }
  // (the first run's barrier in front of its staging is the one behind these writes)

  const int j0 = lane < S ? lane : S - 1;
  const int j1 = (lane + 64) < S ? (lane + 64) : S - 1;
  const int dc = lane < DH ? lane : DH - 1;
  const bool lit = a.literal;  // (uniform) the reference's sequence: every cached value dequantised first, k = float(accS) u + pb
  const float pbv_d = a.pbv[h * DH + dc];
  const int n_loc = a.rows - m0 < 16 ? a.rows - m0 : 16;  // the workgroup's rows of the call (>= 1 by the grid)
  auto source_of = [&](int r) {  // (workgroup-uniform) the source of local row r
    const uint32_t named = a.row_src[m0 + r];
    return __builtin_amdgcn_readfirstlane(named < (uint32_t)a.B ? (int)named : a.B - 1);
  };
  for (int r0 = 0; r0 < n_loc;) {
    const int src = source_of(r0);
    int r1 = r0 + 1;
    while (r1 < n_loc && source_of(r1) == src) ++r1;
    __syncthreads();  // the rows of the run before this one have read the old K / V (first run: qbuf is written)
    {
      const float4 *kb = reinterpret_cast<const float4 *>(a.k + ((size_t)src * a.H + h) * (size_t)(DH / 4) * S * 4);
      for (int i = tid; i < (DH / 4) * S; i += 1024) reinterpret_cast<float4 *>(Ks)[i] = kb[i];
      for (int i = tid; i < (DH / 4) * S; i += 1024) {
        const int j = i / (DH / 4), c4 = i - j * (DH / 4);
        reinterpret_cast<float4 *>(Vs)[i] =
            *reinterpret_cast<const float4 *>(a.v + ((size_t)src * S + j) * a.ldv + h * DH + c4 * 4);
      }
    }
    __syncthreads();
    if (wave >= r0 && wave < r1) {  // (whole waves) the run's rows; no barrier inside
      // 4. scores in the hoisted (PORTABLE) order (dqattn_kernel step 4): the cache holds float(accS); t_j = k-ascending
      // fmaf chain, s_j = alpha * fmaf(t_j, uK, c_h) + mask with c_h = canonical row sum of q_d * pbK[d]
      const float *qrow = qbuf + wave * DH;
      const float ch = wave_sum(lane < DH ? qrow[dc] * a.pbk[h * DH + dc] : 0.0f);
      auto dq4 = [&](float4 v, int i) {
        if (lit) {
          const float4 pb4 = *reinterpret_cast<const float4 *>(a.pbk + h * DH + 4 * i);
          v.x = v.x * a.uk; v.y = v.y * a.uk; v.z = v.z * a.uk; v.w = v.w * a.uk;
          v.x = v.x + pb4.x; v.y = v.y + pb4.y; v.z = v.z + pb4.z; v.w = v.w + pb4.w;
        }
        return v;
      };
      float s0 = 0.0f, s1 = 0.0f;
      // (four planes at a time: unrolled whole, the hoisted 128-bit reads of all DH / 4 planes spill from d_head 32 on; the
      // chain's order is the same)
#pragma unroll 4
      for (int i = 0; i < DH / 4; ++i) {
        const float4 q4 = *reinterpret_cast<const float4 *>(qrow + 4 * i);
        const float4 k4 = dq4(*reinterpret_cast<const float4 *>(Ks + ((size_t)i * S + j0) * 4), i);
        s0 = __builtin_fmaf(q4.x, k4.x, s0);
        s0 = __builtin_fmaf(q4.y, k4.y, s0);
        s0 = __builtin_fmaf(q4.z, k4.z, s0);
        s0 = __builtin_fmaf(q4.w, k4.w, s0);
      }
      if (S > 64) {
#pragma unroll 4
        for (int i = 0; i < DH / 4; ++i) {
          const float4 q4 = *reinterpret_cast<const float4 *>(qrow + 4 * i);
          const float4 k4 = dq4(*reinterpret_cast<const float4 *>(Ks + ((size_t)i * S + j1) * 4), i);
          s1 = __builtin_fmaf(q4.x, k4.x, s1);
          s1 = __builtin_fmaf(q4.y, k4.y, s1);
          s1 = __builtin_fmaf(q4.z, k4.z, s1);
          s1 = __builtin_fmaf(q4.w, k4.w, s1);
        }
      }
      if (!lit) {
        s0 = __builtin_fmaf(s0, a.uk, ch);
        s1 = __builtin_fmaf(s1, a.uk, ch);
      }
      if (a.alpha != 1.0f) {
        s0 = a.alpha * s0;
        s1 = a.alpha * s1;
      }
      const int len = checked_length(a.lengths[src], S);
      const float minus_inf = -99999999.0f;  // Input.cc:56-61
      s0 = s0 + (1.0f - (lane < len ? 1.0f : 0.0f)) * minus_inf;
      s1 = s1 + (1.0f - ((lane + 64) < len ? 1.0f : 0.0f)) * minus_inf;
      const float lowest = -3.402823466e+38f;
      if (lane >= S) s0 = lowest;
      if (lane + 64 >= S) s1 = lowest;
      const float m = wave_max(fmaxf(s0, s1));
      const float e0 = lane < S ? exp_p(s0 - m) : 0.0f;
      const float e1 = (lane + 64) < S ? exp_p(s1 - m) : 0.0f;
      const float sum = wave_sum(e0 + e1);
      const float p0 = e0 / sum, p1 = e1 / sum;
      const float P = wave_sum(p0 + p1);  // P_h
      if (a.attn) {
        float *ap = a.attn + ((size_t)b * a.H + h) * S;
        if (lane < S) ap[lane] = p0;
        if (lane + 64 < S) ap[lane + 64] = p1;
      }
      if (a.align && h == 0 && !a.finished[b]) {  // update_alignment, Model.cc:84-108: the row's block, the source's columns
        const uint32_t t = a.out_len[b];
        if ((int)t < a.Tmax) {
          float *al = a.align + ((size_t)b * a.Tmax + t) * S;
          if (lane < len) al[lane] = p0;
          if (lane + 64 < len) al[lane + 64] = p1;
        }
      }
      // 5. out[d] = fmaf(w_d, uV, pbV[d] * P_h), w_d = key-ascending fmaf chain of p[j] * float(accV[j][d])
      auto dqv = [&](float v) {  // literal: v = float(accS) u + pb per cached value
        if (lit) {
          v = v * a.uv;
          v = v + pbv_d;
        }
        return v;
      };
      float o = 0.0f;
      for (int j = 0; j < S; ++j) {
        const float pj = __shfl(j < 64 ? p0 : p1, j & 63, 64);
        o = __builtin_fmaf(pj, dqv(Vs[(size_t)j * DH + dc]), o);
      }
      if (!lit) o = __builtin_fmaf(o, a.uv, pbv_d * P);
      if (lane < DH) {
        if (a.out_i8) a.out_i8[(size_t)b * D + h * DH + lane] = (int8_t)quantize1(o, a.a_quant_out);
        if (a.out_f32) a.out_f32[(size_t)b * D + h * DH + lane] = o;
      }
    }
    r0 = r1;
  }
}

}  // namespace

size_t dqattn_fanout_lds_bytes(int D, int dh, int S) {
  return 16 * (size_t)(D + 16) + 16 * (size_t)dh * sizeof(float) + (size_t)8 * S * dh;
}

hipError_t launch_dqattn_fanout(const DQAttnArgs &a, hipStream_t st) {
  const int D = a.D;
  if (D % 64 || D <= 0 || D > 512 || a.H <= 0 || D % a.H) return hipErrorInvalidValue;
  const int dh = D / a.H;
  if (a.S < 1 || a.S > 128 || a.ldv % 4) return hipErrorInvalidValue;
  if (a.rows < 1 || a.B < 1 || !a.row_src || a.q_given) return hipErrorInvalidValue;
  const dim3 grid((a.rows + 15) / 16, a.H);
  const size_t lds = dqattn_fanout_lds_bytes(D, dh, a.S);
  const int pf = D <= 256 ? 4 : 8;
  auto run = [&](auto kernel) {
    const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(1024), lds, st, a);
    return hipGetLastError();
  };
  if (pf == 4 && dh == 16) return run(dqattn_fanout_kernel<4, 16>);
  if (pf == 4 && dh == 32) return run(dqattn_fanout_kernel<4, 32>);
  if (pf == 8 && dh == 32) return run(dqattn_fanout_kernel<8, 32>);
  if (pf == 8 && dh == 64) return run(dqattn_fanout_kernel<8, 64>);
  if (pf == 4 && dh == 64) return run(dqattn_fanout_kernel<4, 64>);
  return hipErrorInvalidValue;
}

}  // namespace slimt_hip
