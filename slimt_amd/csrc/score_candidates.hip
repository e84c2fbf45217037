// Candidate scoring (slimt_hip_score_candidates*, slimt_hip_candidates_rank*): N target rows over B <= N encoded sources.
//
// A candidate call is a score call (score_tall.hip) whose row c attends over the K / V of source cand_src[c] instead of
// source c. Everything of the tall pass but the cross-attention is row-wise or indexes the targets alone, and runs
// unchanged with "sentence" read as "candidate"; this file adds the attention that knows the source, and the ranking:
//   score_cand_attn_kernel   cross-attention of a RUN of kScoreCandidateRun consecutive candidates for one head: K and V
//                            of a source are staged in LDS when the next live candidate's source is not the staged one
//   cand_totals_kernel       totals[c] = the f32 sum of a candidate's scores in ascending t, and the candidate's entry in
//                            the per-source maximum (an atomic maximum over a total order that encodes the ranking rule)
//   cand_best_kernel         best[b] from that maximum
// Each row's float sequence is score_attn_kernel's line for line, so a candidate's hidden rows and alignment rows are the
// bits slimt_hip_score writes for that row of the duplicated batch src_ids[cand_src].
//
// Barriers: every branch around a __syncthreads() below depends on values that all 256 threads load from the same
// read-only addresses (tgt_len[c], cand_src[c]) and pass through readfirstlane: the decision is the workgroup's. A dead
// candidate (n_c = 0) is stepped over before its source is looked at: it neither stages nor changes what is staged. No
// thread leaves before the run's last candidate.
//
// No out-of-line device functions, no dynamic stack: helpers are __forceinline__ or lambdas.
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {

namespace {

__device__ __forceinline__ int cand_target_len(const ScoreRows &r, int c) {
  const uint32_t n = r.tgt_len[c];
  return n < (uint32_t)r.T ? (int)n : r.T;
}

// LDS: as score_attn_kernel, K [DH/4][S][4] + V [S][DH] of ONE source, 8 S DH bytes
template <int DH>
__global__ __launch_bounds__(256) void score_cand_attn_kernel(ScoreCandAttnArgs ca) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ScoreAttnArgs &a = ca.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.y;
  const int S = a.S, D = a.D, T = a.rows.T;
  float *Ks = reinterpret_cast<float *>(smem);
  float *Vs = Ks + (size_t)DH * S;
  const int j0 = lane < S ? lane : S - 1;
  const int j1 = (lane + 64) < S ? (lane + 64) : S - 1;
  const int dc = lane < DH ? lane : DH - 1;
  const float pbk_d = a.pbk[h * DH + dc], pbv_d = a.pbv[h * DH + dc];
  const int cl0 = blockIdx.x * kScoreCandidateRun;
  const int cl1 = cl0 + kScoreCandidateRun < a.rows.nb ? cl0 + kScoreCandidateRun : a.rows.nb;
  int staged = -1;  // the source whose K / V the LDS holds (workgroup-uniform)
  int len = 0;
  for (int cl = cl0; cl < cl1; ++cl) {
    const int c = a.rows.b0 + cl;
    const int n = __builtin_amdgcn_readfirstlane(cand_target_len(a.rows, c));
    if (n == 0) continue;  // (whole workgroup) a dead candidate: nothing staged, nothing written
    const uint32_t named = ca.cand_src[c];
    const int b = __builtin_amdgcn_readfirstlane(named < (uint32_t)ca.B ? (int)named : ca.B - 1);
    if (b != staged) {  // (whole workgroup)
      __syncthreads();  // the rows of the candidates before this one have read the old K / V
      const float4 *kb = reinterpret_cast<const float4 *>(a.k + ((size_t)b * a.H + h) * (size_t)(DH / 4) * S * 4);
      for (int i = tid; i < (DH / 4) * S; i += 256) reinterpret_cast<float4 *>(Ks)[i] = kb[i];
      for (int i = tid; i < (DH / 4) * S; i += 256) {
        const int j = i / (DH / 4), c4 = i - j * (DH / 4);
        reinterpret_cast<float4 *>(Vs)[i] =
            *reinterpret_cast<const float4 *>(a.v + ((size_t)b * S + j) * a.ldv + h * DH + c4 * 4);
      }
      __syncthreads();
      staged = b;
      len = checked_length(a.lengths[b], S);
    }
    for (int t = wave; t < n; t += 4) {
      const size_t r = (size_t)cl * T + t;
      const float *qrow = a.q + r * D + h * DH;
      const float ch = wave_sum(lane < DH ? qrow[dc] * pbk_d : 0.0f);
      float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
      for (int i = 0; i < DH / 4; ++i) {
        const float4 q4 = *reinterpret_cast<const float4 *>(qrow + 4 * i);
        const float4 k4 = *reinterpret_cast<const float4 *>(Ks + ((size_t)i * S + j0) * 4);
        s0 = __builtin_fmaf(q4.x, k4.x, s0);
        s0 = __builtin_fmaf(q4.y, k4.y, s0);
        s0 = __builtin_fmaf(q4.z, k4.z, s0);
        s0 = __builtin_fmaf(q4.w, k4.w, s0);
      }
      if (S > 64) {
#pragma unroll
        for (int i = 0; i < DH / 4; ++i) {
          const float4 q4 = *reinterpret_cast<const float4 *>(qrow + 4 * i);
          const float4 k4 = *reinterpret_cast<const float4 *>(Ks + ((size_t)i * S + j1) * 4);
          s1 = __builtin_fmaf(q4.x, k4.x, s1);
          s1 = __builtin_fmaf(q4.y, k4.y, s1);
          s1 = __builtin_fmaf(q4.z, k4.z, s1);
          s1 = __builtin_fmaf(q4.w, k4.w, s1);
        }
      }
      s0 = __builtin_fmaf(s0, a.uk, ch);
      s1 = __builtin_fmaf(s1, a.uk, ch);
      if (a.alpha != 1.0f) {
        s0 = a.alpha * s0;
        s1 = a.alpha * s1;
      }
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
      if (a.align && h == 0) {  // the candidate's row, the source's columns
        float *al = a.align + ((size_t)c * T + t) * S;
        if (lane < len) al[lane] = p0;
        if (lane + 64 < len) al[lane + 64] = p1;
      }
      float o = 0.0f;
      for (int j = 0; j < S; ++j) {
        const float pj = __shfl(j < 64 ? p0 : p1, j & 63, 64);
        o = __builtin_fmaf(pj, Vs[(size_t)j * DH + dc], o);
      }
      o = __builtin_fmaf(o, a.uv, pbv_d * P);
      if (lane < DH) a.out_i8[r * D + h * DH + lane] = (int8_t)quantize1(o, a.a_quant_out);
    }
  }
}

// ---- ranking -----------------------------------------------------------------------------------------------------------
// The order of the rule "the lowest c whose key is >= every other key, keys compared as floats" as ONE unsigned 64-bit
// order: the high word is the key's bits mapped monotonically (negative: all bits flipped; else the sign bit set; -0 is
// made +0 first, so equal floats map to equal words), the low word is ~c (of equal keys the lower c is the larger
// entry). -inf maps to 0x007FFFFF: every entry is above 0, the value of "no candidate". The maximum of a set does not
// depend on the order its members arrive in.
__device__ __forceinline__ unsigned long long cand_entry(float key, uint32_t c) {
  uint32_t u = __float_as_uint(key);
  if ((u << 1) == 0) u = 0;  // -0 -> +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (uint32_t)~c;
}

__global__ __launch_bounds__(256) void cand_totals_kernel(CandRankArgs a) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.N) return;
  const uint32_t tl = a.tgt_len[c];
  const uint32_t n = tl < a.T ? tl : a.T;
  const float *row = a.scores + c * a.T;
  float s = 0.0f;
  for (uint32_t t = 0; t < n; ++t) s = s + row[t];
  a.totals[c] = s;
  if (n == 0) return;  // never competes
  const float key = a.mode == 1 ? s / (float)n : s;
  if (key != key) return;  // NaN never competes
  const uint32_t named = a.cand_src[c];
  const uint32_t b = named < a.B ? named : a.B - 1;
  atomicMax(a.entries + b, cand_entry(key, (uint32_t)c));
}

__global__ __launch_bounds__(256) void cand_best_kernel(CandRankArgs a) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const unsigned long long e = a.entries[b];
  a.best[b] = e ? ~(uint32_t)e : 0xffffffffu;
}

}  // namespace

hipError_t launch_score_candidates_attention(const ScoreCandAttnArgs &ca, hipStream_t st) {
  const ScoreAttnArgs &a = ca.a;
  if (a.rows.nb <= 0 || a.H <= 0 || a.D % a.H || a.S < 1 || a.S > 128 || a.ldv % 4 || ca.B < 1 || !ca.cand_src)
    return hipErrorInvalidValue;
  const int dh = a.D / a.H;
  const size_t lds = score_attention_lds_bytes(a.S, dh);
  const dim3 grid((a.rows.nb + kScoreCandidateRun - 1) / kScoreCandidateRun, a.H);
  auto run = [&](auto kernel) {
    const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, ca);
    return hipGetLastError();
  };
  if (dh == 16) return run(score_cand_attn_kernel<16>);
  if (dh == 32) return run(score_cand_attn_kernel<32>);
  if (dh == 64) return run(score_cand_attn_kernel<64>);
  return hipErrorInvalidValue;
}

hipError_t launch_candidates_rank(const CandRankArgs &a, hipStream_t st) {
  if (a.B < 1 || a.T < 1 || (a.mode != 0 && a.mode != 1) || !a.entries || !a.best) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.entries, 0, (size_t)a.B * 8, st);
  if (e != hipSuccess) return e;
  if (a.N) {
    hipLaunchKernelGGL(cand_totals_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(cand_best_kernel, dim3((a.B + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace slimt_hip
