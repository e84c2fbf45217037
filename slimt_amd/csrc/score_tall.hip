// Teacher-forced scoring (slimt_hip_score*): every target position of a batch as one tall pass.
//
// With the targets known, row (b, t) of the decoder depends on tgt[b][t - 1] and, through the SSRU cell, on the rows
// (b, 0 .. t - 1) of ITS OWN sentence by an elementwise scan; everything else is row-wise. So the B x T positions go
// through the decoder weights as R = B T rows of the tall GEMMs the encoder already has (kernels.hip / gemm_tile.hip,
// bit-identical to the step-wise dgemm), and this file adds what a tall pass needs beside them:
//   score_embed_kernel   row (b, t)'s input -- zero embedding at t = 0, else tgt[b][t - 1] at position 0 -- and the
//                        output-layer column of tgt[b][t] (device_common.h, forced_column: once per row)
//   score_scan_kernel    the SSRU scan over t of one sentence: c_t = highway(c_{t-1}, W x_t, f_t), x + relu(c_t), LayerNorm
//   score_attn_kernel    cross-attention of ALL query rows of one (sentence, head) over K / V staged once in LDS
//   score_out_kernel     the output layer over 128-row blocks with the score as its epilogue: logits are never stored
// Each row's float sequence is the step-wise kernels' (decode_kernels.hip: dssru_kernel, dqattn_kernel's hoisted PORTABLE
// order, dgemm's epilogue), so hidden rows and alignment rows are the oracle's so_decode_step bit for bit.
//
// A chunk of rows is a run of whole sentences b0 .. b0 + nb - 1; local row r = (b - b0) T + t. Rows with t >= n_b =
// min(tgt_len[b], T) ("dead" rows) are carried through the GEMMs (they cost nothing worth a branch there) but neither
// scanned, attended, nor stored; the output layer skips 16-row tiles that are dead altogether.
//
// No out-of-line device functions, no dynamic stack: helpers are __forceinline__ or lambdas.
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {

namespace {

__device__ __forceinline__ int score_target_len(const ScoreRows &r, int b) {
  const uint32_t n = r.tgt_len[b];
  return n < (uint32_t)r.T ? (int)n : r.T;
}

// ---- target embedding rows + target columns: one wave per row -------------------------------------------------------
__global__ __launch_bounds__(256) void score_embed_kernel(EmbedArgs e, ScoreRows rows, const uint32_t *sl, int N, float *x,
                                                          int *tcol) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows.nb * rows.T) return;  // (whole wave)
  const int bl = r / rows.T, t = r - bl * rows.T;
  const int b = rows.b0 + bl;
  const int n = score_target_len(rows, b);
  const uint32_t *tg = rows.tgt_ids + (size_t)b * rows.T;
  float *xr = x + (size_t)r * e.D;
  if (t == 0) {  // Transformer.cc:138-144: the start embedding is zero (times sqrt(D), plus position 0)
    for (int d = lane; d < e.D; d += 64) {
      const float z = 0.0f * e.sqrt_d;
      xr[d] = z + e.pos[d];
    }
  } else {  // Transformer.cc:133-160: the previous token at position 0 (Io.cc:275-283: separate roundings)
    const uint32_t tok = embed_row(e, tg[t - 1]);
    for (int d = lane; d < e.D; d += 64) {
      const float v = (float)e.wemb[(size_t)tok * e.D + d] * e.inv_mult;
      const float s = v * e.sqrt_d;
      xr[d] = s + e.pos[d];
    }
  }
  const int col = forced_column(sl, N, t < n ? tg[t] : 0xffffffffu, lane);  // (every lane calls it)
  if (lane == 0) tcol[r] = col;
}

// ---- SSRU scan (Modules.cc:190-235): one wave per sentence, lane l holds columns l + 64 i -----------------------------
// f / wx: the gate pre-activation affine(Wf, bf)(x) and W x of every row (tall GEMMs). Float sequence: dssru_kernel's
// epilogue (sigmoid_p, highway as t1 + t2, TensorOps.cc:674-678) and rows_layer_norm (TensorOps.cc:542-580).
template <int DPL>
__global__ __launch_bounds__(64) void score_scan_kernel(ScoreRows rows, const float *x, const float *f, const float *wx,
                                                        const float *ln_scale, const float *ln_bias, float eps, float *h) {
  constexpr int D = 64 * DPL;
  const int lane = threadIdx.x;
  const int bl = blockIdx.x;
  const int n = score_target_len(rows, rows.b0 + bl);
  if (n == 0) return;
  float sc[DPL], bi[DPL], c[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) {
    sc[i] = ln_scale[lane + 64 * i];
    bi[i] = ln_bias[lane + 64 * i];
    c[i] = 0.0f;  // Transformer.cc:78-85: the cells start at zero
  }
  float xv[DPL], fv[DPL], wv[DPL];
  auto load = [&](int t, float (&xo)[DPL], float (&fo)[DPL], float (&wo)[DPL]) {
    const size_t o = ((size_t)bl * rows.T + t) * D + lane;
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      xo[i] = x[o + 64 * i];
      fo[i] = f[o + 64 * i];
      wo[i] = wx[o + 64 * i];
    }
  };
  load(0, xv, fv, wv);
  for (int t = 0; t < n; ++t) {
    float xn[DPL], fn[DPL], wn[DPL];
    load(t + 1 < n ? t + 1 : t, xn, fn, wn);  // the next row's operands travel under this row's LayerNorm
    float v[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      const float sg = sigmoid_p(fv[i]);
      const float t1 = sg * c[i];
      const float t2 = (1.0f - sg) * wv[i];
      const float cn = t1 + t2;
      c[i] = cn;
      const float y = cn > 0.0f ? cn : 0.0f;
      v[i] = xv[i] + y;  // x + relu(c'), Modules.cc:230
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) s += v[i];
    s = wave_sum(s);
    const float mean = s / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      const float d = v[i] - mean;
      q += d * d;
    }
    q = wave_sum(q);
    const float sigma = __builtin_sqrtf(q / (float)D + eps);
    float *hr = h + ((size_t)bl * rows.T + t) * D + lane;
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      const float tt = (v[i] - mean) / sigma;
      const float m = sc[i] * tt;
      hr[64 * i] = m + bi[i];
    }
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      xv[i] = xn[i];
      fv[i] = fn[i];
      wv[i] = wn[i];
    }
  }
}

// ---- cross-attention of one (sentence, head): K and V in LDS once, a wave per query row -------------------------------
// LDS: K [DH/4][S][4] (the cache's own layout: a straight copy) + V [S][DH], f32 = 8 S DH bytes: 32 KiB at S = 128,
// DH = 32; 64 KiB at DH = 64. Each row in dqattn_kernel's order (the oracle's cross_attention_portable): t_j = fmaf chain
// over d ascending on float(accS); s_j = alpha fmaf(t_j, uK, c_h) + mask, c_h the canonical row sum of q_d pbK[d];
// softmax in the portable order; w_d = fmaf chain over keys ascending; out_d = fmaf(w_d, uV, pbV[d] P_h).
template <int DH>
__global__ __launch_bounds__(256) void score_attn_kernel(ScoreAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bl = blockIdx.x, h = blockIdx.y;
  const int b = a.rows.b0 + bl;
  const int S = a.S, D = a.D, T = a.rows.T;
  const int n = score_target_len(a.rows, b);
  if (n == 0) return;  // (whole workgroup)
  float *Ks = reinterpret_cast<float *>(smem);
  float *Vs = Ks + (size_t)DH * S;
  {
    const float4 *kb = reinterpret_cast<const float4 *>(a.k + ((size_t)b * a.H + h) * (size_t)(DH / 4) * S * 4);
    for (int i = tid; i < (DH / 4) * S; i += 256) reinterpret_cast<float4 *>(Ks)[i] = kb[i];
    for (int i = tid; i < (DH / 4) * S; i += 256) {
      const int j = i / (DH / 4), c4 = i - j * (DH / 4);
      reinterpret_cast<float4 *>(Vs)[i] =
          *reinterpret_cast<const float4 *>(a.v + ((size_t)b * S + j) * a.ldv + h * DH + c4 * 4);
    }
  }
  __syncthreads();
  const int len = checked_length(a.lengths[b], S);
  const int j0 = lane < S ? lane : S - 1;
  const int j1 = (lane + 64) < S ? (lane + 64) : S - 1;
  const int dc = lane < DH ? lane : DH - 1;
  const float pbk_d = a.pbk[h * DH + dc], pbv_d = a.pbv[h * DH + dc];
  for (int t = wave; t < n; t += 4) {
    const size_t r = (size_t)bl * T + t;
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
    if (a.align && h == 0) {  // update_alignment, Model.cc:84-108: head 0 of the last layer
      float *al = a.align + ((size_t)b * T + t) * S;
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

// ---- output layer with the score as its epilogue ---------------------------------------------------------------------
// One workgroup = 128 rows (quantised once, int8, in LDS) x ALL column tiles; wave w takes the tiles w, w + 4, ... for
// all eight 16-row tiles, so the packed weights cross the CU's L2 path once per 128 rows. Per row and lane (column lr
// of each tile) the epilogue carries the running maximum, the sum of exp(l - max) (scores.h, lse_push) and the logit at
// the row's target column; afterwards the 16 lanes of a row merge by the xor butterfly (masks 1, 2, 4, 8), then the four
// waves in ascending order. Which columns a lane / wave sees and every merge's order follow from the column index alone,
// never from where the row sits: a sentence scores the same bits alone and in any batch.
// logit = float(acc + 127 colsum) u + pb (Intgemm.inl.cc:146-153; dgemm_kernel's epilogue).
template <int KS>
__global__ __launch_bounds__(256) void score_out_kernel(ScoreOutArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int K = 64 * KS, LDA = K + 16, RT = 8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int T = a.rows.T, R = a.rows.nb * T;
  const int m0 = blockIdx.x * 128;
  char *A_lds = smem;
  float *red = reinterpret_cast<float *>(smem + 128 * LDA);  // [4 waves][128 rows][m, s, y]
  int *live_lds = reinterpret_cast<int *>(red + 4 * 128 * 3);  // [128] then [1] tile mask
  // rows: live (t < n_b)? target column; the block's live 16-row tiles
  if (tid < 128) {
    const int r = m0 + tid;
    int lv = 0;
    if (r < R) {
      const int bl = r / T, t = r - bl * T;
      lv = t < score_target_len(a.rows, a.rows.b0 + bl);
    }
    live_lds[tid] = lv;
  }
  for (int u = tid; u < 128 * (K / 16); u += 256) {
    const int r = u / (K / 16), c = u - r * (K / 16);
    v4i v = {0, 0, 0, 0};
    if (m0 + r < R) v = *reinterpret_cast<const v4i *>(a.a_i8 + (size_t)(m0 + r) * K + c * 16);
    *reinterpret_cast<v4i *>(A_lds + r * LDA + c * 16) = v;
  }
  __syncthreads();
  unsigned tiles = 0;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    int any = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) any |= live_lds[rt * 16 + i];
    tiles |= any ? 1u << rt : 0u;
  }
  tiles = __builtin_amdgcn_readfirstlane(tiles);
  if (tiles == 0) return;  // (whole workgroup: no barrier behind this point is skipped by part of it -- all leave)
  float mx[RT][4], sm[RT][4], ty[RT][4];
  int tc[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[rt][r] = -3.402823466e+38f;
      sm[rt][r] = 0.0f;
      ty[rt][r] = -__builtin_inff();
      const int row = m0 + rt * 16 + lg * 4 + r;
      tc[rt][r] = row < R ? a.tcol[row] : -1;
    }
  const v4i *Wp = reinterpret_cast<const v4i *>(a.w.Wp);
  const int n_tiles = a.w.n_tiles, N = a.w.N;
  const float u = a.w.u;
  v4i bf[KS], bn[KS];
  auto load_b = [&](int ntile, v4i (&b)[KS]) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = ntile < n_tiles ? Wp[((size_t)ntile * KS + ks) * 64 + lane] : v4i{0, 0, 0, 0};
  };
  load_b(wave, bf);
  for (int ntile = wave; ntile < n_tiles; ntile += 4) {
    load_b(ntile + 4, bn);  // the next tile's fragments travel under this tile's MFMAs and epilogue
    const int col = ntile * 16 + lr;
    const bool in = col < N;
    const int cs = a.w.colsum[col];  // (colsum / pb are allocated to whole tiles)
    const float pb = a.w.pb[col];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (!((tiles >> rt) & 1u)) continue;  // (uniform) a tile of dead rows
      v4i acc = {0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const v4i af = *reinterpret_cast<const v4i *>(A_lds + (rt * 16 + lr) * LDA + ks * 64 + lg * 16);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = (float)(acc[r] + 127 * cs) * u;
        v = v + pb;
        const bool better = in && v > mx[rt][r];
        lse_push(v, in, better, mx[rt][r], sm[rt][r]);
        mx[rt][r] = better ? v : mx[rt][r];
        ty[rt][r] = (in && col == tc[rt][r]) ? v : ty[rt][r];
      }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf[ks] = bn[ks];
  }
  // the 16 lanes of a row (masks 1, 2, 4, 8), then the waves in ascending order
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = mx[rt][r], s = sm[rt][r], y = ty[rt][r];
#pragma unroll
      for (int k = 1; k < 16; k <<= 1) {
        const float om = __shfl_xor(m, k, 64), os = __shfl_xor(s, k, 64);
        lse_merge(m, s, om, os);
        y = fmaxf(y, __shfl_xor(y, k, 64));
      }
      if (lr == 0) {
        float *o = red + ((size_t)wave * 128 + rt * 16 + lg * 4 + r) * 3;
        o[0] = m;
        o[1] = s;
        o[2] = y;
      }
    }
  __syncthreads();
  if (tid < 128 && live_lds[tid]) {
    float m = red[tid * 3], s = red[tid * 3 + 1], y = red[tid * 3 + 2];
    for (int w = 1; w < 4; ++w) {
      const float *o = red + ((size_t)w * 128 + tid) * 3;
      lse_merge(m, s, o[0], o[1]);
      y = fmaxf(y, o[2]);
    }
    const int r = m0 + tid;
    const int bl = r / T, t = r - bl * T;
    // none: no column beat the start value (scores.h); a NaN logit has made s NaN
    a.scores[(size_t)(a.rows.b0 + bl) * T + t] = forced_score(s, y - m, !(m > -3.402823466e+38f));
  }
}

}  // namespace

hipError_t launch_score_embed(const EmbedArgs &e, const ScoreRows &rows, const uint32_t *sl, int N, float *x, int *tcol,
                              hipStream_t st) {
  const int R = rows.nb * rows.T;
  if (R <= 0 || e.D % 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_embed_kernel, dim3((R + 3) / 4), dim3(256), 0, st, e, rows, sl, N, x, tcol);
  return hipGetLastError();
}

hipError_t launch_score_scan(const ScoreRows &rows, int D, const float *x, const float *f, const float *wx,
                             const float *ln_scale, const float *ln_bias, float eps, float *h, hipStream_t st) {
  if (rows.nb <= 0) return hipErrorInvalidValue;
#define SLIMT_SCAN_CASE(DPL_)                                                                                          \
  if (D == 64 * DPL_) {                                                                                                \
    hipLaunchKernelGGL(score_scan_kernel<DPL_>, dim3(rows.nb), dim3(64), 0, st, rows, x, f, wx, ln_scale, ln_bias, eps, h); \
    return hipGetLastError();                                                                                          \
  }
  SLIMT_SCAN_CASE(1) SLIMT_SCAN_CASE(2) SLIMT_SCAN_CASE(4) SLIMT_SCAN_CASE(8)
#undef SLIMT_SCAN_CASE
  return hipErrorInvalidValue;
}

bool score_supported(int D, int H) {
  if (!(D == 64 || D == 128 || D == 256 || D == 512) || H <= 0 || D % H) return false;
  const int dh = D / H;
  return dh == 16 || dh == 32 || dh == 64;
}

size_t score_attention_lds_bytes(int S, int dh) { return (size_t)8 * S * dh; }

hipError_t launch_score_attention(const ScoreAttnArgs &a, hipStream_t st) {
  if (a.rows.nb <= 0 || a.H <= 0 || a.D % a.H || a.S < 1 || a.S > 128 || a.ldv % 4) return hipErrorInvalidValue;
  const int dh = a.D / a.H;
  const size_t lds = score_attention_lds_bytes(a.S, dh);
  const dim3 grid(a.rows.nb, a.H);
  auto run = [&](auto kernel) {
    const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a);
    return hipGetLastError();
  };
  if (dh == 16) return run(score_attn_kernel<16>);
  if (dh == 32) return run(score_attn_kernel<32>);
  if (dh == 64) return run(score_attn_kernel<64>);
  return hipErrorInvalidValue;
}

hipError_t launch_score_output(const ScoreOutArgs &a, hipStream_t st) {
  const int R = a.rows.nb * a.rows.T;
  if (R <= 0 || a.w.K % 64 || a.w.N <= 0) return hipErrorInvalidValue;
  const int KS = a.w.K / 64;
  const size_t lds = (size_t)128 * (a.w.K + 16) + 4 * 128 * 3 * sizeof(float) + 132 * sizeof(int);
  const dim3 grid((R + 127) / 128);
  auto run = [&](auto kernel) {
    const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a);
    return hipGetLastError();
  };
  if (KS == 1) return run(score_out_kernel<1>);
  if (KS == 2) return run(score_out_kernel<2>);
  if (KS == 4) return run(score_out_kernel<4>);
  if (KS == 8) return run(score_out_kernel<8>);
  return hipErrorInvalidValue;
}

}  // namespace slimt_hip
