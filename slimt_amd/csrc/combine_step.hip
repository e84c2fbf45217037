// Combined decoding (slimt_hip_ctx_set_fanout_combine, slimt_hip_combine_step): one step's selection over the combined
// log-probabilities of a group of m <= 4 fan-out rows (combine.h), and the group's records.
//
// combine_step_kernel<M, RESIDENT, VEC>: one 512-thread workgroup (eight waves) per group, M = m a template constant so
// that every register array is indexed by unrolled constants.
//   ownership  thread t owns the 4-column groups t and t + 512 (t + 1024, ... when streaming) of EVERY member row: one
//              128-bit load per group and row where N is a multiple of 4 and the rows are 16-byte aligned (VEC), four
//              guarded scalar loads otherwise. RESIDENT (N <= kCombineResidentN = 4096, the shortlist case): the M rows
//              are read from memory once and stay in registers, 8 columns a row, 32 logit registers at M = 4; columns
//              past the row hold -inf (no maximum, no weight, never visited). Streaming (N > 4096): the same thread walks
//              the same groups in the same order in each sweep and re-reads them from L2. The bits are the same.
//   sweep A    per member row: the NaN bit and the maximum by wave shuffles, one LDS word per wave and row, a barrier,
//              every thread folds the eight words into M_j; then the uint64 sum of beam.h's integer weights the same way
//              (exact: any order gives the same Q_j), a barrier, and L_j = bm_normaliser(Q_j).
//   sweep B    from the same registers a thread forms lp_j[c] for its columns, s[c] by combine.h's multiply and fmaf chain,
//              the candidate tests, and keeps its first column in cb_before's order as a tuple (candidate, s, l_0, column,
//              lp_0 .. lp_{M-1}). Six shuffle rounds merge the wave's tuples with cb_before -- the full tie rule, a strict
//              order over distinct columns, so both partners of a round keep the same winner -- lane 0 stores the wave's,
//              a barrier, thread 0 merges the eight.
//   records    thread 0 writes the op-level outputs; on an engine step (dx set) it also records the group's token and
//              each row's own score in the rows' outputs (decode_begin_step's record: Model.cc:127-137) and, behind one
//              more barrier, all threads write the next step's input rows (embed1's expression, position 0).
// Every barrier is reached by all 512 threads: the branches around them depend on kernel arguments alone. No out-of-line
// device functions, no dynamic stack, no scratch.
#include <hip/hip_runtime.h>

#include "combine.h"
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {
namespace {

constexpr int kCbThreads = 512;
constexpr int kCbWaves = kCbThreads / 64;
constexpr int kCbQuads = kCombineResidentN / (4 * kCbThreads);  // 4-column groups a thread holds of a resident row
static_assert(kCbQuads * 4 * kCbThreads == kCombineResidentN && kCbQuads == 2, "the register-resident bound is threads x 8 columns");

template <int M>
struct CbShared {
  float pm[M][kCbWaves];                // sweep A: the waves' maxima ...
  uint32_t pnan[M][kCbWaves];           // ... NaN bits ...
  unsigned long long pq[M][kCbWaves];   // ... and weight sums, per member row
  uint32_t b_cand[kCbWaves], b_col[kCbWaves];  // sweep B: the waves' best tuples
  float b_s[kCbWaves], b_l0[kCbWaves], b_lp[M][kCbWaves];
  uint32_t tok;                         // the group's token, for the embedding
};

// a thread's best column so far in cb_before's order
template <int M>
struct CbBest {
  bool cand;
  float s, l0;
  uint32_t col;
  float lp[M];
};

// the four columns from c0 (a multiple of 4) of one row; columns past the row read -inf
template <bool VEC>
__device__ __forceinline__ void cb_load4(const float *__restrict__ row, int N, int c0, float (&x)[4]) {
  const float ninf = -__builtin_inff();
  if constexpr (VEC) {
    float4 q = make_float4(ninf, ninf, ninf, ninf);
    if (c0 < N) q = *reinterpret_cast<const float4 *>(row + c0);
    x[0] = q.x;
    x[1] = q.y;
    x[2] = q.z;
    x[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = c0 + e < N ? row[c0 + e] : ninf;
  }
}

// f(c0, x[M][4]) over the thread's 4-column groups, ascending: from the registers v, or from memory
template <int M, bool RESIDENT, bool VEC, class F>
__device__ __forceinline__ void cb_each(const float (&v)[M][4 * kCbQuads], const float *__restrict__ rows, int N, int tid, F &&f) {
  if constexpr (RESIDENT) {
#pragma unroll
    for (int q = 0; q < kCbQuads; ++q) {
      float x[M][4];
#pragma unroll
      for (int j = 0; j < M; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[j][e] = v[j][4 * q + e];
      f(4 * (q * kCbThreads + tid), x);
    }
  } else {
    for (int c0 = 4 * tid; c0 < N; c0 += 4 * kCbThreads) {  // (N < 2^20: c0 stays an int)
      float x[M][4];
#pragma unroll
      for (int j = 0; j < M; ++j) cb_load4<VEC>(rows + (size_t)j * N, N, c0, x[j]);
      f(c0, x);
    }
  }
}

template <int M>
__device__ __forceinline__ bool cb_takes(const CbBest<M> &b, bool cand, float s, float l0, uint32_t col) {
  return cb_before(cand, s, l0, col, b.cand, b.s, b.l0, b.col);
}

template <int M, bool RESIDENT, bool VEC>
__global__ __launch_bounds__(kCbThreads) void combine_step_kernel(CombineStepArgs a) {
  __shared__ CbShared<M> sh;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const size_t r0 = (size_t)g * M;
  const float *__restrict__ rows = a.logits + r0 * N;
  const float ninf = -__builtin_inff(), qnan = __builtin_nanf("");

  // the one global read of a resident group
  float v[M][4 * kCbQuads];
  if constexpr (RESIDENT) {
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int q = 0; q < kCbQuads; ++q) {
        float x[4];
        cb_load4<VEC>(rows + (size_t)j * N, N, 4 * (q * kCbThreads + tid), x);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][4 * q + e] = x[e];
      }
  }

  // sweep A, first half: NaN bits and maxima
  float mx[M];
  uint32_t nan[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    mx[j] = ninf;
    nan[j] = 0u;
  }
  cb_each<M, RESIDENT, VEC>(v, rows, N, tid, [&](int, const float (&x)[M][4]) {
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        nan[j] |= x[j][e] != x[j][e] ? 1u : 0u;
        mx[j] = fmaxf(mx[j], x[j][e]);
      }
  });
#pragma unroll
  for (int j = 0; j < M; ++j) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      mx[j] = fmaxf(mx[j], __shfl_xor(mx[j], o, 64));
      nan[j] |= (uint32_t)__shfl_xor((int)nan[j], o, 64);
    }
    if (lane == 0) {
      sh.pm[j][wave] = mx[j];
      sh.pnan[j][wave] = nan[j];
    }
  }
  __syncthreads();
  float Mj[M];
  bool usable[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    float m = sh.pm[j][0];
    uint32_t n = sh.pnan[j][0];
#pragma unroll
    for (int w = 1; w < kCbWaves; ++w) {
      m = fmaxf(m, sh.pm[j][w]);
      n |= sh.pnan[j][w];
    }
    Mj[j] = bm_max(m);
    usable[j] = bm_usable(n != 0u, Mj[j]);
  }

  // sweep A, second half: the integer weight sums of the usable rows
  unsigned long long q[M];
#pragma unroll
  for (int j = 0; j < M; ++j) q[j] = 0ull;
  cb_each<M, RESIDENT, VEC>(v, rows, N, tid, [&](int, const float (&x)[M][4]) {
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (usable[j]) {  // (uniform over the workgroup)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[j] += bm_weight(x[j][e], Mj[j]);
      }
  });
#pragma unroll
  for (int j = 0; j < M; ++j) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)q[j], o, 64);
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(q[j] >> 32), o, 64);
      q[j] += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) sh.pq[j][wave] = q[j];
  }
  __syncthreads();
  float Lj[M];
  bool counted[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    unsigned long long Q = 0ull;
#pragma unroll
    for (int w = 0; w < kCbWaves; ++w) Q += sh.pq[j][w];
    Lj[j] = usable[j] ? bm_normaliser(Q) : 0.0f;
    counted[j] = cb_counted(j, a.w[j], usable[j]);
  }

  // sweep B: the thread's first column in the contract's order
  CbBest<M> b;
  b.cand = false;
  b.s = qnan;
  b.l0 = ninf;
  b.col = kCombineNone;
#pragma unroll
  for (int j = 0; j < M; ++j) b.lp[j] = qnan;
  const float gap = a.gap;
  cb_each<M, RESIDENT, VEC>(v, rows, N, tid, [&](int c0, const float (&x)[M][4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t c = (uint32_t)(c0 + e);
      float lp[M];
#pragma unroll
      for (int j = 0; j < M; ++j) lp[j] = usable[j] ? bm_logprob(x[j][e], Mj[j], Lj[j]) : qnan;
      float s = qnan;
      bool cand = false;
      if (usable[0]) {
        s = cb_first(a.w[0], lp[0]);
#pragma unroll
        for (int j = 1; j < M; ++j)
          if (counted[j]) s = cb_add(s, a.w[j], x[j][e], lp[j]);
        cand = cb_plausible(x[0][e], Mj[0], gap) && s == s;
      }
      // an unusable primary: column 0 alone, and no order among its logits
      const bool visit = usable[0] ? c < (uint32_t)N : c == 0u;
      const float l0 = usable[0] ? x[0][e] : ninf;
      if (visit && cb_takes<M>(b, cand, s, l0, c)) {
        b.cand = cand;
        b.s = s;
        b.l0 = l0;
        b.col = c;
#pragma unroll
        for (int j = 0; j < M; ++j) b.lp[j] = lp[j];
      }
    }
  });
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    CbBest<M> t;
    t.cand = __shfl_xor((int)b.cand, o, 64) != 0;
    t.s = __shfl_xor(b.s, o, 64);
    t.l0 = __shfl_xor(b.l0, o, 64);
    t.col = (uint32_t)__shfl_xor((int)b.col, o, 64);
#pragma unroll
    for (int j = 0; j < M; ++j) t.lp[j] = __shfl_xor(b.lp[j], o, 64);
    if (cb_takes<M>(b, t.cand, t.s, t.l0, t.col)) b = t;
  }
  if (lane == 0) {
    sh.b_cand[wave] = b.cand ? 1u : 0u;
    sh.b_s[wave] = b.s;
    sh.b_l0[wave] = b.l0;
    sh.b_col[wave] = b.col;
#pragma unroll
    for (int j = 0; j < M; ++j) sh.b_lp[j][wave] = b.lp[j];
  }
  __syncthreads();

  if (tid == 0) {
    for (int w = 1; w < kCbWaves; ++w) {
      if (cb_takes<M>(b, sh.b_cand[w] != 0u, sh.b_s[w], sh.b_l0[w], sh.b_col[w])) {
        b.cand = sh.b_cand[w] != 0u;
        b.s = sh.b_s[w];
        b.l0 = sh.b_l0[w];
        b.col = sh.b_col[w];
#pragma unroll
        for (int j = 0; j < M; ++j) b.lp[j] = sh.b_lp[j][w];
      }
    }
    // (column 0 is always visited, so a column was taken)
    const uint32_t tok = a.ids ? a.ids[b.col] : b.col;
    if (a.column) a.column[g] = b.col;
    if (a.token) a.token[g] = tok;
    if (a.combined) a.combined[g] = b.cand ? b.s : qnan;
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (a.member_scores) a.member_scores[r0 + j] = b.lp[j];
    if (a.dx) {  // the rows' records: the group's token, each row's own score
      const DecodeState &s = a.st;
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const size_t r = r0 + j;
        s.prev[r] = tok;
        if (!s.finished[r]) {
          const uint32_t n = s.out_len[r];
          if ((int)n < s.Tmax) {
            if (a.scores) a.scores[r * s.Tmax + n] = b.lp[j];
            s.out_ids[r * s.Tmax + n] = tok;
          }
          s.out_len[r] = n + 1;
          if (tok == s.eos) {
            s.finished[r] = 1;
            atomicAdd(s.n_finished, 1);
          }
        }
      }
      sh.tok = tok;
    }
  }
  if (!a.dx) return;  // (the whole grid) the op-level call ends here
  __syncthreads();
  const int D = a.emb.D;
  const size_t erow = (size_t)embed_row(a.emb, sh.tok) * D;
  for (int u = tid; u < M * D; u += kCbThreads) {
    const int d = u % D;
    const float e = (float)a.emb.wemb[erow + d] * a.emb.inv_mult;
    const float x = e * a.emb.sqrt_d;
    a.dx[r0 * D + u] = x + a.emb.pos[d];
  }
}

template <int M>
hipError_t cb_launch(const CombineStepArgs &a, hipStream_t st) {
  // 128-bit loads: every row starts 16-byte aligned
  const bool vec = (a.N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15u) == 0;
  const bool resident = a.N <= kCombineResidentN;
  auto kernel = resident ? (vec ? combine_step_kernel<M, true, true> : combine_step_kernel<M, true, false>)
                         : (vec ? combine_step_kernel<M, false, true> : combine_step_kernel<M, false, false>);
  hipLaunchKernelGGL(kernel, dim3(a.G), dim3(kCbThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_combine_step(const CombineStepArgs &a, hipStream_t st) {
  if (!a.logits || a.G < 1 || a.N < 1 || (uint32_t)a.N >= kBeamMaxN || !cb_valid(a.m, a.w, a.gap)) return hipErrorInvalidValue;
  if (a.dx) {
    const DecodeState &s = a.st;
    if (!s.prev || !s.out_ids || !s.out_len || !s.finished || !s.n_finished || s.Tmax < 1 || !a.emb.wemb || !a.emb.pos || a.emb.D < 1 ||
        a.emb.V < 1)
      return hipErrorInvalidValue;
  } else if (a.scores) {
    return hipErrorInvalidValue;
  }
  switch (a.m) {
    case 1: return cb_launch<1>(a, st);
    case 2: return cb_launch<2>(a, st);
    case 3: return cb_launch<3>(a, st);
    default: return cb_launch<4>(a, st);
  }
}

}  // namespace slimt_hip
