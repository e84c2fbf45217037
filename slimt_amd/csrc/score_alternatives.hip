// Alternatives of teacher-forced scoring (slimt_hip_ctx_set_score_alternatives): the armed twin of score_out_kernel.
//
// The same pass as score_tall.hip's output layer -- 128 rows (int8, LDS) x ALL column tiles on the 16x16x64 int8 MFMA,
// wave w on the tiles w, w + 4, ..., the running (m, s) per row and lane pushed and merged in the same order, so the
// scores have the unarmed kernel's bits -- which additionally keeps, per row,
//   the k best (logit, column) pairs   order: logit descending as floats (+0 == -0), ties to the lower column; NaN logits
//                                      are no candidates
//   the rank of the target's column    the number of valid columns ordered strictly before it
//
// The target's logit first. Row r's target column c is known (tcol), so before the sweep one thread per row forms
// y_r = logit(r, c) as a K-long int8 dot product from the packed weights: the int32 sum is exact in any order and the float
// epilogue is the sweep's own expression, so y_r has the bits the sweep forms at that column. With y_r in hand the rank is
// a count carried through the ONE sweep (v > y, or v == y at a lower column): an exact integer whose sum over lanes and
// waves has no order. A second sweep would pay the whole GEMM again for the same integer.
//
// The lists. 32 rows x k pairs per lane do not fit in registers beside (m, s, y, column, count), so each ROW owns a
// sorted list of 8 keys in LDS (128 x 8 x 8 B = 8 KiB), shared by the four waves, and a threshold word: the value part of
// its k-th key. A key is 64 bits, (ordered(logit) << 32) | ~column, so that "better" is one unsigned comparison; 0 is below
// every real key (an empty slot). The fast path reads the row's threshold (one 16-byte LDS read per 16-row tile: four rows,
// the same address in all 16 lanes of a row group) and compares; a column at or above it enters the slow path. There the
// lane inserts with 64-bit LDS atomic maxima, no lock and no turn-taking: from the first slot its key beats it walks down
// the list, leaving max(slot, carried) in each slot and carrying min(slot, carried) on. Every slot only ever rises, so a
// slot seen above the key stays above it (the walk may start behind it), and slot i ends as the largest key that ever
// passed it, whatever the interleaving of lanes and waves: the list ends as the k largest keys, sorted -- (value, column)
// is a total order, so there is one such list. One list per row instead of one per (wave, row) also makes the threshold
// rise with all N columns, not a quarter of them: about k (1 + ln(N / k)) insertions per row, 58 at N = 4096, k = 8.
//
// No out-of-line device functions, no dynamic stack: helpers are __forceinline__ or lambdas.
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {

namespace {

constexpr int kAltMax = 8;  // SLIMT_HIP_MAX_ALTERNATIVES

__device__ __forceinline__ int alt_target_len(const ScoreRows &r, int b) {
  const uint32_t n = r.tgt_len[b];
  return n < (uint32_t)r.T ? (int)n : r.T;
}

// a float's order as an unsigned word: -inf < ... < -0 == +0 < ... < +inf (not for NaN); never 0
__device__ __forceinline__ uint32_t alt_ordered(float v) {
  const uint32_t b = __float_as_uint(v + 0.0f);  // (-0 + 0 = +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float alt_value(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

template <int KS>
__global__ __launch_bounds__(256) void score_alt_kernel(ScoreOutArgs a, ScoreAltArgs alt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int K = 64 * KS, LDA = K + 16, RT = 8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int T = a.rows.T, R = a.rows.nb * T;
  const int m0 = blockIdx.x * 128;
  const int k = alt.k;
  char *A_lds = smem;
  float *red = reinterpret_cast<float *>(smem + 128 * LDA);     // [4 waves][128 rows][m, s]
  int *live_lds = reinterpret_cast<int *>(red + 4 * 128 * 2);   // [128]
  float *y_lds = reinterpret_cast<float *>(live_lds + 128);     // [128] the target's logit (-inf: none)
  unsigned *cnt_lds = reinterpret_cast<unsigned *>(y_lds + 128);  // [4 waves][128 rows]
  uint32_t *thr = reinterpret_cast<uint32_t *>(cnt_lds + 4 * 128);  // [128 rows]
  unsigned long long *lists = reinterpret_cast<unsigned long long *>(thr + 128);  // [128 rows][8]
  if (tid < 128) {
    const int r = m0 + tid;
    int lv = 0;
    if (r < R) {
      const int bl = r / T, t = r - bl * T;
      lv = t < alt_target_len(a.rows, a.rows.b0 + bl);
    }
    live_lds[tid] = lv;
  }
  for (int u = tid; u < 128 * (K / 16); u += 256) {
    const int r = u / (K / 16), c = u - r * (K / 16);
    v4i v = {0, 0, 0, 0};
    if (m0 + r < R) v = *reinterpret_cast<const v4i *>(a.a_i8 + (size_t)(m0 + r) * K + c * 16);
    *reinterpret_cast<v4i *>(A_lds + r * LDA + c * 16) = v;
  }
  if (tid < 128) thr[tid] = 0u;
  for (int u = tid; u < 128 * kAltMax; u += 256) lists[u] = 0ull;
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
  if (tiles == 0) return;  // (whole workgroup)
  const v4i *Wp = reinterpret_cast<const v4i *>(a.w.Wp);
  const int n_tiles = a.w.n_tiles, N = a.w.N;
  const float u = a.w.u;
  // the target's logit of each row: chunk ch = 4 ks + kg of column c is Wp[(c / 16 KS + ks) 64 + kg 16 + c % 16]
  if (tid < 128) {
    const int row = m0 + tid;
    const int c = row < R ? a.tcol[row] : -1;
    float y = -__builtin_inff();
    if (c >= 0 && c < N) {
      int acc = 0;
      for (int ch = 0; ch < K / 16; ++ch) {
        const v4i w = Wp[((size_t)(c >> 4) * KS + (ch >> 2)) * 64 + (ch & 3) * 16 + (c & 15)];
        const v4i x = *reinterpret_cast<const v4i *>(A_lds + tid * LDA + ch * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc += (int)(int8_t)(x[i] >> (8 * j)) * (int)(int8_t)(w[i] >> (8 * j));
      }
      float v = (float)(acc + 127 * a.w.colsum[c]) * u;
      v = v + a.w.pb[c];
      y = v;
    }
    y_lds[tid] = y;
  }
  __syncthreads();
  float mx[RT][4], sm[RT][4], ty[RT][4];
  int tc[RT][4];
  unsigned cnt[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[rt][r] = -3.402823466e+38f;
      sm[rt][r] = 0.0f;
      cnt[rt][r] = 0u;
      const int row = m0 + rt * 16 + lg * 4 + r;
      tc[rt][r] = row < R ? a.tcol[row] : -1;
      ty[rt][r] = y_lds[rt * 16 + lg * 4 + r];
    }
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
      const int rowb = rt * 16 + lg * 4;  // this lane's four rows of the tile
      const v4i th = *reinterpret_cast<const v4i *>(thr + rowb);  // (a stale threshold is a lower one: more candidates)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = (float)(acc[r] + 127 * cs) * u;
        v = v + pb;
        const bool better = in && v > mx[rt][r];
        lse_push(v, in, better, mx[rt][r], sm[rt][r]);
        mx[rt][r] = better ? v : mx[rt][r];
        const float y = ty[rt][r];
        const bool before = in && (v > y || (v == y && col < tc[rt][r]));
        cnt[rt][r] += before ? 1u : 0u;
        const uint32_t ov = alt_ordered(v);
        if (in && v == v && ov >= (uint32_t)th[r]) {  // the slow path: rare once the list is full
          unsigned long long carry = ((unsigned long long)ov << 32) | (uint32_t)~(uint32_t)col;
          unsigned long long *L = lists + (size_t)(rowb + r) * kAltMax;
          int i = k;  // the first slot the key beats (slots only rise: those before it stay above the key)
          for (int j = k - 1; j >= 0; --j) i = L[j] < carry ? j : i;
          for (; i < k && carry != 0ull; ++i) {
            const unsigned long long old = __hip_atomic_fetch_max(L + i, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long top = old > carry ? old : carry;
            carry = old > carry ? carry : old;
            if (i == k - 1) __hip_atomic_fetch_max(thr + rowb + r, (uint32_t)(top >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
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
      float m = mx[rt][r], s = sm[rt][r];
      unsigned n = cnt[rt][r];
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) {
        const float om = __shfl_xor(m, x, 64), os = __shfl_xor(s, x, 64);
        lse_merge(m, s, om, os);
        n += (unsigned)__shfl_xor((int)n, x, 64);
      }
      if (lr == 0) {
        const int row = rt * 16 + lg * 4 + r;
        float *o = red + ((size_t)wave * 128 + row) * 2;
        o[0] = m;
        o[1] = s;
        cnt_lds[wave * 128 + row] = n;
      }
    }
  __syncthreads();
  if (tid < 128 && live_lds[tid]) {
    float m = red[tid * 2], s = red[tid * 2 + 1];
    unsigned n = cnt_lds[tid];
    for (int w = 1; w < 4; ++w) {
      const float *o = red + ((size_t)w * 128 + tid) * 2;
      lse_merge(m, s, o[0], o[1]);
      n += cnt_lds[w * 128 + tid];
    }
    const float y = y_lds[tid];
    const int r = m0 + tid;
    const int bl = r / T, t = r - bl * T;
    const size_t o = (size_t)(a.rows.b0 + bl) * T + t;
    const bool none = !(m > -3.402823466e+38f);
    // (score_out_kernel's y: a NaN target logit is lost to its fmaxf merges, the row's s is NaN anyway)
    a.scores[o] = forced_score(s, (y == y ? y : -__builtin_inff()) - m, none);
    const int c_t = a.tcol[r];
    if (alt.rank) alt.rank[o] = (c_t >= 0 && c_t < N && y == y) ? n : 0xffffffffu;
    for (int i = 0; i < k; ++i) {
      const unsigned long long best = lists[(size_t)tid * kAltMax + i];
      uint32_t id = 0xffffffffu;
      float sc = -__builtin_inff();
      if (best != 0ull) {
        const int c = (int)~(uint32_t)best;
        id = alt.sl ? alt.sl[c] : (uint32_t)c;
        const float l = c == c_t ? y : alt_value((uint32_t)(best >> 32));  // (the target's own bits: -0 stays -0)
        sc = forced_score(s, l - m, none);
      }
      alt.ids[o * k + i] = id;
      if (alt.scores) alt.scores[o * k + i] = sc;
    }
  }
}

}  // namespace

size_t score_alternatives_lds_bytes(int K) {
  return (size_t)128 * (K + 16) + 4 * 128 * 2 * sizeof(float) + 128 * sizeof(int) + 128 * sizeof(float) +
         4 * 128 * sizeof(uint32_t) + 128 * sizeof(uint32_t) + (size_t)128 * kAltMax * 8;
}

hipError_t launch_score_alternatives(const ScoreOutArgs &a, const ScoreAltArgs &alt, hipStream_t st) {
  const int R = a.rows.nb * a.rows.T;
  if (R <= 0 || a.w.K % 64 || a.w.N <= 0 || alt.k < 1 || alt.k > kAltMax || !alt.ids) return hipErrorInvalidValue;
  const int KS = a.w.K / 64;
  const size_t lds = score_alternatives_lds_bytes(a.w.K);
  const dim3 grid((R + 127) / 128);
  auto run = [&](auto kernel) {
    const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(kernel), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, a, alt);
    return hipGetLastError();
  };
  if (KS == 1) return run(score_alt_kernel<1>);
  if (KS == 2) return run(score_alt_kernel<2>);
  if (KS == 4) return run(score_alt_kernel<4>);
  if (KS == 8) return run(score_alt_kernel<8>);
  return hipErrorInvalidValue;
}

}  // namespace slimt_hip
