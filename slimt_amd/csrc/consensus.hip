// Minimum-Bayes-risk (consensus) selection among the rows of each source (slimt_hip_consensus_select*, and the option
// slimt_hip_ctx_set_fanout_consensus of the fan-out translate calls). include/slimt_hip.h holds the definition; this file
// computes it with integer counts and IEEE doubles in the defined order, so it agrees with a host evaluation bit for bit.
//
//   consensus_kernel   one workgroup of 16 waves per source:
//     1. the workgroup finds its rows by scanning row_src (rows may come in any order): an ordered compaction, wave ballots
//        plus the waves' counts, so the local row order is the ascending row index;
//     2. it stages the rows' tokens in LDS, [row][T + 3], zero behind a row's length (the three extra columns let a 4-gram
//        window start at any position without leaving the row);
//     3. a wave owns a row h and the pairs (h, h + d mod n), d = 1 .. (n - 1) / 2 (and d = n / 2 for the lower half when n
//        is even): every unordered pair exactly once, evenly spread. Its lanes hold 64 positions p of h at a time.
//        For each p: k_p = the earlier positions of h with the same gram (once per row), c_r = the positions of the other
//        row r with that gram (once per pair); M_g = sum over p of [k_p < c_r] -- the clipped match count, exact on 32-bit
//        ids, no hash, no sort. A g-gram match at (p, q) is a (g - 1)-gram match there and one more token comparison, so
//        one sweep over q gives all four orders. The partner's tokens are read at one LDS address per step by all lanes (a
//        broadcast) through a sliding window of four registers;
//     4. thread h forms utility[h] from M in ascending reference order (doubles, added one by one: no tree);
//     5. thread 0 scans the utilities in ascending row order for the first largest.
//
// Barriers: every __syncthreads() is reached by all 1024 threads: the loops around them run over workgroup-uniform bounds
// (N, and the row count n that every thread derives from the same LDS words), and the two early returns (no row, more than
// 64 rows) are taken by the whole workgroup on that same n.
//
// Bounds: row_src is clamped to B - 1 and len to T as it is read. A source with more than kConsensusMaxRows rows gets
// best = 0xFFFFFFFF and utility 0.0 for its rows. ids is read at [row][t < min(len, T)] only; LDS rows are indexed by a
// slot < n <= lds_rows.
//
// LDS: 1088 bytes of row tables, M [rows][rows][4] u16 (a count is <= 256) and the tokens [rows][T + 3] u32 with
// rows = min(N, 64): 99,424 bytes at 64 rows x T = 256 -- above the 64 KiB a kernel gets without asking
// (set_dynamic_lds_once), under the 160 KiB of a gfx950 CU. All of it is dynamic, every carve a multiple of 16 bytes.
//
// The three sweeps over q are kept as plain loops (no unrolling, no vectorising): unrolled by the compiler they take the
// 128 registers a 1024-thread workgroup leaves a lane and spill to scratch; plain they take 31 and none.
// No out-of-line device functions, no dynamic stack, no scratch.
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {

namespace {

constexpr int kConsensusThreads = 1024, kConsensusWaves = kConsensusThreads / 64;
constexpr size_t kConsensusTables = 64 * 8 + 64 * 4 + 64 * 4 + kConsensusWaves * 4;  // util, row, nlen, wcount

__global__ __launch_bounds__(kConsensusThreads) void consensus_kernel(ConsensusArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  const int T = (int)a.T, R = a.lds_rows, ld = T + 3;
  double *util = reinterpret_cast<double *>(smem);                     // [64]
  uint32_t *row = reinterpret_cast<uint32_t *>(smem + 64 * 8);         // [64] the source's rows, ascending
  uint32_t *nlen = row + 64;                                           // [64] their lengths, clamped to T
  uint32_t *wcount = nlen + 64;                                        // [16] a scan step's matches per wave
  uint16_t *M = reinterpret_cast<uint16_t *>(smem + kConsensusTables);  // [R][R][4]
  uint32_t *tok = reinterpret_cast<uint32_t *>(smem + kConsensusTables + (((size_t)R * R * 8 + 15) & ~(size_t)15));  // [R][ld]

  auto source_of = [&](uint32_t c) {
    const uint32_t named = a.row_src[c];
    return named < a.B ? named : a.B - 1;
  };

  // 1. the source's rows, in ascending order (n: workgroup-uniform, counted past the 64 slots)
  int n = 0;
  for (uint32_t c0 = 0; c0 < a.N; c0 += kConsensusThreads) {
    const uint32_t c = c0 + (uint32_t)tid;
    const bool mine = c < a.N && source_of(c) == b;
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kConsensusWaves; ++w) {
      const int k = (int)wcount[w];
      total += k;
      if (w < wave) before += k;
    }
    const int slot = n + before + __popcll(bal & ((1ull << lane) - 1ull));
    if (mine && slot < kConsensusMaxRows) row[slot] = c;
    n += total;
    __syncthreads();
  }
  if (n == 0) {  // (the whole workgroup) a source without rows
    if (tid == 0) a.best[b] = 0xFFFFFFFFu;
    return;
  }
  if (n > kConsensusMaxRows || n > R) {  // (the whole workgroup) more rows than the definition admits: no selection
    for (uint32_t c = (uint32_t)tid; c < a.N; c += kConsensusThreads)
      if (source_of(c) == b) a.utility[c] = 0.0;
    if (tid == 0) a.best[b] = 0xFFFFFFFFu;
    return;
  }

  // 2. lengths and tokens
  if (tid < n) {
    const uint32_t l = a.len[row[tid]];
    nlen[tid] = l < a.T ? l : a.T;
  }
  __syncthreads();
  for (int x = wave; x < n; x += kConsensusWaves) {
    const uint32_t *src = a.ids + (size_t)row[x] * a.T;
    const int nx = (int)nlen[x];
    for (int t = lane; t < ld; t += 64) tok[x * ld + t] = t < nx ? src[t] : 0u;
  }
  __syncthreads();

  // 3. the match counts of every unordered pair of competing rows
  for (int h = wave; h < n; h += kConsensusWaves) {
    const int nh = __builtin_amdgcn_readfirstlane((int)nlen[h]);
    if (nh == 0) continue;  // (whole wave) does not compete: its pairs are never read
    const uint32_t *hrow = tok + h * ld;
    const int half = (n - 1) / 2;
    const int partners = half + (((n & 1) == 0 && h < n / 2) ? 1 : 0);
    for (int p0 = 0; p0 < nh; p0 += 64) {  // (uniform) this lane's position p = p0 + lane: one chunk of the row at a time
      const int p = p0 + lane;
      const bool in = p < nh;
      const uint32_t t0 = in ? hrow[p] : 0u, t1 = in ? hrow[p + 1] : 0u, t2 = in ? hrow[p + 2] : 0u, t3 = in ? hrow[p + 3] : 0u;
      // k_g: the earlier positions q < p of h with the same g-gram (a gram valid at p is valid at q < p; an invalid one is
      // masked where k is used). Every q < p0 is earlier for every lane; behind it the lane decides.
      int k1 = 0, k2 = 0, k3 = 0, k4 = 0;
      {
        uint32_t r0 = hrow[0], r1 = hrow[1], r2 = hrow[2];
        const int qn = nh < p0 + 64 ? nh : p0 + 64;
#pragma clang loop vectorize(disable) unroll(disable)
        for (int q = 0; q < qn; ++q) {
          const uint32_t r3 = hrow[q + 3];
          const uint32_t d1 = (t0 ^ r0) | (uint32_t)(q >= p), d2 = d1 | (t1 ^ r1), d3 = d2 | (t2 ^ r2), d4 = d3 | (t3 ^ r3);
          k1 += d1 == 0u;
          k2 += d2 == 0u;
          k3 += d3 == 0u;
          k4 += d4 == 0u;
          r0 = r1;
          r1 = r2;
          r2 = r3;
        }
      }
      const bool v1 = p + 1 <= nh, v2 = p + 2 <= nh, v3 = p + 3 <= nh, v4 = p + 4 <= nh;  // the grams that exist at p
      for (int d = 1; d <= partners; ++d) {
        int r = h + d;
        if (r >= n) r -= n;
        const int nr = __builtin_amdgcn_readfirstlane((int)nlen[r]);
        if (nr == 0) continue;  // (whole wave)
        const uint32_t *rrow = tok + r * ld;
        // c_g: the positions q of r whose g-gram equals the one at p. Up to q = nr - 4 all four orders fit; the last three
        // positions hold the shorter grams only (lim: the tokens left from q on)
        int c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        uint32_t r0 = rrow[0], r1 = rrow[1], r2 = rrow[2];
        int q = 0;
#pragma clang loop vectorize(disable) unroll(disable)
        for (; q + 4 <= nr; ++q) {
          const uint32_t r3 = rrow[q + 3];
          const uint32_t d1 = t0 ^ r0, d2 = d1 | (t1 ^ r1), d3 = d2 | (t2 ^ r2), d4 = d3 | (t3 ^ r3);
          c1 += d1 == 0u;
          c2 += d2 == 0u;
          c3 += d3 == 0u;
          c4 += d4 == 0u;
          r0 = r1;
          r1 = r2;
          r2 = r3;
        }
#pragma clang loop vectorize(disable) unroll(disable)
        for (; q < nr; ++q) {
          const int lim = nr - q;  // (uniform) 3, 2 or 1
          const uint32_t d1 = t0 ^ r0, d2 = d1 | (t1 ^ r1), d3 = d2 | (t2 ^ r2);
          c1 += d1 == 0u;
          c2 += lim >= 2 && d2 == 0u;
          c3 += lim >= 3 && d3 == 0u;
          r0 = r1;
          r1 = r2;
          r2 = rrow[q + 3];
        }
        const int m1 = __popcll(__ballot(v1 && k1 < c1)), m2 = __popcll(__ballot(v2 && k2 < c2));
        const int m3 = __popcll(__ballot(v3 && k3 < c3)), m4 = __popcll(__ballot(v4 && k4 < c4));
        if (lane == 0) {  // M is symmetric: both slots; the row's first chunk sets them, the others add (this wave alone)
          uint16_t *hr = M + ((size_t)h * R + r) * 4, *rh = M + ((size_t)r * R + h) * 4;
          const bool first = p0 == 0;
          hr[0] = rh[0] = (uint16_t)((first ? 0 : hr[0]) + m1);
          hr[1] = rh[1] = (uint16_t)((first ? 0 : hr[1]) + m2);
          hr[2] = rh[2] = (uint16_t)((first ? 0 : hr[2]) + m3);
          hr[3] = rh[3] = (uint16_t)((first ? 0 : hr[3]) + m4);
        }
      }
    }
  }
  __syncthreads();

  // 4. the utilities: references in ascending row order, orders in ascending g, one IEEE operation after the other
  if (tid < n) {
    const int h = tid, nh = (int)nlen[h];
    double u = 0.0;
    if (nh > 0) {
      double sum = 0.0;
      int refs = 0;
      for (int r = 0; r < n; ++r) {
        const int nr = (int)nlen[r];
        if (r == h || nr == 0) continue;
        const uint16_t *m = M + ((size_t)h * R + r) * 4;
        double us = 0.0;
        int counted = 0;
        for (int g = 1; g <= a.max_order; ++g) {
          const int ch = nh - g + 1 > 0 ? nh - g + 1 : 0, cr = nr - g + 1 > 0 ? nr - g + 1 : 0;
          if (ch == 0 && cr == 0) continue;
          const double f = (double)((1 + a.beta2) * (int)m[g - 1]) / (double)(a.beta2 * cr + ch);
          us = us + f;
          ++counted;
        }
        const double U = counted ? us / (double)counted : 0.0;
        sum = sum + U;
        ++refs;
      }
      u = refs ? sum / (double)refs : 0.0;
    }
    util[h] = u;
    a.utility[row[h]] = u;
  }
  __syncthreads();

  // 5. the lowest competing row whose utility no other exceeds
  if (tid == 0) {
    uint32_t best = 0xFFFFFFFFu;
    double top = 0.0;
    for (int h = 0; h < n; ++h) {
      if (nlen[h] == 0) continue;
      if (best == 0xFFFFFFFFu || util[h] > top) {
        best = row[h];
        top = util[h];
      }
    }
    a.best[b] = best;
  }
}

}  // namespace

size_t consensus_lds_bytes(int rows, int T) {
  return kConsensusTables + (((size_t)rows * rows * 8 + 15) & ~(size_t)15) + (size_t)rows * (T + 3) * 4;
}

hipError_t launch_consensus(const ConsensusArgs &a, hipStream_t st) {
  if (a.B < 1 || a.B > 0x7fffffffu || a.T < 1 || a.T > (uint32_t)kConsensusMaxT || a.N > kConsensusMaxN)
    return hipErrorInvalidValue;
  if (a.max_order < 1 || a.max_order > kConsensusMaxOrder || a.beta2 < 1 || a.beta2 > kConsensusMaxBeta2)
    return hipErrorInvalidValue;
  if (!a.best || (a.N && (!a.ids || !a.len || !a.row_src || !a.utility))) return hipErrorInvalidValue;
  ConsensusArgs k = a;
  k.lds_rows = (int)(a.N < (uint32_t)kConsensusMaxRows ? (a.N ? a.N : 1) : (uint32_t)kConsensusMaxRows);
  const size_t lds = consensus_lds_bytes(k.lds_rows, (int)a.T);
  const hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void *>(consensus_kernel), (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(consensus_kernel, dim3(a.B), dim3(kConsensusThreads), lds, st, k);
  return hipGetLastError();
}

}  // namespace slimt_hip
