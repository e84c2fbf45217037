// Consensus selection over unit rows: the character n-gram F (chrF), orders 1..6 (slimt_hip_consensus_select_units*, and the
// option slimt_hip_ctx_set_fanout_consensus_units of the fan-out translate calls). include/slimt_hip.h holds the definition:
// consensus.hip's, word for word, over the rows' expansions through a unit table. Integer counts and IEEE doubles in the
// defined order: a host evaluation agrees bit for bit.
//
// A unit row is up to 1024 units, 64 of them are 256 KiB and a pair costs the product of two lengths: one workgroup per
// source (consensus.hip) neither holds the rows nor finishes in reasonable time. A one-thread clear and three launches on one
// stream over a workspace sized by the N rows (no array is sized by B, which the definition does not bound):
//
//   consensus_units_expand_kernel   one workgroup of 4 waves per source.
//     1. its rows in ascending order: consensus.hip's ordered compaction (wave ballots plus the waves' counts);
//     2. a wave expands a row, 64 tokens at a time: each lane's piece length, an inclusive prefix sum over the wave
//        (shuffles), the pieces' starts and table offsets to the wave's LDS; then every lane takes output positions
//        j, j + 64, ..., finds j's piece by a 6-step binary search over the 64 starts and writes ws_units[row][base + j]:
//        consecutive lanes, consecutive words. Five zeros go behind the row's length u (a 6-gram window at p < u ends at
//        p + 5 <= u + 4 < 1029), u to ws_ulen. A row over 1024 units stops expanding and marks the source;
//     3. a marked source (over 64 rows, or a row over the limit) gets utility 0.0 and best 0xFFFFFFFF here and nothing
//        more; any other source writes its row list and its row count at its lowest row c0 and appends c0 to the head list
//        (one atomic add on the list's counter: the slots' order is arbitrary and no result depends on it). The later
//        launches run over head slots -- at most min(B, N) -- and a slot past the counter leaves at once.
//   consensus_units_pairs_kernel    grid min(B, N) x chunks in one dimension, workgroup id = slot * chunks + chunk, 4 waves:
//     a source's chunks have consecutive ids, and the device deals consecutive workgroups round its dies. (A grid over rows
//     with the work at each source's lowest row put every working workgroup of a sorted fan-out call, whose sources start
//     at multiples of 8, on one die of eight.) The
//     source's n (n - 1) / 2 unordered pairs are dealt over the chunks' waves, pair q to wave q mod (4 chunks): 32 sources
//     of 8 rows keep 7 workgroups each busy, 64 rows up to 128. A wave owns one pair (h, r) at a time; its lanes hold 64
//     consecutive positions p of h and the six units from p on. consensus.hip's rule with six orders in one sweep: k_p =
//     the earlier positions of h with the same gram, c_r = the positions of r with it, M_g = sum over p of [k_p < c_r]; a
//     g-gram match is a (g - 1)-gram match and one more comparison. The swept row (h itself for k, r for c) streams through
//     the wave's LDS tile of 256 + 5 units: a coalesced global load, then one LDS address per step read by all lanes (a
//     broadcast) into a sliding window of six registers. M_g accumulates in scalar registers over the chunks of h and goes
//     to ws_M [row][partner's place][6] u16 (a count is <= 1024), both ways.
//   consensus_units_finish_kernel   grid min(B, N), one wave. For a head slot, thread h forms F_g, U(h, r) and utility[h] in the defined
//     order (one operation after the other: no tree, no atomics); thread 0 takes the first largest.
//
// No workgroup waits for another; the launches' order on the stream is the only dependence. Barriers: every __syncthreads()
// is reached by the whole workgroup (loops over workgroup-uniform bounds; early returns on values all threads read alike).
// A wave's LDS tile is its own: wave_lds_sync orders its stores and loads (LDS operations of one wave execute in order).
//
// Bounds: row_src is clamped to B - 1, len to T, an id >= V expands to nothing. ws_units[c] is written at < 1029 and read at
// p + 5 <= u + 4 and s0 + x <= u + 4; units is read inside the expansion the table gives (the host checked the table when it
// was uploaded); ws_list / ws_M are indexed by a place < n <= 64; the tile at x + 5 <= 260 < 264.
// The sweeps are plain loops (no unrolling, no vectorising), as in consensus.hip. No out-of-line device functions, no
// dynamic stack, no scratch.
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {

namespace {

constexpr int kUnitsLd = kConsensusMaxUnits + 5;
constexpr int kUnitsThreads = 256, kUnitsWaves = kUnitsThreads / 64;
constexpr int kUnitsTile = 256, kUnitsTileLd = kUnitsTile + 8;
constexpr int kUnitsMaxChunks = 128;
// workgroups of the pair launch worth having when the sources are many: the 2048 that 256 CUs hold at 8 waves a SIMD, four
// times over, so that the last ones to finish leave little of the device idle
constexpr int kUnitsPairBlocks = 8192;

// Kernels of this file are compiled without the packed f32 instructions (v_pk_*_f32), whichever build compiles them: the
// attribute travels with the source, so build.py and the CMake fragment produce the same code object.
#if defined(__HIP_DEVICE_COMPILE__)
#define SLIMT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else  // (the host pass only needs the kernels' stubs, and its target does not know the feature)
#define SLIMT_NO_PACKED_F32
#endif

// the head list's counter back to 0 (the expand launch behind it on the stream adds to it; no memset: a plain kernel)
__global__ SLIMT_NO_PACKED_F32 void consensus_units_clear_kernel(ConsensusUnitsArgs a) { *a.ws_count = 0u; }

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t units_source_of(const ConsensusUnitsArgs &a, uint32_t c) {
  const uint32_t named = a.row_src[c];
  return named < a.B ? named : a.B - 1;
}

__global__ SLIMT_NO_PACKED_F32 __launch_bounds__(kUnitsThreads) void consensus_units_expand_kernel(ConsensusUnitsArgs a) {
  __shared__ uint32_t row[kConsensusMaxRows];      // the source's rows, ascending
  __shared__ uint32_t wcount[kUnitsWaves];         // a scan step's matches per wave
  __shared__ uint32_t over[kUnitsWaves];           // a wave met a row over the limit
  __shared__ uint32_t start[kUnitsWaves][64];      // a token chunk's pieces: their first output position in the chunk
  __shared__ uint32_t piece[kUnitsWaves][64];      // ... and their offset in units
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t b = blockIdx.x;

  // 1. the source's rows, in ascending order (n: workgroup-uniform, counted past the 64 slots)
  int n = 0;
  for (uint32_t c0 = 0; c0 < a.N; c0 += kUnitsThreads) {
    const uint32_t c = c0 + (uint32_t)tid;
    const bool mine = c < a.N && units_source_of(a, c) == b;
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kUnitsWaves; ++w) {
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

  // 2. the unit rows
  if (lane == 0) over[wave] = 0u;
  if (n <= kConsensusMaxRows) {
    uint32_t *st = start[wave], *pc = piece[wave];
    for (int x = wave; x < n; x += kUnitsWaves) {
      const uint32_t c = row[x];
      const uint32_t l0 = a.len[c];
      const int l = (int)(l0 < a.T ? l0 : a.T);
      const uint32_t *src = a.ids + (size_t)c * a.T;
      uint32_t *dst = a.ws_units + (size_t)c * kUnitsLd;
      uint32_t base = 0;  // (uniform) the units of the tokens before this chunk
      for (int t0 = 0; t0 < l; t0 += 64) {
        const int t = t0 + lane;
        uint32_t o = 0u, e = 0u;
        if (t < l) {
          const uint32_t id = src[t];
          if (id < a.V) {
            o = a.unit_off[id];
            e = a.unit_off[id + 1] - o;
          }
        }
        uint32_t inc = e;
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t v = __shfl_up(inc, d);
          if (lane >= d) inc += v;
        }
        const uint32_t total = __shfl(inc, 63);
        st[lane] = inc - e;
        pc[lane] = o;
        wave_lds_sync();
        const uint32_t room = (uint32_t)kConsensusMaxUnits - base;  // (base <= 1024 here)
        const uint32_t lim = total < room ? total : room;
        for (uint32_t j = (uint32_t)lane; j < lim; j += 64u) {
          int k = 0;  // the last piece that starts at or before j: it holds j (empty pieces start where the next one does)
          for (int s = 32; s; s >>= 1)
            if (st[k + s] <= j) k += s;
          dst[base + j] = a.units[pc[k] + (j - st[k])];
        }
        wave_lds_sync();
        base += total;
        if (base > (uint32_t)kConsensusMaxUnits) break;  // (whole wave)
      }
      if (base > (uint32_t)kConsensusMaxUnits) {
        if (lane == 0) over[wave] = 1u;
      } else {
        if (lane < 5) dst[base + (uint32_t)lane] = 0u;
        if (lane == 0) a.ws_ulen[c] = base;
      }
    }
  }
  __syncthreads();

  // 3. the source's record
  bool marked = n > kConsensusMaxRows;
  for (int w = 0; w < kUnitsWaves; ++w) marked = marked || over[w] != 0u;
  if (marked) {  // (the whole workgroup) no selection: nothing of this source reaches the later launches
    for (uint32_t c = (uint32_t)tid; c < a.N; c += kUnitsThreads)
      if (units_source_of(a, c) == b) a.utility[c] = 0.0;
    if (tid == 0) a.best[b] = 0xFFFFFFFFu;
    return;
  }
  if (tid < n) a.ws_list[(size_t)row[0] * kConsensusMaxRows + tid] = row[tid];
  if (tid == 0) {  // the source's record at its lowest row, and that row into the head list: a slot of its own, in any order
    a.ws_head[row[0]] = (uint32_t)n;
    a.ws_heads[atomicAdd(a.ws_count, 1u)] = row[0];
  }
}

// One row swept against the lanes' grams t0..t5 at position p. kSelf: the row is the lanes' own; counts the positions
// q < p with the same gram (a gram valid at p is valid at q < p; an invalid one is masked where k is used). Otherwise counts
// the positions q of the row whose g-gram exists (q + g <= len) and equals the lane's.
template <bool kSelf>
__device__ __forceinline__ void units_sweep(const uint32_t *__restrict__ urow, int len, int p, uint32_t *tile, int lane,
                                            uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t t4, uint32_t t5,
                                            int &c1, int &c2, int &c3, int &c4, int &c5, int &c6) {
  for (int s0 = 0; s0 < len; s0 += kUnitsTile) {  // (uniform)
    const int cnt = len - s0 < kUnitsTile ? len - s0 : kUnitsTile;
    for (int x = lane; x < cnt + 5; x += 64) tile[x] = urow[s0 + x];
    wave_lds_sync();
    uint32_t r0 = tile[0], r1 = tile[1], r2 = tile[2], r3 = tile[3], r4 = tile[4];
#pragma clang loop vectorize(disable) unroll(disable)
    for (int x = 0; x < cnt; ++x) {
      const uint32_t r5 = tile[x + 5];
      const int q = s0 + x;
      uint32_t d1 = t0 ^ r0;
      if (kSelf) d1 |= (uint32_t)(q >= p);
      const uint32_t d2 = d1 | (t1 ^ r1), d3 = d2 | (t2 ^ r2), d4 = d3 | (t3 ^ r3), d5 = d4 | (t4 ^ r4), d6 = d5 | (t5 ^ r5);
      if (kSelf) {
        c1 += d1 == 0u;
        c2 += d2 == 0u;
        c3 += d3 == 0u;
        c4 += d4 == 0u;
        c5 += d5 == 0u;
        c6 += d6 == 0u;
      } else {
        const int left = len - q;  // (uniform) the units from q on
        c1 += d1 == 0u;
        c2 += left >= 2 && d2 == 0u;
        c3 += left >= 3 && d3 == 0u;
        c4 += left >= 4 && d4 == 0u;
        c5 += left >= 5 && d5 == 0u;
        c6 += left >= 6 && d6 == 0u;
      }
      r0 = r1;
      r1 = r2;
      r2 = r3;
      r3 = r4;
      r4 = r5;
    }
    wave_lds_sync();
  }
}

__global__ SLIMT_NO_PACKED_F32 __launch_bounds__(kUnitsThreads) void consensus_units_pairs_kernel(ConsensusUnitsArgs a) {
  __shared__ uint32_t tiles[kUnitsWaves][kUnitsTileLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t slot = blockIdx.x / (uint32_t)a.chunks, chunk = blockIdx.x % (uint32_t)a.chunks;
  if (slot >= *a.ws_count) return;  // (the whole workgroup) fewer selected sources than the grid allows for
  const uint32_t c0 = a.ws_heads[slot];
  const int n = (int)a.ws_head[c0];
  if (n < 2 || n > kConsensusMaxRows) return;  // (the whole workgroup) a source without a pair
  const uint32_t *list = a.ws_list + (size_t)c0 * kConsensusMaxRows;
  uint32_t *tile = tiles[wave];
  const int pairs = n * (n - 1) / 2, stride = a.chunks * kUnitsWaves;
  for (int pair = (int)chunk * kUnitsWaves + wave; pair < pairs; pair += stride) {  // (wave-uniform)
    int i = 0, rem = pair;  // pair -> (i, j), i < j < n: the pairs of i are n - 1 - i
    while (rem >= n - 1 - i) {
      rem -= n - 1 - i;
      ++i;
    }
    const int j = i + 1 + rem;
    const uint32_t ch = __builtin_amdgcn_readfirstlane(list[i]), cr = __builtin_amdgcn_readfirstlane(list[j]);
    const int nh = __builtin_amdgcn_readfirstlane((int)a.ws_ulen[ch]), nr = __builtin_amdgcn_readfirstlane((int)a.ws_ulen[cr]);
    if (nh <= 0 || nr <= 0 || nh > kConsensusMaxUnits || nr > kConsensusMaxUnits) continue;  // (whole wave) a row that does not compete: the pair is never read
    const uint32_t *hrow = a.ws_units + (size_t)ch * kUnitsLd, *rrow = a.ws_units + (size_t)cr * kUnitsLd;
    int m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0, m6 = 0;
    for (int p0 = 0; p0 < nh; p0 += 64) {  // (uniform) this lane's position p = p0 + lane
      const int p = p0 + lane;
      const bool in = p < nh;
      const uint32_t t0 = in ? hrow[p] : 0u, t1 = in ? hrow[p + 1] : 0u, t2 = in ? hrow[p + 2] : 0u;
      const uint32_t t3 = in ? hrow[p + 3] : 0u, t4 = in ? hrow[p + 4] : 0u, t5 = in ? hrow[p + 5] : 0u;
      int k1 = 0, k2 = 0, k3 = 0, k4 = 0, k5 = 0, k6 = 0;
      units_sweep<true>(hrow, nh < p0 + 64 ? nh : p0 + 64, p, tile, lane, t0, t1, t2, t3, t4, t5, k1, k2, k3, k4, k5, k6);
      int c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
      units_sweep<false>(rrow, nr, p, tile, lane, t0, t1, t2, t3, t4, t5, c1, c2, c3, c4, c5, c6);
      m1 += __popcll(__ballot(p + 1 <= nh && k1 < c1));  // (the grams that exist at p)
      m2 += __popcll(__ballot(p + 2 <= nh && k2 < c2));
      m3 += __popcll(__ballot(p + 3 <= nh && k3 < c3));
      m4 += __popcll(__ballot(p + 4 <= nh && k4 < c4));
      m5 += __popcll(__ballot(p + 5 <= nh && k5 < c5));
      m6 += __popcll(__ballot(p + 6 <= nh && k6 < c6));
    }
    if (lane == 0) {  // M is symmetric: both slots
      uint16_t *hr = a.ws_M + ((size_t)ch * kConsensusMaxRows + j) * 6, *rh = a.ws_M + ((size_t)cr * kConsensusMaxRows + i) * 6;
      hr[0] = rh[0] = (uint16_t)m1;
      hr[1] = rh[1] = (uint16_t)m2;
      hr[2] = rh[2] = (uint16_t)m3;
      hr[3] = rh[3] = (uint16_t)m4;
      hr[4] = rh[4] = (uint16_t)m5;
      hr[5] = rh[5] = (uint16_t)m6;
    }
  }
}

__global__ SLIMT_NO_PACKED_F32 __launch_bounds__(64) void consensus_units_finish_kernel(ConsensusUnitsArgs a) {
  __shared__ double util[kConsensusMaxRows];
  __shared__ uint32_t ulen[kConsensusMaxRows];
  const int tid = threadIdx.x;
  if (blockIdx.x >= *a.ws_count) return;  // (the whole workgroup)
  const uint32_t c0 = a.ws_heads[blockIdx.x];
  const int n = (int)a.ws_head[c0];
  if (n < 1 || n > kConsensusMaxRows) return;  // (the whole workgroup)
  const uint32_t *list = a.ws_list + (size_t)c0 * kConsensusMaxRows;
  if (tid < n) ulen[tid] = a.ws_ulen[list[tid]];
  __syncthreads();
  // the utilities: references in ascending row order, orders in ascending g, one IEEE operation after the other
  if (tid < n) {
    const int h = tid, nh = (int)ulen[h];
    const uint32_t ch = list[h];
    double u = 0.0;
    if (nh > 0) {
      double sum = 0.0;
      int refs = 0;
      for (int r = 0; r < n; ++r) {
        const int nr = (int)ulen[r];
        if (r == h || nr == 0) continue;
        const uint16_t *m = a.ws_M + ((size_t)ch * kConsensusMaxRows + r) * 6;
        double us = 0.0;
        int counted = 0;
        for (int g = 1; g <= a.max_order; ++g) {
          const int gh = nh - g + 1 > 0 ? nh - g + 1 : 0, gr = nr - g + 1 > 0 ? nr - g + 1 : 0;
          if (gh == 0 && gr == 0) continue;
          const double f = (double)((1 + a.beta2) * (int)m[g - 1]) / (double)(a.beta2 * gr + gh);
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
    a.utility[ch] = u;
  }
  __syncthreads();
  // the lowest competing row whose utility no other exceeds
  if (tid == 0) {
    uint32_t best = 0xFFFFFFFFu;
    double top = 0.0;
    for (int h = 0; h < n; ++h) {
      if (ulen[h] == 0) continue;
      if (best == 0xFFFFFFFFu || util[h] > top) {
        best = list[h];
        top = util[h];
      }
    }
    a.best[units_source_of(a, c0)] = best;
  }
}

constexpr size_t kUnitsRowBytes = (size_t)kUnitsLd * 4 + 4 + 4 + 4 + (size_t)kConsensusMaxRows * 4 + (size_t)kConsensusMaxRows * 6 * 2;

}  // namespace

size_t consensus_units_workspace_bytes(uint32_t N) { return (size_t)(N ? N : 1) * kUnitsRowBytes + 4; }

hipError_t launch_consensus_units(const ConsensusUnitsArgs &a, void *workspace, hipStream_t st) {
  if (a.B < 1 || a.B > 0x7fffffffu || a.T < 1 || a.T > (uint32_t)kConsensusMaxT || a.N > kConsensusMaxN)
    return hipErrorInvalidValue;
  if (a.max_order < 1 || a.max_order > kConsensusUnitsMaxOrder || a.beta2 < 1 || a.beta2 > kConsensusMaxBeta2)
    return hipErrorInvalidValue;
  if (!a.best || !a.unit_off || (a.N && (!a.ids || !a.len || !a.row_src || !a.utility || !workspace))) return hipErrorInvalidValue;
  ConsensusUnitsArgs k = a;
  const size_t N = a.N;
  char *w = static_cast<char *>(workspace);
  k.ws_units = reinterpret_cast<uint32_t *>(w);
  k.ws_ulen = k.ws_units + N * kUnitsLd;
  k.ws_head = k.ws_ulen + N;
  k.ws_heads = k.ws_head + N;
  k.ws_count = k.ws_heads + N;
  k.ws_list = k.ws_count + 1;
  k.ws_M = reinterpret_cast<uint16_t *>(k.ws_list + N * kConsensusMaxRows);
  if (a.N == 0) {  // (no row: every source gets best 0xFFFFFFFF; no workspace, no head list)
    hipLaunchKernelGGL(consensus_units_expand_kernel, dim3(a.B), dim3(kUnitsThreads), 0, st, k);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(consensus_units_clear_kernel, dim3(1), dim3(1), 0, st, k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(consensus_units_expand_kernel, dim3(a.B), dim3(kUnitsThreads), 0, st, k);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // The later grids run over head slots: at most min(B, N) sources have a row. The pairs' chunks: enough for the most pairs
  // a source of this call can have, one pair per wave, at most kUnitsMaxChunks -- and, where the sources are many, no more
  // than spread kUnitsPairBlocks workgroups over them (a wave then takes several pairs in turn). A source's chunks have
  // consecutive workgroup ids, so they go round the device's dies instead of onto one.
  const uint32_t heads = a.B < a.N ? a.B : a.N;
  const int rows = (int)(a.N < (uint32_t)kConsensusMaxRows ? a.N : (uint32_t)kConsensusMaxRows);
  int chunks = (rows * (rows - 1) / 2 + kUnitsWaves - 1) / kUnitsWaves;
  chunks = chunks < 1 ? 1 : chunks > kUnitsMaxChunks ? kUnitsMaxChunks : chunks;
  const int share = (int)((uint32_t)kUnitsPairBlocks / heads);
  if (chunks > share) chunks = share < 1 ? 1 : share;
  k.chunks = chunks;
  hipLaunchKernelGGL(consensus_units_pairs_kernel, dim3(heads * (uint32_t)chunks), dim3(kUnitsThreads), 0, st, k);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(consensus_units_finish_kernel, dim3(heads), dim3(64), 0, st, k);
  return hipGetLastError();
}

}  // namespace slimt_hip
