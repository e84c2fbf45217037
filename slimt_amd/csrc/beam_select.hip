// Beam search (slimt_hip_translate_beam*, slimt_hip_beam_step): one selection per step, and the walk at the end.
//
// beam_select_kernel: one 256-thread workgroup per source over its k <= 8 rows of the step's f32 logits, which the logits
// gemm has just written (L2-resident: 128 KiB at k = 8, N = 4096); both passes re-read them, so N is arbitrary.
//   pass 1     per live slot: is there a NaN, and the maximum M
//   pass 2     per usable slot: the uint64 sum Q of the integer weights bm_weight(l, M) (beam.h: exact in any order) and
//              the slot's k best (logit, column) pairs, with score_alternatives.hip's technique: a sorted list of 64-bit
//              keys (ordered(logit) << 32) | ~column in LDS, 64-bit atomic maxima behind a threshold word. Within a slot
//              cand = C + lp is monotone in the logit, so only its k best columns can be chosen
//   selection  by wave 0, one candidate per lane: lane 8 s + j holds slot s's j-th best column (a finished slot: itself,
//              in lane 8 s). The lane order is the contract's tie order (slot ascending, then logit descending, then
//              column ascending), so k rounds of a wave-wide "largest cand, lowest lane" take the new slots in order
//   then       the step's records, the new totals / flags / lengths, the rows' step word, the SSRU states of every layer
//              gathered by parent from one block into the other, the next token's embedding, the done count
// beam_finish_kernel: one workgroup per source behind the last step; the first k threads rank the slots by the final key, then a
// wave per hypothesis walks its back-pointers from the last step to the first and writes token, score and alignment row
// of every step at which the chain took a column (a carried finished slot records kBeamNone and only passes the walk on).
//
// Every barrier is reached by every thread; no workgroup waits for another. No out-of-line device functions, no dynamic
// stack: helpers are __forceinline__.
#include <hip/hip_runtime.h>

#include "beam.h"
#include "device_common.h"
#include "kernels.h"

namespace slimt_hip {
namespace {

constexpr int kBmThreads = 256;

struct BmShared {
  unsigned long long lists[kBeamMax][kBeamMax];  // per slot: its best keys, sorted, 0 = empty
  unsigned long long Q[kBeamMax];
  uint32_t thr[kBeamMax];                        // the value part of the slot's k-th key
  float wm[kBeamMax][4];                         // pass 1 per wave
  uint32_t wn[kBeamMax][4];
  uint32_t flag[kBeamMax], len[kBeamMax];        // the slots as the step found them
  float C[kBeamMax];
  uint32_t n_flag[kBeamMax], n_parent[kBeamMax], n_tok[kBeamMax];  // the new slots
};

// a float's order as an unsigned word: -inf < ... < -0 == +0 < ... < +inf (not for NaN); never 0
__device__ __forceinline__ uint32_t bm_ordered(float v) {
  const uint32_t b = __float_as_uint(v + 0.0f);  // (-0 + 0 = +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned long long bm_shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kBmThreads) void beam_select_kernel(BeamSelectArgs a) {
  __shared__ BmShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k, N = a.N, r0 = b * k, D = a.emb.D;
  const float ninf = -__builtin_inff();
  if (a.init) {  // (the whole grid: no barrier below is skipped by part of a workgroup)
    if (tid < k) {
      a.totals_out[r0 + tid] = tid == 0 ? 0.0f : ninf;
      a.flags_out[r0 + tid] = tid == 0 ? kBeamLive : kBeamDead;
      if (a.len_out) a.len_out[r0 + tid] = 0u;
      if (a.step_word) a.step_word[r0 + tid] = 0u;
    }
    if (tid == 0 && a.done) a.done[b] = 0u;
    if (a.dx) {
      for (int u = tid; u < k * D; u += kBmThreads) {
        const float z = 0.0f * a.emb.sqrt_d;
        a.dx[(size_t)r0 * D + u] = z + a.emb.pos[u % D];
      }
    }
    return;
  }
  if (tid < kBeamMax) {
    const bool in = tid < k;
    sh.flag[tid] = in ? a.flags_in[r0 + tid] : kBeamDead;
    sh.C[tid] = in ? a.totals_in[r0 + tid] : ninf;
    sh.len[tid] = in && a.len_in ? a.len_in[r0 + tid] : 0u;
    sh.Q[tid] = 0ull;
    sh.thr[tid] = 0u;
  }
  if (tid < kBeamMax * kBeamMax) sh.lists[tid >> 3][tid & 7] = 0ull;
  __syncthreads();

  // pass 1: NaN test and maximum of every live slot
  for (int s = 0; s < k; ++s) {
    if (sh.flag[s] != kBeamLive) continue;  // (uniform)
    const float *__restrict__ row = a.logits + (size_t)(r0 + s) * N;
    float m = ninf;
    uint32_t nan = 0u;
    for (int c = tid; c < N; c += kBmThreads) {
      const float v = row[c];
      nan |= v != v ? 1u : 0u;
      m = fmaxf(m, v);
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
      m = fmaxf(m, __shfl_xor(m, x, 64));
      nan |= (uint32_t)__shfl_xor((int)nan, x, 64);
    }
    if (lane == 0) {
      sh.wm[s][wave] = m;
      sh.wn[s][wave] = nan;
    }
  }
  __syncthreads();

  // pass 2: the weight sum and the k best columns of every usable slot
  for (int s = 0; s < k; ++s) {
    if (sh.flag[s] != kBeamLive) continue;
    const float M = bm_max(fmaxf(fmaxf(sh.wm[s][0], sh.wm[s][1]), fmaxf(sh.wm[s][2], sh.wm[s][3])));
    const bool any_nan = (sh.wn[s][0] | sh.wn[s][1] | sh.wn[s][2] | sh.wn[s][3]) != 0u;
    if (!bm_usable(any_nan, M)) continue;  // (uniform)
    const float *__restrict__ row = a.logits + (size_t)(r0 + s) * N;
    unsigned long long *L = sh.lists[s];
    unsigned long long q = 0ull;
    for (int c = tid; c < N; c += kBmThreads) {
      const float v = row[c];
      q += bm_weight(v, M);
      const uint32_t ov = bm_ordered(v);
      const uint32_t th = __hip_atomic_load(&sh.thr[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (v > ninf && ov >= th) {  // the slow path: rare once the list is full (a stale threshold is a lower one)
        unsigned long long carry = ((unsigned long long)ov << 32) | (uint32_t)~(uint32_t)c;
        int i = k;  // the first slot the key beats (slots only rise: those before it stay above the key)
        for (int j = k - 1; j >= 0; --j) i = L[j] < carry ? j : i;
        for (; i < k && carry != 0ull; ++i) {
          const unsigned long long old = __hip_atomic_fetch_max(L + i, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const unsigned long long top = old > carry ? old : carry;
          carry = old > carry ? carry : old;
          if (i == k - 1) __hip_atomic_fetch_max(&sh.thr[s], (uint32_t)(top >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) q += bm_shfl_xor_u64(q, x);
    if (lane == 0) atomicAdd(&sh.Q[s], q);
  }
  __syncthreads();

  // selection: wave 0, lane 8 s + j = slot s's j-th candidate
  if (wave == 0) {
    const int s = lane >> 3, j = lane & 7;
    bool valid = false, carried = false;
    float cand = ninf, lp = 0.0f;
    uint32_t col = 0u;
    if (s < k && j < k) {
      const uint32_t f = sh.flag[s];
      if (f == kBeamFinished) {
        valid = j == 0;
        carried = true;
        cand = sh.C[s];
      } else if (f == kBeamLive) {
        const float M = bm_max(fmaxf(fmaxf(sh.wm[s][0], sh.wm[s][1]), fmaxf(sh.wm[s][2], sh.wm[s][3])));
        const bool any_nan = (sh.wn[s][0] | sh.wn[s][1] | sh.wn[s][2] | sh.wn[s][3]) != 0u;
        const unsigned long long key = sh.lists[s][j];
        if (bm_usable(any_nan, M) && key != 0ull) {
          col = ~(uint32_t)key;
          const float l = a.logits[(size_t)(r0 + s) * N + col];  // (the logit's own bits: the key folds -0 into +0)
          lp = bm_logprob(l, M, bm_normaliser(sh.Q[s]));
          cand = sh.C[s] + lp;
          valid = !(cand == ninf);
        }
      }
    }
    // a lane's place in the order: a candidate still to be taken is below 64
    uint32_t ord = valid ? (uint32_t)lane : 64u + (uint32_t)lane;
    uint32_t my_flag = kBeamDead, my_parent = kBeamNone, my_tok = kBeamNone, my_len = 0u;
    float my_lp = 0.0f, my_C = ninf;
    for (int i = 0; i < k; ++i) {
      float bc = cand;
      uint32_t bo = ord;
#pragma unroll
      for (int x = 1; x < 64; x <<= 1) {
        const float oc = __shfl_xor(bc, x, 64);
        const uint32_t oo = (uint32_t)__shfl_xor((int)bo, x, 64);
        const bool ov = oo < 64u, bv = bo < 64u;
        const bool better = ov != bv ? ov : (ov ? (oc > bc || (oc == bc && oo < bo)) : oo < bo);
        bc = better ? oc : bc;
        bo = better ? oo : bo;
      }
      if (bo >= 64u) break;  // (uniform: every lane holds the same winner) fewer than k candidates: the rest stay dead
      const int w = (int)bo;
      const int ws = w >> 3;
      const uint32_t wcol = (uint32_t)__shfl((int)col, w, 64);
      const float wlp = __shfl(lp, w, 64);
      const float wcand = __shfl(cand, w, 64);
      const int wcar = __shfl((int)carried, w, 64);
      if (lane == w) ord = 64u + (uint32_t)lane;
      if (lane == i) {
        my_parent = (uint32_t)ws;
        my_C = wcand;
        if (wcar) {
          my_flag = kBeamFinished;
          my_len = sh.len[ws];
        } else {
          my_tok = a.ids ? a.ids[wcol] : wcol;
          my_lp = wlp;
          my_flag = my_tok == a.eos ? kBeamFinished : kBeamLive;
          my_len = (uint32_t)a.t + 1u;
        }
      }
    }
    if (lane < k) {
      const int r = r0 + lane;
      a.parent[r] = my_parent;
      a.token[r] = my_tok;
      a.token_score[r] = my_lp;
      a.totals_out[r] = my_C;
      a.flags_out[r] = my_flag;
      if (a.len_out) a.len_out[r] = my_len;
      if (a.step_word) a.step_word[r] = (uint32_t)a.t + 1u;
      sh.n_flag[lane] = my_flag;
      sh.n_parent[lane] = my_parent;
      sh.n_tok[lane] = my_tok;
    }
  }
  __syncthreads();
  if (!a.state_dst) return;  // (the whole grid) the op-level call ends here

  if (tid == 0) {  // a source is done when no slot is live: counted once
    bool live = false;
    for (int i = 0; i < k; ++i) live = live || sh.n_flag[i] == kBeamLive;
    if (!live && a.done[b] == 0u) {
      a.done[b] = 1u;
      atomicAdd(a.n_finished, 1);
    }
  }
  // the SSRU states by parent, from one block into the other (a dead slot: zeros)
  const size_t R = (size_t)a.B * k;
  const int D4 = D >> 2;
  for (int u = tid; u < a.Ld * k * D4; u += kBmThreads) {
    const int l = u / (k * D4), rem = u - l * (k * D4);
    const int i = rem / D4, d4 = rem - i * D4;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sh.n_flag[i] != kBeamDead)
      v = reinterpret_cast<const float4 *>(a.state_src + ((size_t)l * R + (size_t)(r0 + (int)sh.n_parent[i])) * D)[d4];
    reinterpret_cast<float4 *>(a.state_dst + ((size_t)l * R + (size_t)(r0 + i)) * D)[d4] = v;
  }
  // the next step's input rows: the token's embedding of a live slot (embed1's expression), the zero embedding otherwise
  for (int u = tid; u < k * D; u += kBmThreads) {
    const int i = u / D, d = u - i * D;
    float x;
    if (sh.n_flag[i] == kBeamLive) {
      const float v = (float)a.emb.wemb[(size_t)embed_row(a.emb, sh.n_tok[i]) * D + d] * a.emb.inv_mult;
      x = v * a.emb.sqrt_d;
    } else {
      x = 0.0f * a.emb.sqrt_d;
    }
    a.dx[(size_t)r0 * D + u] = x + a.emb.pos[d];
  }
}

__global__ __launch_bounds__(kBmThreads) void beam_finish_kernel(BeamFinishArgs a) {
  __shared__ int rank_slot[kBeamMax];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k, r0 = b * k, S = a.S;
  const size_t R = (size_t)a.B * k;
  const float ninf = -__builtin_inff();
  if (tid < k) {  // slot tid's rank: the slots ordered before it (live or finished before dead, key descending, ties to the lower slot)
    auto alive_of = [&](int s) { return a.flags[r0 + s] != kBeamDead; };
    auto key_of = [&](int s) {
      const float C = a.totals[r0 + s];
      return a.mode == 1 ? C / (float)a.len[r0 + s] : C;
    };
    const bool al = alive_of(tid);
    const float ky = key_of(tid);
    int rank = 0;
    for (int s = 0; s < k; ++s) {
      if (s == tid) continue;
      const bool al2 = alive_of(s);
      const float k2 = key_of(s);
      const bool before = al2 != al ? al2 : (al ? (k2 > ky || (k2 == ky && s < tid)) : s < tid);
      rank += before ? 1 : 0;
    }
    rank_slot[rank] = tid;
  }
  __syncthreads();
  const uint32_t src_len = a.lengths[b] < (uint32_t)S ? a.lengths[b] : (uint32_t)S;
  for (int j = wave; j < k; j += 4) {  // a wave per hypothesis; every lane follows the same chain
    const int f = rank_slot[j];
    const size_t o = (size_t)r0 + j;
    const bool al = a.flags[r0 + f] != kBeamDead;
    if (lane == 0) {
      a.out_len[o] = al ? a.len[r0 + f] : 0u;
      a.out_totals[o] = al ? a.totals[r0 + f] : ninf;
    }
    if (!al) continue;
    int cur = f;
    for (int t = a.T - 1; t >= 0; --t) {
      const size_t h = (size_t)t * R + (size_t)(r0 + cur);
      const uint32_t p = a.parent[h], tk = a.token[h];
      if (tk != kBeamNone && t < a.Tmax) {
        if (lane == 0) {
          a.out_ids[o * a.Tmax + t] = tk;
          if (a.out_scores) a.out_scores[o * a.Tmax + t] = a.token_score[h];
        }
        if (a.out_align) {
          const float *from = a.align_hist + ((size_t)(r0 + (int)p) * a.Tmax + t) * S;
          float *to = a.out_align + (o * a.Tmax + t) * S;
          if ((uint32_t)lane < src_len) to[lane] = from[lane];
          if ((uint32_t)lane + 64u < src_len) to[lane + 64] = from[lane + 64];
        }
      }
      if (p >= (uint32_t)k) break;  // (never: a live or finished slot's ancestors are live)
      cur = (int)p;
    }
  }
}

}  // namespace

hipError_t launch_beam_select(const BeamSelectArgs &a, hipStream_t st) {
  if (a.B < 1 || a.k < 1 || a.k > kBeamMax || !a.totals_out || !a.flags_out) return hipErrorInvalidValue;
  if ((a.len_in != nullptr) != (a.len_out != nullptr) && !a.init) return hipErrorInvalidValue;
  if (!a.init) {
    if (!a.logits || a.N < 1 || (uint32_t)a.N >= kBeamMaxN || !a.totals_in || !a.flags_in || !a.parent || !a.token || !a.token_score)
      return hipErrorInvalidValue;
  }
  if (a.state_dst) {
    if (!a.state_src || a.state_src == a.state_dst || a.Ld < 1 || !a.dx || !a.done || !a.n_finished || !a.emb.wemb || !a.emb.pos ||
        a.emb.D < 4 || a.emb.D % 4)
      return hipErrorInvalidValue;
  } else if (a.init && a.dx && (!a.emb.pos || a.emb.D < 1)) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(beam_select_kernel, dim3(a.B), dim3(kBmThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_beam_finish(const BeamFinishArgs &a, hipStream_t st) {
  if (a.B < 1 || a.k < 1 || a.k > kBeamMax || a.T < 1 || a.Tmax < 1 || a.S < 1 || a.S > 128 || (a.mode != 0 && a.mode != 1))
    return hipErrorInvalidValue;
  if (!a.parent || !a.token || !a.token_score || !a.totals || !a.flags || !a.len || !a.lengths || !a.out_ids || !a.out_len || !a.out_totals)
    return hipErrorInvalidValue;
  if (a.out_align && !a.align_hist) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_finish_kernel, dim3(a.B), dim3(kBmThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace slimt_hip
