// Step constraints (slimt_hip_ctx_set_step_constraints): a step's choice conditioned on what the row has already emitted.
//
// A row has the history h[0 .. L): the tokens recorded so far, forced-prefix tokens included. At a step that is not forced:
//   banned   the suppress list; eos while L < min_length; and, for n = no_repeat_ngram >= 1 and L >= n - 1, every
//            h[q + n - 1] with 0 <= q <= L - n whose window h[q .. q + n - 2] equals the suffix h[L - n + 1 .. L - 1]
//            (cn_window_bans; windows may overlap the suffix; n = 1 has empty windows and bans every emitted token)
//   seen     every h[q]
//   column   an id's output-layer column (cn_column): the id itself without a shortlist, its place in the sorted shortlist
//            with one; an id without a column constrains nothing
//   penalty  a seen column's logit l becomes l > 0 ? l * inv_theta : l * theta (cn_penalise): one float32 product, once
//            per column however often its id occurs; inv_theta = 1.0f / theta is formed once on the host. Then
//            z = l' * inv_T (inv_T = 1: a greedy call)
//   C        the valid (non-NaN z) columns that are not banned; all valid columns when that leaves none (the bans are
//            lifted for the step, the penalty stays)
//   token    greedy: the first maximum of z over C from -FLT_MAX with strict >; sampled: the first maximum of
//            fmaf(l', inv_T, g) (sampling.h) over C. The score is log softmax(z over C) at the chosen column, from the float
//            sum of exp(z - M), M the maximum over C; a NaN anywhere in the row makes it NaN, as in every scored path.
// A forced step is not constrained: every valid column, no penalty. Sets are sets: any order of marking gives the same.
//
// Host-compilable, like floor.h.
#pragma once

#include "sampling.h"

namespace slimt_hip {

constexpr uint32_t kConstraintMaxNgram = 8;      // SLIMT_HIP_CONSTRAINT_MAX_NGRAM
constexpr uint32_t kConstraintMaxSuppress = 64;  // SLIMT_HIP_CONSTRAINT_MAX_SUPPRESS
constexpr int kConstraintMaxHistory = 1024;      // SLIMT_HIP_CONSTRAINT_MAX_HISTORY: the history row a workgroup holds in LDS
constexpr int kConstraintMaxN = 1 << 19;         // two bitmaps over the columns, 128 KiB, beside the history in a CU's 160 KiB
constexpr uint32_t kConstraintFallback = 0x80000000u;  // SLIMT_HIP_CONSTRAINT_FALLBACK: the step lifted its bans

// The setting as the kernel takes it (a kernel argument: the suppress list travels by value).
struct StepConstraints {
  uint32_t no_repeat_ngram = 0;  // 0: off
  float theta = 1.0f, inv_theta = 1.0f;  // 1: off
  uint32_t min_length = 0;  // 0: off
  uint32_t n_suppress = 0;  // 0: off
  uint32_t suppress[kConstraintMaxSuppress] = {};
};

// finite theta > 0 (a NaN fails the comparison), n <= 8, at most 64 suppressed ids
SLIMT_SM_HD bool cn_valid(uint32_t no_repeat_ngram, float theta, uint32_t n_suppress) {
  return no_repeat_ngram <= kConstraintMaxNgram && theta > 0.0f && theta <= 3.402823466e+38f && n_suppress <= kConstraintMaxSuppress;
}

SLIMT_SM_HD bool cn_armed(const StepConstraints &c) {
  return c.no_repeat_ngram != 0 || c.theta != 1.0f || c.min_length != 0 || c.n_suppress != 0;
}

// whether the window of n - 1 tokens at q equals the history's suffix, so that h[q + n - 1] is banned; n >= 1
SLIMT_SM_HD bool cn_window_bans(const uint32_t *h, uint32_t L, uint32_t n, uint32_t q) {
  if (q + n > L) return false;  // (also L < n - 1)
  bool same = true;
  for (uint32_t j = 0; j + 1 < n; ++j) same = same && h[q + j] == h[L - n + 1 + j];
  return same;
}

SLIMT_SM_HD bool cn_eos_banned(uint32_t L, uint32_t min_length) { return L < min_length; }

// the column of a vocabulary id among N: the id without a shortlist, its index in the sorted shortlist with one, -1: none
SLIMT_SM_HD int cn_column(const uint32_t *sl, int N, uint32_t id) {
  if (!sl) return id < (uint32_t)N ? (int)id : -1;
  int lo = 0, hi = N;  // the first index whose id is not below `id`
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (sl[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo < N && sl[lo] == id ? lo : -1;
}

SLIMT_SM_HD float cn_penalise(float l, float theta, float inv_theta) { return l > 0.0f ? l * inv_theta : l * theta; }

// the bans are lifted for a step whose valid columns are all banned
SLIMT_SM_HD bool cn_lift(uint32_t n_candidates, uint32_t n_valid) { return n_candidates == 0 && n_valid > 0; }

// whether a column of value z belongs to C
SLIMT_SM_HD bool cn_candidate(float z, bool banned, bool lift) { return z == z && !(banned && !lift); }

#if !defined(__HIP_DEVICE_COMPILE__)
// One greedy row on the host, column by column, from the functions above: the whole contract in one place, for the checker
// program and for reading. banned, seen [N] (0 / 1) and z [N] are written; returns the chosen column (-1: none beat the
// start value) and whether the bans were lifted.
inline int cn_greedy_row(const float *l, int N, const uint32_t *sl, const uint32_t *h, uint32_t L, const StepConstraints &c,
                         uint32_t eos, unsigned char *banned, unsigned char *seen, float *z, bool *lifted) {
  for (int i = 0; i < N; ++i) banned[i] = seen[i] = 0;
  auto mark = [&](unsigned char *set, uint32_t id) {
    const int col = cn_column(sl, N, id);
    if (col >= 0) set[col] = 1;
  };
  for (uint32_t q = 0; q < L; ++q) {
    mark(seen, h[q]);
    if (c.no_repeat_ngram != 0 && cn_window_bans(h, L, c.no_repeat_ngram, q)) mark(banned, h[q + c.no_repeat_ngram - 1]);
  }
  for (uint32_t i = 0; i < c.n_suppress; ++i) mark(banned, c.suppress[i]);
  if (cn_eos_banned(L, c.min_length)) mark(banned, eos);
  uint32_t n_valid = 0, n_cand = 0;
  for (int i = 0; i < N; ++i) {
    z[i] = seen[i] ? cn_penalise(l[i], c.theta, c.inv_theta) : l[i];
    n_valid += z[i] == z[i];
    n_cand += cn_candidate(z[i], banned[i] != 0, false);
  }
  *lifted = cn_lift(n_cand, n_valid);
  float best = -3.402823466e+38f;
  int col = -1;
  for (int i = 0; i < N; ++i)
    if (cn_candidate(z[i], banned[i] != 0, *lifted) && z[i] > best) {
      best = z[i];
      col = i;
    }
  return col;
}
#endif

}  // namespace slimt_hip
