// Combined decoding (slimt_hip_ctx_set_fanout_combine, slimt_hip_combine_step): one token per group of fan-out rows.
//
// A group has m member rows, 1 <= m <= kCombineMax = 4; member 0 is the primary. The setting: weights w[0..m), w[0] finite
// and > 0, the others finite with |w[j]| <= 16; a plausibility gap <= 0, a log-ratio (-inf: off). Negative weights make
// source-contrastive decoding (log p(y | x) - lambda log p(y | x')), positive ones an ensemble over several sources.
//
// Per member row j with logits l_j over N < 2^20 columns: usable, M_j, Q_j, L_j and lp_j[c] = (l_j[c] - M_j) - L_j are
// beam.h's (bm_usable, bm_max, bm_weight, bm_normaliser, bm_logprob) -- integer sums, so every order gives the same bits.
//   counted     the primary always; a member j > 0 if w[j] != 0 and its row is usable. Others contribute nothing.
//   candidate   (primary usable) l_0[c] > -inf and l_0[c] - M_0 >= gap (one f32 subtraction), and s[c] is not NaN
//   score       s[c] = w[0] * lp_0[c] (one f32 multiply), then for the counted j = 1 .. m - 1 ascending
//               s = fmaf(w[j], lp_j[c], s); a term whose l_j[c] is -inf is left out
//   order       s descending compared as floats (+0 == -0), then l_0[c] descending, then the lower column: cb_before.
//               Columns that are no candidates come behind every candidate, ordered by l_0 and the column alone, so with
//               no candidate left the first column is the primary's arg-max; with m = 1 or every other weight 0 the
//               first candidate is that arg-max too.
//   unusable    primary: column 0 and s = NaN, the arg-max path's rule for a row without a maximum
//   records     every member row records the group's token ids[column] and its own lp_j[column] (NaN for an unusable
//               member); the combined score reported is s[column], NaN where no candidate was left.
//
// Host-compilable, like beam.h: every fused operation an explicit fmaf, nothing else contracted (-ffp-contract=off).
#pragma once

#include "beam.h"

namespace slimt_hip {

constexpr int kCombineMax = 4;               // == SLIMT_HIP_MAX_COMBINE
constexpr float kCombineMaxWeight = 16.0f;   // |w[j]|, j > 0
constexpr uint32_t kCombineNone = 0xffffffffu;  // the column of "nothing seen yet": behind every column in cb_before

// the setting as the setters and the launcher check it (a NaN fails every comparison)
SLIMT_SM_HD bool cb_valid(int m, const float *w, float gap) {
  if (m < 1 || m > kCombineMax || !(gap <= 0.0f)) return false;
  if (!(w[0] > 0.0f && w[0] < INFINITY)) return false;
  for (int j = 1; j < m; ++j)
    if (!(w[j] >= -kCombineMaxWeight && w[j] <= kCombineMaxWeight)) return false;
  return true;
}

// whether member j of weight w contributes to s
SLIMT_SM_HD bool cb_counted(int j, float w, bool usable) { return j == 0 || (w != 0.0f && usable); }

// the first two candidate tests, on the primary's logit alone (the third is s == s)
SLIMT_SM_HD bool cb_plausible(float l0, float M0, float gap) {
  const float d = l0 - M0;
  return l0 > -INFINITY && d >= gap;
}

// s from the primary, and one counted member's term onto it
SLIMT_SM_HD float cb_first(float w0, float lp0) { return w0 * lp0; }
SLIMT_SM_HD float cb_add(float s, float w, float l, float lp) { return l == -INFINITY ? s : fmaf(w, lp, s); }

// whether column a comes before column b in the contract's order (cand: a candidate; s is read for candidates only)
SLIMT_SM_HD bool cb_before(bool cand_a, float s_a, float l0_a, uint32_t col_a, bool cand_b, float s_b, float l0_b, uint32_t col_b) {
  if (cand_a != cand_b) return cand_a;
  if (cand_a && s_a != s_b) return s_a > s_b;
  if (l0_a != l0_b) return l0_a > l0_b;
  return col_a < col_b;
}

}  // namespace slimt_hip
