// Beam search (slimt_hip_translate_beam*, slimt_hip_beam_step): the arithmetic of one decoder row's column scores.
//
// A beam compares totals of log-probabilities across rows, and a comparison has no tolerance: a candidate on the other
// side of a tie changes the hypothesis. So the row's normaliser is defined on integers, like the nucleus of truncation.h:
// every column of a usable row (no NaN, a finite maximum M, -0 read as +0) gets the weight
//   w = bm_weight(l, M) = 2^40 where l == M, 0 where l - M <= -28, else (uint64_t)((double)tr_exp(l - M) * 2^40),
// the row's Q is the uint64 sum of the weights -- exact, so every order of accumulation gives the same bits; below 2^60
// for fewer than 2^20 columns -- and
//   L = sm_log((float)((double)Q * 2^-40)),     lp_c = (l_c - M) - L      (two f32 subtractions, in this order).
// tr_exp (truncation.h) on (-28, 0]: n >= -41, so the result is normal; the conversion to double and the product with
// 2^40 are exact, the truncation to uint64 is the only rounding. Q >= 2^40 (the maximum's column), so L >= 0 is the
// logarithm of a normal float >= 1. tests/test_beam_checker.py measures tr_exp there and lp against float64.
//
// Host-compilable, like truncation.h and sampling.h: every fused operation an explicit fmaf, nothing else contracted.
#pragma once

#include <math.h>
#include <stdint.h>

#include "truncation.h"

namespace slimt_hip {

constexpr int kBeamMax = 8;                     // == SLIMT_HIP_MAX_BEAM
constexpr uint32_t kBeamMaxN = 1u << 20;        // an output layer of this many columns or more is refused (Q < 2^60)
constexpr uint32_t kBeamNone = 0xffffffffu;     // the token of a carried finished slot; parent and token of a dead one
constexpr uint32_t kBeamDead = 0u, kBeamLive = 1u, kBeamFinished = 2u;  // a slot's flag

// the row's maximum as the weights and scores use it: -0 becomes +0 (fmaxf may return either zero of a tie)
SLIMT_SM_HD float bm_max(float m) { return m + 0.0f; }

// a row is usable if it holds no NaN and its maximum is finite
SLIMT_SM_HD bool bm_usable(bool any_nan, float M) { return !any_nan && M > -INFINITY && M < INFINITY; }

// the integer weight in [0, 2^40] of column l (not NaN) in a usable row of maximum M
SLIMT_SM_HD uint64_t bm_weight(float l, float M) {
  if (l == M) return 1099511627776ull;
  const float d = l - M;
  if (d <= -28.0f) return 0ull;
  return (uint64_t)((double)tr_exp(d) * 1099511627776.0);
}

// L of a row whose weights sum to Q (2^40 <= Q < 2^60)
SLIMT_SM_HD float bm_normaliser(uint64_t Q) { return sm_log((float)((double)Q * 9.094947017729282379150390625e-13)); }

// the column's log-probability
SLIMT_SM_HD float bm_logprob(float l, float M, float L) {
  const float d = l - M;
  return d - L;
}

}  // namespace slimt_hip
