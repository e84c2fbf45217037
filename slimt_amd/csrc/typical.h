// Locally typical sampling (slimt_hip_ctx_set_sampling_typical): the columns of one sampled step whose surprisal is closest
// to the step's entropy, up to a mass (Meister et al. 2022).
//
// With p_c = exp(z_c - M) / Z the surprisal minus the entropy is (M - z_c) - E_p[M - z]: log Z cancels, so the set hangs on
// the expected gap to the maximum alone, and that can be an integer. On truncation.h's weights w = tr_weight(z, M) in
// [0, 2^24] of a row with maximum valid z M:
//   gap      G = 0 where z == M (first: M = +-inf never forms inf - inf), else (uint32_t)(-(z - M) * 65536.0f) -- the
//            subtraction tr_weight makes, an exact product, a truncating conversion. Read only where w > 0: there
//            z - M > -17 and G < 17 * 2^16 < 2^21
//   totals   Q = sum w and A = sum w G over the valid columns, uint64: every product is below 2^45, so both sums are exact in
//            any order for N <= 2^19 (kTypicalMaxN); Ebar = A / Q by uint64 floor division (Q >= 2^24 where a column is valid)
//   key      |G - Ebar|, below 2^21 (kTypicalKeyBits): Ebar is a weighted mean of gaps
//   kappa    the smallest v among the keys of the columns with w > 0 for which
//            (double)(sum of w over w > 0, key <= v) >= (double)mass * (double)Q -- the nucleus's comparison: the sum is an
//            exact integer below 2^53, the right side one IEEE double product. mass <= 1 makes the sum over all keys reach
// and the kept set K holds the valid columns with w > 0 and key <= kappa: ties at the boundary are all in, K depends on values
// alone, K is never empty while a valid column exists, and K need not hold the most probable column -- that is the method.
//
// Host-compilable, like truncation.h and floor.h.
#pragma once

#include "truncation.h"

namespace slimt_hip {

constexpr int kTypicalMaxN = 1 << 19;  // A <= N 2^45 stays below 2^64, Q <= N 2^24 below 2^53
constexpr int kTypicalKeyBits = 21;

// finite with 0 < mass <= 1 (a NaN fails every comparison)
SLIMT_SM_HD bool ty_valid(float mass) { return mass > 0.0f && mass <= 1.0f; }

// mass 1 arms nothing: the call is the plain sampled call
SLIMT_SM_HD bool ty_armed(float mass) { return mass != 1.0f; }

// the gap of a valid column of weight tr_weight(z, M) > 0
SLIMT_SM_HD uint32_t ty_gap(float z, float M) {
  if (z == M) return 0u;
  const float d = z - M;
  return (uint32_t)(-d * 65536.0f);
}

SLIMT_SM_HD uint32_t ty_mean(uint64_t A, uint64_t Q) { return (uint32_t)(A / Q); }

SLIMT_SM_HD uint32_t ty_key(uint32_t G, uint32_t Ebar) { return G >= Ebar ? G - Ebar : Ebar - G; }

// the mass as a weight, formed once per row: the sum s of the weights up to a key reaches it iff (double)s >= ty_target
SLIMT_SM_HD double ty_target(float mass, uint64_t Q) { return (double)mass * (double)Q; }

}  // namespace slimt_hip
