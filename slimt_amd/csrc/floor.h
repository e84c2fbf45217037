// Floored sampling (slimt_hip_ctx_set_sampling_floor): min-p and epsilon truncation of one sampled step.
//
// Both are floors under a column's probability: min-p against a fraction of the most probable column's, epsilon against
// an absolute value. Like the nucleus of truncation.h the set has no tolerance, so it is defined on that header's integer
// weights w = tr_weight(z, M) in [0, 2^24] of a row with maximum valid z M, and their uint64 sum Q over the valid columns
// (exact in any order, below 2^53 for N < 2^29: kFloorMaxN):
//   min-p     (double)w >= (double)min_p * 2^24      the product is exact (a float times a power of two)
//   epsilon   (double)w >= (double)epsilon * (double)Q   one IEEE double product; Q converts exactly
// and the kept set K holds the valid columns that pass every armed test (a floor of 0 is not armed and passes everything,
// a column of weight 0 included) plus every column with z == M -- the fallback when epsilon exceeds the largest
// probability, so K is never empty while a valid column exists. K depends on values alone; ties are all in or all out.
// min-p alone needs no Q: fl_needs_total says so, and the kernel then skips that reduction.
//
// Host-compilable, like truncation.h.
#pragma once

#include "truncation.h"

namespace slimt_hip {

constexpr int kFloorMaxN = (1 << 29) - 1;  // Q <= N 2^24 < 2^53: (double)Q is exact

// 0 <= min_p <= 1 and 0 <= epsilon < 1, both finite (a NaN fails every comparison)
SLIMT_SM_HD bool fl_valid(float min_p, float epsilon) {
  return min_p >= 0.0f && min_p <= 1.0f && epsilon >= 0.0f && epsilon < 1.0f;
}

SLIMT_SM_HD bool fl_armed(float min_p, float epsilon) { return min_p != 0.0f || epsilon != 0.0f; }

// whether the tests read Q at all
SLIMT_SM_HD bool fl_needs_total(float epsilon) { return epsilon != 0.0f; }

// The two floors as doubles, formed once per row: fl_min is min_p 2^24, fl_eps is epsilon Q (0 where epsilon is off: every
// weight passes).
SLIMT_SM_HD double fl_min(float min_p) { return (double)min_p * 16777216.0; }
SLIMT_SM_HD double fl_eps(float epsilon, uint64_t Q) { return epsilon != 0.0f ? (double)epsilon * (double)Q : 0.0; }

// whether a valid column z of weight w = tr_weight(z, M) is kept. The fallback goes by z == M, not by w == 2^24: a z just
// under M may round to the full weight, and is out with every other column when the maximum itself is under the floor.
SLIMT_SM_HD bool fl_keep(float z, float M, uint32_t w, double floor_min, double floor_eps) {
  const double dw = (double)w;
  return (dw >= floor_min && dw >= floor_eps) || z == M;
}

}  // namespace slimt_hip
