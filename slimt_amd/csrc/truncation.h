// Truncated sampling (slimt_hip_ctx_set_sampling_truncation): which columns of a step's output layer stay in the draw.
//
// Top-k is a comparison of floats and needs no arithmetic. The nucleus (top-p) is a set defined by sums of
// probabilities, and a set has no tolerance: a column on the other side of the boundary changes the token. scores.h
// sums __expf on the device and expf on the host, which is fine for a score and fatal here. So the nucleus is defined
// on integers: every column of a row with maximum M gets the weight
//   w = tr_weight(z, M) = 2^24 where z == M, 0 where z - M <= -17, else (uint32_t)(tr_exp(z - M) * 2^24),
// sums of weights are uint64 -- exact, so every order of accumulation gives the same bits -- and the boundary is the
// comparison (double)sum >= (double)top_p * (double)total, both sides exact integers below 2^53 or one IEEE product.
//
// tr_exp is this header's own exponential of d in (-17, 0], so that host and device agree bit for bit: n = d log2(e)
// rounded to nearest (by adding and subtracting 1.5 * 2^23, a pure float operation), r = d - n ln2 with ln2 split as in
// sampling.h, exp(r) = 1 + r + r^2 P(r) with the degree-5 polynomial of Cephes' expf, every fused operation an explicit
// fmaf and nothing else contracted (-ffp-contract=off), and the factor 2^n added to the exponent bits. d > -17 keeps
// n >= -25 and the result normal. Over a sweep of (-17, 0] the weight is within 1 of floor(exp64(d) 2^24) and never
// decreases as d grows (tests/test_truncation_checker.py bounds it by 2).
//
// tr_ord is the usual order-preserving map of a float's bits to uint32 (what the kernel's radix select descends on);
// +0 and -0 map to neighbours, and equal floats otherwise to equal words.
//
// Host-compilable, like sampling.h and scores.h.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sampling.h"

namespace slimt_hip {

// exp(d) of d in (-17, 0]
SLIMT_SM_HD float tr_exp(float d) {
  const float t = d * 1.44269504088896341f;
  const float n = (t + 12582912.0f) - 12582912.0f;  // round to nearest even: |t| < 2^22
  float r = fmaf(n, -0.693359375f, d);              // (exact: n has at most 5 bits)
  r = fmaf(n, 2.12194440e-4f, r);
  const float z = r * r;
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  const float y = fmaf(p, z, r) + 1.0f;
  return sm_float(sm_bits(y) + ((uint32_t)(int32_t)n << 23));
}

// the integer weight in [0, 2^24] of a valid (non-NaN) z in a row whose maximum valid z is M
SLIMT_SM_HD uint32_t tr_weight(float z, float M) {
  if (z == M) return 16777216u;  // (first: M = +-inf never evaluates inf - inf)
  const float d = z - M;
  if (d <= -17.0f) return 0u;
  return (uint32_t)(tr_exp(d) * 16777216.0f);
}

// order-preserving: a < b as floats (neither NaN, not +-0 against each other) <=> tr_ord(a) < tr_ord(b)
SLIMT_SM_HD uint32_t tr_ord(float x) {
  const uint32_t b = sm_bits(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

SLIMT_SM_HD float tr_unord(uint32_t o) {
  return sm_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

}  // namespace slimt_hip
