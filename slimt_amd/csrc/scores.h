// Per-token log-probabilities of the greedy decoder's choices (slimt_hip_ctx_set_scores).
//
// The arg-max epilogues already keep each row's running maximum m of the output layer's logits. Beside it they keep
// s = sum_j exp(l_j - m) over the columns seen so far; the chosen token is the maximum, so its log-softmax is
//   score = l[y] - logsumexp(l) = -log(s).
// One exponential per logit: exp(-|v - m|) is exp(l_j - m) when v is no larger than m, and the factor that rescales the
// old sum when v is the new maximum (s' = s e + 1).
//
// Partial results (m1, s1), (m2, s2) of disjoint column sets merge as
//   (m1, s1) + (m2, s2) = (M, s1 exp(m1 - M) + s2 exp(m2 - M)),  M = max(m1, m2);
// the sum is commutative, so both partners of a butterfly step get the same bits.
//
// NaN: a NaN logit makes its exponential NaN and s stays NaN from there (the caller reports NaN for the step);
// a -inf logit adds exp(-inf) = 0. The running maximum starts at -FLT_MAX (the arg-max's start value), never at -inf,
// so v - m is never -inf - (-inf).
//
// Host-compilable (tests/test_scores_api.py checks the merge against float64 on adversarial orders).
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SLIMT_SC_HD __host__ __device__ __forceinline__
#else
#define SLIMT_SC_HD inline
#endif

namespace slimt_hip {

SLIMT_SC_HD float lse_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __expf(x);
#else
  return expf(x);
#endif
}

// one logit v of a row whose running maximum BEFORE it is m (the arg-max's value); in: the column belongs to the
// output layer; better: in && v > m (the arg-max's own test: the maximum moves to v)
SLIMT_SC_HD void lse_push(float v, bool in, bool better, float m, float &s) {
  float e = lse_exp(-fabsf(v - m));
  e = in ? e : 0.0f;
  s = better ? fmaf(s, e, 1.0f) : s + e;
}

// (m, s) += (om, os)
SLIMT_SC_HD void lse_merge(float &m, float &s, float om, float os) {
  const float M = fmaxf(m, om);
  s = s * lse_exp(m - M) + os * lse_exp(om - M);
  m = M;
}

// the step's score from the row's final sum; none: no column beat the start value (every logit NaN or -inf) or
// logit 0 is NaN -- the token is class 0 and its score NaN (float64 l[y] - logsumexp(l) is NaN in both cases)
SLIMT_SC_HD float lse_score(float s, bool none) {
  return none ? __builtin_nanf("") : -logf(s);
}

// A forced step (slimt_hip_ctx_set_target_prefix): the recorded token y is the prefix's, not the arg-max. With the row's
// maximum M and final sum s as above, its log-softmax is l[y] - M - log(s); d = l[y] - M. Written -(log(s) - d) so
// that d == 0 (the forced token IS a maximum) gives lse_score's bits, -0 at s == 1 included. A token outside the
// output layer is captured as l[y] = -inf: d = -inf and the score -inf (probability 0 under the shortlisted softmax).
// none: as for lse_score -- NaN, whatever was forced; a NaN logit elsewhere makes s NaN and the score with it.
SLIMT_SC_HD float forced_score(float s, float d, bool none) {
  return none ? __builtin_nanf("") : -(logf(s) - d);
}

}  // namespace slimt_hip
