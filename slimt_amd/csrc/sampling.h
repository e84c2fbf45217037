// Sampled decoding (slimt_hip_ctx_set_sampling): Gumbel-max over the output layer, with noise that is a pure function of
// (sentence key, step, vocabulary id) and the same bits on the host and on the device.
//
// The arg-max epilogues compare, instead of the logit l_c of column c (vocabulary id y_c),
//   key_c = fmaf(l_c, inv_T, g(k, t, y_c)),      g = -log(-log(u)) standard Gumbel noise,
// and take the first maximum as before: the token is a draw from softmax(l / T). Beside the key they keep the running
// log-sum-exp of z_c = l_c * inv_T (scores.h, now with a maximum of its own) and the winner's z: the step's score is
// log softmax(z)[token] = -(log(s) - (z_token - M)) (scores.h, forced_score).
//
// The hash. Once per sentence and step, two 32-bit words from a splitmix64 finaliser over key and step:
//   x = k + (t + 1) * 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
//   x *= 0x94D049BB133111EB;  x ^= x >> 31;                 s0 = low word of x, s1 = high word
// and per vocabulary id a murmur3-style 32-bit finaliser that takes the two words in turn:
//   h = id * 0x9E3779B1 + s0;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h += s1;  h *= 0xC2B2AE35;  h ^= h >> 16
//   h23 = h >> 9,  u = (h23 + 0.5) * 2^-23 = (2 h23 + 1) * 2^-24:  an exact float in (0, 1), at most 1 - 2^-24.
// The key of sentence `index` of a request seeded `seed` (slimt_hip_sampling_key) is the same splitmix64 finaliser over
// seed + (index + 1) * 0x9E3779B97F4A7C15 -- a bijection of the index for a fixed seed.
//
// The logarithm (sm_log) is this header's own, so that host and device agree bit for bit: x = 2^e * m with m in
// [sqrt(1/2), sqrt(2)), f = m - 1, log(x) = e ln2 + f - f^2/2 + f^3 P(f) with the degree-8 polynomial of Cephes' logf,
// every fused operation an explicit fmaf and nothing else contracted (-ffp-contract=off). For u in [sqrt(1/2), 1) e is 0
// and the result is f (1 + ...): relatively accurate as u -> 1, where -log(u) -> 2^-24. Over all 2^23 values of u,
// |g - float64(-log(-log(u)))| < 2e-6 (tests/test_sampling_checker.py bounds it by 2e-4) and g is monotone in u.
//
// Host-compilable, like scores.h.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SLIMT_SM_HD __host__ __device__ __forceinline__
#else
#define SLIMT_SM_HD inline
#endif

namespace slimt_hip {

SLIMT_SM_HD uint64_t sm_mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// the key of sentence `index` of a request seeded `seed`
SLIMT_SM_HD uint64_t sm_sentence_key(uint64_t seed, uint64_t index) {
  return sm_mix64(seed + (index + 1) * 0x9E3779B97F4A7C15ull);
}

// the two words of a sentence's step (t: its count of recorded tokens)
SLIMT_SM_HD uint64_t sm_step_words(uint64_t key, uint32_t t) {
  return sm_mix64(key + ((uint64_t)t + 1) * 0x9E3779B97F4A7C15ull);
}

SLIMT_SM_HD uint32_t sm_hash23(uint32_t s0, uint32_t s1, uint32_t id) {
  uint32_t h = id * 0x9E3779B1u + s0;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h += s1;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h >> 9;
}

SLIMT_SM_HD float sm_uniform(uint32_t h23) {
  return (float)(2u * h23 + 1u) * 5.9604644775390625e-8f;  // (2 h23 + 1) 2^-24: both factors exact, and so the product
}

SLIMT_SM_HD uint32_t sm_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(x);
#else
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
#endif
}

SLIMT_SM_HD float sm_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float x;
  memcpy(&x, &b, 4);
  return x;
#endif
}

// log(x) of a positive, finite, normal x
SLIMT_SM_HD float sm_log(float x) {
  // m in [sqrt(1/2), sqrt(2)): subtracting the bits of sqrt(1/2) (0x3f3504f3) makes the exponent field count from there
  const uint32_t b = sm_bits(x) - 0x3f3504f3u;
  const float e = (float)((int32_t)b >> 23);
  const float f = sm_float((b & 0x007fffffu) + 0x3f3504f3u) - 1.0f;
  const float z = f * f;
  float p = 7.0376836292e-2f;
  p = fmaf(p, f, -1.1514610310e-1f);
  p = fmaf(p, f, 1.1676998740e-1f);
  p = fmaf(p, f, -1.2420140846e-1f);
  p = fmaf(p, f, 1.4249322787e-1f);
  p = fmaf(p, f, -1.6668057665e-1f);
  p = fmaf(p, f, 2.0000714765e-1f);
  p = fmaf(p, f, -2.4999993993e-1f);
  p = fmaf(p, f, 3.3333331174e-1f);
  float y = (f * z) * p;
  y = fmaf(e, -2.12194440e-4f, y);  // ln2 = 0.693359375 - 2.12194440e-4: the large part is exact in e
  y = fmaf(-0.5f, z, y);
  return fmaf(e, 0.693359375f, f + y);
}

// standard Gumbel noise of a uniform u in (0, 1)
SLIMT_SM_HD float sm_gumbel_of(float u) {
  return -sm_log(-sm_log(u));
}

SLIMT_SM_HD float sm_gumbel(uint32_t s0, uint32_t s1, uint32_t id) {
  return sm_gumbel_of(sm_uniform(sm_hash23(s0, s1, id)));
}

// the compared value of a column: its logit l at inverse temperature inv_T plus the noise of its vocabulary id
SLIMT_SM_HD float sm_key(float l, float inv_T, uint32_t s0, uint32_t s1, uint32_t id) {
  return fmaf(l, inv_T, sm_gumbel(s0, s1, id));
}

}  // namespace slimt_hip
