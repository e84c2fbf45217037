// Sampling without replacement on a beam call (slimt_hip_ctx_set_beam_sampling, slimt_hip_beam_step_sampled): stochastic
// beam search (Kool, van Hoof and Welling 2019), the arithmetic of one slot's candidates.
//
// Everything of beam.h holds word for word: usable rows, bm_weight, Q, L, lp_c, the slot flags, and the totals C as f32
// sums of lp. A slot also carries a perturbed value G (f32), a source a 64-bit key K (slimt_hip_sampling_key). Before
// step 0, slot 0 is live with C = +0 and G = +0.
//   noise         at step t, slot s has the row key k_s = sm_sentence_key(K, s) and the words (s0, s1) = the low and the
//                 high half of sm_step_words(k_s, t); column c with vocabulary id y_c gets g_c = sm_gumbel(s0, s1, y_c)
//   perturbation  for a live slot with a usable row and every column with lp_c > -inf:
//                 phi_c = C_s + lp_c,  psi_c = sb_perturb(phi_c, g_c) = (phi_c + g_c) + 0.0f  (two f32 adds; -0 becomes +0)
//                 A slot's columns are ordered by psi descending as floats, then column ascending; only the first k of
//                 that order are the slot's candidates, and the first one's psi is Z_s
//   conditioning  candidate j of slot s gets cand = sb_condition(G_s, Z_s, psi), the real function
//                 -log(exp(-G_s) - exp(-Z_s) + exp(-psi)) in the paper's stable form
//                   v = G_s - psi + log1p(-exp(psi - Z_s)),  cand = G_s - max(0, v) - log1p(exp(-|v|))
//                 with psi == Z_s giving exactly G_s and an exponent at or below -28 an exp of 0 (the expression below is
//                 the definition). The result never exceeds G_s.
//   selection     a finished slot is a candidate itself with cand = G_s; candidates are ordered by cand descending as
//                 floats, then slot ascending, then the within-slot rank ascending; the first k become the slots 0..k-1
//                 with C = phi_c and G = cand (a carried slot keeps both)
// The k hypotheses are a draw without replacement from the model's distribution over sequences truncated at Tmax.
//
// 1 - exp(d) near d = 0 would cancel in tr_exp's result, so above -0.25 it is -d times the Taylor polynomial of
// expm1(d) / d to degree 6 (the next term is below 2e-9 of the sum there); the value is kept normal for sm_log.
// tests/test_beam_sampled_checker.py compares sb_condition bit for bit with its NumPy restatement and measures it against
// float64.
//
// Host-compilable, like beam.h, truncation.h and sampling.h: every fused operation an explicit fmaf, nothing else contracted.
#pragma once

#include <math.h>
#include <stdint.h>

#include "beam.h"

namespace slimt_hip {

// the perturbed score of a column: its total so far plus its noise
SLIMT_SM_HD float sb_perturb(float phi, float g) { return (phi + g) + 0.0f; }

// exp(d) of d <= 0, 0 at or below -28
SLIMT_SM_HD float sb_exp(float d) { return d <= -28.0f ? 0.0f : tr_exp(d); }

// log(1 - exp(d)) of d < 0 (not NaN)
SLIMT_SM_HD float sb_log1mexp(float d) {
  float om;
  if (d > -0.25f) {
    float p = 1.98412698e-4f;            // 1/5040
    p = fmaf(p, d, 1.38888889e-3f);      // 1/720
    p = fmaf(p, d, 8.33333333e-3f);      // 1/120
    p = fmaf(p, d, 4.16666667e-2f);      // 1/24
    p = fmaf(p, d, 1.66666667e-1f);      // 1/6
    p = fmaf(p, d, 0.5f);
    p = fmaf(p, d, 1.0f);
    om = fmaxf(-d * p, 1.17549435e-38f);
  } else {
    om = 1.0f - sb_exp(d);
  }
  return sm_log(om);
}

// the perturbed value of a candidate psi <= Z of a slot whose own value is G and whose largest candidate is Z (all finite)
SLIMT_SM_HD float sb_condition(float G, float Z, float psi) {
  if (psi == Z) return G;
  const float gp = G - psi;
  const float v = gp + sb_log1mexp(psi - Z);
  const float a = -fabsf(v);
  const float top = G - fmaxf(0.0f, v);
  return top - sm_log(1.0f + sb_exp(a));
}

}  // namespace slimt_hip
