// Concurrency plan of one persistent decoder launch (decode_fused.hip): sentences per workgroup, admission
// depth and the K/V cache policy. Pure host code (no HIP): engine.cpp calls it under the admission lock, and
// tests compile it without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace slimt_hip {

struct DecoderPlanIn {
  int B = 0, S = 0, Ld = 0;
  int rows = 16;              // sentences per workgroup before the plan (16, or what a decode mode forces)
  bool adaptive = false;      // the plan may narrow 16 to 8 or 4 (decode mode 0, adaptive rows on, nothing forced)
  bool narrow_ok = false;     // the kernel has the 8- and 4-sentence tilings for this shape (fused_decode_rows)
  double kv_bytes = 0;        // this launch's K/V caches
  double pending_kv = 0;      // K/V caches of every context with a decoder pending, this launch's included
  size_t contexts = 1;        // contexts with a decoder pending, this one included
  int queues = 4;             // hardware queues the HIP runtime started with (GPU_MAX_HW_QUEUES, default 4)
  int budget = 0;             // decoder workgroups admitted at a time (> 0: the admission is on)
  int kv_policy = 0;          // 0 = chosen per launch, 1 = temporal, 2 = non-temporal
  size_t ring = 64;           // admission events kept (engine.cpp, kRing): n is at most this
  // the engine's environment overrides (engine.cpp)
  double rows_oversub = 1.0;  // SLIMT_ROWS_OVERSUB
  double kv_budget = 300e6;   // SLIMT_KV_BUDGET_MB
  int kv_grain = 8;           // SLIMT_KV_GRAIN
  int by_launch = -1;         // SLIMT_KV_BY_LAUNCH
  double launch_budget = 300e6;  // SLIMT_KV_LAUNCH_BUDGET_MB
};

struct DecoderPlan {
  int rows = 16;            // sentences per workgroup
  int wgs = 0;              // workgroups that work (ceil(B / rows))
  size_t in_flight = 1;     // decoders that can run at once: min(pending contexts, queues)
  bool queue_bound = false; // more pending contexts than hardware queues
  size_t n = 1;             // admission depth: launch k waits for launch k - n ...
  bool wait = true;         // ... unless the queues alone keep the decoders within the budget
  int eighths = 0;          // K/V temporal eighths (kernels.h, kv_temporal_eighths) before the by-launch rule
  bool by_launch = false;   // the by-launch keep rule applies: ...
  int k = 8;                // ... both layers of k launches of every 8 stay temporal, the others stream
};

// Decoders in flight. A context is a stream, and the runtime maps the streams onto `queues` hardware queues; kernels
// that share a queue run one after the other. So at most min(pending contexts, queues) decoders run at a time, and
// the sentences per workgroup, the admission depth and the K/V policy are sized for that many, not for every pending
// context.
//
// The budget stays 7/8 of the CUs for the decoders in flight together, queue-bound or not. At the runtime's default
// four queues the headline (20 contexts, B = 256, S = 32) then takes the 8-sentence tiling (4 x 32 workgroups = 128
// CUs) and reaches 15.16-15.22 M tok/s on one box, against 12.87-12.91 M for the parent's plan (16 sentences, n = 14,
// K/V kept by launch). Giving the four decoders the whole chip instead (CUs / queues each: 4 x 64 workgroups of 4
// sentences) measured 14.16-14.25 M, and 16 sentences without waits 13.20-13.24 M: the CUs the decoders leave go to
// the encoders on the other queues. Queue-bound (more pending contexts than queues), a launch never waits for an
// admission event while the queues alone keep the decoders within the budget (n >= queues): a waiting kernel blocks
// its whole hardware queue, the encoders behind it included.
//
// With at least as many queues as pending contexts (GPU_MAX_HW_QUEUES = 32, 20 contexts) the plan is the one the
// engine has made since round 4: in_flight = contexts, n = budget / workgroups, waits on.
inline DecoderPlan decoder_plan(const DecoderPlanIn &in) {
  DecoderPlan p;
  const size_t queues = (size_t)std::max(1, in.queues);
  const size_t contexts = std::max<size_t>(1, in.contexts);
  p.in_flight = std::min(contexts, queues);
  p.queue_bound = contexts > queues;
  const double budget = (double)in.budget;
  p.rows = in.rows;
  // Sentences per workgroup: the fewest of 4 / 8 with which the decoders in flight (this launch's shape taken for all
  // of them) still fit the budget; else what was asked (16). A workgroup of fewer sentences streams the same weights
  // for them: worth it only for CUs that would idle. Results do not depend on it.
  if (in.adaptive && in.narrow_ok && in.rows == 16) {
    for (int spw : {4, 8}) {
      if ((double)(p.in_flight * (size_t)((in.B + spw - 1) / spw)) <= in.rows_oversub * budget) {
        p.rows = spw;
        break;
      }
    }
  }
  p.wgs = (in.B + p.rows - 1) / p.rows;
  p.n = (size_t)std::max(1, (int)(budget / (double)p.wgs));
  if (p.n > in.ring) p.n = in.ring;
  p.wait = !(p.queue_bound && p.n >= p.in_flight);
  // K/V caches read at any moment: those of the decoders in flight, in eighths of a layer's caches (engine.cpp)
  const double active = in.pending_kv / (double)contexts * (double)std::min(p.in_flight, p.n);
  const int all = 8 * in.Ld;
  p.eighths = in.kv_policy == 1 ? all : in.kv_policy == 2 ? 0
              : (int)std::min((double)all, std::floor((double)all * in.kv_budget / active));
  if (in.kv_policy == 0) p.eighths = p.eighths / in.kv_grain * in.kv_grain;
  if (in.kv_policy == 0 && in.by_launch != 0 && p.eighths < all && in.S <= 32 && 4.0 * in.kv_bytes <= in.launch_budget) {
    p.by_launch = true;
    p.k = in.by_launch > 0 ? std::min(in.by_launch, 8) : (int)std::min(8.0, std::floor(8.0 * in.launch_budget / active));
  }
  return p;
}

}  // namespace slimt_hip
