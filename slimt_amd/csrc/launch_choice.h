// What the engine decides before it launches: the K/V cache form of a batch, who calibrates the tight form's centres, the
// decoder's tiling, clusters, and which launches keep their caches temporal. Pure host code (no HIP, no context), like
// decoder_plan.h: plain values in, plain values out. The *_supported() predicates are defined beside the kernels (the .hip
// files) and enter as booleans, the way narrow_ok enters DecoderPlanIn. The engine's files call these where they fill the
// launch arguments; tests compile this header without a GPU.
#pragma once

#include <cstddef>

namespace slimt_hip {

// ---- K/V cache slots ------------------------------------------------------------------------------------------------
// The packed 24-bit form caches V in groups of four keys: a sentence's block must fit the f32 form's plane (S = 1, 2, 5
// would not).
inline bool kv24_slot_fits(size_t S) { return ((S + 3) & ~(size_t)3) * 3 <= S * 4; }

// The narrow (20-bit) form caches V in groups of eight keys: a sentence's block must fit the slot of its 24-bit form
// (groups of four): not S = 1..4, 9..12.
inline bool kv20_slot_fits(int S) { return ((S + 7) / 8) * 5120 <= ((S + 3) / 4) * 3072; }

// Where the narrow form has a writer and a reader: behind the fused / 64-row encoders D = 256 (S <= 64: 33..64 tokens are
// the 64-row encoder with one sentence per workgroup) or D = 512 (S <= 32); behind the per-sentence encoder D = 256, every S.
inline bool kv_narrow_shape(int D, int S, bool long_encoder) {
  return (long_encoder ? D == 256 : ((D == 256 && S <= 64) || (D == 512 && S <= 32))) && kv20_slot_fits(S);
}

// ---- the K/V cache form of a batch ------------------------------------------------------------------------------------
struct KvFormIn {
  int D = 0, F = 0, H = 1;
  int kv_format = 0;   // slimt_hip_model_set_kv_cache_format: 0 packed (20 / 24 bits), 1 f32, 2 packed 24 bits, 3 literal
  size_t S = 0;        // tokens the sources are padded to
  int encode_rows = 0; // slimt_hip_ctx_set_encode_rows: 0 auto, 32, 64
  int decode_mode = 0; // slimt_hip_ctx_set_decode_mode
  bool lean = false;   // the persistent decoder behind a persistent encoder
  // the kernels' *_supported() for the model's (D, F, H, Le, Ld) and this S
  bool fused_encode_ok = false, tall_encode_ok = false, long_encode_ok = false;
  bool decode_packed_ok = false, decode_mid_ok = false, decode_long24_ok = false;
};

struct KvForm {
  bool mid = false;     // 33..64 tokens, D = 256 / F = 1536: the 64-row encoder with one sentence per workgroup
  bool long24 = false;  // 65..128 tokens of that shape: the per-sentence encoder, attention_packed128 with Form24
  bool packed = false;  // the batch's cache is the packed form (fused encoder -> fused decoder)
};

// packed 24-bit K/V cache: fused encoder -> fused decoder, D = 256 / d_head 32 or D = 512 / d_head 64, S <= 32, and the
// two longer classes above
inline KvForm kv_cache_form(const KvFormIn &in) {
  KvForm f;
  f.mid = in.S > 32 && in.S <= 64 && in.encode_rows != 32 && in.decode_mode != 3 && in.decode_mid_ok && in.tall_encode_ok;
  f.long24 = in.S > 64 && in.S <= 128 && in.decode_mode != 3 && in.decode_long24_ok && in.long_encode_ok;
  f.packed = in.lean && (in.kv_format == 0 || in.kv_format == 2) &&
             ((in.D == 256 && in.D / in.H == 32) || (in.D == 512 && in.D / in.H == 64 && in.F == 2048)) &&
             ((in.S <= 32 && kv24_slot_fits(in.S) && in.fused_encode_ok && in.decode_packed_ok) || f.mid || f.long24);
  return f;
}

// The tight form's centres are the column means of the first batch of enough rows that could take the form. (Who gets to
// be that batch is an atomic claim on the model: the engine's.)
inline bool kv_calibration_rows(size_t B, size_t S) { return B * S >= 1024; }

// ---- the tight (16-bit) form --------------------------------------------------------------------------------------------
struct KvTightIn {
  bool enabled = true;  // SLIMT_KV_TIGHT
  bool writer = false;  // the batch's encoder has a writer for the form (kv_tight_writer)
  int tight_limit = 0;  // slimt_hip_model::kv_tight_limit (0 = never tried)
  int kv_format = 0;
  int D = 0, S = 0;
  int decode_mode = 0;
  bool expect_large_output = false;  // this context's last decoder launch had an output layer of > 16384 columns
  // fused_decode_tight_mid_supported (for S > 64 ? 2 : 1), _tight_rows32_supported, _tight_supported
  bool mid_ok = false, rows32_ok = false, tight_ok = false;
};

// Where the tight form has a writer and a reader: D = 256 / F = 1536 (S <= 128; the 32-sentence tiling: S <= 32) and D = 512 /
// F = 2048 (S <= 32), not clusters, and an encoder with a writer for it.
inline bool kv_tight_shape(const KvTightIn &in) {
  if (!in.enabled || !in.writer || in.tight_limit <= 0 || in.kv_format != 0) return false;
  if (in.S > 32)  // longer sentences: D = 256 only (33..64 tokens: one per 64-row workgroup; 65..128: the per-sentence encoder)
    return in.S <= 128 && in.D == 256 && in.decode_mode != 3 && in.decode_mode != 6 && in.decode_mode != 1 && in.mid_ok;
  // (the 32-sentence tiling -- mode 3, or mode 0 with a large output layer, which only the decoder launch knows: what the
  // context's last one saw stands in for it -- has the reader too where its LDS allows; else a batch that meets it is
  // decoded by the 16-sentence tiling)
  const bool rows32 = in.D == 256 && (in.decode_mode == 3 || (in.decode_mode == 0 && in.expect_large_output));
  if (rows32) return in.rows32_ok;
  if (!(in.decode_mode == 0 || in.decode_mode == 2 || in.decode_mode == 3 || in.decode_mode == 4 || in.decode_mode == 5)) return false;
  return in.tight_ok;
}

// A decoder launch reads the tight form when its batch's encoder was allowed it: that encoder recorded the forms (fmt_valid)
// of this very batch (fmt_B) with some sentence-layers tight (enc_tight).
inline bool kv_tight_launch(bool kv24, bool enc_tight, bool fmt_valid, int fmt_B, int B) {
  return kv24 && enc_tight && fmt_valid && fmt_B == B;
}

// ---- the decoder's tiling -----------------------------------------------------------------------------------------------
// Output layers of more than 16k columns may be SHARED by clusters of four 16-sentence workgroups where the kernel has it
// -- under the decoder admission only: the members wait for each other, and the admission is what guarantees every admitted
// workgroup a CU.
inline bool cluster_ok(bool kv24, int D, int F, size_t S, int decoder_budget) {
  return kv24 && D == 256 && F == 1536 && S <= 32 && decoder_budget > 0;
}
// ... on request only (decode mode 6), never with the tight form, merged or scored
inline bool clusters_chosen(bool ok, int decode_mode, bool tight, bool merged, bool scored) {
  return ok && decode_mode == 6 && !tight && !merged && !scored;
}

// Sentences per workgroup asked of fused_decode_rows (0: its default, which the plan may narrow). Scored calls and clusters:
// the 16-sentence tilings; decode modes 2 / 3 / 4 / 5 force 16 / 32 / 8 / 4; mode 0 takes 32 once the output layer dominates
// the weights a step streams (> 16384 columns). A tight batch takes 32 only where that tiling has the reader; merged
// launches have the 16-row tilings only.
inline int fused_rows_requested(bool clusters, bool scored, int decode_mode, size_t n_expected, bool tight, size_t S,
                                bool tight_rows32_ok, bool merged) {
  int rows = clusters || scored ? 16 : decode_mode == 2 ? 16 : decode_mode == 3 ? 32 : decode_mode == 4 ? 8 : decode_mode == 5 ? 4
             : (n_expected > 16384 ? 32 : 0);
  if (tight && rows == 32 && !(S <= 32 && tight_rows32_ok)) rows = 16;
  if (merged && rows == 32) rows = 16;
  return rows;
}

// ---- the K/V policy of one launch ---------------------------------------------------------------------------------------
// Bytes per cached value: tight 2, narrow (what the model's sentences are expected to take where the forms are recorded)
// 2.5, 24-bit 3, f32 4.
inline double kv_bytes_per_value(bool tight, bool fmt_recorded, bool kv24) {
  return tight ? 2.0 : fmt_recorded ? 2.5 : kv24 ? 3.0 : 4.0;
}

// The by-launch keep rule (decoder_plan.h, DecoderPlan::by_launch): both layers of k launches of every 8 stay temporal, by
// the slot the call drew when it started. With SLIMT_KV_STORE_NT=1 the encoder already wrote a streamed cache past the
// Infinity Cache, judging by the k of the admission before (call_k): the decoder then follows the same k.
inline int kv_launch_eighths(bool by_launch, int plan_eighths, int plan_k, unsigned long long call_slot, int call_k,
                             bool store_nt_rule, int all) {
  if (!by_launch) return plan_eighths;
  return (int)(call_slot % 8) < (store_nt_rule ? call_k : plan_k) ? all : 0;
}
// ... and whether the encoder of that call writes its cache non-temporally (SLIMT_KV_STORE_NT=1)
inline bool kv_store_streamed(bool store_nt, bool kv24, unsigned long long call_slot, int call_k) {
  return store_nt && kv24 && call_k < 8 && (int)(call_slot % 8) >= call_k;
}

}  // namespace slimt_hip
