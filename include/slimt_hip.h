/*
 * slimt_hip.h -- C ABI of the MI355X (gfx950) backend for slimt's int8
 * transformer-NMT hot path. Plain pointers and sizes only; every function
 * returns 0 on success or a non-zero status (slimt_hip_last_error() gives the
 * message): a POSITIVE status is the hipError_t of a failed runtime call -- work
 * may already be queued on the context's stream, so synchronise or destroy the
 * context before freeing the buffers the call was given --, a NEGATIVE one is a
 * check of the library's own (arguments, sizes, state). No exceptions cross this boundary; nothing here falls back to a
 * CPU implementation -- without a HIP device the compute entry points fail.
 *
 * Citations are file:line in the reference checkout (jerinphilip/slimt).
 * The op-level group is what a `Provider::Hip` in slimt/QMM.cc would forward
 * to (INTEGRATION.md shows the .inl.cc); the engine-level group is what
 * `Encoder::forward` / `Decoder::step` / `Model::forward` dispatch to under
 * SLIMT_HAS_HIP.
 *
 * Weight layout at this boundary is slimt's canonical prepared layout: int8
 * [N][K], K contiguous (== the Marian intgemm8 payload, slimt/Io.cc:225-239),
 * i.e. what prepare_weight_quantized_transposed below emits.
 */
#ifndef SLIMT_HIP_H
#define SLIMT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLIMT_HIP_ABI_VERSION 3

/* ---- status -------------------------------------------------------------- */
int slimt_hip_abi_version(void);
const char *slimt_hip_last_error(void); /* thread-local, never NULL */
int slimt_hip_device_count(int *count);

/* ---- process-wide setup (optional) ---------------------------------------
 * The library itself never reads or writes the environment when it is loaded.
 * One HIP stream per translate worker: the HIP runtime multiplexes streams onto
 * FOUR hardware queues unless GPU_MAX_HW_QUEUES says otherwise, which caps the
 * batches really in flight (20 blocking workers: 10.4 M tok/s with 4 queues,
 * 26.5 M with 32). The runtime reads that variable once, at ITS first call from
 * anywhere in the process. _request_hw_queues(n) sets it (only if the process
 * has not chosen a value) and returns 0, or returns 1 -- changing nothing -- when
 * this library has already called into HIP (too late). It calls setenv: call it
 * from main() before threads start and before any model is created, or set the
 * variable in the launcher instead (bench.py, slimt_amd.frontend and host_test
 * do one of the two; host/Service warns once when it is started with more than
 * two workers per device and fewer than 8 queues). _hw_queues() returns the
 * value the environment holds now (0 = unset). */
int slimt_hip_request_hw_queues(int n);
int slimt_hip_hw_queues(void);

/* ---- op level: slimt::qmm::* (slimt/QMM.hh:48-63) ------------------------ */
/* Host pointers in, host pointers out (H2D, kernels, D2H on `device` 0
 * unless slimt_hip_set_device was called on this thread). Stateless and
 * re-entrant like the reference providers (slimt/QMM.cc:36-75). */
int slimt_hip_set_device(int device);

/* qmm::affine (QMM.hh:48; Intgemm.inl.cc:92-156). bias == NULL gives
 * qmm::dot (QMM.hh:56; Intgemm.inl.cc:158-226). x f32 [M,K] row-major,
 * W int8 [N][K], y f32 [M,N]. Requires K % 64 == 0 (intgemm's own tile
 * constraint), K <= 4096. */
int slimt_hip_affine(const float *x, size_t M, size_t K, const int8_t *W_nk,
                     size_t N, const float *bias, float a_quant,
                     float b_quant, float *y);
/* qmm::affine_with_select (QMM.hh:51; Intgemm.inl.cc:7-90): y [M,n_idx],
 * column c is vocabulary id idx[c]. */
int slimt_hip_affine_select(const float *x, size_t M, size_t K,
                            const int8_t *W_nk, size_t N, const float *bias,
                            float a_quant, float b_quant, const uint32_t *idx,
                            size_t n_idx, float *y);
/* Debug/parity: the raw int32 accumulators of Int8Shift::Multiply,
 * accS[i,j] = sum_k (q[i,k]+127) * W[k,j]  (Intgemm.inl.cc:149-153). */
int slimt_hip_affine_acc_i32(const float *x, size_t M, size_t K,
                             const int8_t *W_nk, size_t N, float a_quant,
                             int32_t *accS);
/* qmm::prepare_weight_transposed (QMM.hh:59; Intgemm.inl.cc:228-235):
 * weights f32 B^T [rows][cols] -> int8 canonical [rows][cols]. Runs on the
 * host (load-time only, slimt/Io.cc:215). */
int slimt_hip_prepare_weight_transposed(const float *weights, int8_t *prepared,
                                        float quantization_multiplier,
                                        size_t cols, size_t rows);
/* qmm::prepare_weight_quantized_transposed (QMM.hh:62;
 * Intgemm.inl.cc:237-243): the canonical layout IS the file layout, so this
 * is a copy (like the Ruy provider, Ruy.inl.cc:267-274). Host side. */
int slimt_hip_prepare_weight_quantized_transposed(const int8_t *input,
                                                  int8_t *output, size_t rows,
                                                  size_t cols);

/* ---- op level: slimt/TensorOps.hh float ops ------------------------------ */
/* layer_norm (TensorOps.cc:542-580) */
int slimt_hip_layer_norm(const float *x, const float *scale, const float *bias,
                         float eps, size_t rows, size_t cols, float *y);
/* softmax (TensorOps.cc:282-315) */
int slimt_hip_softmax(const float *x, size_t rows, size_t cols, float *y);
/* One truncated sampled step over the caller's logits [M][N] (host pointers; the
 * kernel of slimt_hip_ctx_set_sampling_truncation alone, which states the rule).
 * N at most 2^31 - 257. ids: the columns' vocabulary ids [N] (NULL: the column); keys: the rows' sentence
 * keys [M] (NULL: the row index); steps: the rows' step t [M] (NULL: 0).
 * columns[r]: the drawn column, or 0 with scores[r] NaN when nothing is kept or
 * logit 0 of the row is NaN; thresholds[r] = max(tau_k, tau_p) as a value (-inf
 * where nothing is cut; compare with ==, +-0 are the same threshold); kept[r] = |K|;
 * scores[r]: the step's score. */
int slimt_hip_sample_truncated(const float *logits, size_t M, size_t N, const uint32_t *ids,
                               float temperature, uint32_t top_k, float top_p,
                               const uint64_t *keys, const uint32_t *steps,
                               uint32_t *columns, float *thresholds, uint32_t *kept, float *scores);
/* highway (TensorOps.cc:662-682): out = sigmoid(g)*x + (1-sigmoid(g))*y */
int slimt_hip_highway(const float *x, const float *y, const float *g, size_t n,
                      float *out);
/* scaled_dot_product_attention (Modules.cc:24-86) on already split heads:
 * q [B,H,Tq,dh], k,v [B,H,S,dh], mask [B,S] additive -> out [B,H,Tq,dh],
 * attn [B,H,Tq,S] (nullable). */
int slimt_hip_sdpa(const float *q, const float *k, const float *v,
                   const float *mask, size_t B, size_t H, size_t Tq, size_t S,
                   size_t dh, float *out, float *attn);

/* ---- engine level -------------------------------------------------------- */
typedef struct slimt_hip_model slimt_hip_model; /* weights on one device */
typedef struct slimt_hip_ctx slimt_hip_ctx;     /* stream + workspace, one per
                                                   worker thread (Frontend.cc:212-226) */

/* One named tensor as held by slimt::Transformer::items_ after
 * io::load_items, or straight from the Marian .bin (Io.cc:114-161). */
typedef struct slimt_hip_param {
  const char *name; /* Marian parameter name (Modules.cc:336-406) */
  int32_t type;     /* 0 = f32 [rows,cols]; 1 = intgemm8: int8 payload in file
                       order ([cols][rows]; Wemb: [rows][cols]) followed by one
                       f32 quantisation multiplier (Io.cc:225-239) */
  int32_t rows;     /* shape[-2] */
  int32_t cols;     /* shape[-1] */
  const void *data; /* host memory, borrowed for the duration of the call */
  uint64_t bytes;   /* size of `data`; checked against rows * cols (+ the trailing
                       multiplier) before anything is read. 0 = not stated */
} slimt_hip_param;

typedef struct slimt_hip_dims { /* Model::Config (Model.hh:33-51) */
  int32_t encoder_layers;
  int32_t decoder_layers;
  int32_t num_heads;
} slimt_hip_dims;

/* Transformer::Transformer (Transformer.cc:87-94) + load_parameters
 * (:185-225) + the Wemb handling of Io.cc:182-224: uploads and re-tiles the
 * int8 weights for the MFMA B operand, precomputes column sums and prepared
 * biases. Unknown names are ignored, missing ones are an error.
 * Accepted shapes (anything else is refused here, with the offending size in the
 * message): embedding size 64, 128, 256 or 512; head size (embedding / heads) 16,
 * 32 or 64, at embedding size 512 only 32 or 64; FFN size a multiple of 64 up to
 * 2048; any number of encoder / decoder layers, any vocabulary. These are the
 * shapes the per-stage kernels (decode mode 1, slimt_hip_decode_step) exist for;
 * the persistent kernels serve a subset of them (slimt_hip_ctx_plan) with the
 * same results. */
int slimt_hip_model_create(const slimt_hip_param *params, size_t n_params,
                           const slimt_hip_dims *dims, int device,
                           slimt_hip_model **out);
/* The same from the Marian .bin container itself (the `View model` that
 * Transformer::Transformer receives, Transformer.cc:87-94; format Io.cc:114-161):
 * the items are located inside `bin` (bounds-checked, nothing is copied on the
 * host) and handed to slimt_hip_model_create. */
int slimt_hip_model_create_from_bin(const void *bin, size_t size,
                                    const slimt_hip_dims *dims, int device,
                                    slimt_hip_model **out);
int slimt_hip_model_destroy(slimt_hip_model *model);
/* Admission of the persistent decoders of all contexts of `model`: at most
 * about `workgroups` decoder workgroups (one CU each, 16 sentences) run at a
 * time, later launches wait on their own stream; the remaining CUs stay with
 * the encoders of the batches behind them. Default: 7/8 of the device's CUs;
 * 0 = no limit. Results do not depend on it. */
int slimt_hip_model_set_decoder_budget(slimt_hip_model *model, int workgroups);
/* Cache policy of the persistent decoder's K/V cache loads: 0 (default) = chosen
 * per launch (non-temporal once the K/V of the contexts with a pending decoder
 * exceeds what the Infinity Cache can serve), 1 = always
 * temporal, 2 = always non-temporal. Results do not depend on it. Needs the
 * decoder admission (budget > 0) for 0 and 2. */
int slimt_hip_model_set_kv_cache_policy(slimt_hip_model *model, int policy);
/* XCD-affine placement of the persistent decoder (needs the decoder admission, budget > 0):
 * 0 (default) = a batch's workgroups run wherever the dispatcher puts them; 1 / 2 / 4 = a batch
 * of up to 16 / 32 / 64 workgroups is over-launched on every XCD and its tiles are claimed only by
 * workgroups that find themselves (HW_REG_XCC_ID) on the batch's one / two / four home XCDs, so that the
 * batch's own shortlisted output layer streams through those L2s only (each MI355X XCD has a private
 * 4 MB L2). Placement changes speed only; results do not depend on it. */
int slimt_hip_model_set_xcd_affinity(slimt_hip_model *model, int xcds);
/* Storage format of the cross-attention K/V cache that slimt_hip_translate* keeps between
 * its encoder and decoder launches (the reference recomputes K and V every step,
 * slimt/Modules.cc:248-249). Every format caches the int8 GEMM's ACCUMULATORS, and the
 * attention applies the projections' unquantisation multiplier and prepared bias after its
 * sums (the same real numbers as the reference's dequantise-then-attend, other
 * roundings, <= 2.5e-5 apart; every format gives the same floats as every other):
 *   0 (default) = packed integers where the kernels support it (emb 256 / head dim 32 with
 *       sources of up to 128 tokens, emb 512 / head dim 64 up to 32 tokens and three
 *       decoder layers), f32 elsewhere. Packed
 *       means, per sentence and decoder layer and decided by the encoder: 16 bits per value
 *       where every accumulator less its column's centre lies in [-2^15, 2^15)
 *       (slimt_hip_model_set_kv_centres; the first batch of >= 1024 rows is cached as f32
 *       to calibrate the centres when none were set), else 20 bits where every accumulator
 *       lies in [-2^19, 2^19), else 24 bits (holds any accumulator);
 *   1 = always f32 (float(acc), exact);
 *   2 = packed, always 24 bits;
 *   3 = f32, and the attention in the reference's LITERAL sequence: every cached value
 *       dequantised first (k = float(acc) * unquant + bias, Intgemm.inl.cc:146-153), then
 *       Modules.cc:24-86 on those floats. Runs the decoder one launch per stage (the
 *       persistent decoder has the hoisted order only): for checking, not for speed.
 * Formats 0 / 1 / 2 give the same floats as each other; format 3 differs from them by
 * roundings only (<= 2.5e-5 of the context vectors' scale), which can move an arg-max on a
 * near-tie: see DESIGN 2 for what that means for translate output. */
int slimt_hip_model_set_kv_cache_format(slimt_hip_model *model, int format);
/* Sentences per workgroup of the persistent decoder in decode mode 0 (needs the decoder admission,
 * budget > 0): on (default) = a launch uses 8 or 4 sentences per workgroup instead of 16 while the
 * decoders of all contexts with one pending still fit the budget at that size -- a batch of 256 alone
 * then runs on 64 CUs instead of 16 (the reference's default is ONE worker, slimt/Frontend.hh:25) --,
 * off = always 16. Results do not depend on it. */
int slimt_hip_model_set_adaptive_decoder_rows(slimt_hip_model *model, int on);
int slimt_hip_model_info(const slimt_hip_model *model, int32_t *dim_emb,
                         int32_t *dim_ffn, int32_t *vocab, int32_t *heads);
/* the device the model's weights live on (-1 for NULL) */
int slimt_hip_model_device(const slimt_hip_model *model);

/* stream: a hipStream_t to run on (borrowed), or NULL to create one. */
int slimt_hip_ctx_create(slimt_hip_model *model, size_t max_batch,
                         size_t max_source_length, void *stream,
                         slimt_hip_ctx **out);
/* Same, for token-budget batching (slimt/Batcher.cc:95-120: many short
 * sentences or few long ones, (B + 1) * S <= max_words): the workspace holds
 * batches with B <= max_batch, S <= max_source_length and B * S <= max_tokens. */
int slimt_hip_ctx_create_budget(slimt_hip_model *model, size_t max_batch,
                                size_t max_source_length, size_t max_tokens, void *stream,
                                slimt_hip_ctx **out);
int slimt_hip_ctx_destroy(slimt_hip_ctx *ctx);
/* Contexts alive on `device` in this process. A context is a stream; past 22 of
 * them on one device the hardware queues are time-sliced whatever
 * GPU_MAX_HW_QUEUES says (20 contexts 33 M tok/s, 24: 23.8 M, 32: 20.4 M on the
 * headline workload), so the library says so once on stderr when the 23rd is
 * created (SLIMT_HIP_QUIET=1 silences it). slimt runs `workers` Async threads
 * (Frontend.hh:25), one context each: keep workers <= 22 per device and process. */
int slimt_hip_contexts_on_device(int device, int *count);
int slimt_hip_ctx_stream(slimt_hip_ctx *ctx, void **stream);
int slimt_hip_ctx_synchronize(slimt_hip_ctx *ctx);
/* Execution strategy of slimt_hip_translate* / slimt_hip_encode: 0 = automatic
 * (persistent fused encoder / decoder kernels when the model shape supports
 * them), 1 = one launch per stage (and per decode step; the kernels behind
 * slimt_hip_decode_step), 2 / 3 / 4 / 5 = automatic, but the persistent decoder
 * is forced to 16 / 32 / 8 / 4 sentences per workgroup where it has that
 * variant, 6 = automatic, but output layers are shared by clusters of four
 * 16-sentence workgroups where the kernel has that (emb 256, sources of up to 32
 * tokens, decoder admission on) (tuning and tests; 0 picks 32 for output layers
 * of more than 16k columns -- clusters measured 6 % below it on the full
 * vocabulary --, and 8 or 4 while CUs would idle:
 * slimt_hip_model_set_adaptive_decoder_rows). Same results in every mode. */
int slimt_hip_ctx_set_decode_mode(slimt_hip_ctx *ctx, int mode);
/* Rows (source tokens) per workgroup of the persistent encoder for emb 256 models: 0
 * (default) = chosen per call (64-row tiles from 32 of them on),
 * 32 or 64 = forced (tuning and tests). Same results either way. */
int slimt_hip_ctx_set_encode_rows(slimt_hip_ctx *ctx, int rows);
/* Per-token scores for the NEXT translate call on ctx (any of the slimt_hip_translate*
 * entry points), which consumes the setting whether it succeeds or fails; n = 0 arms
 * nothing. scores[j] is the [B_j][Tmax_j] f32 destination of batch j: n = 1 for the
 * single-batch calls, n = n_batches for the _many_ ones; in the memory of that
 * call's outputs (host for the host calls -- pinned where the outputs are, so the
 * kernels write it in place --, device for the _device ones). A mismatched n or a
 * NULL entry fails that call.
 * scores[b][t] for t < out_len[b] (EOS included) is the natural-log softmax
 * probability of out_ids[b][t] over that step's output layer (the shortlist's
 * columns, or the full vocabulary): the distribution the greedy arg-max chooses
 * from. Entries at t >= out_len[b] are not defined. A step whose logits hold a NaN
 * (this includes "logit 0 is NaN -> class 0") or are all -inf scores NaN. Tokens,
 * lengths and alignments are the same as without scores. Scored calls decode with
 * the 16-sentence tilings (decode modes 2-6 act as 2 for them). */
int slimt_hip_ctx_set_scores(slimt_hip_ctx *ctx, float *const *scores, size_t n);
/* Forced target prefixes for the NEXT translate call on ctx (any of the
 * slimt_hip_translate* entry points), which consumes them whether it succeeds or
 * fails; n = 0 arms nothing. prefix_ids[j] is batch j's [B_j][Tmax_j] uint32 array
 * (laid out like out_ids), prefix_len[j] its [B_j] lengths P_b <= Tmax_j: n = 1 for
 * the single-batch calls, n = n_batches for the _many_ ones; in the memory of that
 * call's inputs (host for the host calls, device for the _device ones). A mismatched
 * n or a NULL entry fails that call; so do, for host arrays, a P_b > Tmax_j or a
 * prefix id >= the vocabulary.
 * At step t < P_b, sentence b records and feeds prefix_ids[b][t] instead of the
 * arg-max; from step P_b on it decodes greedily, P_b = 0 is an unforced sentence.
 * Everything else is unchanged: alignments, the step limit, and the end of a
 * sentence at EOS, forced or chosen (a prefix holding EOS ends the sentence there).
 * Scoring a given translation: its tokens plus EOS as the prefix -- out_ids echoes
 * them, out_len[b] = P_b, and the scores (slimt_hip_ctx_set_scores, optional) are
 * the teacher-forced log-probabilities. A forced token outside the step's output
 * layer (not in the shortlist, fixed or generated) is still recorded and fed; its
 * score is -inf. A step whose logits hold a NaN scores NaN, forced or not. Forced
 * calls decode with the 16-sentence tilings (decode modes 2-6 act as 2), like
 * scored ones. Device arrays: see slimt_hip_translate_device. Host arrays: pinned
 * ones (slimt_hip_host_alloc) are read in place by the kernels, pageable ones are
 * copied asynchronously on the context's stream; for the _async calls either kind
 * must stay valid and unchanged until the context is synchronised, like the
 * other inputs. */
int slimt_hip_ctx_set_target_prefix(slimt_hip_ctx *ctx, const uint32_t *const *prefix_ids,
                                    const uint32_t *const *prefix_len, size_t n);
/* Sampled decoding: the key of sentence `index` of a request seeded `seed` (a host
 * function; what the batching service and the Python frontend use). For a fixed
 * seed it is a bijection of the index. */
uint64_t slimt_hip_sampling_key(uint64_t seed, uint64_t index);
/* Temperature sampling for the NEXT translate call on ctx (any of the
 * slimt_hip_translate* entry points), which consumes it whether it succeeds or
 * fails, like the scores and the prefixes; n = 0 arms nothing. temperature must be
 * finite and > 0, else a negative status. keys[j] is batch j's [B_j] uint64 array of
 * sentence keys, n = 1 for the single-batch calls and n = n_batches for the _many_
 * ones (a mismatched n fails that call), in the memory of that call's inputs: host
 * for the host calls (pinned arrays are read in place by the kernels, pageable ones
 * are copied asynchronously on the context's stream and must stay valid until the
 * context is synchronised), device for the _device ones. keys == NULL or
 * keys[j] == NULL: the key of sentence b of that batch is its row index b.
 * At step t of sentence b -- t its count of recorded tokens -- the token is the
 * vocabulary id y_c of the FIRST maximum over the output layer's columns c of
 *   key_c = fmaf(logit_c, 1.0f / temperature, g(k_b, t, y_c)),
 * g standard Gumbel noise that is a pure function of the sentence's key, the step
 * and the vocabulary id (slimt_amd/csrc/sampling.h: the hash, and a logarithm that
 * gives the same bits on the host): a draw from softmax(logit / temperature) over
 * the step's output layer (the shortlist, where there is one). The NaN and
 * start-value rules are the arg-max's, applied to the key. So a sentence's sampled
 * translation depends on its key and on nothing else: not on its row or its
 * neighbours in the batch, the decode mode, the entry point, or whether the launch
 * is merged. EOS, the step limit, alignments and out_len are as for greedy calls.
 * Sampled calls are scored internally: with slimt_hip_ctx_set_scores the scores are
 * log softmax(logit / temperature) at the recorded token; without, the engine keeps
 * them in a scratch of its own. Like scored calls they decode with the 16-sentence
 * tilings (decode modes 2-6 act as 2), or with the per-stage kernels in mode 1.
 * With a target prefix (slimt_hip_ctx_set_target_prefix) as well, steps below P_b
 * are forced and scored at that temperature, and the first sampled step is t = P_b
 * with the noise of step t. Such calls run the persistent decoder's sampled-and-
 * forced twin (decode_fused_kernel<..., SC, FP, SM>) or, in mode 1, the per-stage
 * kernels; the results are the same. */
int slimt_hip_ctx_set_sampling(slimt_hip_ctx *ctx, float temperature, const uint64_t *const *keys, size_t n);
/* Top-k and nucleus (top-p) truncation of the NEXT translate call on ctx, which must
 * be a sampled one (slimt_hip_ctx_set_sampling): armed for that call, which consumes
 * it whether it succeeds or fails, like the scores, the prefix and the sampling.
 * top_k == 0: no top-k; top_p == 1.0f: no top-p; with both off nothing is armed and
 * the call is the plain sampled call, same kernels included. top_p must be finite
 * with 0 < top_p <= 1, else a negative status at once. A translate call that finds
 * truncation armed but no sampling armed fails with a negative status and a
 * message; it still consumes the setting.
 *
 * One drawn step: a step of a sentence that is NOT forced at that step. l_c are the
 * output layer's logits over its N columns, inv_T = 1.0f / temperature and
 * z_c = l_c * inv_T one float32 product.
 *  1. A column is valid if z_c is not NaN; n_valid is their count. With
 *     n_valid == 0 nothing is kept: class 0 and score NaN, the arg-max's "none" rule.
 *  2. Top-k. top_k == 0 or top_k >= n_valid: tau_k = -inf. Otherwise tau_k is the
 *     top_k-th largest valid z. K1 = {valid c : z_c >= tau_k} by float comparison:
 *     ties at the threshold are all kept (K1 may hold more than top_k columns), and
 *     the set depends on values alone, never on column order.
 *  3. Top-p (skipped when top_p == 1). M is the maximum valid z and
 *     w_c = tr_weight(z_c, M) for c in K1 (slimt_amd/csrc/truncation.h), an integer
 *     in [0, 2^24]: 2^24 if z_c == M (tested first, so M = +-inf never evaluates
 *     inf - inf), else 0 if d = z_c - M <= -17.0f, else
 *     (uint32_t)(tr_exp(d) * 16777216.0f), tr_exp an exponential with the same bits
 *     on host and device. Q = sum over K1 of w_c as uint64. tau_p is the largest
 *     value v among {z_c : c in K1} such that
 *       (double)(sum of w_c over c in K1 with z_c >= v) >= (double)top_p * (double)Q
 *     (one IEEE double product; both sides exact integers below 2^53).
 *     K = {c in K1 : z_c >= tau_p}: ties at the boundary are kept, and K always
 *     holds the maximal columns. Without top-p, K = K1.
 *  4. The token is the vocabulary id of the FIRST maximum over c in K of
 *     key_c = fmaf(l_c, inv_T, g(k_b, t, y_c)) as in slimt_hip_ctx_set_sampling:
 *     start value -FLT_MAX, strict >, the lowest column wins a tie, and "logit 0 is
 *     NaN -> class 0" holds.
 *  5. The score is log softmax of z over K at the drawn column:
 *     forced_score(sum over K of exp(z_c - M), z_token - M, none)
 *     (slimt_amd/csrc/scores.h). A row whose logits hold a NaN anywhere, kept or
 *     not, scores NaN.
 * Forced steps (slimt_hip_ctx_set_target_prefix) draw nothing, so nothing is
 * truncated: they are recorded, fed and scored over the WHOLE layer at the
 * temperature, as in an untruncated sampled call. A forced token outside the layer
 * scores -inf (or NaN) either way.
 * A sentence's truncated translation depends on its key, the temperature, top_k and
 * top_p and on nothing else: not on its row, its neighbours, the decode mode, the
 * entry point or the shortlist's layout.
 * Execution: the threshold needs the whole row before the draw, and the persistent
 * decoder never stores logits. A truncated call therefore DECODES with the per-stage
 * kernels (as decode mode 1 does, K/V cache format 3 included) whatever mode the
 * context is in, with the logits gemm storing the row and one selection kernel
 * (slimt_amd/csrc/sample_truncate.hip) per step; its encoder is the one the
 * context's mode chooses. The context's mode itself is not changed, and
 * slimt_hip_ctx_plan, which does not know about armed settings, keeps reporting it.
 * The _many_ entry points do not merge a truncated call: it is translated batch by
 * batch, in order, on the same stream, each batch within its own step limit. */
int slimt_hip_ctx_set_sampling_truncation(slimt_hip_ctx *ctx, uint32_t top_k, float top_p);
/* Which kernels a translate call with source length S would use in the current
 * mode: *encoder_fused / *decoder_fused = 1 for the persistent kernels, 0 for
 * the per-stage ones. */
int slimt_hip_ctx_plan(const slimt_hip_ctx *ctx, size_t S, int *encoder_fused,
                       int *decoder_fused);

/* Model::forward (Model.cc:187-204) = embed + Encoder::forward + the greedy
 * loop of Model::decode (Model.cc:111-185). Host buffers.
 *  src_ids  [B,S] padded token ids, lengths [B]
 *  shortlist sorted unique target ids (Shortlist.cc:115-175), n_shortlist == 0
 *            => full vocabulary (Transformer.cc:181)
 *  out_ids  [B,Tmax], Tmax = max(1, (size_t)(limit_factor * S)): the first step is
 *           unconditional, the loop then runs while i < limit_factor * S (Model.cc:144-161)
 *  out_len  [B] tokens recorded per sentence, EOS included (Model.cc:127-137)
 *  align    nullable [B,Tmax,S]: row t = attention of head 0 of the LAST
 *           decoder layer over the first lengths[b] keys (Model.cc:84-108) */
int slimt_hip_translate(slimt_hip_ctx *ctx, const uint32_t *src_ids,
                        const uint32_t *lengths, size_t B, size_t S,
                        const uint32_t *shortlist, size_t n_shortlist,
                        float limit_factor, uint32_t eos_id, uint32_t *out_ids,
                        uint32_t *out_len, float *align);
/* Same without the final wait: the work is queued on the ctx stream and the call
 * returns; slimt_hip_ctx_synchronize(ctx) waits for it. Every buffer must stay
 * valid (and unchanged) until then, and should be pinned (slimt_hip_host_alloc):
 * with src_ids, lengths, out_ids, out_len (and align) all pinned the persistent
 * kernels read and write them in host memory themselves and no copy is queued at
 * all; otherwise H2D / D2H copies bracket the kernels (and asynchronous copies of
 * many contexts queue behind each other's kernels). The shortlist is uploaded
 * only when it differs from the previous call's. One call in flight per ctx: a
 * worker that wants to assemble its next batch while this one runs uses two
 * contexts (host/Service.cc). */
int slimt_hip_translate_async(slimt_hip_ctx *ctx, const uint32_t *src_ids,
                              const uint32_t *lengths, size_t B, size_t S,
                              const uint32_t *shortlist, size_t n_shortlist,
                              float limit_factor, uint32_t eos_id,
                              uint32_t *out_ids, uint32_t *out_len, float *align);
/* Pinned (page-locked) host memory for the staging buffers of the call above. */
int slimt_hip_host_alloc(size_t bytes, void **out);
int slimt_hip_host_free(void *p);
/* Same with every buffer already resident in device memory; asynchronous on
 * the ctx stream when `steps_hint` > 0 (runs exactly that many decode steps,
 * no early-exit read-back), otherwise syncs every few steps to stop as soon
 * as every sentence has emitted EOS.
 * Wait for an asynchronous call with slimt_hip_ctx_synchronize(ctx), not on the
 * stream yourself: a bounded wait INSIDE the launches (the in-launch shortlist
 * hand-over, the cluster logits' hand-overs) that ran out is reported through a
 * word only that function reads and clears -- it then fails with the reason, and
 * the batch's outputs must be discarded. A caller that waits on the stream alone
 * sees rc 0 for such a batch and the error on the NEXT call that does synchronise
 * through the library. */
/* Device arrays cannot be checked by the host: a token or shortlist id >= the vocabulary reads the table's last
 * row instead of faulting -- that sentence's result is undefined (as in the reference, which does not check
 * either), the other sentences' results are not affected. A target prefix
 * (slimt_hip_ctx_set_target_prefix) in device memory is not checked either: a length
 * past Tmax is taken as Tmax, and a prefix id >= the vocabulary leaves that
 * sentence's result undefined and no other sentence's. The row_src of
 * slimt_hip_translate_fanout_device is not checked either: a value >= B is taken
 * as B - 1, which leaves that row's result undefined and no other row's. */
int slimt_hip_translate_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids,
                               const uint32_t *d_lengths, size_t B, size_t S,
                               const uint32_t *d_shortlist, size_t n_shortlist,
                               float limit_factor, uint32_t eos_id,
                               uint32_t *d_out_ids, uint32_t *d_out_len,
                               float *d_align, int steps_hint);

/* ---- several batches in one launch pair -----------------------------------
 * What `workers` concurrent Model::forward calls are in the reference (Async,
 * slimt/Frontend.cc:207-227, each worker translating the batch the Batcher hands
 * it, Batcher.cc:95-120): n batches, each with its own padded source length (at
 * most S, the launch's), its own arrays, its own shortlist and its own outputs,
 * translated by ONE encoder and ONE decoder launch on ctx's stream. A batch padded
 * to fewer tokens than the launch keeps ITS length's step limit and alignment
 * width (Model.cc:159-161, 84-108); the extra positions are padding like any
 * other (masked keys of weight exactly 0, Input.cc:49-63). The reference's default batch is 1024
 * padded tokens (Frontend.hh:21-39: 32 sentences of 32 tokens) -- one such batch
 * per launch pair occupies 2 of 256 CUs in the decoder; merged, k of them fill
 * what one batch of k x B would. Every sentence's arithmetic is independent of
 * its neighbours, so each batch's outputs equal those of its own
 * slimt_hip_translate* call bit for bit (tests/test_gpu_translate_many.py).
 *
 * The launch works on sum_j roundup(B_j, 32) "global" sentences (_rows below),
 * every one padded to the call's S: ctx must hold that many (max_batch) and that
 * many times S padded tokens.
 * Limits: n <= 8; the persistent kernels for sources of up to 64 tokens. Whatever
 * cannot be merged (more batches, longer sources, decode modes 1 / 6, K/V cache
 * format 3) is translated batch by batch, in order, on the same stream: same
 * results, same asynchrony. Batches that give the SAME shortlist pointer and
 * size share one packed output layer. */
typedef struct slimt_hip_batch {
  const uint32_t *src_ids;   /* [B][S] */
  const uint32_t *lengths;   /* [B]; a device length past this batch's own S is that S (host lengths past it: an error) */
  size_t B;
  size_t S;                  /* this batch's padded length, <= the call's S; 0 = the call's S */
  const uint32_t *shortlist; /* sorted unique target ids, or NULL with n_shortlist == 0: full vocabulary */
  size_t n_shortlist;
  uint32_t *out_ids;         /* [B][Tmax], Tmax = max(1, (size_t)(limit_factor * S)), S = this batch's */
  uint32_t *out_len;         /* [B] */
  float *align;              /* nullable [B][Tmax][S] */
} slimt_hip_batch;

/* global sentences a merged launch of these batch sizes occupies in its context */
size_t slimt_hip_translate_many_rows(const size_t *B, size_t n_batches);
/* every array (shortlists included) resident in device memory; steps_hint as for _translate_device */
int slimt_hip_translate_many_device(slimt_hip_ctx *ctx, const slimt_hip_batch *batches, size_t n_batches,
                                    size_t S, float limit_factor, uint32_t eos_id, int steps_hint);
/* host arrays, asynchronous like _translate_async (slimt_hip_ctx_synchronize waits): ids, lengths and
 * outputs should be pinned (slimt_hip_host_alloc) -- the kernels then read and write them in place;
 * batches whose arrays are not are translated one by one through _translate_async. The shortlists
 * are host arrays; the merged path needs them to be ONE array (or none) for all batches. */
int slimt_hip_translate_many_async(slimt_hip_ctx *ctx, const slimt_hip_batch *batches, size_t n_batches,
                                   size_t S, float limit_factor, uint32_t eos_id);

/* Step-wise mirrors for parity tests ------------------------------------- */
/* Model.cc:195-201: embed + Encoder::forward (Transformer.cc:57-69). Keeps
 * the encoder output in the ctx for slimt_hip_decode_*. enc_out nullable
 * host [B,S,D]; layer_out nullable host [Le,B,S,D] (every layer's output);
 * embed_out nullable host [B,S,D]. */
int slimt_hip_encode(slimt_hip_ctx *ctx, const uint32_t *src_ids,
                     const uint32_t *lengths, size_t B, size_t S,
                     float *embed_out, float *layer_out, float *enc_out);
/* Decoder::start_states (Transformer.cc:78-85) + per-batch setup (cross
 * attention K/V, shortlist gather). */
int slimt_hip_decode_begin(slimt_hip_ctx *ctx, const uint32_t *shortlist,
                           size_t n_shortlist);
/* Decoder::step (Transformer.cc:120-183). prev == NULL => first step.
 * logits host [B,N] (N = n_shortlist or vocab), attn nullable host [B,H,S]
 * (last decoder layer), states nullable host [Ld,B,D] (SSRU cells after the
 * step). */
int slimt_hip_decode_step(slimt_hip_ctx *ctx, const uint32_t *prev,
                          float *logits, float *attn, float *states);

/* The same three steps with the reference's own ARGUMENTS, for the class-level
 * mirror (host/Transformer.hh): Encoder::forward takes the transformed embedding
 * and the mask (Transformer.cc:57-69), Decoder::step takes encoder_out, mask and
 * the caller's states on every call (Transformer.cc:120-183).
 * _encode_embedded: embedding host [B,S,D] (after transform_embedding), lengths
 *   [B] (= the mask: the first lengths[b] keys are tokens) -> enc_out host [B,S,D].
 *   Always the per-stage kernels (the persistent encoder starts from token ids).
 * _decode_begin_from: like _decode_begin for an encoder output handed in from
 *   the host (uploads it, computes the cross-attention K/V, gathers the shortlist).
 * _decode_step_states: like _decode_step, but the SSRU cells are the caller's:
 *   states_in [Ld,B,D] is uploaded first, states_out receives them after the step. */
int slimt_hip_encode_embedded(slimt_hip_ctx *ctx, const float *embedding,
                              const uint32_t *lengths, size_t B, size_t S,
                              float *enc_out);
int slimt_hip_decode_begin_from(slimt_hip_ctx *ctx, const float *encoder_out,
                                const uint32_t *lengths, size_t B, size_t S,
                                const uint32_t *shortlist, size_t n_shortlist);
int slimt_hip_decode_step_states(slimt_hip_ctx *ctx, const uint32_t *prev,
                                 const float *states_in, float *logits,
                                 float *attn, float *states_out);

/* ---- lexical shortlist (next row f3: slimt/Shortlist.{hh,cc}) --------------
 * Replaces ShortlistGenerator (Shortlist.hh:38-90): _create = the constructor's
 * load() over the binary shortlist blob (Shortlist.cc:41-104; layout
 * Shortlist.hh:77-84), _generate = generate() (Shortlist.cc:115-175) as Model::
 * forward calls it per batch on Input::words() (Model.cc:117-120, Input.cc:24).
 * The blob is copied to the device; the caller keeps ownership of `blob`.
 * check != 0 also verifies the header checksum (Shortlist.cc:66-76). Offsets and
 * ids are always range-checked at load (out-of-range data is undefined
 * behaviour in the reference; here it is rejected). */
typedef struct slimt_hip_shortlist slimt_hip_shortlist;
int slimt_hip_shortlist_create(const void *blob, size_t blob_size, size_t source_vocab,
                               size_t target_vocab, int shared, int check, int device,
                               slimt_hip_shortlist **out);
int slimt_hip_shortlist_destroy(slimt_hip_shortlist *sl);
/* header fields (Shortlist.cc:78-81) */
int slimt_hip_shortlist_info(const slimt_hip_shortlist *sl, uint64_t *frequent, uint64_t *best);
/* Threading: a handle may be shared by any number of threads, like the reference's
 * const generate() on one shared generator (Model.cc:117-120). _generate stages
 * through buffers of the handle and serialises its callers internally;
 * _generate_device / slimt_hip_translate_device_generated only read the handle and
 * use the calling context's scratch and stream, so they run concurrently (one
 * context per thread, as everywhere).
 * Host arrays: src_ids [B][S] padded rows, lengths [B] (only the first lengths[b]
 * tokens of a row are words). out_ids: capacity >= target_vocab; *n_out = number
 * of ids written (sorted, unique, a multiple of 8 when enough ids are free). */
int slimt_hip_shortlist_generate(slimt_hip_shortlist *sl, const uint32_t *src_ids,
                                 const uint32_t *lengths, size_t B, size_t S, uint32_t *out_ids,
                                 size_t *n_out);
/* Device arrays, asynchronous on ctx's stream (d_out_ids: capacity >=
 * target_vocab uint32, d_n_out: one uint32), e.g. ahead of
 * slimt_hip_translate_device on the same context. */
int slimt_hip_shortlist_generate_device(slimt_hip_shortlist *sl, slimt_hip_ctx *ctx,
                                        const uint32_t *d_src_ids, const uint32_t *d_lengths,
                                        size_t B, size_t S, uint32_t *d_out_ids,
                                        uint32_t *d_n_out);

/* Model::forward with its shortlist step on the device (Model.cc:117-120,195-203):
 * generates the batch's lexical shortlist on ctx's stream, then translates with
 * it. With the persistent kernels nothing returns to the host in between (the
 * shortlist's size stays on the device: three launches in all, asynchronous like
 * slimt_hip_translate_device); with the stage kernels one 4-byte read-back sizes
 * the launches. The shortlist's target vocabulary must be the model's. */
int slimt_hip_translate_device_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                         const uint32_t *d_src_ids, const uint32_t *d_lengths,
                                         size_t B, size_t S, float limit_factor, uint32_t eos_id,
                                         uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align,
                                         int steps_hint);

/* The same on HOST buffers -- Model::forward as the reference's workers call it (Model.cc:111-204),
 * shortlist step included: _translate_generated waits for the result, _translate_async_generated
 * queues the work on ctx's stream like slimt_hip_translate_async (same buffer rules: with every
 * array pinned the kernels read ids / lengths from, and write tokens, lengths and alignment rows to,
 * host memory themselves; nothing is copied, nothing synchronises, and no host shortlist exists at
 * all). A handle may be shared by every context of its device. */
int slimt_hip_translate_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                  const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                  float limit_factor, uint32_t eos_id, uint32_t *out_ids,
                                  uint32_t *out_len, float *align);
int slimt_hip_translate_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                        const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                        size_t S, float limit_factor, uint32_t eos_id,
                                        uint32_t *out_ids, uint32_t *out_len, float *align);

/* Several batches in one launch pair (slimt_hip_translate_many_* above) with every batch's OWN lexical shortlist, generated from its source words inside the encoder launch
 * (Model.cc:117-120 per batch; slimt_hip_translate_*_generated below): the first n workgroups to start each
 * generate one batch's list and publish it, every workgroup packs its share of the n output layers at the end of
 * its encoder work. batches[].shortlist / n_shortlist are ignored. Falls back batch by batch like the others
 * (also when the generator's bitmaps do not fit the encoder's LDS). */
int slimt_hip_translate_many_device_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const slimt_hip_batch *batches,
                                              size_t n_batches, size_t S, float limit_factor, uint32_t eos_id, int steps_hint);
int slimt_hip_translate_many_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const slimt_hip_batch *batches,
                                             size_t n_batches, size_t S, float limit_factor, uint32_t eos_id);

/* ---- teacher-forced scoring: every target position in one pass ------------- */
/* Scores GIVEN targets tgt_ids [B][T] with lengths tgt_len [B] (n_b = tgt_len[b] <= T) against a source batch, and
 * optionally aligns them. With the targets known the decoder is position-parallel: the B x T rows go through the
 * decoder weights as one tall batch (the SSRU is an elementwise scan over t; everything else is row-wise), where the
 * forced-prefix path (slimt_hip_ctx_set_target_prefix) runs the persistent decoder step by step. For every t < n_b:
 *   - row (b, t)'s decoder input is the zero embedding at t = 0, else tgt_ids[b][t - 1] at position 0;
 *   - scores[b][t] is the natural-log softmax probability of tgt_ids[b][t] over the output layer (the shortlist's
 *     columns, or the full vocabulary when n_shortlist == 0), as slimt_hip_ctx_set_scores defines it: -inf for a token
 *     the layer does not hold (it is still fed to row t + 1), NaN for a row whose logits hold a NaN;
 *   - align[b][t][j], j < lengths[b] (align nullable, [B][T][S]), is head 0 of the last decoder layer (Model.cc:84-108).
 * Nothing stops at EOS: an EOS inside the target is a token like any other. Through the first EOS, and for n_b <=
 * max(1, limit_factor * S), the results are those of the forced-prefix call with the same prefix. There is no such cap
 * here: T is the caller's. Entries with t >= n_b and alignment columns j >= lengths[b] are NOT written.
 * Arithmetic: the PORTABLE contract; every hidden row and alignment row equals the step-wise decoder's bit for bit, and
 * a sentence's results do not depend on its place in the batch or on the batch around it.
 * The K/V cache format (slimt_hip_model_set_kv_cache_format) concerns the persistent decoder's packed cache only: these
 * calls always attend over the f32 float(accS) cache in the hoisted order. A model set to format 3 (the literal order)
 * is REFUSED with a message, not scored in another order.
 * Score calls are not translate calls: options armed with slimt_hip_ctx_set_scores / _set_target_prefix / _set_sampling
 * are neither used nor consumed by them.
 * Limits: B <= max_batch, S <= max_source_length, which is itself at most 128 (slimt_hip_ctx_create; the scoring attention
 * keeps two keys per lane, so S <= 128 is also the scoring kernels' own limit), 1 <= T <= 65536, B * T <= 2^24. The
 * workspace for the rows (18 D + F + 4 bytes each) is allocated on a context's first scoring call and grows when a later call needs more (the
 * context is synchronised before the old block is freed); rows are processed in chunks of whole sentences of at most
 * max(T, 8192) rows, and results do not depend on the chunking.
 * slimt_hip_score waits for the result. slimt_hip_score_async queues the work on ctx's stream: pinned ids / lengths /
 * targets are read in place and pinned scores written in place; other arrays are bracketed by copies on the stream (the
 * copies back restore what the call does not write) and must stay valid until slimt_hip_ctx_synchronize. Host entry points
 * check lengths[b] <= S, tgt_len[b] <= T and every id (source, target below tgt_len, shortlist) against the vocabulary.
 * slimt_hip_score_device takes device pointers and is asynchronous on ctx's stream; device arrays cannot be checked: a
 * tgt_len[b] > T is taken as T, a lengths[b] > S as S, and an id past the embedding table reads its last row (that
 * sentence alone is undefined). slimt_hip_score_async_generated generates the batch's lexical shortlist on the device
 * first (one 4-byte read-back sizes the output layer, as with the stage kernels of _translate_generated). */
int slimt_hip_score(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                    const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids, const uint32_t *tgt_len,
                    size_t T, float *scores, float *align);
int slimt_hip_score_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                          const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                          const uint32_t *tgt_len, size_t T, float *scores, float *align);
int slimt_hip_score_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths, size_t B, size_t S,
                           const uint32_t *d_shortlist, size_t n_shortlist, const uint32_t *d_tgt_ids,
                           const uint32_t *d_tgt_len, size_t T, float *d_scores, float *d_align);
int slimt_hip_score_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist, const uint32_t *src_ids,
                                    const uint32_t *lengths, size_t B, size_t S, const uint32_t *tgt_ids,
                                    const uint32_t *tgt_len, size_t T, float *scores, float *align);

/* ---- alternatives of a score call: the k best tokens and the target's rank at every position ---- */
/* Arms the NEXT score call of ctx (slimt_hip_score, _score_async, _score_device or _score_async_generated) to report, for
 * every row (b, t) with t < n_b, what the model would have said instead and how far down its list the given token is.
 * k = 0 disarms. k > SLIMT_HIP_MAX_ALTERNATIVES is refused at once, and so is alt_ids == NULL with k > 0. The next score
 * call takes the setting, WHATEVER ITS OUTCOME (a refused call included), and disarms it. Translate calls neither take
 * nor clear it, and what slimt_hip_ctx_set_scores / _set_target_prefix / _set_sampling armed stays armed, as for every
 * score call. alt_ids [B][T][k], alt_scores [B][T][k] (nullable) and rank [B][T] (nullable) are of the SAME KIND as that
 * call's scores: host memory for slimt_hip_score, pinned or pageable host memory -- all three like scores -- for the
 * asynchronous host calls (pinned arrays are written in place; pageable ones are bracketed by copies on the stream, the
 * copy down first, so that entries the pass does not write survive), device memory for slimt_hip_score_device. A call
 * whose arrays are of another kind is refused with a message. A context's first armed call with pageable arrays
 * allocates their device staging ((2 k + 1) B T words, grown when a later call needs more); no other context pays it.
 *
 * For a row (b, t), t < n_b, take the output layer's N columns (the shortlist's, or the vocabulary's) with the logits l_c
 * the scorer forms, float(acc + 127 colsum) * u + pb:
 *   - the VALID columns are those with a non-NaN logit;
 *   - the ORDER is descending l_c compared as floats (+0 equals -0, infinities order like any value), ties to the
 *     ascending column: the greedy arg-max's first-maximum rule continued;
 *   - alt_ids[b][t][i] is the vocabulary id of the i-th valid column in that order; positions i >= the number of valid
 *     columns hold 0xFFFFFFFF. Padding columns of the layer's last 16-column tile never appear;
 *   - alt_scores[b][t][i] = forced_score(s, l_c - m, none) with the row's own final (m, s), the pair behind scores[b][t]
 *     in the same merge order: the natural-log softmax probability of that column. A row holding a NaN logit gives NaN
 *     scores while its ids are still the order of its valid columns; positions past the valid columns hold -inf;
 *   - rank[b][t] is the number of valid columns ordered strictly before the target's column, 0xFFFFFFFF when the target
 *     is not in the layer or its logit is NaN. Hence rank < k  <=>  alt_ids[b][t][rank] == tgt_ids[b][t], and then
 *     alt_scores[b][t][rank] has the BITS of scores[b][t].
 * Entries with t >= n_b are NOT written. scores and align of an armed call are bit-identical to the unarmed call's, and
 * no result depends on where a sentence sits in the batch or on the row chunking. A model set to K/V cache format 3 is
 * refused, as by every score call. */
#define SLIMT_HIP_MAX_ALTERNATIVES 8
int slimt_hip_ctx_set_score_alternatives(slimt_hip_ctx *ctx, uint32_t k, uint32_t *alt_ids, float *alt_scores,
                                         uint32_t *rank);


/* ---- candidates: several target rows per source from one encoding ---------- */
/* The score calls above with N candidate targets tgt_ids [N][T] / tgt_len [N] over a source batch src_ids [B][S] /
 * lengths [B]: cand_src [N] names each candidate's source, cand_src[c] < B. The B sources are encoded ONCE and the N
 * candidates go through the tall pass; scores [N][T] and the nullable align [N][T][S] are indexed by candidate.
 * THE CONTRACT: for candidate c and t < n_c = min(tgt_len[c], T), every value written is bit for bit what slimt_hip_score
 * writes for row c when called on the duplicated batch src_ids[cand_src], lengths[cand_src] with the same targets and
 * output layer (alignment columns j < lengths[cand_src[c]]); nothing else is written. It holds because every row's
 * arithmetic is independent of its neighbours.
 * cand_src may be in ANY order; a source may have no candidate and a candidate may be empty (n_c = 0). The order affects
 * speed only: the attention keeps one source's K / V staged for a run of SLIMT_HIP_CANDIDATE_RUN consecutive candidates
 * and restages when the next live candidate names another source, so candidates sorted by source cost least.
 * The context bounds B (max_batch), S and B * S only; N is bounded by 1 <= T <= 65536 and N * T <= 2^24, and everything
 * sized by N (the row workspace, the staging of pageable targets, scores, alignments and alternatives) grows on demand.
 * N = 0 is a successful call that writes nothing. Rows are chunked in whole candidates of at most max(T, 8192) rows.
 * Host calls check cand_src[c] < B, tgt_len[c] <= T and every id, and refuse with a message; pinned arrays are read and
 * written in place, pageable ones bracketed by copies (the copy down first), as for slimt_hip_score_async. Device
 * arrays cannot be checked: a cand_src[c] >= B is taken as B - 1 and a length past T as T (that candidate alone is
 * undefined; nothing is read or written out of bounds).
 * A candidate call IS a score call: it takes and disarms slimt_hip_ctx_set_score_alternatives (the arrays are then
 * [N][T][k], [N][T][k] and [N][T]), leaves translate options armed, and refuses K/V cache format 3. */
#define SLIMT_HIP_CANDIDATE_RUN 2
int slimt_hip_score_candidates(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                               const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                               const uint32_t *tgt_len, size_t T, const uint32_t *cand_src, size_t N, float *scores,
                               float *align);
int slimt_hip_score_candidates_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                     size_t S, const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                                     const uint32_t *tgt_len, size_t T, const uint32_t *cand_src, size_t N,
                                     float *scores, float *align);
int slimt_hip_score_candidates_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths, size_t B,
                                      size_t S, const uint32_t *d_shortlist, size_t n_shortlist,
                                      const uint32_t *d_tgt_ids, const uint32_t *d_tgt_len, size_t T,
                                      const uint32_t *d_cand_src, size_t N, float *d_scores, float *d_align);
int slimt_hip_score_candidates_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                               const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                               const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T,
                                               const uint32_t *cand_src, size_t N, float *scores, float *align);

/* Ranks the candidates of each source by their scores [N][T] (as a candidate call wrote them):
 *   - totals[c] is the f32 sum of scores[c][t] over t < n_c = min(tgt_len[c], T), accumulated in ascending t from +0.0f
 *     with one f32 add per term (a host loop reproduces the bits; -inf and NaN propagate); n_c = 0 gives 0.0f;
 *   - key_c = totals[c] (mode 0, sum) or totals[c] / (float)n_c (mode 1, mean per token: one IEEE division); any other
 *     mode is refused;
 *   - best[b] is the lowest c with cand_src[c] == b, n_c > 0 and key_c not NaN whose key is >= every other such key,
 *     keys compared as floats (+0 equals -0; -inf competes and loses to anything finite); 0xFFFFFFFF when the source has
 *     no such candidate.
 * The result does not depend on the order of cand_src or on scheduling. totals [N] f32, best [B] u32; B >= 1, T >= 1,
 * N * T <= 2^24; N = 0 writes best only. slimt_hip_candidates_rank takes host pointers, is stateless and waits (it
 * refuses a cand_src[c] >= B and a tgt_len[c] > T); slimt_hip_candidates_rank_device runs on ctx's stream over device
 * arrays, e.g. behind slimt_hip_score_candidates_device without a host round trip (values it cannot check are clamped
 * as by that call). */
int slimt_hip_candidates_rank(const float *scores, const uint32_t *tgt_len, const uint32_t *cand_src, size_t N, size_t T,
                              size_t B, int mode, float *totals, uint32_t *best);
int slimt_hip_candidates_rank_device(slimt_hip_ctx *ctx, const float *d_scores, const uint32_t *d_tgt_len,
                                     const uint32_t *d_cand_src, size_t N, size_t T, size_t B, int mode, float *d_totals,
                                     uint32_t *d_best);

/* ---- fan-out: several decoder rows per source from one encoding ------------ */
/* slimt_hip_translate with N decoder rows over a source batch src_ids [B][S] / lengths [B]: row_src [N] names each
 * row's source, row_src[r] < B. The B sources are encoded ONCE, their cross-attention K / V are projected and cached
 * once, and the N rows decode step by step over them -- n samples of a sentence (slimt_hip_ctx_set_sampling) without
 * repeating its row n times. out_ids [N][Tmax], out_len [N] and the nullable align [N][Tmax][S] are indexed by row; Tmax
 * follows slimt_hip_translate's rule from S.
 * The options armed on the context apply as to a call of one batch of N rows: scores [N][Tmax], prefix ids [N][Tmax] and
 * lengths [N], keys [N] (NULL: row r's key is r); truncation applies as to any sampled call. A fan-out call consumes
 * what was armed whether it succeeds or fails, like every translate call.
 * THE CONTRACT: for every row r, every value written -- tokens, out_len, alignment rows, scores -- is bit for bit what
 * slimt_hip_translate in decode mode 1 writes for row r of the duplicated batch src_ids[row_src], lengths[row_src] with
 * the same shortlist ids and the same per-row options: greedy, scored, forced, sampled, truncated, sampled + forced. It
 * holds because every row's arithmetic is independent of its neighbours.
 * row_src may be in ANY order and a source may have no row. The order affects speed only: the attention stages a
 * source's K / V once per run of consecutive rows that name it (within 16 rows), so rows sorted by source cost least.
 * A fan-out call decodes with the per-stage kernels whatever the context's decode mode, which is not changed
 * (slimt_hip_ctx_plan keeps reporting it; the mode still chooses the encoder); K/V cache format 3 works. Merged launches
 * (slimt_hip_translate_many_*) of fan-out calls do not exist.
 * Bounds: B <= max_batch, B * S within the context's padded tokens, and 1 <= N <= max_batch -- the per-row decoder
 * workspaces (states, step rows, partials) are sized by max_batch when the context is created.
 * Host calls check every id and length as slimt_hip_translate does, and refuse N = 0 and a row_src[r] >= B with a
 * message; _async queues the work like slimt_hip_translate_async (pinned or pageable buffers; copies bracket the kernels).
 * _device takes device pointers like slimt_hip_translate_device (steps_hint as there); device arrays cannot be checked:
 * a row_src[r] >= B is taken as B - 1 (that row alone is undefined; nothing is read or written out of bounds).
 * _async_generated generates the lexical shortlist from the B sources GIVEN: a source without rows still contributes its
 * words to it. */
int slimt_hip_translate_fanout(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                               const uint32_t *row_src, size_t N, const uint32_t *shortlist, size_t n_shortlist,
                               float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *align);
int slimt_hip_translate_fanout_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                     size_t S, const uint32_t *row_src, size_t N, const uint32_t *shortlist,
                                     size_t n_shortlist, float limit_factor, uint32_t eos_id, uint32_t *out_ids,
                                     uint32_t *out_len, float *align);
int slimt_hip_translate_fanout_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths, size_t B,
                                      size_t S, const uint32_t *d_row_src, size_t N, const uint32_t *d_shortlist,
                                      size_t n_shortlist, float limit_factor, uint32_t eos_id, uint32_t *d_out_ids,
                                      uint32_t *d_out_len, float *d_align, int steps_hint);
int slimt_hip_translate_fanout_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                               const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                               const uint32_t *row_src, size_t N, float limit_factor, uint32_t eos_id,
                                               uint32_t *out_ids, uint32_t *out_len, float *align);

/* ---- consensus: minimum-Bayes-risk pick among each source's rows ---------- */
/* Of the rows ids [N][T] u32 with lengths len [N] that row_src [N] assigns to B sources (n samples of a sentence, as a
 * fan-out call returns them), keeps for each source the row that agrees most with the source's other rows: the token
 * n-gram F score (chrF's formula over token ids). Integer counts and IEEE doubles in a fixed order: host and device agree
 * bit for bit. With n_c = min(len[c], T), G = max_order in 1..SLIMT_HIP_CONSENSUS_MAX_ORDER and the integer
 * beta2 = beta^2 in 1..SLIMT_HIP_CONSENSUS_MAX_BETA2 (4: chrF's beta = 2; 1: the balanced F):
 *   - the g-grams of row c are the sequences ids[c][p .. p + g) for p <= n_c - g; there are c_g(c) = max(n_c - g + 1, 0);
 *   - M_g(h, r) = the sum over the distinct g-grams x of min(count of x in h, count of x in r): clipped counts, symmetric.
 *     Tokens are compared as full 32-bit ids;
 *   - F_g(h, r) = ((1 + beta2) * M_g) / (beta2 * c_g(r) + c_g(h)): both sides exact integers converted to double, one IEEE
 *     division; an order with c_g(h) = c_g(r) = 0 is skipped;
 *   - U(h, r) = (F_1 + F_2 + ... over the counted orders, added in ascending g from +0.0) / (the number of counted orders),
 *     0.0 when no order counts;
 *   - a row COMPETES when n_c > 0; the references of a competing row h are the other competing rows of its source;
 *   - utility[h] = (the sum of U(h, r) over h's references in ascending row index, added from +0.0) / (their number); 0.0
 *     when h has no reference and for a row that does not compete. No NaN arises;
 *   - best[b] is the lowest competing row h of source b whose utility is >= every other competing row's; 0xFFFFFFFF when the
 *     source has no competing row.
 * Rows may name sources in any order: the result depends on the row order only through the two "ascending / lowest row
 * index" rules. utility [N] f64, best [B] u32. Bounds: B >= 1, 1 <= T <= SLIMT_HIP_CONSENSUS_MAX_T, N <= 65536, at most
 * SLIMT_HIP_CONSENSUS_MAX_ROWS rows per source (a source's tokens then fit 64 KiB of LDS). N = 0 writes best only.
 * slimt_hip_consensus_select takes host pointers, is stateless and waits; it refuses, with a message, a source with more
 * than SLIMT_HIP_CONSENSUS_MAX_ROWS rows, a row_src[c] >= B, a len[c] > T and a max_order or beta2 out of range.
 * slimt_hip_consensus_select_device runs on ctx's stream over device arrays, which it cannot check: a row_src[c] >= B is
 * taken as B - 1, a len[c] > T as T, and a source with more than SLIMT_HIP_CONSENSUS_MAX_ROWS rows gets best 0xFFFFFFFF and
 * utility 0.0 for its rows; nothing is read or written out of bounds. */
#define SLIMT_HIP_CONSENSUS_MAX_ORDER 4
#define SLIMT_HIP_CONSENSUS_MAX_BETA2 16
#define SLIMT_HIP_CONSENSUS_MAX_ROWS 64
#define SLIMT_HIP_CONSENSUS_MAX_T 256
int slimt_hip_consensus_select(const uint32_t *ids, const uint32_t *len, const uint32_t *row_src, size_t N, size_t T, size_t B,
                               int max_order, int beta2, double *utility, uint32_t *best);
int slimt_hip_consensus_select_device(slimt_hip_ctx *ctx, const uint32_t *d_ids, const uint32_t *d_len,
                                      const uint32_t *d_row_src, size_t N, size_t T, size_t B, int max_order, int beta2,
                                      double *d_utility, uint32_t *d_best);
/* A per-call option in the style of slimt_hip_ctx_set_scores: the NEXT fan-out call (slimt_hip_translate_fanout, _async,
 * _device, _async_generated) runs the selection over its own out_ids / out_len / row_src (T = its Tmax) on the device,
 * behind its last decode step, and writes best [B] and utility [N] beside its outputs -- arrays of the same kind as the
 * call's own outputs (host for the host calls, read after the call or slimt_hip_ctx_synchronize; device for _device).
 * Every other output of the call is bit for bit what the call writes without the option. The option is consumed by the next
 * translate call whatever its outcome; a translate call that is not a fan-out call fails with a message when it is armed.
 * max_order = 0 with both arrays NULL disarms (beta2 is then not looked at). Refused at once: max_order = 0 with an array
 * given, max_order or beta2 out of range, a NULL array. An armed fan-out call whose Tmax exceeds SLIMT_HIP_CONSENSUS_MAX_T is refused with a message. */
int slimt_hip_ctx_set_fanout_consensus(slimt_hip_ctx *ctx, int max_order, int beta2, uint32_t *best, double *utility);

/* ---- beam search with n-best output ---------------------------------------- */
/* slimt_hip_translate over B sources with `beam` = k slots per source, 1 <= k <= SLIMT_HIP_MAX_BEAM: a fan-out call of
 * B k decoder rows (row r = b k + s belongs to source b) whose every step ends in one selection. THE CONTRACT, which a
 * host checker reproduces bit for bit (slimt_amd/csrc/beam.h is host-compilable; every fused operation is an fmaf and
 * nothing else is contracted):
 * Arithmetic, for one decoder row with logits l_c over the output layer's N columns (the shortlist's, or the
 * vocabulary's) as the logits GEMM forms them:
 *   - the row is usable if no logit is NaN and its maximum M (-0 read as +0) is finite; an unusable row contributes no
 *     candidate;
 *   - weight bm_weight(l, M): 2^40 if l == M (tested first); else with d = l - M, 0 if d <= -28.0f; else
 *     (uint64_t)((double)tr_exp(d) * 1099511627776.0) (tr_exp: truncation.h);
 *   - Q is the sum of the row's weights as uint64 (exact in any order; below 2^60 for N < 2^20 -- an output layer of 2^20
 *     columns or more is refused) and L = sm_log((float)((double)Q * 0x1p-40)) (sm_log: sampling.h);
 *   - the column's score lp_c = (l_c - M) - L: two f32 subtractions, in this order.
 *   tr_exp on (-28, 0] is normal and monotone with relative error 8.3e-8 against float64; on random rows of 1 to 32,000
 *   columns lp is within 3.6e-6 of the float64 log-softmax where that is above -64 (tests/test_beam_checker.py measures
 *   both and asserts the project's score tolerance 5e-5).
 * Search. A slot is dead (flag 0), live (1) or finished (2) and carries a total C (f32). Before step 0, slot 0 is live
 * with C = +0.0f and the other slots are dead. Candidates at step t: for every live slot s with a usable row and every
 * column c, cand = C_s + lp_c (one f32 add), candidates equal to -inf dropped; for every finished slot, itself with
 * cand = C_s unchanged. Candidates are ordered by cand descending, compared as floats (+0 equals -0); then slot
 * ascending; then logit descending (as floats); then column ascending -- within one slot the arg-max's first-maximum
 * rule continued, and cand is monotone in the logit, so beam 1 is greedy decoding. The first k candidates become the new
 * slots 0..k-1 in that order, each with parent = the candidate's slot, token = the column's vocabulary id, token
 * score = lp_c and C = cand. A new slot whose token is EOS is finished with length t + 1; a carried finished slot keeps
 * its length and tokens; with fewer than k candidates the remaining slots are dead. A source is done when no slot is
 * live; the call runs until every source is done, or for Tmax steps (Tmax follows slimt_hip_translate's rule); a slot
 * still live at the end is reported with length Tmax and no EOS.
 * Output, n-best with n = k per source: out_ids [B][k][Tmax], out_len [B][k] (0 for a dead slot), totals [B][k] (C; -inf
 * for a dead slot), and the nullable token_scores [B][k][Tmax] and align [B][k][Tmax][S]. The k hypotheses are sorted by
 * key descending, ties to the lower final slot, dead slots last; the key is totals (length_mode 0) or
 * totals / (float)out_len (length_mode 1) -- the two modes of slimt_hip_candidates_rank; any other mode is refused.
 * Alignment row t of a hypothesis is the row the decoder computed at step t for the slot that hypothesis was extended
 * from (head 0 of the last layer over the source's lengths[b] keys). Entries at t >= out_len are not written by the
 * search (host calls and _device zero out_ids, out_len and align first, as slimt_hip_translate does; a host call's
 * token_scores come back 0 there). A source's result depends on the source, the output layer, k and the mode only: not
 * on its place in the batch or on its neighbours.
 * A beam call is a translate call: it consumes whatever is armed on the context, and is refused with a message if
 * scores, a prefix, sampling, truncation or consensus are armed. It decodes with the per-stage kernels whatever the
 * context's decode mode, like a fan-out call; K/V cache format 3 works. Bounds: B * beam <= max_batch (the per-row
 * workspaces are sized by it), B * S within the context's padded tokens. Host calls check ids and lengths as
 * slimt_hip_translate does; _async, _device (steps_hint as there: at most Tmax steps run) and _async_generated are as the
 * fan-out call's. */
#define SLIMT_HIP_MAX_BEAM 8
int slimt_hip_translate_beam(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S, int beam,
                             int length_mode, const uint32_t *shortlist, size_t n_shortlist, float limit_factor, uint32_t eos_id,
                             uint32_t *out_ids, uint32_t *out_len, float *totals, float *token_scores, float *align);
int slimt_hip_translate_beam_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                   int beam, int length_mode, const uint32_t *shortlist, size_t n_shortlist, float limit_factor,
                                   uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *totals, float *token_scores,
                                   float *align);
int slimt_hip_translate_beam_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths, size_t B, size_t S,
                                    int beam, int length_mode, const uint32_t *d_shortlist, size_t n_shortlist,
                                    float limit_factor, uint32_t eos_id, uint32_t *d_out_ids, uint32_t *d_out_len,
                                    float *d_totals, float *d_token_scores, float *d_align, int steps_hint);
int slimt_hip_translate_beam_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist, const uint32_t *src_ids,
                                             const uint32_t *lengths, size_t B, size_t S, int beam, int length_mode,
                                             float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len,
                                             float *totals, float *token_scores, float *align);
/* One selection of the search above over the caller's arrays: host pointers, stateless, waits. logits [B beam][N], ids [N]
 * (NULL: the column is the id), totals_in / flags_in [B beam] (a live slot's total finite, a finished one's not NaN;
 * the step-0 state is flags 1, 0, 0, ... and totals +0, -inf, -inf, ...). Writes, each [B beam]: parent (the slot within
 * the source), token, token_score, totals_out, flags_out. A carried finished slot has token 0xFFFFFFFF and token score
 * 0; a dead slot has parent and token 0xFFFFFFFF, token score 0, total -inf and flag 0. */
int slimt_hip_beam_step(const float *logits, size_t B, int beam, size_t N, const uint32_t *ids, const float *totals_in,
                        const uint32_t *flags_in, uint32_t eos_id, uint32_t *parent, uint32_t *token, float *token_score,
                        float *totals_out, uint32_t *flags_out);

/* ---- measurement --------------------------------------------------------- */
/* When enabled, HIP events bracket every launch of kernel family `kernel_id`
 * on the ctx stream; slimt_hip_profile_read returns the number of launches
 * and their summed duration since the last reset. */
enum {
  SLIMT_HIP_K_NONE = 0,
  SLIMT_HIP_K_GEMM_ENC = 1,    /* encoder projections (M = B*S rows)       */
  SLIMT_HIP_K_GEMM_DEC = 2,    /* decoder projections (M = B rows)         */
  SLIMT_HIP_K_LOGITS = 3,      /* output projection + fused argmax         */
  SLIMT_HIP_K_ATTN_ENC = 4,
  SLIMT_HIP_K_ATTN_DEC = 5,
  SLIMT_HIP_K_SSRU = 6,
  SLIMT_HIP_K_DECODE_FUSED = 7, /* persistent whole-loop decoder           */
  SLIMT_HIP_K_ENCODE_FUSED = 8, /* persistent whole-stack encoder          */
  SLIMT_HIP_K_CONSENSUS = 9,    /* consensus selection (one launch per call) */
  SLIMT_HIP_K_COUNT = 10
};
int slimt_hip_profile_enable(slimt_hip_ctx *ctx, int kernel_id);
int slimt_hip_profile_read(slimt_hip_ctx *ctx, uint64_t *launches,
                           double *total_ms, double *int8_macs,
                           double *weight_bytes);
int slimt_hip_profile_reset(slimt_hip_ctx *ctx);
/* Diagnostic: returns (into out[0..n), n <= 64) the 100 MHz wall-clock stamps
 * the persistent decoder's workgroup 0 wrote at its phase boundaries during
 * the previously selected step, then selects `step` for the next translate
 * call (step < 0 disables stamping). */
int slimt_hip_debug_decode_stamps(slimt_hip_ctx *ctx, int step, uint64_t *out,
                                  size_t n);
/* Diagnostic: the decoder's cross-attention proper (Modules.cc:24-86 as Attention::forward calls it,
 * Modules.cc:287-306) of decoder layer `layer` on the caller's projected queries yq [B][D], over
 * the f32 K/V cache of ctx's current batch (slimt_hip_decode_begin[_from] first): joined [B][D] =
 * the joined heads before the output projection, attn (nullable) [B][H][S] = the probabilities.
 * literal = 0: the hoisted order every decoder here runs; 1: the reference's literal sequence
 * (K/V cache format 3). Tests bound one against the other and both against the checker. */
int slimt_hip_debug_cross_attention(slimt_hip_ctx *ctx, int layer, int literal, const float *yq,
                                    float *joined, float *attn);
/* Diagnostic: break (broken != 0) or restore the hand-over of a shortlist generated inside the
 * encoder launch (slimt_hip_translate*_generated): the waiting workgroups then look for a
 * publication that never comes and give up after `poll_limit` polls (1..2^24; the default 2^24
 * is about two seconds). A waiter that gives up packs nothing and the context's next wait --
 * slimt_hip_ctx_synchronize, or the blocking translate calls -- FAILS: the batch's results are
 * not to be used. Tests use it to reach that path. */
int slimt_hip_debug_break_shortlist_handoff(slimt_hip_ctx *ctx, int broken, unsigned poll_limit);
/* Diagnostic: put ctx's launch bookkeeping where it would be after `value` tickets. Waits for ctx's
 * stream, then sets the device's decoder and encoder ticket counters and both halves of the 64-bit
 * XCD-affine claim word to `value`, the host's bases of all four to the same, the epoch of the
 * in-launch shortlist hand-over to `value`, and clears the hand-over's flags where they exist. The
 * counters run modulo 2^32, so results do not depend on it; tests start a context shortly before
 * 2^32 (and the epoch before its reserved 0xffffffff), which a loaded service reaches in a day. */
int slimt_hip_debug_ctx_set_counters(slimt_hip_ctx *ctx, uint32_t value);
/* Diagnostic: what ctx's shortlist buffer holds after a *_generated call: waits for ctx's stream, then for j < n_batches writes
 * counts[j] (the device's count of sub-batch j; j = 0 for an unmerged call) and the first min(counts[j], capacity) ids
 * of that list to ids + j * capacity. Reads only what the context has reserved; fails otherwise (n_batches not in 1..8,
 * or a context that has generated fewer lists). A count above the vocabulary is reported as it is and never followed.
 * Tests compare the lists generated inside an encoder launch with the reference's, id for id. */
int slimt_hip_debug_ctx_shortlists(slimt_hip_ctx *ctx, size_t n_batches, uint32_t *ids, size_t capacity, uint32_t *counts);
/* Diagnostic: which form each sentence-layer of ctx's last batch was cached in -- out[l * B + b],
 * 0 = 20-bit, 1 = 24-bit, 2 = 16-bit (the tight form); *batch = B, or 0 when the batch's caches
 * are all in one form (f32 or 24-bit: formats 1 / 2, a shape without the narrow form, or the
 * centres' calibration batch). Waits for ctx's stream. */
int slimt_hip_debug_kv_formats(slimt_hip_ctx *ctx, uint8_t *out, size_t n, size_t *batch);
/* Diagnostic: format 0's watch. The library counts the sentence-layers it cached (submitted) and those
 * that needed the 24-bit form (wide; updated by the device, a few batches behind); once more than one
 * in 32 did (after 1024 were submitted) the model caches every batch in the 24-bit form from then on
 * (*switched_to_24_bit = 1): a model whose accumulators do not fit 20 bits then runs at the 24-bit
 * form's own speed instead of through its per-sentence fallback. slimt_hip_model_set_kv_cache_format
 * and slimt_hip_debug_kv_narrow_limit start the watch afresh. Any pointer may be NULL. */
int slimt_hip_debug_kv_watch(slimt_hip_model *model, int *switched_to_24_bit, uint64_t *wide, uint64_t *submitted);
/* Diagnostic: accumulators must lie in [-limit, limit) for the 20-bit form (default and
 * maximum 2^19, what 20 bits hold). Tests lower it so that some sentences of a batch take the
 * 24-bit form next to narrow ones. Results do not depend on it. */
int slimt_hip_debug_kv_narrow_limit(slimt_hip_model *model, int limit);
/* Diagnostic: whether the model's load proved that its tied output layer (Wemb dequantised and re-quantised by
 * its own multiplier) equals the int8 table byte for byte -- true for every table without a -128. The fused
 * decoder then takes a step's next embedding row from the output layer's packed tile (the same bytes, addressed
 * by the winning column) instead of from the table. Results do not depend on it. */
int slimt_hip_debug_out_tied_exact(slimt_hip_model *model, int *exact);
/* ... and the proof alone, on a caller's table [rows][cols] with its multiplier: host code, needs no device. */
int slimt_hip_debug_tied_output_proof(const int8_t *wemb, size_t rows, size_t cols, float multiplier, int *exact);
/* Diagnostic: the dynamic LDS the persistent decoder's launcher asks for, for a shape (D, F, decoder layers), the
 * sentences per workgroup (32 / 16 / 8 / 4), a packed cache (kv24), a sentence-length class (mid: 0 = up to 32 tokens,
 * 1 = 33..64, 2 = 65..128), the tight cache form and what else picks the kernel (flags: bit 0 merged, 1 non-temporal
 * cache loads, 2 scored, 3 forced, 4 sampled) -- and whether the LayerNorm constants and the output layer's epilogue
 * constants are part of it. Host code, needs no device. */
int slimt_hip_debug_fused_decode_lds_bytes(int D, int F, int Ld, int sentences_per_wg, int kv24, int mid, int tight,
                                           unsigned flags, size_t *bytes, int *ln_in_lds, int *epi_in_lds);
/* Diagnostic: the tight (16-bit) form below the 20-bit one. Where the decoder has a reader for it (D = 256 /
 * F = 1536 with sentences of up to 128 tokens, D = 512 / F = 2048 up to 32) format 0 caches a
 * sentence-layer whose K and V accumulators, less their columns' centres (slimt_hip_model_set_kv_centres),
 * all lie in [-limit, limit) as plain int16 (default and maximum 2^15; 0 = never tried; tests lower it so
 * that a batch mixes all three forms). Results do not depend on it. Starts the watches afresh. */
int slimt_hip_debug_kv_tight_limit(slimt_hip_model *model, int limit);
/* The tight form's per-column centres, [Ld][K, V][D] int32 (n = Ld * 2 * D, each within (-2^24, 2^24): a float holds it exactly):
 * the 16-bit form caches accumulator - centre, the decoder adds the centre back (exact), so the centres
 * decide which sentences fit the form and nothing else -- every result is the same for any centres.
 * Without this call the library calibrates them itself: the first batch of at least 1024 rows that could
 * take the form is cached as f32, its column means (floor(sum / rows + 1/2), integer arithmetic) become
 * the centres, and the form is tried from the first batch submitted after that reduction has finished.
 * Call it before the first translate, or with no batch of this model in flight; it fails while a
 * calibration batch is in flight. A deployment that wants the same form for the same sentence on
 * every run sets centres it has stored (slimt_hip_debug_kv_centres reads the calibrated ones). */
int slimt_hip_model_set_kv_centres(slimt_hip_model *model, const int32_t *centres, size_t n);
/* Diagnostic: *ready = 1 and out[0 .. Ld * 2 * D) = the centres once they exist (set, or calibrated and
 * the reduction finished), else *ready = 0. out may be NULL (state only). */
int slimt_hip_debug_kv_centres(slimt_hip_model *model, int32_t *out, size_t n, int *ready);
/* Diagnostic: the tight form's watch, per decoder layer l < 4: submitted[l] sentences were allowed to
 * try it, missed[l] of them did not fit (updated by the device, a few batches behind); once more than
 * one in 32 of a layer's sentences missed (after 1024 were submitted) that layer stops trying (bit l of
 * *layers_off): the 20-bit form is an out-of-line fallback in the kernels with the tight reader. Any pointer may be NULL; the arrays hold 4 entries. */
int slimt_hip_debug_kv_tight_watch(slimt_hip_model *model, unsigned *layers_off, uint64_t *missed, uint64_t *submitted);
/* Re-calibration of the centres (round 6): the first calibration batch need not look like the traffic behind
 * it, so the first `max_recalibrations` times a layer's watch trips (above) the engine starts a new GENERATION
 * of centres instead of switching the layer off: the next batch of >= 1024 rows is cached as f32 and calibrates
 * them (into a buffer of its own: batches in flight keep the generation they were encoded with), and the form
 * is tried again. Only a trip past that limit switches a layer off for good. Default 2, at most 3;
 * max_recalibrations < 0 leaves the limit alone. *generations_started (nullable): 0 until the first trip.
 * The counters of _kv_tight_watch are those of the current generation. Results never depend on any of this. */
int slimt_hip_debug_kv_recalibrations(slimt_hip_model *model, int *generations_started, int max_recalibrations);
/* Diagnostic (process-wide): while device_buf != NULL, thread 0 of every
 * workgroup of the persistent encoder / decoder appends a begin and an end
 * event to it: device_buf[0] = event counter (zero it first), then 3 uint64
 * per event {kernel (1 = decoder, 2 = encoder) | end << 8 | blockIdx << 16,
 * HW_ID | XCC_ID << 32, 100 MHz wall clock}; events past `capacity` are
 * dropped. NULL switches it off. tools/occupancy_trace.py reads it. */
int slimt_hip_debug_occupancy_trace(void *device_buf, size_t capacity);
/* Diagnostic: the plan of ctx's last fused decoder launch under the decoder admission (engine.cpp,
 * decoder_plan.h): out[0] sentences per workgroup, out[1] contexts with a decoder pending (this one included),
 * out[2] decoders in flight (min(pending contexts, hardware queues)), out[3] admission depth n (0 = the launch
 * waited for no event), out[4] K/V temporal eighths, out[5] the hardware queues the model saw (GPU_MAX_HW_QUEUES
 * when it was created, else 4). All 0 before the first such launch. Results never depend on any of this. */
int slimt_hip_debug_decoder_plan(slimt_hip_ctx *ctx, int out[6]);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_H */
