/* Teacher-forced scoring through the batching service (include/slimt_hip_service.h), exported by the same library:
 * include/slimt_hip.h, slimt_hip_score, for the sentence pairs of one request. */
#ifndef SLIMT_HIP_SERVICE_SCORE_H
#define SLIMT_HIP_SERVICE_SCORE_H

#include "slimt_hip_service.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scores (and aligns) GIVEN translations: sentence i is tokens[offsets[i] .. offsets[i + 1]), its target
 * tgt_tokens[tgt_offsets[i] .. tgt_offsets[i + 1]) -- with its EOS when that is to be scored. Every target position
 * goes through the decoder in one pass (slimt_hip_score), where slimt_hip_service_translate_prefixed decodes step by
 * step; nothing stops at EOS, and there is NO target-length cap: a target may be any length up to 65536 tokens,
 * whatever the limit factor (an empty one gives an empty result). Batches are formed by the source-length rule of
 * slimt_hip_service_translate, each batch's target rows are as long as its longest target, and the output layer is the
 * one the service translates with: its lexical shortlist per batch, its fixed list, or the full vocabulary. A token
 * outside that layer scores -inf. The call runs on the caller's thread and on a device context of its own (built by the
 * first call, on the service's first model): it is neither queued behind nor merged with translate requests, and
 * concurrent callers take turns.
 * Results come back through slimt_hip_result_view: the result's targets are the given tokens, slimt_hip_result_scores
 * their natural-log probabilities (always, whatever slimt_hip_service_set_scores says), the alignment rows head 0 of the
 * last decoder layer, [target tokens][source tokens] per sentence (when the service keeps alignments). A NULL argument,
 * decreasing offsets, an empty sentence, one longer than the service accepts or an id >= the vocabulary fail the call. */
int slimt_hip_service_score(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                            const uint32_t *tgt_tokens, const uint64_t *tgt_offsets, size_t n, slimt_hip_result **out);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_SCORE_H */
