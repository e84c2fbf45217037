/* Several candidate translations per sentence through the batching service (include/slimt_hip_service.h), scored from one
 * encoding of each sentence: include/slimt_hip.h, slimt_hip_score_candidates, for the sentences of one request. */
#ifndef SLIMT_HIP_SERVICE_CANDIDATES_H
#define SLIMT_HIP_SERVICE_CANDIDATES_H
#include "slimt_hip_service.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Sentence i (tokens[offsets[i] .. offsets[i + 1]), as for slimt_hip_service_translate) owns the candidates
 * cand_offsets[i] .. cand_offsets[i + 1] - 1 (cand_offsets [n + 1], ascending from 0; a sentence may own none); candidate c
 * is tgt_tokens[tgt_offsets[c] .. tgt_offsets[c + 1]) (with its EOS when that is to be scored; any length, 0 included).
 * Batches are formed by the service's source-length rule; all candidates of a sentence travel in its batch, sorted by
 * source, and each sentence is encoded once. The output layer is the service's, as for slimt_hip_service_score; the call
 * is synchronous on the caller's thread and the scoring context. The result holds ONE ENTRY PER CANDIDATE, in the order
 * given: slimt_hip_result_view's targets are the candidates' tokens, slimt_hip_result_scores their log-probabilities --
 * bit for bit those slimt_hip_service_score gives for the pair (sentence, candidate).
 * mode: 0 ranks by the sum of a candidate's scores, 1 by the sum divided by its tokens; another value is refused. */
int slimt_hip_service_score_candidates(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets, size_t n,
                                       const uint32_t *tgt_tokens, const uint64_t *tgt_offsets, const uint64_t *cand_offsets,
                                       int mode, slimt_hip_result **out);
/* Of such a result: totals [entries] -- per candidate the f32 sum of its scores, ascending from +0.0f, one add per token --
 * and best [n] -- per SENTENCE of the request the index among its own candidates of the best one by slimt_hip_candidates_rank's rule
 * (the lowest index of the largest key; candidates without tokens or with a NaN key aside), 0xFFFFFFFF when none is left.
 * Any pointer may be NULL. The arrays live as long as the result. */
int slimt_hip_result_candidates(const slimt_hip_result *result, const float **totals, const uint32_t **best);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_CANDIDATES_H */
