/* Alternatives of teacher-forced scoring through the batching service (include/slimt_hip_service_score.h), exported by the
 * same library: include/slimt_hip.h, slimt_hip_ctx_set_score_alternatives, for the sentence pairs of one request. */
#ifndef SLIMT_HIP_SERVICE_ALTERNATIVES_H
#define SLIMT_HIP_SERVICE_ALTERNATIVES_H

#include "slimt_hip_service_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* slimt_hip_service_score with, for every target token, the k (1 .. 8; anything else fails the call) most probable tokens
 * of its position and the given token's rank among the columns of the output layer the service scores with. Batching,
 * limits and failures are those of slimt_hip_service_score, and the result holds what that call's result holds. */
int slimt_hip_service_score_alternatives(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                         const uint32_t *tgt_tokens, const uint64_t *tgt_offsets, size_t n, uint32_t k,
                                         slimt_hip_result **out);

/* Sentence i of such a result, with n_i target tokens: *k as given; ids [n_i][k], the vocabulary ids in the order of
 * slimt_hip_ctx_set_score_alternatives (0xFFFFFFFF past the layer's valid columns); scores [n_i][k], their natural-log
 * probabilities (-inf there); ranks [n_i], the given token's place in that order (0xFFFFFFFF for a token outside the
 * layer). Each out-pointer is nullable; the arrays live as long as the result. Fails for a result of another call and for
 * i past the request's sentences. */
int slimt_hip_result_alternatives(const slimt_hip_result *result, size_t i, uint32_t *k, const uint32_t **ids,
                                  const float **scores, const uint32_t **ranks);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_ALTERNATIVES_H */
