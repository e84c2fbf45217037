/* Per-token scores of the batching service (include/slimt_hip_service.h), exported by the same library:
 * the natural-log softmax probability of every target token over its step's output layer (the shortlist's
 * columns, or the full vocabulary), EOS included -- include/slimt_hip.h, slimt_hip_ctx_set_scores. */
#ifndef SLIMT_HIP_SERVICE_SCORES_H
#define SLIMT_HIP_SERVICE_SCORES_H

#include "slimt_hip_service.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scores on (on != 0) or off for every later slimt_hip_service_translate. Only before the first
 * slimt_hip_service_translate on `service`: refused (non-zero, slimt_hip_service_last_error) afterwards.
 * Merged launches, the lexical shortlist and the fixed list all score. */
int slimt_hip_service_set_scores(slimt_hip_service *service, int on);

/* *scores = one f32 per target token, indexed like the targets (target_offsets of slimt_hip_result_view),
 * or NULL when the service that produced `result` does not score. Valid until slimt_hip_result_destroy.
 * A sentence's score is the sum of its tokens' (no length normalisation). */
int slimt_hip_result_scores(const slimt_hip_result *result, const float **scores);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_SCORES_H */
