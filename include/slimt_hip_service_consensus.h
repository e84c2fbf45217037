/* The consensus (minimum-Bayes-risk) pick among several sampled translations per sentence through the batching service
 * (include/slimt_hip_service.h): include/slimt_hip_service_samples.h's call with the selection of include/slimt_hip.h,
 * slimt_hip_ctx_set_fanout_consensus, made on the device behind each fan-out call. */
#ifndef SLIMT_HIP_SERVICE_CONSENSUS_H
#define SLIMT_HIP_SERVICE_CONSENSUS_H
#include "slimt_hip_service.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Draws `samples` translations of every sentence exactly as slimt_hip_service_translate_samples does -- the same batches, the
 * same keys slimt_hip_sampling_key(seed, i * samples + j) -- and keeps, for each sentence, the sample that agrees most with
 * the sentence's other samples: the utility of slimt_hip_consensus_select at max_order (1..4) and the integer beta2 (1..16;
 * 4 is chrF's beta = 2). No second encoding and no scorer pass. The result holds ONE ENTRY PER SENTENCE: the winner's tokens,
 * scores (always filled) and alignment are bit for bit entry i * samples + sample_index of slimt_hip_service_translate_samples
 * with the same seed. samples = 1 returns the lone sample with utility 0. Refused: what that call refuses, samples > 64
 * (SLIMT_HIP_CONSENSUS_MAX_ROWS), max_order or beta2 out of range. */
int slimt_hip_service_translate_consensus(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets, size_t n,
                                          size_t samples, uint64_t seed, int max_order, int beta2, slimt_hip_result **out);
/* Of such a result: per entry the winner's utility and its index j among its sentence's samples (arrays of the result's
 * entries, valid until the result is destroyed). Refuses any other result. */
int slimt_hip_result_consensus(const slimt_hip_result *result, const double **utility, const uint32_t **sample_index);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_CONSENSUS_H */
