/* Several sampled translations per sentence through the batching service (include/slimt_hip_service.h), drawn from one
 * encoding of each sentence: include/slimt_hip.h, slimt_hip_translate_fanout, for the sentences of one request. */
#ifndef SLIMT_HIP_SERVICE_SAMPLES_H
#define SLIMT_HIP_SERVICE_SAMPLES_H
#include "slimt_hip_service.h"
#ifdef __cplusplus
extern "C" {
#endif

/* `samples` translations of every sentence (tokens[offsets[i] .. offsets[i + 1]), as for slimt_hip_service_translate) of a
 * sampling service (include/slimt_hip_service_sampling.h, slimt_hip_service_set_sampling; its truncation applies). Batches
 * are formed by the service's source-length rule; all rows of a sentence travel in its batch, sorted by source, each
 * sentence is encoded once, and a call never holds more than max_words rows. Sample j of sentence i is drawn under
 * slimt_hip_sampling_key(seed, i * samples + j), wherever the batcher puts it: it is bit for bit row j of
 * slimt_hip_translate_fanout on that sentence alone, padded to its batch's length, with those keys. The call is synchronous
 * on the caller's thread and the scoring context. The result holds ONE ENTRY PER SAMPLE, sample j of sentence i at
 * i * samples + j: slimt_hip_result_view's targets are the samples' tokens, slimt_hip_result_scores their log-probabilities
 * (always filled). Refused: a service that does not sample, samples = 0, samples > max_words. */
int slimt_hip_service_translate_samples(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets, size_t n,
                                        size_t samples, uint64_t seed, slimt_hip_result **out);
/* Of such a result: the samples per sentence (entries = sentences * samples). Refuses any other result. */
int slimt_hip_result_samples(const slimt_hip_result *result, size_t *samples);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_SAMPLES_H */
