/* Temperature sampling through the batching service (include/slimt_hip_service.h), exported by the same library:
 * include/slimt_hip.h, slimt_hip_ctx_set_sampling, with reproducible per-sentence keys. */
#ifndef SLIMT_HIP_SERVICE_SAMPLING_H
#define SLIMT_HIP_SERVICE_SAMPLING_H

#include "slimt_hip_service.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every request of the service is sampled at `temperature` (finite and > 0) instead of decoded greedily. A service-wide
 * setting like slimt_hip_service_set_scores: only before the first request. With slimt_hip_service_set_scores the
 * results' scores are log softmax(logit / temperature) at the drawn tokens. */
int slimt_hip_service_set_sampling(slimt_hip_service *service, float temperature);

/* Every sampled request is truncated to the top_k largest columns (0: no top-k) and the nucleus of mass top_p (finite,
 * 0 < top_p <= 1; 1: no top-p): include/slimt_hip.h, slimt_hip_ctx_set_sampling_truncation. Service-wide, only after
 * slimt_hip_service_set_sampling and before the first request. The engine does not merge truncated calls, so such a
 * service sends every batch as a launch of its own. */
int slimt_hip_service_set_sampling_truncation(slimt_hip_service *service, uint32_t top_k, float top_p);

/* slimt_hip_service_translate on a sampling service, seeded: sentence i is drawn under the key
 * slimt_hip_sampling_key(seed, i), wherever the batcher puts it and whatever shares its launch, so a request's
 * translations depend on its sentences and its seed alone. prefix_tokens / prefix_offsets (both NULL: none): forced
 * target prefixes as for slimt_hip_service_translate_prefixed; sampling starts behind each prefix. The plain
 * slimt_hip_service_translate and _translate_prefixed on a sampling service use seed 0. Fails on a service that does not
 * sample. */
int slimt_hip_service_translate_sampled(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                        const uint32_t *prefix_tokens, const uint64_t *prefix_offsets, uint64_t seed, size_t n,
                                        slimt_hip_result **out);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_SAMPLING_H */
