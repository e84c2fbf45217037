/* Forced target prefixes through the batching service (include/slimt_hip_service.h), exported by the same library:
 * include/slimt_hip.h, slimt_hip_ctx_set_target_prefix, for the sentences of one request. */
#ifndef SLIMT_HIP_SERVICE_PREFIX_H
#define SLIMT_HIP_SERVICE_PREFIX_H

#include "slimt_hip_service.h"

#ifdef __cplusplus
extern "C" {
#endif

/* slimt_hip_service_translate, with sentence i forced through
 * prefix_tokens[prefix_offsets[i] .. prefix_offsets[i + 1]) (an empty range: not forced). At step t of
 * sentence i's target below its prefix length the prefix's token is recorded and fed instead of the
 * arg-max; from there on it decodes greedily, and it ends at EOS, forced or chosen: to score a given
 * translation, pass it with its EOS. A prefix longer than max(1, (size_t)(limit_factor * source length
 * of sentence i)) or holding an id >= the vocabulary fails the call. Results come back as for
 * slimt_hip_service_translate (slimt_hip_result_view), with the teacher-forced log-probabilities in
 * slimt_hip_result_scores when the service scores (slimt_hip_service_set_scores). Batching and merging
 * are as for slimt_hip_service_translate; sentences of other requests in the same launch are not forced. */
int slimt_hip_service_translate_prefixed(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                         const uint32_t *prefix_tokens, const uint64_t *prefix_offsets, size_t n,
                                         slimt_hip_result **out);

#ifdef __cplusplus
}
#endif
#endif /* SLIMT_HIP_SERVICE_PREFIX_H */
