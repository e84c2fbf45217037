// extern "C" face of host/Service (include/slimt_hip_service.h).
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <memory>
#include <vector>

#include "Service.hh"
#include "slimt_hip_service.h"
#include "slimt_hip_service_prefix.h"
#include "slimt_hip_service_candidates.h"
#include "slimt_hip_service_samples.h"
#include "slimt_hip_service_consensus.h"
#include "slimt_hip_service_score.h"
#include "slimt_hip_service_sampling.h"
#include "slimt_hip_service_scores.h"
#include "slimt_hip_service_alternatives.h"

namespace {
thread_local char g_err[512] = "";
int fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}
}  // namespace

struct slimt_hip_service {
  std::vector<std::unique_ptr<slimt::Model>> models;  // non-owning views of the caller's replicas
  std::unique_ptr<slimt::Service> service;
  bool scores = false;  // slimt_hip_service_set_scores
  float temperature = 0.0f;  // slimt_hip_service_set_sampling
};

struct slimt_hip_result {
  std::vector<uint32_t> targets, padded;
  std::vector<uint64_t> target_offsets, batch, align_offsets;
  std::vector<float> alignments;
  std::vector<float> scores;  // per target token, by target_offsets (a scoring service only)
  bool scored = false;
  // slimt_hip_service_score_alternatives: per target token, by target_offsets ([k] ids and scores, one rank)
  uint32_t alternatives = 0;
  std::vector<uint32_t> alt_ids, ranks;
  std::vector<float> alt_scores;
  // slimt_hip_service_score_candidates: one total per entry (candidate), one best index per source sentence
  bool ranked = false;
  std::vector<float> totals;
  std::vector<uint32_t> best;
  // slimt_hip_service_translate_samples: entries per sentence (0: another kind of result)
  size_t samples = 0;
  // slimt_hip_service_translate_consensus: per entry (sentence) the winner's utility and its index among the samples
  bool selected = false;
  std::vector<double> utility;
  std::vector<uint32_t> sample_index;
};

extern "C" const char *slimt_hip_service_last_error(void) { return g_err; }

extern "C" int slimt_hip_service_create(const slimt_hip_service_config *config, slimt_hip_model *const *replicas,
                                        size_t n_replicas, slimt_hip_service **out) {
  if (!config || !replicas || !out || n_replicas == 0) return fail("null argument");
  *out = nullptr;
  try {
    auto s = std::make_unique<slimt_hip_service>();
    std::vector<const slimt::Model *> views;
    for (size_t i = 0; i < n_replicas; ++i) {
      if (!replicas[i]) return fail("replica %zu is NULL", i);
      slimt::Model::Config mc;
      mc.eos_id = config->eos_id;
      s->models.push_back(std::make_unique<slimt::Model>(mc, replicas[i]));
      views.push_back(s->models.back().get());
    }
    slimt::ServiceConfig sc;
    sc.max_words = config->max_words;
    sc.wrap_length = config->wrap_length;
    sc.tgt_length_limit_factor = config->limit_factor;
    sc.workers_per_device = config->workers_per_device;
    sc.pad_id = config->pad_id;
    if (config->merge_batches) sc.merge_batches = config->merge_batches;
    if (config->merge_words) sc.merge_words = config->merge_words;
    sc.alignments = config->alignments != 0;
    sc.flat_alignments = true;  // arrays out: one block per sentence
    if (config->lexical_shortlist && config->lexical_shortlist_bytes) {
      sc.lexical_shortlist = slimt::View{config->lexical_shortlist, static_cast<size_t>(config->lexical_shortlist_bytes)};
      sc.source_vocab = config->source_vocab;
      sc.target_vocab = config->target_vocab;
      sc.shortlist_shared_vocab = config->shortlist_shared_vocab != 0;
      sc.shortlist_check = config->shortlist_check != 0;
    } else if (config->shortlist && config->n_shortlist) {
      sc.shortlist = slimt::Words(config->shortlist, config->shortlist + config->n_shortlist);
    }
    s->service = std::make_unique<slimt::Service>(sc, views);
    *out = s.release();
    return 0;
  } catch (const std::exception &e) {
    return fail("%s", e.what());
  }
}

extern "C" int slimt_hip_service_destroy(slimt_hip_service *service) {
  delete service;
  return 0;
}

namespace {
// Histories -> the arrays of a result (scored: with every token's log-probability)
int flatten(const slimt::Histories &hs, size_t n, bool scored, std::unique_ptr<slimt_hip_result> &out, uint32_t alternatives = 0) {
  auto r = std::make_unique<slimt_hip_result>();
  r->alternatives = alternatives;
  r->target_offsets.assign(n + 1, 0);
  r->align_offsets.assign(n + 1, 0);
  r->padded.resize(n);
  r->batch.resize(n);
  size_t n_tok = 0, n_al = 0;
  for (size_t i = 0; i < n; ++i) {
    n_tok += hs[i]->target.size();
    n_al += hs[i]->alignment_flat.size();
  }
  r->targets.reserve(n_tok);
  r->alignments.reserve(n_al);
  r->scored = scored;
  if (r->scored) r->scores.reserve(n_tok);
  for (size_t i = 0; i < n; ++i) {
    const slimt::Hypothesis &h = *hs[i];
    r->targets.insert(r->targets.end(), h.target.begin(), h.target.end());
    r->alignments.insert(r->alignments.end(), h.alignment_flat.begin(), h.alignment_flat.end());
    if (r->scored) {
      if (h.scores.size() != h.target.size()) return fail("sentence %zu: %zu scores for %zu tokens", i, h.scores.size(), h.target.size());
      r->scores.insert(r->scores.end(), h.scores.begin(), h.scores.end());
    }
    if (alternatives) {
      const size_t nt = h.target.size();
      if (h.alternatives != alternatives || h.alt_ids.size() != nt * alternatives || h.alt_scores.size() != nt * alternatives ||
          h.ranks.size() != nt)
        return fail("sentence %zu: alternatives of %zu tokens do not match k = %u", i, nt, alternatives);
      r->alt_ids.insert(r->alt_ids.end(), h.alt_ids.begin(), h.alt_ids.end());
      r->alt_scores.insert(r->alt_scores.end(), h.alt_scores.begin(), h.alt_scores.end());
      r->ranks.insert(r->ranks.end(), h.ranks.begin(), h.ranks.end());
    }
    r->target_offsets[i + 1] = r->targets.size();
    r->align_offsets[i + 1] = r->alignments.size();
    r->padded[i] = static_cast<uint32_t>(h.padded_length);
    r->batch[i] = h.batch;
  }
  out = std::move(r);
  return 0;
}

// tokens + offsets -> one Words per sentence. Several arrays (the sentences with their prefixes or targets) are walked
// together, sentence by sentence, so the first decreasing offset of any of them is the one reported: "<label> decrease"
struct Ragged {
  const uint32_t *tokens;
  const uint64_t *offsets;
  const char *label;
  std::vector<slimt::Words> *rows;
};
int to_rows(std::initializer_list<Ragged> arrays, size_t n) {
  for (const Ragged &a : arrays) a.rows->assign(n, slimt::Words());
  for (size_t i = 0; i < n; ++i)
    for (const Ragged &a : arrays) {
      if (a.offsets[i + 1] < a.offsets[i]) return fail("%s decrease at sentence %zu", a.label, i);
      if (a.offsets[i + 1] > a.offsets[i]) (*a.rows)[i].assign(a.tokens + a.offsets[i], a.tokens + a.offsets[i + 1]);
    }
  return 0;
}

// The shell of every call that returns a result: *out is what `fill` leaves (status 0), else NULL with the message of
// what it refused or threw.
template <class Fill>
int result_of(slimt_hip_result **out, Fill &&fill) {
  *out = nullptr;
  try {
    std::unique_ptr<slimt_hip_result> r;
    if (const int rc = fill(r)) return rc;
    *out = r.release();
    return 0;
  } catch (const std::exception &e) {
    return fail("%s", e.what());
  }
}

// slimt_hip_service_translate[_prefixed]: prefix_tokens / prefix_offsets NULL = no prefixes
int translate(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets, const uint32_t *prefix_tokens,
              const uint64_t *prefix_offsets, size_t n, slimt_hip_result **out, uint64_t seed = 0) {
  return result_of(out, [&](std::unique_ptr<slimt_hip_result> &r) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<slimt::Words> sentences, prefixes;
    const Ragged src{tokens, offsets, "offsets", &sentences}, pre{prefix_tokens, prefix_offsets, "prefix offsets", &prefixes};
    if (const int rc = prefix_offsets ? to_rows({src, pre}, n) : to_rows({src}, n)) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    slimt::Histories hs = service->service->translate(std::move(sentences), std::move(prefixes), seed).get();
    const auto t2 = std::chrono::steady_clock::now();
    if (const int rc = flatten(hs, n, service->scores, r)) return rc;
    if (std::getenv("SLIMT_SERVICE_STATS")) {
      const auto t3 = std::chrono::steady_clock::now();
      auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
      std::fprintf(stderr, "service-call: %zu sentences: copy in %.1f ms, translate %.1f ms, flatten %.1f ms\n", n,
                   ms(t0, t1), ms(t1, t2), ms(t2, t3));
    }
    return 0;
  });
}
}  // namespace

extern "C" int slimt_hip_service_translate(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                           size_t n, slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets))) return fail("null argument");
  return translate(service, tokens, offsets, nullptr, nullptr, n, out);
}

extern "C" int slimt_hip_service_translate_prefixed(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                                    const uint32_t *prefix_tokens, const uint64_t *prefix_offsets, size_t n,
                                                    slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets || !prefix_offsets)) || (n && prefix_offsets[n] > prefix_offsets[0] && !prefix_tokens))
    return fail("null argument");
  return translate(service, tokens, offsets, prefix_tokens, prefix_offsets, n, out);
}

namespace {
int score(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets, const uint32_t *tgt_tokens,
          const uint64_t *tgt_offsets, size_t n, uint32_t alternatives, slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets || !tgt_offsets)) || (n && tgt_offsets[n] > tgt_offsets[0] && !tgt_tokens))
    return fail("null argument");
  return result_of(out, [&](std::unique_ptr<slimt_hip_result> &r) {
    std::vector<slimt::Words> sentences, targets;
    if (const int rc = to_rows({{tokens, offsets, "offsets", &sentences}, {tgt_tokens, tgt_offsets, "target offsets", &targets}}, n))
      return rc;
    const slimt::Histories hs = service->service->score(std::move(sentences), std::move(targets), alternatives);
    return flatten(hs, n, true, r, alternatives);
  });
}
}  // namespace

extern "C" int slimt_hip_service_score(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                       const uint32_t *tgt_tokens, const uint64_t *tgt_offsets, size_t n, slimt_hip_result **out) {
  return score(service, tokens, offsets, tgt_tokens, tgt_offsets, n, 0, out);
}

extern "C" int slimt_hip_service_score_alternatives(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                                    const uint32_t *tgt_tokens, const uint64_t *tgt_offsets, size_t n, uint32_t k,
                                                    slimt_hip_result **out) {
  if (k < 1 || k > SLIMT_HIP_MAX_ALTERNATIVES)
    return fail("score_alternatives: k %u is not in 1..%d", k, SLIMT_HIP_MAX_ALTERNATIVES);
  return score(service, tokens, offsets, tgt_tokens, tgt_offsets, n, k, out);
}

extern "C" int slimt_hip_service_score_candidates(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets, size_t n,
                                                  const uint32_t *tgt_tokens, const uint64_t *tgt_offsets,
                                                  const uint64_t *cand_offsets, int mode, slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets || !cand_offsets))) return fail("null argument");
  const size_t N = n ? cand_offsets[n] : 0;
  if (n && cand_offsets[0] != 0) return fail("candidate offsets start at %llu, not 0", (unsigned long long)cand_offsets[0]);
  if (N && (!tgt_offsets || (tgt_offsets[N] > tgt_offsets[0] && !tgt_tokens))) return fail("null argument");
  return result_of(out, [&](std::unique_ptr<slimt_hip_result> &r) {
    std::vector<slimt::Words> sentences(n);
    std::vector<std::vector<slimt::Words>> candidates(n);
    for (size_t i = 0; i < n; ++i) {  // (its own walk: two levels of offsets, checked sentence by sentence)
      if (offsets[i + 1] < offsets[i]) return fail("offsets decrease at sentence %zu", i);
      if (cand_offsets[i + 1] < cand_offsets[i]) return fail("candidate offsets decrease at sentence %zu", i);
      sentences[i].assign(tokens + offsets[i], tokens + offsets[i + 1]);
      for (uint64_t c = cand_offsets[i]; c < cand_offsets[i + 1]; ++c) {
        if (tgt_offsets[c + 1] < tgt_offsets[c]) return fail("target offsets decrease at candidate %llu", (unsigned long long)c);
        candidates[i].emplace_back(tgt_tokens + tgt_offsets[c], tgt_tokens + tgt_offsets[c + 1]);
      }
    }
    slimt::Service::CandidateScores cs = service->service->score_candidates(std::move(sentences), std::move(candidates), mode);
    if (const int rc = flatten(cs.candidates, cs.candidates.size(), true, r)) return rc;
    r->ranked = true;
    r->totals = std::move(cs.totals);
    r->best = std::move(cs.best);
    return 0;
  });
}

extern "C" int slimt_hip_result_candidates(const slimt_hip_result *r, const float **totals, const uint32_t **best) {
  if (!r) return fail("null argument");
  if (!r->ranked) return fail("result_candidates: not a result of slimt_hip_service_score_candidates");
  if (totals) *totals = r->totals.data();
  if (best) *best = r->best.data();
  return 0;
}

extern "C" int slimt_hip_service_translate_samples(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                                   size_t n, size_t samples, uint64_t seed, slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets))) return fail("null argument");
  return result_of(out, [&](std::unique_ptr<slimt_hip_result> &r) {
    std::vector<slimt::Words> sentences;
    if (const int rc = to_rows({{tokens, offsets, "offsets", &sentences}}, n)) return rc;
    const slimt::Histories hs = service->service->translate_samples(std::move(sentences), samples, seed);
    if (const int rc = flatten(hs, hs.size(), true, r)) return rc;
    r->samples = samples;
    return 0;
  });
}

extern "C" int slimt_hip_result_samples(const slimt_hip_result *r, size_t *samples) {
  if (!r || !samples) return fail("null argument");
  if (!r->samples) return fail("result_samples: not a result of slimt_hip_service_translate_samples");
  *samples = r->samples;
  return 0;
}

extern "C" int slimt_hip_service_translate_consensus(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                                     size_t n, size_t samples, uint64_t seed, int max_order, int beta2,
                                                     slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets))) return fail("null argument");
  return result_of(out, [&](std::unique_ptr<slimt_hip_result> &r) {
    std::vector<slimt::Words> sentences;
    if (const int rc = to_rows({{tokens, offsets, "offsets", &sentences}}, n)) return rc;
    const slimt::Histories hs = service->service->translate_consensus(std::move(sentences), samples, seed, max_order, beta2);
    if (const int rc = flatten(hs, hs.size(), true, r)) return rc;
    r->selected = true;
    r->utility.reserve(hs.size());
    r->sample_index.reserve(hs.size());
    for (const slimt::History &h : hs) {
      r->utility.push_back(h->utility);
      r->sample_index.push_back(h->sample_index);
    }
    return 0;
  });
}

extern "C" int slimt_hip_result_consensus(const slimt_hip_result *r, const double **utility, const uint32_t **sample_index) {
  if (!r || !utility || !sample_index) return fail("null argument");
  if (!r->selected) return fail("result_consensus: not a result of slimt_hip_service_translate_consensus");
  *utility = r->utility.data();
  *sample_index = r->sample_index.data();
  return 0;
}

extern "C" int slimt_hip_result_alternatives(const slimt_hip_result *r, size_t i, uint32_t *k, const uint32_t **ids,
                                             const float **scores, const uint32_t **ranks) {
  if (!r) return fail("result is NULL");
  if (!r->alternatives) return fail("result_alternatives: not a result of slimt_hip_service_score_alternatives");
  if (i >= r->padded.size()) return fail("result_alternatives: sentence %zu of %zu", i, r->padded.size());
  const size_t at = r->target_offsets[i];
  if (k) *k = r->alternatives;
  if (ids) *ids = r->alt_ids.data() + at * r->alternatives;
  if (scores) *scores = r->alt_scores.data() + at * r->alternatives;
  if (ranks) *ranks = r->ranks.data() + at;
  return 0;
}

extern "C" int slimt_hip_result_view(const slimt_hip_result *r, size_t *n, const uint32_t **targets,
                                     const uint64_t **target_offsets, const uint32_t **padded_length,
                                     const uint64_t **batch, const float **alignments, const uint64_t **align_offsets) {
  if (!r) return fail("result is NULL");
  if (n) *n = r->padded.size();
  if (targets) *targets = r->targets.data();
  if (target_offsets) *target_offsets = r->target_offsets.data();
  if (padded_length) *padded_length = r->padded.data();
  if (batch) *batch = r->batch.data();
  if (alignments) *alignments = r->alignments.data();
  if (align_offsets) *align_offsets = r->align_offsets.data();
  return 0;
}

extern "C" int slimt_hip_result_destroy(slimt_hip_result *result) {
  delete result;
  return 0;
}

extern "C" int slimt_hip_service_set_scores(slimt_hip_service *service, int on) {
  if (!service) return fail("null argument");
  if (!service->service->set_scores(on != 0)) return fail("set_scores: only before the first slimt_hip_service_translate");
  service->scores = on != 0;
  return 0;
}

extern "C" int slimt_hip_service_set_sampling(slimt_hip_service *service, float temperature) {
  if (!service) return fail("null argument");
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return fail("set_sampling: temperature %g is not finite and > 0", (double)temperature);
  if (!service->service->set_sampling(temperature)) return fail("set_sampling: only before the first slimt_hip_service_translate");
  service->temperature = temperature;
  return 0;
}

extern "C" int slimt_hip_service_set_sampling_truncation(slimt_hip_service *service, uint32_t top_k, float top_p) {
  if (!service) return fail("null argument");
  if (!(top_p > 0.0f && top_p <= 1.0f)) return fail("set_sampling_truncation: top_p %g is not in (0, 1]", (double)top_p);
  if (!(service->temperature > 0.0f))
    return fail("set_sampling_truncation: the service does not sample (slimt_hip_service_set_sampling first)");
  if (!service->service->set_sampling_truncation(top_k, top_p))
    return fail("set_sampling_truncation: only before the first slimt_hip_service_translate");
  return 0;
}

extern "C" int slimt_hip_service_translate_sampled(slimt_hip_service *service, const uint32_t *tokens, const uint64_t *offsets,
                                                   const uint32_t *prefix_tokens, const uint64_t *prefix_offsets, uint64_t seed,
                                                   size_t n, slimt_hip_result **out) {
  if (!service || !out || (n && (!tokens || !offsets)) ||
      (n && prefix_offsets && prefix_offsets[n] > prefix_offsets[0] && !prefix_tokens))
    return fail("null argument");
  if (!(service->temperature > 0.0f))
    return fail("translate_sampled: the service does not sample (slimt_hip_service_set_sampling)");
  return translate(service, tokens, offsets, prefix_tokens, prefix_offsets, n, out, seed);
}

extern "C" int slimt_hip_result_scores(const slimt_hip_result *r, const float **scores) {
  if (!r || !scores) return fail("null argument");
  *scores = r->scored ? r->scores.data() : nullptr;
  return 0;
}
