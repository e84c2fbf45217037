// Every call kind of host/Service and of its C face (service_capi.cc) over the fake engine (fake_hip_engine.cc): the
// scorer, candidates, samples, consensus, the asynchronous translate with prefixes / scores / sampling / truncation from
// several client threads, and the refusals with their exact messages. Linked into service_stress (its main calls
// service_calls()), so it runs under ThreadSanitizer and AddressSanitizer. The expected values are computed HERE, from the
// request alone (namespace want): a value delivered to the wrong sentence, candidate, sample, key or offset differs.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>

#include "Service.hh"
#include "slimt_hip_service.h"
#include "slimt_hip_service_alternatives.h"
#include "slimt_hip_service_candidates.h"
#include "slimt_hip_service_consensus.h"
#include "slimt_hip_service_prefix.h"
#include "slimt_hip_service_samples.h"
#include "slimt_hip_service_sampling.h"
#include "slimt_hip_service_score.h"
#include "slimt_hip_service_scores.h"

using namespace slimt;

extern "C" long fake_hip_merged_launches(void);

namespace {
std::atomic<int> g_wrong{0};
void wrong(const char *fmt, ...) {
  char line[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(line, sizeof(line), fmt, ap);
  va_end(ap);
  std::printf("WRONG: %s\n", line);
  ++g_wrong;
}

constexpr float kLimit = 1.5f;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// ---- what the engine's double computes, restated from its description ----------------------------------------------
namespace want {
uint64_t scramble(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
uint64_t key(uint64_t seed, uint64_t index) { return scramble(scramble(seed) + index); }
uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  return u;
}
uint64_t weight(const Words &w) {
  uint64_t s = 0;
  for (size_t j = 0; j < w.size(); ++j) s += (j + 1) * static_cast<uint64_t>(w[j]);
  return s;
}
float score(const Words &src, uint32_t token, size_t t) { return -static_cast<float>(1 + (weight(src) + 31ull * token + 7ull * t) % 1000) / 64.0f; }

struct Draw {  // how a service samples (temperature 0: greedy) and the sentence's key
  float temperature = 0.0f;
  uint32_t top_k = 0;
  float top_p = 1.0f;
  uint64_t key = 0;
};

// the translation of `src` in a batch padded to S, forced through `prefix`
Words translation(const Words &src, size_t S, const Words &prefix, const Draw &d) {
  const size_t T = std::max<size_t>(1, static_cast<size_t>(kLimit * static_cast<float>(S)));
  Words out;
  uint64_t h = 0;
  for (uint32_t tok : prefix) {
    out.push_back(tok);
    if (tok == 0) return out;  // a forced EOS ends the sentence
    h = scramble(h ^ tok);
  }
  const bool sampled = d.temperature > 0.0f;
  if (sampled) {
    uint64_t call = scramble(bits(d.temperature));
    if (d.top_k != 0 || d.top_p != 1.0f) call = scramble(scramble(call ^ d.top_k) ^ bits(d.top_p));
    h = scramble(scramble(h ^ d.key) ^ call);
  }
  const size_t n = std::min(T, std::max(prefix.size(), std::min(src.size() - 1, T - 1)) + 1);
  while (out.size() + 1 < n) {
    const size_t t = out.size();
    const uint32_t base = t + 1 < src.size() ? src[src.size() - 2 - t] : static_cast<uint32_t>(7 * t + 1);
    out.push_back(prefix.empty() && !sampled ? base : 2 + static_cast<uint32_t>((base + scramble(h + t)) % 500));
  }
  if (out.size() < n) out.push_back(0);
  return out;
}
// the source column that row t of its alignment puts weight 1 on
size_t aligned(const Words &src, const Words &out, size_t t, bool plain) {
  if (!plain) return (out[t] + t) % src.size();
  return t + 1 < out.size() && src.size() >= 2 + t ? src.size() - 2 - t : src.size() - 1;
}
float score_alignment(const Words &src, size_t j, uint32_t token, size_t t) { return static_cast<float>(1 + (src[j] + 3 * t + token) % 64) / 64.0f; }
uint32_t alt_id(uint32_t token, size_t t, size_t i) { return static_cast<uint32_t>((token + 13 * t + 17 * i + 1) % 512); }
float alt_score(uint32_t token, size_t t, size_t i) { return -static_cast<float>(i + 1 + (token + t) % 5) / 8.0f; }
uint32_t rank(uint32_t token, size_t t) { return static_cast<uint32_t>((token + 3 * t) % 11); }
// consensus among one sentence's samples: the winner's index and utility
std::pair<uint32_t, double> consensus(const std::vector<Words> &rows) {
  uint32_t best = 0;
  double top = 0.0;
  for (size_t i = 0; i < rows.size(); ++i) {
    double total = 0.0;
    for (size_t o = 0; o < rows.size(); ++o)
      if (o != i) total += static_cast<double>((weight(rows[i]) ^ weight(rows[o])) % 17) / 16.0;
    const double u = rows.size() > 1 ? total / static_cast<double>(rows.size() - 1) : 0.0;
    if (i == 0 || u > top) {
      top = u;
      best = static_cast<uint32_t>(i);
    }
  }
  return {best, top};
}
}  // namespace want

// ---- requests ----------------------------------------------------------------------------------------------------
Words sentence(std::mt19937 &rng, size_t len) {
  Words s(len);
  for (auto &w : s) w = 2 + rng() % 500;
  s.back() = 0;
  return s;
}
std::vector<Words> request(std::mt19937 &rng) {  // 1 to 9 sentences of 1 to 16 tokens
  std::vector<Words> sents(1 + rng() % 9);
  for (auto &s : sents) s = sentence(rng, 1 + rng() % 16);
  return sents;
}
Words tokens(std::mt19937 &rng, size_t len) {  // any tokens: a target, a candidate, a prefix
  Words s(len);
  for (auto &w : s) w = rng() % 10 == 0 ? 0 : 2 + rng() % 500;
  return s;
}

ServiceConfig small_config(bool alignments, size_t workers = 1) {
  ServiceConfig sc;
  sc.max_words = 64;
  sc.wrap_length = 16;
  sc.workers_per_device = workers;
  sc.alignments = alignments;
  return sc;
}

template <class E, class F>
void refused(const char *what, const std::string &message, F &&call) {
  try {
    call();
    wrong("%s: accepted", what);
  } catch (const E &e) {
    if (message != e.what()) wrong("%s: refused with \"%s\", not \"%s\"", what, e.what(), message.c_str());
  } catch (const std::exception &e) {
    wrong("%s: another exception type: %s", what, e.what());
  }
}

// ---- checks of a Hypothesis ----------------------------------------------------------------------------------------
// a translated sentence (translate, translate_samples): tokens, scores when `scored`, one-hot alignment rows when `aligned`
bool translated(const char *what, const Words &src, const Hypothesis &h, const Words &prefix, const want::Draw &d, bool scored,
                bool aligned) {
  const Words out = want::translation(src, h.padded_length, prefix, d);
  bool ok = h.target == out && h.padded_length >= src.size();
  if (scored) {
    ok = ok && h.scores.size() == out.size();
    for (size_t t = 0; ok && t < out.size(); ++t) ok = h.scores[t] == want::score(src, out[t], t);
  } else {
    ok = ok && h.scores.empty();
  }
  if (aligned) {
    ok = ok && h.alignment.size() == out.size();
    for (size_t t = 0; ok && t < out.size(); ++t) {
      ok = h.alignment[t].size() == src.size();
      const size_t col = want::aligned(src, out, t, prefix.empty() && !(d.temperature > 0.0f));
      for (size_t j = 0; ok && j < src.size(); ++j) ok = h.alignment[t][j] == (j == col ? 1.0f : 0.0f);
    }
  } else {
    ok = ok && h.alignment.empty();
  }
  if (!ok) wrong("%s: a sentence of %zu tokens came back wrong", what, src.size());
  return ok;
}

// a scored target (score, score_candidates)
bool scored_target(const char *what, const Words &src, const Words &tgt, const Hypothesis &h, size_t k, bool aligned) {
  bool ok = h.target == tgt && h.scores.size() == tgt.size() && h.padded_length >= src.size();
  for (size_t t = 0; ok && t < tgt.size(); ++t) ok = h.scores[t] == want::score(src, tgt[t], t);
  if (aligned) {
    ok = ok && h.alignment.size() == tgt.size();
    for (size_t t = 0; ok && t < tgt.size(); ++t) {
      ok = h.alignment[t].size() == src.size();
      for (size_t j = 0; ok && j < src.size(); ++j) ok = h.alignment[t][j] == want::score_alignment(src, j, tgt[t], t);
    }
  } else {
    ok = ok && h.alignment.empty();
  }
  ok = ok && h.alternatives == k && h.alt_ids.size() == tgt.size() * k && h.alt_scores.size() == tgt.size() * k &&
       h.ranks.size() == (k ? tgt.size() : 0);
  for (size_t t = 0; ok && k && t < tgt.size(); ++t) {
    ok = h.ranks[t] == want::rank(tgt[t], t);
    for (size_t i = 0; ok && i < k; ++i)
      ok = h.alt_ids[t * k + i] == want::alt_id(tgt[t], t, i) && h.alt_scores[t * k + i] == want::alt_score(tgt[t], t, i);
  }
  if (!ok) wrong("%s: a target of %zu tokens for a sentence of %zu came back wrong", what, tgt.size(), src.size());
  return ok;
}

bool same(const Hypothesis &a, const Hypothesis &b) {
  return a.target == b.target && a.scores == b.scores && a.alignment == b.alignment && a.padded_length == b.padded_length;
}

// ---- Service::score -------------------------------------------------------------------------------------------------
std::vector<Words> targets_for(std::mt19937 &rng, size_t n) {  // lengths 0, 1 and longer than any source among them
  std::vector<Words> targets(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t pick = (i + rng()) % 5;
    targets[i] = tokens(rng, pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? 20 : 1 + rng() % 12);
  }
  return targets;
}

size_t check_score(Service &service, std::mt19937 &rng, bool aligned) {
  size_t n = 0;
  for (size_t k : {0, 1, 8})
    for (int r = 0; r < 4; ++r) {
      std::vector<Words> sents = request(rng);
      if (r == 0) sents.resize(3, sentence(rng, 5));  // targets of 0, 1 and 20 tokens in one request
      std::vector<Words> targets = targets_for(rng, sents.size());
      if (r == 0) targets = {Words{}, tokens(rng, 1), tokens(rng, 20)};
      const Histories hs = service.score(sents, targets, k);
      if (hs.size() != sents.size()) wrong("score: %zu results for %zu sentences", hs.size(), sents.size());
      for (size_t i = 0; i < hs.size(); ++i) n += scored_target("score", sents[i], targets[i], *hs[i], k, aligned);
    }
  return n;
}

void score_refusals(Service &service) {
  const Words ok{5, 6, 0};
  refused<std::invalid_argument>("score, 9 alternatives", "9 alternatives: more than 8", [&] { service.score({ok}, {ok}, 9); });
  refused<std::invalid_argument>("score, counts", "1 targets for 2 sentences", [&] { service.score({ok, ok}, {ok}); });
  refused<std::invalid_argument>("score, empty sentence", "empty sentence (a sentence holds at least its EOS)",
                                 [&] { service.score({ok, Words{}}, {ok, ok}); });
  refused<std::invalid_argument>("score, long sentence", "sentence of 17 tokens: longer than 16 (wrap it first)",
                                 [&] { service.score({Words(17, 3)}, {ok}); });
  // the checks go sentence by sentence: sentence 0's target before sentence 1's emptiness
  refused<std::invalid_argument>("score, long target", "target of sentence 0: 65537 tokens, more than 65536",
                                 [&] { service.score({ok, Words{}}, {Words(65537, 3), ok}); });
  if (!service.score({}, {}).empty()) wrong("score: an empty request gave results");
}

// ---- Service::score_candidates ----------------------------------------------------------------------------------------
size_t check_candidates(Service &service, std::mt19937 &rng, bool aligned) {
  size_t n = 0;
  for (int mode = 0; mode < 2; ++mode)
    for (int r = 0; r < 5; ++r) {
      std::vector<Words> sents = request(rng);
      // r = 0: eight sentences of 16 tokens go as two batches of four; the first four have no candidates
      if (r == 0) {
        sents.resize(8);
        for (auto &s : sents) s = sentence(rng, 16);
      }
      std::vector<std::vector<Words>> cands(sents.size());
      for (size_t i = 0; i < sents.size(); ++i) {
        const size_t count = r == 0 ? (i < 4 ? 0 : 2) : r == 1 ? 0 : rng() % 4;  // r = 1: nobody has one
        for (size_t j = 0; j < count; ++j) cands[i].push_back(tokens(rng, rng() % 4 == 0 ? 0 : 1 + rng() % 20));
      }
      const Service::CandidateScores cs = service.score_candidates(sents, cands, mode);
      size_t at = 0;
      bool ok = cs.best.size() == sents.size();
      for (size_t i = 0; ok && i < sents.size(); ++i) {
        uint32_t best = kNone;
        float top = 0.0f;
        for (size_t j = 0; ok && j < cands[i].size(); ++j, ++at) {
          ok = at < cs.candidates.size() && cs.totals.size() == cs.candidates.size() &&
               scored_target("score_candidates", sents[i], cands[i][j], *cs.candidates[at], 0, aligned);
          float total = 0.0f;
          for (size_t t = 0; t < cands[i][j].size(); ++t) total = total + want::score(sents[i], cands[i][j][t], t);
          ok = ok && cs.totals[at] == total;
          if (cands[i][j].empty()) continue;
          const float key = mode == 1 ? total / static_cast<float>(cands[i][j].size()) : total;
          if (best == kNone || key > top) {
            top = key;
            best = static_cast<uint32_t>(j);
          }
          n += ok;
        }
        ok = ok && cs.best[i] == best;
      }
      if (!ok || at != cs.candidates.size()) wrong("score_candidates (mode %d, request %d): totals, best or the count are wrong", mode, r);
    }
  return n;
}

void candidates_refusals(Service &service) {
  const Words ok{5, 6, 0};
  refused<std::invalid_argument>("score_candidates, mode", "mode 2: neither 0 (sum) nor 1 (mean per token)",
                                 [&] { service.score_candidates({ok}, {{ok}}, 2); });
  refused<std::invalid_argument>("score_candidates, counts", "1 candidate lists for 2 sentences",
                                 [&] { service.score_candidates({ok, ok}, {{ok}}); });
  refused<std::invalid_argument>("score_candidates, empty sentence", "empty sentence (a sentence holds at least its EOS)",
                                 [&] { service.score_candidates({Words{}}, {{ok}}); });
  refused<std::invalid_argument>("score_candidates, long sentence", "sentence of 17 tokens: longer than 16 (wrap it first)",
                                 [&] { service.score_candidates({Words(17, 3)}, {{ok}}); });
  refused<std::invalid_argument>("score_candidates, long candidate", "candidate of sentence 1: 65537 tokens, more than 65536",
                                 [&] { service.score_candidates({ok, ok}, {{ok}, {ok, Words(65537, 3)}}); });
}

// ---- translate_samples and translate_consensus ---------------------------------------------------------------------
size_t check_samples(Service &service, std::mt19937 &rng, const want::Draw &draw, bool aligned) {
  size_t count = 0;
  for (size_t n : {1, 9, 64}) {  // 9: seven sentences per fan-out call (64 / 9); 64: one
    std::vector<Words> sents(9);
    for (auto &s : sents) s = sentence(rng, 3 + rng() % 4);  // one batch of nine: split for n = 9
    if (n != 9) sents = request(rng);
    const uint64_t seed = rng();
    const Histories hs = service.translate_samples(sents, n, seed);
    if (hs.size() != sents.size() * n) wrong("translate_samples: %zu results for %zu x %zu", hs.size(), sents.size(), n);
    for (size_t e = 0; e < hs.size(); ++e) {
      want::Draw d = draw;
      d.key = want::key(seed, e);  // i * n + j: the request's numbering
      count += translated("translate_samples", sents[e / n], *hs[e], {}, d, true, aligned);
    }
    // sentence 0 sent alone: the same samples
    const Histories alone = service.translate_samples({sents[0]}, n, seed);
    for (size_t j = 0; j < n; ++j)
      if (alone.size() != n || !(alone[j]->target == hs[j]->target && alone[j]->scores == hs[j]->scores && alone[j]->alignment == hs[j]->alignment))
        wrong("translate_samples: sample %zu of a sentence sent alone differs", j);
  }
  return count;
}

size_t check_consensus(Service &service, std::mt19937 &rng) {
  size_t count = 0, moved = 0;
  for (size_t n : {1, 5, 9, 64})
    for (int r = 0; r < 2; ++r) {
      std::vector<Words> sents = request(rng);
      if (n == 9) {  // one batch of nine: split into two fan-out calls
        sents.resize(9);
        for (auto &s : sents) s = sentence(rng, 3 + rng() % 4);
      }
      const uint64_t seed = rng();
      const Histories all = service.translate_samples(sents, n, seed);
      const Histories won = service.translate_consensus(sents, n, seed);
      if (won.size() != sents.size() || all.size() != sents.size() * n) {
        wrong("translate_consensus: %zu winners for %zu sentences", won.size(), sents.size());
        continue;
      }
      for (size_t i = 0; i < sents.size(); ++i) {
        std::vector<Words> rows;
        for (size_t j = 0; j < n; ++j) rows.push_back(all[i * n + j]->target);
        const auto [best, utility] = want::consensus(rows);
        const Hypothesis &h = *won[i];
        if (h.sample_index != best || h.utility != utility || !same(h, *all[i * n + h.sample_index]) || (n == 1 && h.utility != 0.0))
          wrong("translate_consensus: sentence %zu of %zu, n = %zu: sample %u with utility %g, not %u with %g", i, sents.size(), n,
                h.sample_index, h.utility, best, utility);
        else
          ++count;
        moved += h.sample_index != 0;
      }
    }
  if (moved == 0) wrong("translate_consensus: sample 0 won everywhere");
  return count;
}

void sampling_refusals(Service &sampling, Service &greedy) {
  const Words ok{5, 6, 0};
  refused<std::invalid_argument>("translate_samples, greedy", "translate_samples: the service does not sample (set_sampling first)",
                                 [&] { greedy.translate_samples({ok}, 2); });
  refused<std::invalid_argument>("translate_consensus, greedy", "translate_samples: the service does not sample (set_sampling first)",
                                 [&] { greedy.translate_consensus({ok}, 2); });
  refused<std::invalid_argument>("translate_samples, n = 65", "65 samples per sentence: not in 1..64", [&] { sampling.translate_samples({ok}, 65); });
  refused<std::invalid_argument>("translate_samples, n = 0", "0 samples per sentence: not in 1..64", [&] { sampling.translate_samples({ok}, 0); });
  refused<std::invalid_argument>("translate_samples, empty sentence", "empty sentence (a sentence holds at least its EOS)",
                                 [&] { sampling.translate_samples({Words{}}, 2); });
  refused<std::invalid_argument>("translate_samples, long sentence", "sentence of 17 tokens: longer than 16 (wrap it first)",
                                 [&] { sampling.translate_samples({Words(17, 3)}, 2); });
  refused<std::invalid_argument>("translate_consensus, n = 65", "65 samples per sentence: the consensus selection takes at most 64",
                                 [&] { sampling.translate_consensus({ok}, 65); });
  refused<std::invalid_argument>("translate_consensus, order", "consensus: max_order 5 or beta2 4 out of range",
                                 [&] { sampling.translate_consensus({ok}, 2, 0, 5, 4); });
  refused<std::invalid_argument>("translate_consensus, beta2", "consensus: max_order 4 or beta2 17 out of range",
                                 [&] { sampling.translate_consensus({ok}, 2, 0, 4, 17); });
  if (!sampling.translate_samples({}, 3).empty() || !sampling.translate_consensus({}, 3).empty()) wrong("an empty request gave samples");
}

// ---- the asynchronous translate with its options, from several threads, beside score callers ---------------------------
struct Mode {
  const char *name;
  size_t merge_batches;
  bool scores;
  want::Draw draw;  // temperature 0: greedy
};

size_t limit_of(const Words &s) { return std::max<size_t>(1, static_cast<size_t>(kLimit * static_cast<float>(s.size()))); }

size_t check_async(const Model &a, const Model &b, const Mode &mode, int clients, int requests) {
  ServiceConfig sc = small_config(true, 2);
  sc.merge_batches = mode.merge_batches;
  Service service(sc, {&a, &b});
  const bool sampled = mode.draw.temperature > 0.0f, truncated = mode.draw.top_k != 0 || mode.draw.top_p != 1.0f;
  if (mode.scores && !service.set_scores(true)) wrong("%s: set_scores refused", mode.name);
  if (sampled && !service.set_sampling(mode.draw.temperature)) wrong("%s: set_sampling refused", mode.name);
  if (truncated && !service.set_sampling_truncation(mode.draw.top_k, mode.draw.top_p)) wrong("%s: set_sampling_truncation refused", mode.name);
  if (service.set_sampling(-1.0f) || service.set_sampling_truncation(3, 0.0f)) wrong("%s: a bad sampling setting was accepted", mode.name);
  const long merged_before = fake_hip_merged_launches();
  std::atomic<size_t> good{0};
  std::vector<std::thread> ts;
  for (int c = 0; c < clients; ++c)
    ts.emplace_back([&, c]() {
      std::mt19937 rng(300 + c);
      if (c == clients - 1) {  // a scorer beside the translate callers: score_mu_ against mutex_
        for (int r = 0; r < requests; ++r) {
          const std::vector<Words> sents = request(rng), targets = targets_for(rng, sents.size());
          const Histories hs = service.score(sents, targets, r % 2 ? 8 : 0);
          for (size_t i = 0; i < hs.size(); ++i) good += scored_target(mode.name, sents[i], targets[i], *hs[i], r % 2 ? 8 : 0, true);
          if (sampled) {
            const uint64_t seed = rng();
            const Histories ss = service.translate_samples(sents, 3, seed);
            for (size_t e = 0; e < ss.size(); ++e) {
              want::Draw d = mode.draw;
              d.key = want::key(seed, e);
              good += translated(mode.name, sents[e / 3], *ss[e], {}, d, true, true);
            }
          }
        }
        return;
      }
      struct Sent {
        std::vector<Words> sents, prefixes;
        uint64_t seed;
        std::future<Histories> result;
      };
      std::vector<Sent> inflight;
      auto drain = [&]() {
        Sent &p = inflight.front();
        const Histories hs = p.result.get();
        if (hs.size() != p.sents.size()) wrong("%s: %zu results for %zu sentences", mode.name, hs.size(), p.sents.size());
        for (size_t i = 0; i < hs.size(); ++i) {
          want::Draw d = mode.draw;
          d.key = want::key(p.seed, i);
          good += translated(mode.name, p.sents[i], *hs[i], p.prefixes.empty() ? Words{} : p.prefixes[i], d, mode.scores, true);
        }
        inflight.erase(inflight.begin());
      };
      for (int r = 0; r < requests; ++r) {
        Sent s;
        s.sents = request(rng);
        if (r == 1) {  // ten batches of four at once: merged where the service merges
          s.sents.resize(40);
          for (auto &w : s.sents) w = sentence(rng, 16);
        }
        if (r % 3 != 2) {  // prefixes: some empty, one at its sentence's limit, the rest shorter
          s.prefixes.resize(s.sents.size());
          for (size_t i = 0; i < s.sents.size(); ++i)
            s.prefixes[i] = tokens(rng, i == 0 ? limit_of(s.sents[i]) : i % 3 == 1 ? 0 : rng() % (limit_of(s.sents[i]) + 1));
        }
        s.seed = sampled ? rng() : 0;
        s.result = sampled || r % 2 ? service.translate(s.sents, s.prefixes, s.seed) : service.translate(s.sents, s.prefixes);
        inflight.push_back(std::move(s));
        if (inflight.size() > 3) drain();
      }
      while (!inflight.empty()) drain();
      // a prefix over its sentence's limit, and a count that differs
      const Words two{7, 0};
      refused<std::invalid_argument>("translate, long prefix", "prefix of sentence 1: 4 tokens, more than 3",
                                     [&] { service.translate({two, two}, {Words{}, Words{9, 9, 9, 9}}); });
      refused<std::invalid_argument>("translate, prefix count", "1 prefixes for 2 sentences", [&] { service.translate({two, two}, {Words{}}); });
    });
  for (auto &t : ts) t.join();
  if (service.set_scores(false)) wrong("%s: set_scores accepted after the first translate", mode.name);
  const long merged = fake_hip_merged_launches() - merged_before;
  if ((mode.merge_batches == 1 || truncated) && merged != 0) wrong("%s: %ld merged launches", mode.name, merged);
  if (mode.merge_batches > 1 && !truncated && merged == 0) wrong("%s: no merged launch", mode.name);
  return good.load();
}

// ---- the C face -----------------------------------------------------------------------------------------------------
struct Flat {  // sentences as the C face takes them
  std::vector<uint32_t> tokens;
  std::vector<uint64_t> offsets{0};
  explicit Flat(const std::vector<Words> &rows) {
    for (const Words &w : rows) {
      tokens.insert(tokens.end(), w.begin(), w.end());
      offsets.push_back(tokens.size());
    }
    tokens.push_back(0);  // (never empty: data() is not NULL)
  }
};

void c_refused(const char *what, int rc, const std::string &message) {
  if (rc == 0) wrong("C face, %s: accepted", what);
  else if (message != slimt_hip_service_last_error()) wrong("C face, %s: \"%s\", not \"%s\"", what, slimt_hip_service_last_error(), message.c_str());
}

struct ResultView {  // slimt_hip_result_view of a result
  size_t n = 0;
  const uint32_t *targets = nullptr, *padded = nullptr;
  const uint64_t *target_offsets = nullptr, *batch = nullptr, *align_offsets = nullptr;
  const float *alignments = nullptr, *scores = nullptr;
  explicit ResultView(const slimt_hip_result *r) {
    if (slimt_hip_result_view(r, &n, &targets, &target_offsets, &padded, &batch, &alignments, &align_offsets) ||
        slimt_hip_result_scores(r, &scores))
      wrong("C face: result_view failed: %s", slimt_hip_service_last_error());
  }
  Hypothesis entry(size_t i, size_t src_len) const {  // entry i as the C++ face would return it
    Hypothesis h;
    h.target.assign(targets + target_offsets[i], targets + target_offsets[i + 1]);
    if (scores) h.scores.assign(scores + target_offsets[i], scores + target_offsets[i + 1]);
    h.padded_length = padded[i];
    const float *row = alignments + align_offsets[i];
    if (align_offsets[i + 1] - align_offsets[i] != h.target.size() * src_len) wrong("C face: alignment block of entry %zu", i);
    else
      for (size_t t = 0; t < h.target.size(); ++t, row += src_len) h.alignment.emplace_back(row, row + src_len);
    return h;
  }
};

size_t check_c_face(slimt_hip_model *model) {
  size_t good = 0;
  std::mt19937 rng(900);
  slimt_hip_service_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.max_words = 64;
  cfg.wrap_length = 16;
  cfg.limit_factor = kLimit;
  cfg.workers_per_device = 2;
  cfg.alignments = 1;
  slimt_hip_service *greedy = nullptr, *sampling = nullptr;
  slimt_hip_model *replicas[1] = {model};
  c_refused("create, null", slimt_hip_service_create(nullptr, replicas, 1, &greedy), "null argument");
  if (slimt_hip_service_create(&cfg, replicas, 1, &greedy) || slimt_hip_service_create(&cfg, replicas, 1, &sampling)) {
    wrong("C face: create failed: %s", slimt_hip_service_last_error());
    return 0;
  }
  c_refused("set_sampling_truncation, greedy", slimt_hip_service_set_sampling_truncation(sampling, 4, 0.5f),
            "set_sampling_truncation: the service does not sample (slimt_hip_service_set_sampling first)");
  if (slimt_hip_service_set_scores(greedy, 1) || slimt_hip_service_set_sampling(sampling, 0.7f) || slimt_hip_service_set_scores(sampling, 1))
    wrong("C face: a setting was refused: %s", slimt_hip_service_last_error());
  want::Draw draw;
  draw.temperature = 0.7f;

  const std::vector<Words> sents = {sentence(rng, 5), sentence(rng, 16), sentence(rng, 1), sentence(rng, 9)};
  const Flat src(sents);
  const size_t n = sents.size();
  slimt_hip_result *r = nullptr;
  const uint64_t decreasing[5] = {0, 5, 3, 6, 9};

  {  // translate_prefixed
    const std::vector<Words> prefixes = {tokens(rng, 3), Words{}, Words{}, tokens(rng, 13)};
    const Flat pre(prefixes);
    if (slimt_hip_service_translate_prefixed(greedy, src.tokens.data(), src.offsets.data(), pre.tokens.data(), pre.offsets.data(), n, &r)) {
      wrong("C face: translate_prefixed: %s", slimt_hip_service_last_error());
    } else {
      const ResultView v(r);
      for (size_t i = 0; i < n && v.n == n; ++i) good += translated("C translate_prefixed", sents[i], v.entry(i, sents[i].size()), prefixes[i], {}, true, true);
      size_t samples = 0;
      const float *totals = nullptr;
      const uint32_t *best = nullptr, *index = nullptr;
      const double *utility = nullptr;
      c_refused("result_samples of a translation", slimt_hip_result_samples(r, &samples), "result_samples: not a result of slimt_hip_service_translate_samples");
      c_refused("result_candidates of a translation", slimt_hip_result_candidates(r, &totals, &best), "result_candidates: not a result of slimt_hip_service_score_candidates");
      c_refused("result_consensus of a translation", slimt_hip_result_consensus(r, &utility, &index), "result_consensus: not a result of slimt_hip_service_translate_consensus");
      c_refused("result_alternatives of a translation", slimt_hip_result_alternatives(r, 0, nullptr, nullptr, nullptr, nullptr),
                "result_alternatives: not a result of slimt_hip_service_score_alternatives");
      slimt_hip_result_destroy(r);
    }
    c_refused("translate_prefixed, null", slimt_hip_service_translate_prefixed(greedy, src.tokens.data(), src.offsets.data(), pre.tokens.data(), nullptr, n, &r), "null argument");
    c_refused("translate_prefixed, offsets", slimt_hip_service_translate_prefixed(greedy, src.tokens.data(), decreasing, pre.tokens.data(), pre.offsets.data(), n, &r),
              "offsets decrease at sentence 1");
    c_refused("translate_prefixed, prefix offsets", slimt_hip_service_translate_prefixed(greedy, src.tokens.data(), src.offsets.data(), pre.tokens.data(), decreasing, n, &r),
              "prefix offsets decrease at sentence 1");
    c_refused("translate, null", slimt_hip_service_translate(greedy, nullptr, src.offsets.data(), n, &r), "null argument");
    c_refused("translate_sampled, greedy", slimt_hip_service_translate_sampled(greedy, src.tokens.data(), src.offsets.data(), nullptr, nullptr, 1, n, &r),
              "translate_sampled: the service does not sample (slimt_hip_service_set_sampling)");
  }
  {  // translate_sampled, with prefixes
    const std::vector<Words> prefixes = {Words{}, tokens(rng, 2), Words{}, tokens(rng, 4)};
    const Flat pre(prefixes);
    if (slimt_hip_service_translate_sampled(sampling, src.tokens.data(), src.offsets.data(), pre.tokens.data(), pre.offsets.data(), 77, n, &r)) {
      wrong("C face: translate_sampled: %s", slimt_hip_service_last_error());
    } else {
      const ResultView v(r);
      for (size_t i = 0; i < n && v.n == n; ++i) {
        draw.key = want::key(77, i);
        good += translated("C translate_sampled", sents[i], v.entry(i, sents[i].size()), prefixes[i], draw, true, true);
      }
      slimt_hip_result_destroy(r);
    }
    c_refused("translate_sampled, offsets", slimt_hip_service_translate_sampled(sampling, src.tokens.data(), decreasing, nullptr, nullptr, 77, n, &r),
              "offsets decrease at sentence 1");
  }
  const std::vector<Words> targets = {tokens(rng, 20), Words{}, tokens(rng, 1), tokens(rng, 7)};
  const Flat tgt(targets);
  for (uint32_t k : {0u, 8u}) {  // score and score_alternatives
    const int rc = k ? slimt_hip_service_score_alternatives(greedy, src.tokens.data(), src.offsets.data(), tgt.tokens.data(), tgt.offsets.data(), n, k, &r)
                     : slimt_hip_service_score(greedy, src.tokens.data(), src.offsets.data(), tgt.tokens.data(), tgt.offsets.data(), n, &r);
    if (rc) {
      wrong("C face: score (k = %u): %s", k, slimt_hip_service_last_error());
      continue;
    }
    const ResultView v(r);
    for (size_t i = 0; i < n && v.n == n; ++i) {
      Hypothesis h = v.entry(i, sents[i].size());
      if (k) {
        uint32_t got = 0;
        const uint32_t *ids = nullptr, *ranks = nullptr;
        const float *scores = nullptr;
        if (slimt_hip_result_alternatives(r, i, &got, &ids, &scores, &ranks)) wrong("C face: result_alternatives: %s", slimt_hip_service_last_error());
        h.alternatives = got;
        h.alt_ids.assign(ids, ids + h.target.size() * got);
        h.alt_scores.assign(scores, scores + h.target.size() * got);
        h.ranks.assign(ranks, ranks + h.target.size());
      }
      good += scored_target("C score", sents[i], targets[i], h, k, true);
    }
    if (k) c_refused("result_alternatives, sentence", slimt_hip_result_alternatives(r, n, nullptr, nullptr, nullptr, nullptr), "result_alternatives: sentence 4 of 4");
    slimt_hip_result_destroy(r);
  }
  c_refused("score, null", slimt_hip_service_score(greedy, src.tokens.data(), src.offsets.data(), tgt.tokens.data(), nullptr, n, &r), "null argument");
  c_refused("score, offsets", slimt_hip_service_score(greedy, src.tokens.data(), decreasing, tgt.tokens.data(), tgt.offsets.data(), n, &r),
            "offsets decrease at sentence 1");
  c_refused("score, target offsets", slimt_hip_service_score(greedy, src.tokens.data(), src.offsets.data(), tgt.tokens.data(), decreasing, n, &r),
            "target offsets decrease at sentence 1");
  c_refused("score_alternatives, k", slimt_hip_service_score_alternatives(greedy, src.tokens.data(), src.offsets.data(), tgt.tokens.data(), tgt.offsets.data(), n, 9, &r),
            "score_alternatives: k 9 is not in 1..8");
  {  // score_candidates: sentence 0 has two, sentence 1 none, sentence 2 one, sentence 3 three (one of them empty)
    const std::vector<Words> cands = {tokens(rng, 4), tokens(rng, 18), tokens(rng, 2), tokens(rng, 6), Words{}, tokens(rng, 3)};
    const size_t owner[6] = {0, 0, 2, 3, 3, 3};
    const uint64_t cand_offsets[5] = {0, 2, 2, 3, 6};
    const Flat cand(cands);
    if (slimt_hip_service_score_candidates(greedy, src.tokens.data(), src.offsets.data(), n, cand.tokens.data(), cand.offsets.data(), cand_offsets, 1, &r)) {
      wrong("C face: score_candidates: %s", slimt_hip_service_last_error());
    } else {
      const ResultView v(r);
      const float *totals = nullptr;
      const uint32_t *best = nullptr;
      if (slimt_hip_result_candidates(r, &totals, &best) || v.n != cands.size()) {
        wrong("C face: result_candidates: %s", slimt_hip_service_last_error());
      } else {
        std::vector<uint32_t> want_best(n, kNone);
        std::vector<float> top(n, 0.0f);
        for (size_t c = 0; c < cands.size(); ++c) {
          const Words &s = sents[owner[c]];
          good += scored_target("C score_candidates", s, cands[c], v.entry(c, s.size()), 0, true);
          float total = 0.0f;
          for (size_t t = 0; t < cands[c].size(); ++t) total = total + want::score(s, cands[c][t], t);
          if (totals[c] != total) wrong("C face: total of candidate %zu", c);
          if (cands[c].empty()) continue;
          const float key = total / static_cast<float>(cands[c].size());
          if (want_best[owner[c]] == kNone || key > top[owner[c]]) {
            top[owner[c]] = key;
            want_best[owner[c]] = static_cast<uint32_t>(c - cand_offsets[owner[c]]);
          }
        }
        for (size_t i = 0; i < n; ++i)
          if (best[i] != want_best[i]) wrong("C face: best candidate of sentence %zu", i);
      }
      slimt_hip_result_destroy(r);
    }
    const uint64_t late[5] = {1, 2, 2, 3, 6}, back[5] = {0, 2, 1, 3, 6};
    c_refused("score_candidates, null", slimt_hip_service_score_candidates(greedy, src.tokens.data(), src.offsets.data(), n, cand.tokens.data(), cand.offsets.data(), nullptr, 0, &r),
              "null argument");
    c_refused("score_candidates, first offset", slimt_hip_service_score_candidates(greedy, src.tokens.data(), src.offsets.data(), n, cand.tokens.data(), cand.offsets.data(), late, 0, &r),
              "candidate offsets start at 1, not 0");
    c_refused("score_candidates, candidate offsets", slimt_hip_service_score_candidates(greedy, src.tokens.data(), src.offsets.data(), n, cand.tokens.data(), cand.offsets.data(), back, 0, &r),
              "candidate offsets decrease at sentence 1");
    const uint64_t bad_tgt[7] = {0, 4, 22, 21, 30, 30, 33};
    c_refused("score_candidates, target offsets", slimt_hip_service_score_candidates(greedy, src.tokens.data(), src.offsets.data(), n, cand.tokens.data(), bad_tgt, cand_offsets, 0, &r),
              "target offsets decrease at candidate 2");
    c_refused("score_candidates, offsets", slimt_hip_service_score_candidates(greedy, src.tokens.data(), decreasing, n, cand.tokens.data(), cand.offsets.data(), cand_offsets, 0, &r),
              "offsets decrease at sentence 1");
    c_refused("score_candidates, mode", slimt_hip_service_score_candidates(greedy, src.tokens.data(), src.offsets.data(), n, cand.tokens.data(), cand.offsets.data(), cand_offsets, 2, &r),
              "mode 2: neither 0 (sum) nor 1 (mean per token)");
  }
  {  // translate_samples and translate_consensus
    const size_t samples = 5;
    slimt_hip_result *all = nullptr;
    if (slimt_hip_service_translate_samples(sampling, src.tokens.data(), src.offsets.data(), n, samples, 31, &all) ||
        slimt_hip_service_translate_consensus(sampling, src.tokens.data(), src.offsets.data(), n, samples, 31, 4, 4, &r)) {
      wrong("C face: translate_samples / _consensus: %s", slimt_hip_service_last_error());
    } else {
      const ResultView va(all), vw(r);
      size_t got = 0;
      const double *utility = nullptr;
      const uint32_t *index = nullptr;
      if (slimt_hip_result_samples(all, &got) || got != samples || va.n != n * samples || vw.n != n || slimt_hip_result_consensus(r, &utility, &index)) {
        wrong("C face: result_samples / result_consensus: %s", slimt_hip_service_last_error());
      } else {
        for (size_t i = 0; i < n; ++i) {
          std::vector<Words> rows;
          for (size_t j = 0; j < samples; ++j) {
            draw.key = want::key(31, i * samples + j);
            const Hypothesis h = va.entry(i * samples + j, sents[i].size());
            good += translated("C translate_samples", sents[i], h, {}, draw, true, true);
            rows.push_back(h.target);
          }
          const auto [best, u] = want::consensus(rows);
          if (index[i] != best || utility[i] != u || !same(vw.entry(i, sents[i].size()), va.entry(i * samples + best, sents[i].size())))
            wrong("C face: consensus of sentence %zu", i);
          else
            ++good;
        }
      }
      size_t none = 0;
      c_refused("result_samples of a consensus", slimt_hip_result_samples(r, &none), "result_samples: not a result of slimt_hip_service_translate_samples");
      c_refused("result_consensus of samples", slimt_hip_result_consensus(all, &utility, &index), "result_consensus: not a result of slimt_hip_service_translate_consensus");
      c_refused("result_consensus, null", slimt_hip_result_consensus(r, nullptr, &index), "null argument");
      slimt_hip_result_destroy(r);
    }
    slimt_hip_result_destroy(all);
    c_refused("translate_samples, null", slimt_hip_service_translate_samples(sampling, src.tokens.data(), nullptr, n, 2, 0, &r), "null argument");
    c_refused("translate_samples, offsets", slimt_hip_service_translate_samples(sampling, src.tokens.data(), decreasing, n, 2, 0, &r), "offsets decrease at sentence 1");
    c_refused("translate_samples, n", slimt_hip_service_translate_samples(sampling, src.tokens.data(), src.offsets.data(), n, 65, 0, &r),
              "65 samples per sentence: not in 1..64");
    c_refused("translate_consensus, null", slimt_hip_service_translate_consensus(sampling, src.tokens.data(), src.offsets.data(), n, 2, 0, 4, 4, nullptr), "null argument");
    c_refused("translate_consensus, offsets", slimt_hip_service_translate_consensus(sampling, src.tokens.data(), decreasing, n, 2, 0, 4, 4, &r),
              "offsets decrease at sentence 1");
    c_refused("translate_consensus, n", slimt_hip_service_translate_consensus(sampling, src.tokens.data(), src.offsets.data(), n, 65, 0, 4, 4, &r),
              "65 samples per sentence: the consensus selection takes at most 64");
    c_refused("translate_samples, greedy", slimt_hip_service_translate_samples(greedy, src.tokens.data(), src.offsets.data(), n, 2, 0, &r),
              "translate_samples: the service does not sample (set_sampling first)");
  }
  c_refused("set_scores, late", slimt_hip_service_set_scores(greedy, 0), "set_scores: only before the first slimt_hip_service_translate");
  c_refused("set_sampling, late", slimt_hip_service_set_sampling(sampling, 0.5f), "set_sampling: only before the first slimt_hip_service_translate");
  c_refused("set_sampling, zero", slimt_hip_service_set_sampling(sampling, 0.0f), "set_sampling: temperature 0 is not finite and > 0");
  c_refused("set_sampling_truncation, top_p", slimt_hip_service_set_sampling_truncation(sampling, 4, 1.5f), "set_sampling_truncation: top_p 1.5 is not in (0, 1]");
  c_refused("set_sampling_truncation, late", slimt_hip_service_set_sampling_truncation(sampling, 4, 0.5f),
            "set_sampling_truncation: only before the first slimt_hip_service_translate");
  slimt_hip_service_destroy(greedy);
  slimt_hip_service_destroy(sampling);
  return good;
}
}  // namespace

// Returns the number of wrong values or messages (each printed as a WRONG: line); prints one summary line per call kind.
int service_calls(const Model &a, const Model &b, slimt_hip_model *handle, int clients, int requests) {
  for (int aligned = 0; aligned < 2; ++aligned) {
    std::mt19937 rng(500 + aligned);
    Service greedy(small_config(aligned != 0), {&a});
    std::printf("score (alignments %d): %zu targets right\n", aligned, check_score(greedy, rng, aligned != 0));
    std::printf("score_candidates (alignments %d): %zu candidates right\n", aligned, check_candidates(greedy, rng, aligned != 0));
    Service sampling(small_config(aligned != 0), {&a});
    want::Draw draw;
    draw.temperature = 0.8f;
    if (aligned) {  // ... and once truncated
      draw.top_k = 5;
      draw.top_p = 0.9f;
    }
    if (!sampling.set_sampling(draw.temperature) || (aligned && !sampling.set_sampling_truncation(draw.top_k, draw.top_p)))
      wrong("a sampling setting was refused");
    std::printf("translate_samples (alignments %d): %zu samples right\n", aligned, check_samples(sampling, rng, draw, aligned != 0));
    std::printf("translate_consensus (alignments %d): %zu winners right\n", aligned, check_consensus(sampling, rng));
    if (aligned) {
      score_refusals(greedy);
      candidates_refusals(greedy);
      sampling_refusals(sampling, greedy);
    }
  }
  {  // a service with a lexical shortlist: the calls that generate each batch's list on the device
    std::mt19937 rng(600);
    ServiceConfig sc = small_config(true);
    const char blob[8] = {0};
    sc.lexical_shortlist = slimt::View{blob, sizeof(blob)};
    sc.source_vocab = sc.target_vocab = 512;
    Service lexical(sc, {&a});
    if (!lexical.set_sampling(0.8f)) wrong("a sampling setting was refused");
    want::Draw draw;
    draw.temperature = 0.8f;
    const size_t n = check_score(lexical, rng, true) + check_candidates(lexical, rng, true) + check_samples(lexical, rng, draw, true) + check_consensus(lexical, rng);
    std::printf("generated shortlists: %zu results right\n", n);
  }
  want::Draw sampled, truncated;
  sampled.temperature = 0.6f;
  truncated.temperature = 1.3f;
  truncated.top_k = 7;
  truncated.top_p = 0.95f;
  const Mode modes[] = {{"prefixes, merged", 8, true, {}},       {"prefixes, one batch a launch", 1, false, {}},
                        {"sampled, merged", 8, true, sampled},   {"sampled, one batch a launch", 1, true, sampled},
                        {"truncated, never merged", 8, false, truncated}};
  for (const Mode &m : modes) std::printf("translate (%s): %zu results right\n", m.name, check_async(a, b, m, clients, requests));
  std::printf("C face: %zu results right\n", check_c_face(handle));
  std::printf("service calls: %d wrong\n", g_wrong.load());
  return g_wrong.load();
}
