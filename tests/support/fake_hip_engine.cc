// TEST DOUBLE of the engine-level C ABI (include/slimt_hip.h), CPU only: just enough for
// host/Service.{hh,cc} to run WITHOUT a GPU, so that its threading (queue, double-buffered workers,
// retiring workers, futures) and its index arithmetic can be exercised under ThreadSanitizer /
// AddressSanitizer in the CPU test suite. Not the product and never linked into it. A call completes on
// a helper thread after a short sleep, like a kernel would on a stream.
//
// Every value is a deterministic function of what it belongs to, so that a value delivered to the wrong
// sentence, candidate, sample, key or offset comes out different:
//  * translate: a plain row (no prefix, not sampled) is its own tokens reversed (EOS kept last), capped at
//    max(1, floor(limit_factor * S)), its alignment row t one-hot on source position (len - 2 - t) (or the
//    EOS column). A forced row records its prefix (ending at a forced EOS), then goes on to max(its prefix,
//    its plain length) tokens + EOS; the tokens behind the prefix, and all tokens of a sampled row, are the
//    plain ones shifted by a hash of the prefix, the key, the temperature, the truncation and the position;
//    their alignment rows are one-hot on (token + t) % len. score[t] = fake score of (row, token, t);
//  * score calls: score[t] of (row, target token, t), alignment (source token, target token, t), k
//    alternatives and a rank of (target token, t); nothing is written at t >= tgt_len or columns >= lengths[b];
//  * fan-out: row r is the translate row of source row_src[r] under row r's options; the consensus utility of
//    a row is the mean over its source's other rows of a symmetric function of the two rows' tokens, best
//    the lowest row with the largest utility.
// Options armed with slimt_hip_ctx_set_* are taken and cleared by the next translate (or score) call,
// whatever its outcome.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <future>
#include <thread>
#include <vector>

#include "slimt_hip.h"

namespace {
constexpr uint32_t kVocab = 512;

struct Armed {  // what the next translate call takes
  std::vector<float *> scores;
  std::vector<const uint32_t *> prefix_ids, prefix_len;
  bool sampled = false;
  float temperature = 0.0f;
  bool keyed = false;  // (keys == NULL: a sentence's key is its row)
  std::vector<const uint64_t *> keys;
  size_t n_keys = 0;
  bool truncated = false;
  uint32_t top_k = 0;
  float top_p = 1.0f;
  bool consensus = false;
  uint32_t *best = nullptr;
  double *utility = nullptr;
};
struct Alternatives {  // what the next score call takes
  uint32_t k = 0;
  uint32_t *ids = nullptr;
  float *scores = nullptr;
  uint32_t *rank = nullptr;
};
}  // namespace

struct slimt_hip_model { int device = 0; int heads = 2; std::atomic<int> contexts{0}; };
struct slimt_hip_ctx {
  slimt_hip_model *model;
  size_t max_B, max_S, max_M;
  std::future<void> pending;
  Armed armed;
  Alternatives alternatives;
};
struct slimt_hip_shortlist { int device = 0; };

static thread_local char g_err[256] = "";
static int fail(const char *m) { std::strncpy(g_err, m, sizeof(g_err) - 1); return -1; }
static std::atomic<long> g_host_allocs{0};
static std::atomic<long> g_merged_launches{0};

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// what identifies a source row: its tokens, each with its place
static uint64_t row_sum(const uint32_t *src, size_t len) {
  uint64_t s = 0;
  for (size_t j = 0; j < len; ++j) s += (j + 1) * (uint64_t)src[j];
  return s;
}
static float fake_score(uint64_t row, uint32_t token, size_t t) { return -(float)(1 + (row + 31ull * token + 7ull * t) % 1000) / 64.0f; }

// one row's options in a translate call
struct RowOptions {
  const uint32_t *prefix = nullptr;
  uint32_t P = 0;
  bool sampled = false;
  uint64_t key = 0;
  uint64_t call = 0;  // the temperature and the truncation of a sampled call
  float *scores = nullptr;
};

// one row's "translation"; out [T], align nullable [T][S]
static void fake_row(const uint32_t *src, size_t len, size_t S, size_t T, uint32_t eos, const RowOptions &o, uint32_t *out,
                     uint32_t *out_len, float *align) {
  const bool plain = !o.sampled && o.P == 0;
  uint64_t h = 0;
  for (uint32_t t = 0; t < o.P; ++t) h = mix(h ^ o.prefix[t]);
  if (o.sampled) h = mix(mix(h ^ o.key) ^ o.call);
  size_t n = std::min(T, std::max<size_t>(o.P, std::min(len - 1, T - 1)) + 1);
  for (uint32_t t = 0; t < o.P; ++t)
    if (o.prefix[t] == eos) { n = t + 1; break; }
  for (size_t t = 0; t < n; ++t) {
    const uint32_t base = t + 1 < len ? src[len - 2 - t] : (uint32_t)(7 * t + 1);
    if (t < o.P) out[t] = o.prefix[t];
    else if (t + 1 == n) out[t] = eos;
    else out[t] = plain ? base : 2 + (uint32_t)((base + mix(h + t)) % 500);
  }
  for (size_t t = n; t < T; ++t) out[t] = 0;
  *out_len = (uint32_t)n;
  if (o.scores) {
    const uint64_t row = row_sum(src, len);
    for (size_t t = 0; t < n; ++t) o.scores[t] = fake_score(row, out[t], t);
  }
  if (align) {
    std::fill(align, align + T * S, 0.0f);
    for (size_t t = 0; t < n; ++t) {
      const size_t col = plain ? (t + 1 < n && len >= 2 + t ? len - 2 - t : len - 1) : (out[t] + t) % len;
      align[t * S + col] = 1.0f;
    }
  }
}

// one row of a score call: nothing at t >= n, no alignment column >= len
static void score_row(const uint32_t *src, size_t len, size_t S, const uint32_t *tgt, size_t n, float *scores, float *align,
                      const Alternatives &alt, size_t alt_at) {
  const uint64_t row = row_sum(src, len);
  for (size_t t = 0; t < n; ++t) {
    scores[t] = fake_score(row, tgt[t], t);
    if (align)
      for (size_t j = 0; j < len; ++j) align[t * S + j] = (float)(1 + (src[j] + 3 * t + tgt[t]) % 64) / 64.0f;
    for (uint32_t i = 0; i < alt.k; ++i) {
      alt.ids[(alt_at + t) * alt.k + i] = (uint32_t)((tgt[t] + 13 * t + 17 * i + 1) % kVocab);
      if (alt.scores) alt.scores[(alt_at + t) * alt.k + i] = -(float)(i + 1 + (tgt[t] + t) % 5) / 8.0f;
    }
    if (alt.k && alt.rank) alt.rank[alt_at + t] = (uint32_t)((tgt[t] + 3 * t) % 11);
  }
}

static int check_one(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, const void *out_ids,
                     const void *out_len) {
  if (!c || !ids || !lengths || !out_ids || !out_len) return fail("null argument");
  if (B == 0 || S == 0 || B > c->max_B || S > c->max_S || B * S > c->max_M) return fail("batch exceeds the context's workspace");
  for (size_t b = 0; b < B; ++b) {
    if (lengths[b] == 0 || lengths[b] > S) return fail("sentence length out of range");
    for (size_t j = 0; j < lengths[b]; ++j)
      if (ids[b * S + j] >= kVocab) return fail("token id out of range");
  }
  return 0;
}

// one batch of a translate call: B sources, N rows (row_src NULL: row r is source r), its place j among the call's batches
struct Rows {
  const uint32_t *ids, *lengths;
  size_t B, S;
  const uint32_t *row_src;
  size_t N;
  uint32_t *out_ids, *out_len;
  float *align;
};

static int check_armed(const Armed &a, const Rows *batches, size_t n, float limit, bool fanout) {
  if (!a.scores.empty() && a.scores.size() != n) return fail("scores armed for another number of batches");
  if (!a.prefix_ids.empty() && a.prefix_ids.size() != n) return fail("prefixes armed for another number of batches");
  if (a.sampled && a.keyed && a.n_keys != n) return fail("sampling keys armed for another number of batches");
  if (a.truncated && !a.sampled) return fail("sampling truncation armed without sampling");
  if (a.consensus && !fanout) return fail("consensus armed for a call that is not a fan-out call");
  for (size_t j = 0; j < n; ++j) {
    const Rows &r = batches[j];
    const size_t T = std::max<size_t>(1, (size_t)(limit * (float)r.S));
    if (a.consensus && T > SLIMT_HIP_CONSENSUS_MAX_T) return fail("consensus: rows longer than SLIMT_HIP_CONSENSUS_MAX_T");
    if (!a.scores.empty() && !a.scores[j]) return fail("scores: NULL entry");
    if (a.prefix_ids.empty()) continue;
    if (!a.prefix_ids[j] || !a.prefix_len[j]) return fail("prefixes: NULL entry");
    for (size_t i = 0; i < r.N; ++i) {
      if (a.prefix_len[j][i] > T) return fail("prefix longer than the row of outputs");
      for (uint32_t t = 0; t < a.prefix_len[j][i]; ++t)
        if (a.prefix_ids[j][i * T + t] >= kVocab) return fail("prefix id out of range");
    }
  }
  return 0;
}

static void translate_rows(const Rows &r, size_t j, const Armed &a, float limit, uint32_t eos) {
  const size_t T = std::max<size_t>(1, (size_t)(limit * (float)r.S));
  uint64_t call = mix(bits(a.temperature));
  if (a.truncated) call = mix(mix(call ^ a.top_k) ^ bits(a.top_p));
  for (size_t i = 0; i < r.N; ++i) {
    const size_t b = r.row_src ? r.row_src[i] : i;
    RowOptions o;
    if (!a.prefix_ids.empty()) {
      o.prefix = a.prefix_ids[j] + i * T;
      o.P = a.prefix_len[j][i];
    }
    o.sampled = a.sampled;
    o.key = a.keyed && a.keys[j] ? a.keys[j][i] : i;
    o.call = call;
    o.scores = a.scores.empty() ? nullptr : a.scores[j] + i * T;
    fake_row(r.ids + b * r.S, r.lengths[b], r.S, T, eos, o, r.out_ids + i * T, r.out_len + i, r.align ? r.align + i * T * r.S : nullptr);
  }
  if (!a.consensus) return;
  std::vector<uint64_t> sum(r.N, 0);  // what identifies a row's tokens
  for (size_t i = 0; i < r.N; ++i)
    for (size_t t = 0; t < r.out_len[i]; ++t) sum[i] += (t + 1) * (uint64_t)r.out_ids[i * T + t];
  std::fill(a.best, a.best + r.B, 0xFFFFFFFFu);
  for (size_t i = 0; i < r.N; ++i) {
    double total = 0.0;
    size_t others = 0;
    for (size_t o = 0; o < r.N; ++o)
      if (o != i && r.row_src[o] == r.row_src[i]) {
        total += (double)((sum[i] ^ sum[o]) % 17) / 16.0;
        ++others;
      }
    a.utility[i] = others ? total / (double)others : 0.0;
    uint32_t &best = a.best[r.row_src[i]];
    if (best == 0xFFFFFFFFu || a.utility[i] > a.utility[best]) best = (uint32_t)i;
  }
}

// a translate call of n batches: takes what was armed, whatever its outcome
static int run(slimt_hip_ctx *c, std::vector<Rows> batches, float limit, uint32_t eos, bool wait, bool fanout = false) {
  if (!c) return fail("ctx is NULL");
  const Armed armed = std::move(c->armed);
  c->armed = Armed();
  for (const Rows &r : batches)
    if (int rc = check_one(c, r.ids, r.lengths, r.B, r.S, r.out_ids, r.out_len)) return rc;
  if (int rc = check_armed(armed, batches.data(), batches.size(), limit, fanout)) return rc;
  const size_t work = batches.size() > 1 ? batches.size() : batches[0].B;
  c->pending = std::async(std::launch::async, [=]() {
    std::this_thread::sleep_for(std::chrono::microseconds(200 + 13 * (work % 7)));
    for (size_t j = 0; j < batches.size(); ++j) translate_rows(batches[j], j, armed, limit, eos);
  });
  if (wait) c->pending.get();
  return 0;
}

static int run_one(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, float limit, uint32_t eos,
                   uint32_t *out_ids, uint32_t *out_len, float *align, bool wait) {
  return run(c, {Rows{ids, lengths, B, S, nullptr, B, out_ids, out_len, align}}, limit, eos, wait);
}

// several batches in one "launch pair" (include/slimt_hip.h, slimt_hip_translate_many_async): each with its own padded
// length, arrays, results and armed options, all of them completed by the one asynchronous task
static int run_many(slimt_hip_ctx *c, const slimt_hip_batch *batches, size_t n, size_t S, float limit, uint32_t eos) {
  if (!c || !batches || n == 0) {
    if (c) c->armed = Armed();
    return fail("null argument");
  }
  std::vector<Rows> rows;
  size_t total = 0;
  int rc = 0;
  for (size_t j = 0; j < n && !rc; ++j) {
    const slimt_hip_batch &b = batches[j];
    const size_t own = b.S ? b.S : S;
    if (own > S) rc = fail("a batch is padded to more tokens than the launch");
    rows.push_back(Rows{b.src_ids, b.lengths, b.B, own, nullptr, b.B, b.out_ids, b.out_len, b.align});
    total += b.B;
  }
  if (!rc && (total > c->max_B || total * S > c->max_M)) rc = fail("merged batches exceed the context's workspace");
  if (rc) {
    c->armed = Armed();
    return rc;
  }
  if (n > 1) g_merged_launches += 1;
  return run(c, std::move(rows), limit, eos, false);
}

static int run_fanout(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, const uint32_t *row_src,
                      size_t N, float limit, uint32_t eos, uint32_t *out_ids, uint32_t *out_len, float *align, bool wait) {
  int rc = 0;
  if (!c) return fail("ctx is NULL");
  if (!row_src) rc = fail("null argument");
  else if (N == 0 || N > c->max_B) rc = fail("fan-out rows exceed the context's workspace");
  for (size_t r = 0; r < N && !rc; ++r)
    if (row_src[r] >= B) rc = fail("row_src out of range");
  if (rc) {
    c->armed = Armed();
    return rc;
  }
  return run(c, {Rows{ids, lengths, B, S, row_src, N, out_ids, out_len, align}}, limit, eos, wait, true);
}

// a score call over N candidates (cand_src NULL: candidate c is source c): takes the armed alternatives, whatever its outcome
static int run_score(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, const uint32_t *tgt_ids,
                     const uint32_t *tgt_len, size_t T, const uint32_t *cand_src, size_t N, float *scores, float *align, bool wait) {
  if (!c) return fail("ctx is NULL");
  const Alternatives alt = c->alternatives;
  c->alternatives = Alternatives();
  if (int rc = check_one(c, ids, lengths, B, S, ids, lengths)) return rc;
  if (N == 0) return 0;
  if (!tgt_ids || !tgt_len || !scores) return fail("null argument");
  if (T == 0 || T > 65536 || N * T > (1u << 24)) return fail("target rows out of range");
  for (size_t i = 0; i < N; ++i) {
    if (cand_src && cand_src[i] >= B) return fail("cand_src out of range");
    if (tgt_len[i] > T) return fail("target longer than its row");
    for (size_t t = 0; t < tgt_len[i]; ++t)
      if (tgt_ids[i * T + t] >= kVocab) return fail("target id out of range");
  }
  c->pending = std::async(std::launch::async, [=]() {
    std::this_thread::sleep_for(std::chrono::microseconds(200 + 13 * (N % 7)));
    for (size_t i = 0; i < N; ++i) {
      const size_t b = cand_src ? cand_src[i] : i;
      score_row(ids + b * S, lengths[b], S, tgt_ids + i * T, tgt_len[i], scores + i * T, align ? align + i * T * S : nullptr, alt, i * T);
    }
  });
  if (wait) c->pending.get();
  return 0;
}

extern "C" {
long fake_hip_merged_launches(void) { return g_merged_launches.load(); }  // (the tests': _many_ calls of more than one batch)
const char *slimt_hip_last_error(void) { return g_err; }
int slimt_hip_model_create(const slimt_hip_param *, size_t, const slimt_hip_dims *dims, int device, slimt_hip_model **out) {
  auto *m = new slimt_hip_model();
  m->device = device;
  if (dims) m->heads = dims->num_heads;
  *out = m;
  return 0;
}
int slimt_hip_model_destroy(slimt_hip_model *m) { delete m; return 0; }
int slimt_hip_model_device(const slimt_hip_model *m) { return m ? m->device : -1; }
int slimt_hip_hw_queues(void) { return 32; }
int slimt_hip_request_hw_queues(int) { return 0; }
int slimt_hip_model_info(const slimt_hip_model *m, int32_t *d, int32_t *f, int32_t *v, int32_t *h) {
  if (!m) return fail("model is NULL");
  if (d) *d = 64;
  if (f) *f = 128;
  if (v) *v = kVocab;
  if (h) *h = m->heads;
  return 0;
}
int slimt_hip_ctx_create_budget(slimt_hip_model *model, size_t max_batch, size_t max_len, size_t max_tokens, void *,
                                slimt_hip_ctx **out) {
  if (!model) return fail("model is NULL");
  if (std::getenv("FAKE_HIP_FAIL_CTX_AFTER")) {  // the Nth context and every later one cannot be built
    if (model->contexts.fetch_add(1) >= std::atoi(std::getenv("FAKE_HIP_FAIL_CTX_AFTER"))) return fail("fake: out of device memory");
  }
  *out = new slimt_hip_ctx{model, max_batch, max_len, max_tokens, {}, {}, {}};
  return 0;
}
int slimt_hip_ctx_destroy(slimt_hip_ctx *c) {
  if (c && c->pending.valid()) c->pending.wait();
  delete c;
  return 0;
}
int slimt_hip_ctx_synchronize(slimt_hip_ctx *c) {
  if (!c) return fail("ctx is NULL");
  if (c->pending.valid()) c->pending.get();
  return 0;
}
int slimt_hip_host_alloc(size_t bytes, void **out) {
  *out = std::malloc(bytes ? bytes : 1);
  g_host_allocs += 1;
  return *out ? 0 : fail("malloc");
}
int slimt_hip_host_free(void *p) { std::free(p); return 0; }

// the per-call options: recorded here, taken by the next translate (the alternatives: score) call
int slimt_hip_ctx_set_scores(slimt_hip_ctx *c, float *const *scores, size_t n) {
  if (!c || (n && !scores)) return fail("null argument");
  c->armed.scores.assign(scores, scores + n);
  return 0;
}
int slimt_hip_ctx_set_target_prefix(slimt_hip_ctx *c, const uint32_t *const *ids, const uint32_t *const *len, size_t n) {
  if (!c || (n && (!ids || !len))) return fail("null argument");
  c->armed.prefix_ids.assign(ids, ids + n);
  c->armed.prefix_len.assign(len, len + n);
  return 0;
}
uint64_t slimt_hip_sampling_key(uint64_t seed, uint64_t index) { return mix(mix(seed) + index); }
int slimt_hip_ctx_set_sampling(slimt_hip_ctx *c, float temperature, const uint64_t *const *keys, size_t n) {
  if (!c) return fail("ctx is NULL");
  if (!(temperature > 0.0f) || temperature > 3.0e38f) return fail("temperature is not finite and > 0");
  if (n == 0) return 0;
  c->armed.sampled = true;
  c->armed.temperature = temperature;
  c->armed.keyed = keys != nullptr;
  c->armed.n_keys = n;
  if (keys) c->armed.keys.assign(keys, keys + n);
  return 0;
}
int slimt_hip_ctx_set_sampling_truncation(slimt_hip_ctx *c, uint32_t top_k, float top_p) {
  if (!c) return fail("ctx is NULL");
  if (!(top_p > 0.0f && top_p <= 1.0f)) return fail("top_p is not in (0, 1]");
  c->armed.truncated = top_k != 0 || top_p != 1.0f;
  c->armed.top_k = top_k;
  c->armed.top_p = top_p;
  return 0;
}
int slimt_hip_ctx_set_score_alternatives(slimt_hip_ctx *c, uint32_t k, uint32_t *alt_ids, float *alt_scores, uint32_t *rank) {
  if (!c) return fail("ctx is NULL");
  if (k > SLIMT_HIP_MAX_ALTERNATIVES) return fail("more alternatives than SLIMT_HIP_MAX_ALTERNATIVES");
  if (k && !alt_ids) return fail("alt_ids is NULL");
  c->alternatives = Alternatives{k, alt_ids, alt_scores, rank};
  return 0;
}
int slimt_hip_ctx_set_fanout_consensus(slimt_hip_ctx *c, int max_order, int beta2, uint32_t *best, double *utility) {
  if (!c) return fail("ctx is NULL");
  if (max_order == 0 && !best && !utility) {
    c->armed.consensus = false;
    return 0;
  }
  if (max_order < 1 || max_order > SLIMT_HIP_CONSENSUS_MAX_ORDER || beta2 < 1 || beta2 > SLIMT_HIP_CONSENSUS_MAX_BETA2)
    return fail("consensus: max_order or beta2 out of range");
  if (!best || !utility) return fail("null argument");
  c->armed.consensus = true;
  c->armed.best = best;
  c->armed.utility = utility;
  return 0;
}

int slimt_hip_translate_many_async(slimt_hip_ctx *c, const slimt_hip_batch *batches, size_t n, size_t S, float limit, uint32_t eos) {
  return run_many(c, batches, n, S, limit, eos);
}
int slimt_hip_translate_many_async_generated(slimt_hip_ctx *c, slimt_hip_shortlist *sl, const slimt_hip_batch *batches, size_t n,
                                             size_t S, float limit, uint32_t eos) {
  if (!sl) return fail("shortlist is NULL");
  return run_many(c, batches, n, S, limit, eos);
}
int slimt_hip_translate(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, const uint32_t *,
                        size_t, float limit, uint32_t eos, uint32_t *out_ids, uint32_t *out_len, float *align) {
  return run_one(c, ids, lengths, B, S, limit, eos, out_ids, out_len, align, true);
}
int slimt_hip_translate_async(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S,
                              const uint32_t *, size_t, float limit, uint32_t eos, uint32_t *out_ids, uint32_t *out_len,
                              float *align) {
  return run_one(c, ids, lengths, B, S, limit, eos, out_ids, out_len, align, false);
}
int slimt_hip_shortlist_create(const void *, size_t, size_t, size_t, int, int, int device, slimt_hip_shortlist **out) {
  *out = new slimt_hip_shortlist{device};
  return 0;
}
int slimt_hip_shortlist_destroy(slimt_hip_shortlist *s) { delete s; return 0; }
int slimt_hip_shortlist_generate(slimt_hip_shortlist *, const uint32_t *, const uint32_t *, size_t, size_t, uint32_t *out, size_t *n) {
  for (uint32_t i = 0; i < 8; ++i) out[i] = i;
  *n = 8;
  return 0;
}
int slimt_hip_translate_generated(slimt_hip_ctx *c, slimt_hip_shortlist *sl, const uint32_t *ids, const uint32_t *lengths, size_t B,
                                  size_t S, float limit, uint32_t eos, uint32_t *out_ids, uint32_t *out_len, float *align) {
  if (!sl) return fail("shortlist is NULL");
  return run_one(c, ids, lengths, B, S, limit, eos, out_ids, out_len, align, true);
}
int slimt_hip_translate_async_generated(slimt_hip_ctx *c, slimt_hip_shortlist *sl, const uint32_t *ids, const uint32_t *lengths,
                                        size_t B, size_t S, float limit, uint32_t eos, uint32_t *out_ids, uint32_t *out_len,
                                        float *align) {
  if (!sl) return fail("shortlist is NULL");
  return run_one(c, ids, lengths, B, S, limit, eos, out_ids, out_len, align, false);
}

int slimt_hip_score(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, const uint32_t *, size_t,
                    const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T, float *scores, float *align) {
  return run_score(c, ids, lengths, B, S, tgt_ids, tgt_len, T, nullptr, B, scores, align, true);
}
int slimt_hip_score_async_generated(slimt_hip_ctx *c, slimt_hip_shortlist *sl, const uint32_t *ids, const uint32_t *lengths, size_t B,
                                    size_t S, const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T, float *scores, float *align) {
  if (!sl) return fail("shortlist is NULL");
  return run_score(c, ids, lengths, B, S, tgt_ids, tgt_len, T, nullptr, B, scores, align, false);
}
int slimt_hip_score_candidates(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S, const uint32_t *,
                               size_t, const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T, const uint32_t *cand_src, size_t N,
                               float *scores, float *align) {
  if (N && !cand_src) return fail("null argument");
  return run_score(c, ids, lengths, B, S, tgt_ids, tgt_len, T, cand_src, N, scores, align, true);
}
int slimt_hip_score_candidates_async_generated(slimt_hip_ctx *c, slimt_hip_shortlist *sl, const uint32_t *ids, const uint32_t *lengths,
                                               size_t B, size_t S, const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T,
                                               const uint32_t *cand_src, size_t N, float *scores, float *align) {
  if (!sl) return fail("shortlist is NULL");
  if (N && !cand_src) return fail("null argument");
  return run_score(c, ids, lengths, B, S, tgt_ids, tgt_len, T, cand_src, N, scores, align, false);
}
int slimt_hip_translate_fanout(slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *lengths, size_t B, size_t S,
                               const uint32_t *row_src, size_t N, const uint32_t *, size_t, float limit, uint32_t eos,
                               uint32_t *out_ids, uint32_t *out_len, float *align) {
  return run_fanout(c, ids, lengths, B, S, row_src, N, limit, eos, out_ids, out_len, align, true);
}
int slimt_hip_translate_fanout_async_generated(slimt_hip_ctx *c, slimt_hip_shortlist *sl, const uint32_t *ids, const uint32_t *lengths,
                                               size_t B, size_t S, const uint32_t *row_src, size_t N, float limit, uint32_t eos,
                                               uint32_t *out_ids, uint32_t *out_len, float *align) {
  if (!sl) return fail("shortlist is NULL");
  return run_fanout(c, ids, lengths, B, S, row_src, N, limit, eos, out_ids, out_len, align, false);
}
}
