// Multi-device translation service of the HIP backend.
//
// What it replaces in slimt: the request -> batch -> worker plumbing between
// `Async::translate` and `Model::forward` (slimt/Frontend.cc:207-227 with
// slimt/Batcher.{hh,cc}). This is NOT that code: the reference keeps ordered
// sets of segment references per length and hands one batch at a time to a
// worker that blocks in `forward`. Here
//   * waiting sentences live in per-length binary heaps keyed by arrival order
//     (LengthQueue) -- only the batch-FORMING RULE is the reference's, because
//     the padding a sentence travels with is visible in its result: walk the
//     lengths upwards and keep adding sentences while (count + 1) * length fits
//     the word budget (slimt/Batcher.cc:95-120);
//   * every worker owns TWO device contexts with pinned staging buffers and keeps
//     one batch running on the GPU while it assembles, uploads and launches the
//     next one and then unpacks the previous one's results (double buffering over
//     slimt_hip_translate_async): host work and PCIe copies hide behind kernels;
//   * workers are spread over any number of model replicas (one per GPU).
// Text processing is out of scope, so a request is its tokenised sentences.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>
#include <utility>
#include <vector>

#include "Model.hh"
#include "Shortlist.hh"

namespace slimt {

// One translate() call in flight: its sentences, the slots for their results and
// the promise that is fulfilled by whichever worker delivers the last one.
class Pending {
 public:
  explicit Pending(std::vector<Words> sentences, std::vector<Words> prefixes = {}, uint64_t seed = 0);
  size_t size() const { return sentences_.size(); }
  const Words &sentence(size_t i) const { return sentences_[i]; }
  // sentence i's forced target prefix (empty: none; Service::translate with prefixes)
  bool has_prefixes() const { return !prefixes_.empty(); }
  const Words &prefix(size_t i) const { return prefixes_[i]; }
  // the request's sampling seed (a sampling service: sentence i's key is slimt_hip_sampling_key(seed, i))
  uint64_t seed() const { return seed_; }
  std::future<Histories> future() { return promise_.get_future(); }
  void deliver(size_t i, History history);   // thread-safe; the last delivery fulfils the promise
  void fail(const std::exception_ptr &error);  // first failure wins; later deliveries are dropped

 private:
  std::vector<Words> sentences_;
  std::vector<Words> prefixes_;  // empty, or one per sentence
  uint64_t seed_ = 0;
  Histories results_;
  std::atomic<size_t> left_;
  std::atomic<bool> settled_{false};
  std::promise<Histories> promise_;
};

// A sentence waiting for a batch.
struct Unit {
  uint64_t order = 0;  // (request sequence number << 24) | sentence index: FIFO among equal lengths
  std::shared_ptr<Pending> owner;
  uint32_t index = 0;
  uint32_t length = 0;
};

// Waiting sentences, grouped by length. Not thread-safe (the service locks around it).
class LengthQueue {
 public:
  // `longest` = the longest sentence accepted; the budget must hold at least one
  // such sentence (the reference's check, slimt/Batcher.cc:85-91).
  LengthQueue(size_t max_words, size_t longest);
  // Units arrive in ascending `order` (the service numbers requests under the lock it pushes
  // under), so every length is a FIFO: O(1) per sentence -- a request of 65,536 sentences used to
  // hold the lock for its whole heap insertion while every worker waited.
  void push(Unit unit);
  // Next batch under the reference's rule (slimt/Batcher.cc:95-120): lengths
  // ascending, arrival order within a length, stop at the first sentence that
  // would push (count + 1) * its length over the budget. Empty when nothing waits.
  std::vector<Unit> take();
  // the padded length of the batch take() would return now (the length of its last sentence); 0 when nothing waits
  size_t peek_length() const;
  size_t waiting() const { return waiting_; }
  size_t longest() const { return fifos_.size() - 1; }

 private:
  size_t max_words_;
  std::vector<std::deque<Unit>> fifos_;  // fifos_[len]: ascending Unit::order
  size_t low_ = 0, high_ = 0;            // lengths outside [low_, high_] are empty
  size_t waiting_ = 0;
};

// Contexts (streams) one process can hold on one device before its hardware queues are time-sliced.
constexpr size_t kContextsPerDeviceCliff = 22;

struct ServiceConfig {
  size_t max_words = 8192;   // word budget of a batch: (B + 1) * S <= max_words
  size_t wrap_length = 128;  // longest sentence (slimt wraps there, Frontend.hh:27)
  float tgt_length_limit_factor = 1.5F;
  size_t workers_per_device = 10;  // x 2 contexts each: about 20 batches in flight per GPU
  // Merged launches (slimt_hip_translate_many_async): a worker that has taken a batch keeps taking the batches that
  // follow it in the queue -- each formed by the reference's rule under max_words, each with its own padded length,
  // arrays and results -- up to merge_batches of them, while the launch's rows x its longest length stay within
  // merge_words and no batch runs padded by more than a quarter; all of them run as ONE encoder and ONE decoder launch.
  // The reference's default batch is 1024 padded words (Frontend.hh:21-39): 32 sentences of 32 tokens fill 2 of 256 CUs
  // in the decoder; eight of them per launch pair fill what one batch of 8192 words does. 1 = never merge. With a lexical
  // shortlist every merged batch still gets ITS OWN list (Model.cc:117-120), generated inside the one encoder launch.
  size_t merge_batches = 8;
  size_t merge_words = 8192;
  uint32_t pad_id = 0;
  // one line on stderr when started with > 2 workers per device and < 8 hardware queues, or with more than
  // kContextsPerDeviceCliff contexts (2 per worker) on one device
  bool warn_hw_queues = true;
  bool alignments = true;
  bool flat_alignments = false;  // Hypothesis::alignment_flat instead of ::alignment (one block per sentence)
  bool scores = false;           // Hypothesis::scores: every target token's log-probability (Service::set_scores)
  float temperature = 0.0f;      // > 0: every launch samples at this temperature (Service::set_sampling); 0: greedy
  uint32_t top_k = 0;            // sampled launches keep the top_k largest (0: all) ...
  float top_p = 1.0f;            // ... and the nucleus of this mass (1: all): Service::set_sampling_truncation
  // Output vocabulary of a batch, one policy for the service's lifetime:
  //  * lexical_shortlist set: the reference's own -- ShortlistGenerator::generate on every batch's
  //    source words (Model.cc:60-82,117-120; Shortlist.cc:115-175) -- run on the device, on the
  //    worker's stream, from the batch's ids in pinned memory: no host shortlist, no upload, no
  //    synchronisation. `lexical_shortlist` is the binary shortlist file (Shortlist.hh:77-84), borrowed
  //    for the constructor; one generator per device is built from it;
  //  * else `shortlist`: one fixed sorted id list (tests, benchmarks), or nullopt: the full vocabulary.
  View lexical_shortlist;
  size_t source_vocab = 0, target_vocab = 0;  // Vocabulary::size() of the two vocabularies
  bool shortlist_shared_vocab = false;        // ShortlistGenerator's `shared` (Shortlist.hh:51)
  bool shortlist_check = false;               // verify the file's checksum (Shortlist.cc:66-76)
  std::optional<Words> shortlist;
  // Test hook: called by every worker before it builds its contexts; throwing from it makes that
  // worker fail the way a failed allocation would (the others must keep serving).
  std::function<void(const Model *)> fail_worker_setup;
};

class Service {
 public:
  // replicas[d]: the model on GPU d. Worker w of device d = thread d * workers_per_device + w.
  Service(const ServiceConfig &config, std::vector<const Model *> replicas);
  ~Service();  // drains the queue, then joins the workers
  Service(const Service &) = delete;
  Service &operator=(const Service &) = delete;
  // Queue one request. Throws std::invalid_argument for an empty sentence or one longer
  // than the service accepts; a failure on a worker arrives through the future.
  std::future<Histories> translate(std::vector<Words> sentences);
  // ... each sentence forced through its target prefix (include/slimt_hip.h, slimt_hip_ctx_set_target_prefix; an
  // empty prefix: none). Throws std::invalid_argument for a count that differs from the sentences' or a prefix longer
  // than max(1, (size_t)(limit factor * the sentence's length)).
  std::future<Histories> translate(std::vector<Words> sentences, std::vector<Words> prefixes);
  // ... on a sampling service (set_sampling) under this seed: sentence i is drawn under slimt_hip_sampling_key(seed, i),
  // wherever the batcher puts it (the other overloads use seed 0); prefixes may be empty
  std::future<Histories> translate(std::vector<Words> sentences, std::vector<Words> prefixes, uint64_t seed);
  // Teacher-forced scoring (include/slimt_hip.h, slimt_hip_score): targets[i] is the given translation of sentences[i]
  // (with its EOS when that is to be scored), of ANY length -- there is no limit-factor cap. Batches are formed by the
  // source-length rule of translate(); each batch's target rows are as long as its longest target; the output layer is
  // the one the service translates with (its lexical shortlist per batch, its fixed list, or the full vocabulary). One
  // Hypothesis per sentence: target = the given tokens, scores = their log-probabilities (always filled, whatever
  // set_scores says), the alignment rows as translate() returns them. Synchronous, on the caller's thread and a context
  // of its own (built on the first call, on the first replica): it neither queues behind translate requests nor is
  // merged with them; concurrent callers take turns. Throws std::invalid_argument for counts that differ, an empty
  // sentence or one longer than the service accepts, or a target of more than 65536 tokens.
  // alternatives = k (1 .. 8): each Hypothesis also carries, per target token, the k most probable ids of its position with
  // their log-probabilities and the token's rank among the layer's columns (Hypothesis::alt_ids / alt_scores / ranks;
  // include/slimt_hip.h, slimt_hip_ctx_set_score_alternatives). More than 8 is refused.
  Histories score(std::vector<Words> sentences, std::vector<Words> targets, size_t alternatives = 0);
  // Several candidate translations per sentence, scored from ONE encoding of each sentence (include/slimt_hip.h,
  // slimt_hip_score_candidates): candidates[i] are sentence i's (any number, 0 included; each of any length). Batches are
  // formed by the source-length rule of translate(); all candidates of a sentence travel in its batch, sorted by source,
  // and a batch's T is its longest candidate. The output layer, the context and the mutex are those of score(). Returns one
  // Hypothesis per candidate in the order given (sentence 0's first), as score() fills them; totals: per candidate the f32
  // sum of its scores in ascending order from +0; best: per SENTENCE the index among its own candidates of the lowest
  // one whose key -- the total (mode 0) or the total / tokens (mode 1) -- is >= every other's, candidates without tokens
  // or with a NaN key aside; 0xFFFFFFFF when none is left (slimt_hip_candidates_rank's rule). Another mode is refused.
  struct CandidateScores {
    Histories candidates;
    std::vector<float> totals;
    std::vector<uint32_t> best;
  };
  CandidateScores score_candidates(std::vector<Words> sentences, std::vector<std::vector<Words>> candidates, int mode = 0);
  // n sampled translations of every sentence from ONE encoding of it (include/slimt_hip.h, slimt_hip_translate_fanout), on a
  // sampling service (set_sampling; set_sampling_truncation applies). Batches are formed by the source-length rule of
  // translate(); all n rows of a sentence travel in its batch, sorted by source, and a batch of more than max_words / n
  // sentences goes as several calls at the batch's padded length (n * sentences of a call <= the context's max_batch).
  // Sample j of sentence i is drawn under slimt_hip_sampling_key(seed, i * n + j), wherever the batcher puts it. Returns
  // n Hypotheses per sentence, sample j of sentence i at i * n + j, each with its scores (always filled) and alignment rows
  // as translate() returns them. The context and the mutex are those of score(): synchronous, on the caller's thread.
  // Throws std::invalid_argument on a greedy service, for n = 0 or n > max_words, an empty sentence or one too long.
  Histories translate_samples(std::vector<Words> sentences, size_t n, uint64_t seed = 0);
  // translate_samples followed by the consensus (minimum-Bayes-risk) pick among each sentence's n samples, made on the device
  // behind the fan-out call's last step (include/slimt_hip.h, slimt_hip_ctx_set_fanout_consensus): no second encoding, no
  // scorer pass. The same batching and the same keys as translate_samples -- the winner of sentence i is bit for bit entry
  // i * n + sample_index of that call with this seed. Returns ONE Hypothesis per sentence: the winning sample with its
  // tokens, scores and alignment, plus its utility and its index j among the samples (Hypothesis::utility, sample_index);
  // n = 1 returns the lone sample with utility 0. Throws as translate_samples does, and for n > 64
  // (SLIMT_HIP_CONSENSUS_MAX_ROWS) or max_order / beta2 out of range.
  Histories translate_consensus(std::vector<Words> sentences, size_t n, uint64_t seed = 0, int max_order = 4, int beta2 = 4);
  // per-token scores on or off (ServiceConfig::scores): only before the first translate(); false once one has been made
  bool set_scores(bool on);
  // temperature sampling for every request (include/slimt_hip.h, slimt_hip_ctx_set_sampling; 0: greedy again): only before
  // the first translate(); false once one has been made, or for a temperature that is not finite and >= 0
  bool set_sampling(float temperature);
  // top-k / nucleus truncation of every sampled launch (slimt_hip_ctx_set_sampling_truncation; (0, 1): none): only before
  // the first translate(); false once one has been made, or for a top_p outside (0, 1]. The engine does not merge
  // truncated calls, so a truncating service sends every batch as a launch of its own, whatever merge_batches says.
  bool set_sampling_truncation(uint32_t top_k, float top_p);
  // restart the SLIMT_SERVICE_STATS counters (benchmarks: after the warm-up pass)
  void stats_reset() {
    stats_base_ = batches_.load();
    launches_base_ = launches_.load();
    merged_base_ = merged_launches_.load();
    for (auto *c : {&ns_idle_, &ns_lock_, &ns_starved_, &ns_launch_, &ns_wait_, &ns_collect_, &ns_deliver_}) c->store(0);
  }

 private:
  // translate_samples (select = false: n entries per sentence) and translate_consensus (select = true: the winner alone)
  Histories fanout_samples(std::vector<Words> sentences, size_t n, uint64_t seed, bool select, int max_order, int beta2);
  // what score(), score_candidates() and fanout_samples() share (and translate(): the first)
  void check_sentence(const Words &sentence) const;  // throws for an empty one or one longer than the service accepts
  LengthQueue request_queue(const std::vector<Words> &sentences) const;  // a request's own queue: translate()'s batches
  std::unique_lock<std::mutex> lock_score_worker();  // score_mu_ held, score_worker_ built
  struct Sources {  // a call's sources: ids [B][S] padded with pad_id, lengths [B]; reused from batch to batch
    std::vector<uint32_t> ids, lengths;
  };
  void stage_sources(const std::vector<Words> &sentences, const Unit *units, size_t B, size_t S, Sources &sources) const;
  std::pair<const uint32_t *, size_t> fixed_shortlist() const;  // the service's fixed list, or (nullptr, 0)
  // a call's N rows of T tokens as Histories, numbered as the next batch: tokens cut at len[r], alignment rows at
  // row_len[r], scores [N][T] cut at len[r]
  Histories collect_scored(const uint32_t *tokens, const std::vector<uint32_t> &len, const std::vector<uint32_t> &row_len, size_t S,
                           size_t T, const std::vector<float> &scores, const std::vector<float> &align);
  struct Slot;
  void work(const Model *model, slimt_hip_shortlist *generator);
  std::vector<Unit> next_batch(bool may_block, std::vector<size_t> *parts = nullptr);
  void launch(Slot &slot, std::vector<Unit> &batch, slimt_hip_shortlist *generator, std::vector<size_t> &parts);
  void finish(Slot &slot);
  void retire(const std::exception_ptr &error);

  ServiceConfig config_;
  size_t longest_;
  LengthQueue queue_;
  std::vector<std::unique_ptr<ShortlistGenerator>> generators_;  // one per device in use (lexical shortlist)
  uint64_t sequence_ = 0;
  std::atomic<uint64_t> batches_{0};  // batches launched so far (Hypothesis::batch)
  std::atomic<uint64_t> launches_{0}, merged_launches_{0};  // launch pairs so far, and those that carried more than one batch
  uint64_t stats_base_ = 0, launches_base_ = 0, merged_base_ = 0;
  // where the workers' time goes, in nanoseconds (printed by the destructor when SLIMT_SERVICE_STATS is set)
  std::atomic<uint64_t> ns_idle_{0}, ns_lock_{0}, ns_starved_{0}, ns_launch_{0}, ns_wait_{0}, ns_collect_{0}, ns_deliver_{0};
  bool closing_ = false;
  size_t live_workers_ = 0;          // workers that can take batches
  std::exception_ptr dead_error_;    // set once the last of them has failed: requests fail with it
  std::mutex mutex_;
  std::mutex setup_mu_;              // one worker at a time builds its two contexts (work())
  std::condition_variable wake_;
  std::vector<std::thread> threads_;
  // score(): the first replica, its generator (nullable), and the context the calls share (built by the first one)
  const Model *score_model_ = nullptr;
  slimt_hip_shortlist *score_generator_ = nullptr;
  std::mutex score_mu_;
  std::unique_ptr<Worker> score_worker_;
};

}  // namespace slimt
