// C ABI (include/slimt_hip.h) + host-side engine of the MI355X slimt backend.
#include "engine.h"
#include "decoder_plan.h"
#include "sampling.h"
#include "scores.h"
#include "truncation.h"
#include "beam.h"
#include "launch_choice.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

using namespace slimt_hip;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code ? code : -1;
}

// Set on this library's first call into the HIP runtime (every path to the device goes through one of
// DevBuf::reserve, slimt_hip_device_count, slimt_hip_set_device, slimt_hip_host_alloc): the runtime reads
// GPU_MAX_HW_QUEUES once, when it initialises, so slimt_hip_request_hw_queues is of no use afterwards.
static std::atomic<bool> g_hip_called{false};

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail((int)e_, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
  } while (0)

#define RCCHK(expr)        \
  do {                     \
    int rc_ = (expr);      \
    if (rc_) return rc_;   \
  } while (0)

// ---------------------------------------------------------------------------
// environment knobs
// ---------------------------------------------------------------------------
// Every SLIMT_* variable the engine reads, read once, when env() is first called. (GPU_MAX_HW_QUEUES is not one of them: it
// is the runtime's, read by slimt_hip_hw_queues alone.) DESIGN.md has the table.
struct EnvKnobs {
  bool kv_watch = true;             // SLIMT_KV_WATCH=0: format 0's watches never switch a form off (measurements of the fallbacks)
  bool kv_tight = true;             // SLIMT_KV_TIGHT=0: the tight (16-bit) K/V form is never tried
  bool host_timing = false;         // SLIMT_HOST_TIMING set: where a translate call's host time goes, printed at model destroy
  bool submit_lock = true;          // SLIMT_SUBMIT_LOCK=0: persistent translates are queued without the model's submit lock
  bool kv_store_nt = false;         // SLIMT_KV_STORE_NT=1: encoders write a cache non-temporally when its decoder will stream it
  double rows_oversub = 1.0;        // SLIMT_ROWS_OVERSUB: decoder workgroups in flight the plan allows, as a multiple of the budget
  double kv_budget = 300e6;         // SLIMT_KV_BUDGET_MB: K/V bytes in flight that stay temporal (per-layer rule)
  int kv_grain = 8;                 // SLIMT_KV_GRAIN: ... in steps of this many eighths of a layer's caches (at least 1)
  int kv_by_launch = -1;            // SLIMT_KV_BY_LAUNCH: 0 = the per-layer rule only, 1..8 = keep that many launches of every 8
  double kv_launch_budget = 300e6;  // SLIMT_KV_LAUNCH_BUDGET_MB: K/V bytes in flight the by-launch rule keeps temporal
  bool shortlist_fold = true;       // SLIMT_SHORTLIST_FOLD=0: a generated shortlist is a launch of its own, not inside the encoder's
  bool merge_dense = true;          // SLIMT_MERGE_DENSE=0: sub-batches that share an output layer are still tile-aligned (A/B)
  bool idle_streams = true;         // SLIMT_IDLE_STREAMS=0: no idle streams level the hardware queues before the first context
  bool quiet = false;               // SLIMT_HIP_QUIET=1: the warning about too many contexts on a device is not printed
};

static const EnvKnobs &env() {
  static const EnvKnobs knobs = [] {
    EnvKnobs k;
    auto is = [](const char *name, char c) { return std::getenv(name) && std::getenv(name)[0] == c; };
    auto real = [](const char *name, double otherwise) { return std::getenv(name) ? std::atof(std::getenv(name)) : otherwise; };
    k.kv_watch = !is("SLIMT_KV_WATCH", '0');
    k.kv_tight = !is("SLIMT_KV_TIGHT", '0');
    k.host_timing = std::getenv("SLIMT_HOST_TIMING") != nullptr;
    k.submit_lock = !is("SLIMT_SUBMIT_LOCK", '0');
    k.kv_store_nt = is("SLIMT_KV_STORE_NT", '1');
    k.rows_oversub = real("SLIMT_ROWS_OVERSUB", 1.0);
    k.kv_budget = real("SLIMT_KV_BUDGET_MB", 300.0) * 1e6;
    k.kv_grain = std::getenv("SLIMT_KV_GRAIN") ? std::max(1, std::atoi(std::getenv("SLIMT_KV_GRAIN"))) : 8;
    k.kv_by_launch = std::getenv("SLIMT_KV_BY_LAUNCH") ? std::atoi(std::getenv("SLIMT_KV_BY_LAUNCH")) : -1;
    k.kv_launch_budget = real("SLIMT_KV_LAUNCH_BUDGET_MB", 300.0) * 1e6;
    k.shortlist_fold = !is("SLIMT_SHORTLIST_FOLD", '0');
    k.merge_dense = !is("SLIMT_MERGE_DENSE", '0');
    k.idle_streams = !is("SLIMT_IDLE_STREAMS", '0');
    k.quiet = is("SLIMT_HIP_QUIET", '1');
    return k;
  }();
  return knobs;
}

// The persistent decoder runs the hoisted cross-attention order over a cache of accumulators; the reference's literal
// sequence (K/V cache format 3) exists in the stage-wise attention kernel only (decode_kernels.hip, DQAttnArgs::literal)
// ... and a truncated sampled call needs each step's whole row of logits, which only the stage-wise decoder stores; a
// fan-out call's cross-attention looks a row's source up, which only the stage-wise one does (decode_fanout.hip). Every
// decision that hangs on the persistent decoder -- the lean path, pinned arrays read in place, merged launches -- asks here;
// the encoder is chosen as the context's mode says.
static bool fused_decoder_allowed(const slimt_hip_ctx *c) {
  return c->decode_mode != 1 && c->model->kv_format != 3 && !c->call.truncated && !c->call.fanout;
}
// The decoder rows of the call in progress: a fan-out call's N, else one per source.
static int decoder_rows(const slimt_hip_ctx *c) { return c->call.fanout ? c->call.rows : c->B; }

// The lean path for sources padded to S tokens: the persistent decoder, allowed and compiled for the model, behind a
// persistent encoder (the fused one, or the per-sentence one of 65..128 tokens).
static bool persistent_path(const slimt_hip_ctx *c, size_t S) {
  const slimt_hip_model *m = c->model;
  return fused_decoder_allowed(c) && fused_decode_supported(m->D, m->F, m->H, m->Ld) &&
         (fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S) ||
          long_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S));
}

// The narrow K/V form for this model's next batch (engine.h, kv_auto_wide): format 0, and the sentences so far mostly fit.
// Called under the model's submit / gate discipline by encode_device; the counter lags the device by a few batches.
static bool kv_narrow_wanted(slimt_hip_model *m, unsigned long long **count_dev) {
  *count_dev = nullptr;
  if (m->kv_format != 0 || m->kv_auto_wide.load(std::memory_order_relaxed)) return false;
  {
    std::lock_guard<std::mutex> lock(m->gate_mu);
    if (!m->kv_wide_count) {
      void *p = nullptr;
      if (hipHostMalloc(&p, 256, hipHostMallocDefault) != hipSuccess) {  // [0] 24-bit, [1 + 4 gen + layer] not-16-bit (engine.h)
        (void)hipGetLastError();
        return true;  // (no counter: narrow without the watch)
      }
      std::memset(p, 0, 256);
      m->kv_wide_count = static_cast<unsigned long long *>(p);
    }
  }
  const unsigned long long wide = *static_cast<volatile unsigned long long *>(m->kv_wide_count);
  const unsigned long long total = m->kv_layers_submitted.load(std::memory_order_relaxed);
  // one sentence-layer in 32 is enough to make most 16-sentence workgroups wait for a fallback call every step
  // (SLIMT_KV_WATCH=0: never switch -- measurements of the fallback itself)
  const bool watch = env().kv_watch;
  if (watch && total >= 1024 && wide * 32 > total) {
    m->kv_auto_wide.store(true, std::memory_order_relaxed);
    return false;
  }
  void *dev = nullptr;
  if (hipHostGetDevicePointer(&dev, m->kv_wide_count, 0) == hipSuccess) *count_dev = static_cast<unsigned long long *>(dev);
  else (void)hipGetLastError();
  return true;
}

// Where the tight form has a writer and a reader (launch_choice.h, kv_tight_shape), for this context's next batch of
// sentences padded to S tokens behind an encoder with (`writer`: kv_tight_writer) or without a writer for it.
static bool kv_tight_shape(const slimt_hip_ctx *c, int S, bool writer) {
  const slimt_hip_model *m = c->model;
  KvTightIn in;
  in.enabled = env().kv_tight;
  in.writer = writer;
  in.tight_limit = m->kv_tight_limit;
  in.kv_format = m->kv_format;
  in.D = m->D;
  in.S = S;
  in.decode_mode = c->decode_mode;
  in.expect_large_output = c->expect_large_output;
  // (only the reader a batch of this length could take is asked about: the rule reads mid_ok for S > 32 alone)
  in.mid_ok = S > 32 && fused_decode_tight_mid_supported(m->D, m->F, m->H, m->Ld, S > 64 ? 2 : 1);
  in.rows32_ok = S <= 32 && fused_decode_tight_rows32_supported(m->D, m->F, m->H, m->Ld);
  in.tight_ok = S <= 32 && fused_decode_tight_supported(m->D, m->F, m->H, m->Ld);
  return slimt_hip::kv_tight_shape(in);
}

static bool kv_centres_ready(slimt_hip_model *m) {
  const int state = m->kv_centre_state.load(std::memory_order_acquire);
  if (state == 2) return true;
  if (state == 1 && hipEventQuery(m->kv_centre_ev) == hipSuccess) {
    m->kv_centre_state.store(2, std::memory_order_release);
    return true;
  }
  (void)hipGetLastError();  // (hipErrorNotReady)
  return false;
}

// The tight form for this batch's decoder layers (engine.h, kv_tight_off): a mask of the layers that try it. Only where the
// decoder launch that follows will be one with the reader inlined (kv_tight_shape), and once the centres are there.
static unsigned kv_tight_wanted(slimt_hip_ctx *c, int S, bool writer, unsigned long long **count_dev) {
  slimt_hip_model *m = c->model;
  *count_dev = nullptr;
  if (!kv_tight_shape(c, S, writer) || !m->kv_wide_count || !kv_centres_ready(m)) return 0;
  const bool watch = env().kv_watch;
  unsigned off = m->kv_tight_off.load(std::memory_order_relaxed);
  const int gen = m->kv_gen.load(std::memory_order_relaxed);
  unsigned tripped = 0;
  for (int l = 0; l < m->Ld && watch; ++l) {
    const unsigned long long missed = static_cast<volatile unsigned long long *>(m->kv_wide_count)[1 + 4 * gen + l];
    const unsigned long long total = m->kv_tight_submitted[l].load(std::memory_order_relaxed);
    // (as for the narrow form: the fallback is an out-of-line call its whole workgroup waits for)
    if (!((off >> l) & 1u) && total >= 1024 && missed * 32 > total) tripped |= 1u << l;
  }
  if (tripped) {
    if (gen < m->kv_recal_max && gen + 1 < slimt_hip_model::kKvGens) {
      // these centres do not fit the traffic: a new generation, calibrated from the next suitable batch (translate_device);
      // until it is ready nobody tries the form, and this generation's buffer stays as it is for the batches in flight
      for (auto &n : m->kv_tight_submitted) n.store(0, std::memory_order_relaxed);
      m->kv_gen.store(gen + 1, std::memory_order_relaxed);
      m->kv_centre_state.store(0, std::memory_order_release);
      m->kv_centre_claimed.store(false, std::memory_order_release);
      return 0;
    }
    off |= tripped;
    m->kv_tight_off.fetch_or(tripped, std::memory_order_relaxed);
  }
  const unsigned layers = ((1u << m->Ld) - 1u) & ~off;
  if (!layers) return 0;
  void *dev = nullptr;
  if (hipHostGetDevicePointer(&dev, m->kv_wide_count, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  *count_dev = static_cast<unsigned long long *>(dev) + 1 + 4 * gen;
  c->kv_gen = gen;
  return layers;
}

static void kv_watch_restart(slimt_hip_model *model) {
  model->kv_auto_wide.store(false, std::memory_order_relaxed);
  model->kv_layers_submitted.store(0, std::memory_order_relaxed);
  model->kv_tight_off.store(0, std::memory_order_relaxed);
  for (auto &n : model->kv_tight_submitted) n.store(0, std::memory_order_relaxed);
  if (model->kv_wide_count)
    for (int i = 0; i < 32; ++i) static_cast<volatile unsigned long long *>(model->kv_wide_count)[i] = 0;
}

// A translate call's claim on calibrating the current generation's centres. A call that took it and leaves before its
// reduction is queued -- an error on the way -- gives it back: a claim without centres would keep every batch from
// calibrating, and the form would silently never be used.
struct ClaimGuard {
  slimt_hip_model *m;
  bool armed = false;
  explicit ClaimGuard(slimt_hip_model *model) : m(model) {}
  void take() { armed = !m->kv_centre_claimed.exchange(true, std::memory_order_acq_rel); }
  ~ClaimGuard() {
    if (armed && m->kv_centre_state.load(std::memory_order_acquire) == 0) m->kv_centre_claimed.store(false, std::memory_order_release);
  }
};

// The claimed batch's column means into this generation's buffer, behind its encoder on the context's stream. No centres
// -- an allocation or a launch failed --: the state stays 0, the guard gives the claim back and the next suitable batch
// tries again; this one goes on with its f32 cache.
static void queue_centre_reduction(slimt_hip_ctx *c, int B, int S) {
  slimt_hip_model *gm = c->model;
  hipStream_t st = c->stream;
  DevBuf &centres = gm->kv_centre[gm->kv_gen.load(std::memory_order_relaxed)];  // this generation's own buffer
  if (centres.reserve((size_t)gm->Ld * 2 * gm->D * 4) != hipSuccess || gm->kv_centre_sums.reserve((size_t)gm->Ld * 2 * gm->D * 8) != hipSuccess ||
      (!gm->kv_centre_ev && hipEventCreateWithFlags(&gm->kv_centre_ev, hipEventDisableTiming) != hipSuccess) ||
      launch_kv_centres(c->kv.as<float>(), gm->Ld, B, S, gm->D, gm->kv_centre_sums.as<unsigned long long>(), centres.as<int>(), st) != hipSuccess ||
      hipEventRecord(gm->kv_centre_ev, st) != hipSuccess)
    (void)hipGetLastError();
  else
    gm->kv_centre_state.store(1, std::memory_order_release);
}

hipError_t DevBuf::reserve(size_t n) {
  if (n <= bytes && p) return hipSuccess;
  g_hip_called.store(true, std::memory_order_relaxed);
  if (p) {
    hipError_t e = hipFree(p);
    if (e != hipSuccess) return e;
    p = nullptr;
    bytes = 0;
  }
  if (n == 0) n = 16;
  hipError_t e = hipMalloc(&p, n);
  if (e == hipSuccess) bytes = n;
  return e;
}

void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
}

namespace {
// SLIMT_HOST_TIMING=1: where a translate call's host time goes (printed when a model is destroyed)
struct HostTiming {
  std::atomic<uint64_t> ns[8] = {};
  std::atomic<uint64_t> calls{0};
} g_timing;
const char *kTimingNames[8] = {"validate", "encode: prepare + launch", "submit + gate locks", "gate: wait-event call",
                               "decoder launch call", "gate: event record", "pinned-pointer views", "other"};
struct StageClock {
  std::chrono::steady_clock::time_point t;
  StageClock() { if (env().host_timing) t = std::chrono::steady_clock::now(); }
  void lap(int stage) {
    if (!env().host_timing) return;
    const auto now = std::chrono::steady_clock::now();
    g_timing.ns[stage] += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now - t).count();
    t = now;
  }
};
void timing_report() {
  if (!env().host_timing || g_timing.calls == 0) return;
  std::fprintf(stderr, "host-timing: %llu translate calls; us per call:", (unsigned long long)g_timing.calls.load());
  for (int i = 0; i < 8; ++i)
    if (g_timing.ns[i]) std::fprintf(stderr, " [%s %.1f]", kTimingNames[i], 1e-3 * g_timing.ns[i] / g_timing.calls);
  std::fprintf(stderr, "\n");
}
}  // namespace

// Nothing here runs when the library is loaded, and nothing but this function writes the environment.
extern "C" int slimt_hip_request_hw_queues(int n) {
  if (n < 1 || n > 1024) return fail(-1, "hardware queues %d not in 1..1024", n);
  if (g_hip_called.load(std::memory_order_relaxed)) return 1;
  char value[16];
  snprintf(value, sizeof value, "%d", n);
  if (setenv("GPU_MAX_HW_QUEUES", value, /*overwrite=*/0)) return fail(-1, "setenv failed");
  return 0;
}

extern "C" int slimt_hip_hw_queues(void) {
  const char *v = getenv("GPU_MAX_HW_QUEUES");
  return v ? atoi(v) : 0;
}

namespace slimt_hip {
hipError_t set_dynamic_lds_once(const void *kernel, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void *>, int> largest;
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  int &have = largest[{device, kernel}];
  if (bytes <= have) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}
}  // namespace slimt_hip

extern "C" int slimt_hip_abi_version(void) { return SLIMT_HIP_ABI_VERSION; }
extern "C" const char *slimt_hip_last_error(void) { return g_err; }

extern "C" int slimt_hip_device_count(int *count) {
  if (!count) return fail(-1, "count is NULL");
  int n = 0;
  g_hip_called.store(true, std::memory_order_relaxed);
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail((int)e, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return 0;
}

extern "C" int slimt_hip_set_device(int device) {
  g_hip_called.store(true, std::memory_order_relaxed);
  HIPCHK(hipSetDevice(device));
  return 0;
}

// ---------------------------------------------------------------------------
// host-side weight preparation (load time; slimt/Io.cc:215,234)
// ---------------------------------------------------------------------------
extern "C" int slimt_hip_prepare_weight_transposed(const float *weights, int8_t *prepared,
                                                   float quantization_multiplier, size_t cols,
                                                   size_t rows) {
  if (!weights || !prepared) return fail(-1, "null argument");
  const size_t n = rows * cols;
  for (size_t i = 0; i < n; ++i) {
    float v = rintf(weights[i] * quantization_multiplier);
    if (v != v) v = -127.0f;  // NaN: what intgemm's convert + saturating packs + max yield
    v = v < -127.0f ? -127.0f : v;
    v = v > 127.0f ? 127.0f : v;
    prepared[i] = (int8_t)v;
  }
  return 0;
}

extern "C" int slimt_hip_prepare_weight_quantized_transposed(const int8_t *input, int8_t *output,
                                                             size_t rows, size_t cols) {
  if (!input || !output) return fail(-1, "null argument");
  if (input != output) memmove(output, input, rows * cols);
  return 0;
}

// ---------------------------------------------------------------------------
// op level
// ---------------------------------------------------------------------------
// process-wide diagnostic switch (slimt_hip_debug_occupancy_trace)
static slimt_hip::OccTrace g_occ_trace;

namespace {

struct TmpAffine {  // device temporaries of one stateless qmm call
  DevBuf x, W, bias, idx, y;
  AffineW aw;
  ~TmpAffine() {
    x.release(); W.release(); bias.release(); idx.release(); y.release();
    aw.Wp.release(); aw.colsum.release(); aw.pb.release();
  }
};

// buffers + descriptor of a prepared weight; the packing itself is a PackArgs job
int prepare_affine_meta(AffineW &aw, const int8_t *dW, int K, int N, const uint32_t *d_idx,
                        const float *d_bias, float a_quant, float b_quant, PackArgs &job, int n_src = 0) {
  const int n_tiles = (N + 15) / 16;
  HIPCHK(aw.Wp.reserve(packed_weight_bytes(K, N)));
  HIPCHK(aw.colsum.reserve(colsum_alloc_bytes(N)));
  HIPCHK(aw.pb.reserve((size_t)n_tiles * 16 * sizeof(float)));
  job.W = dW; job.K = K; job.N = N; job.idx = d_idx; job.bias = d_bias;
  job.n_src = n_src;
  job.mult = pack_mult(a_quant, b_quant);
  job.Wp = aw.Wp.p; job.colsum = aw.colsum.as<int>(); job.pb = aw.pb.as<float>();
  aw.w.Wp = aw.Wp.p;
  aw.w.colsum = aw.colsum.as<int>();
  aw.w.cp4 = aw.colsum.as<int>() + epi_pair_offset_ints(N);
  aw.w.pb = aw.pb.as<float>();
  aw.w.u = 1.0f / (a_quant * b_quant);  // Intgemm.inl.cc:146
  aw.w.a_quant = a_quant;
  aw.w.b_quant = b_quant;
  aw.w.K = K;
  aw.w.N = N;
  aw.w.n_tiles = n_tiles;
  return 0;
}

int prepare_affine(AffineW &aw, const int8_t *dW, int K, int N, const uint32_t *d_idx,
                   const float *d_bias, float a_quant, float b_quant, hipStream_t st) {
  const int n_tiles = (N + 15) / 16;
  HIPCHK(aw.Wp.reserve(packed_weight_bytes(K, N)));
  HIPCHK(aw.colsum.reserve(colsum_alloc_bytes(N)));
  HIPCHK(aw.pb.reserve((size_t)n_tiles * 16 * sizeof(float)));
  HIPCHK(launch_pack_weight(dW, K, N, d_idx, d_bias, a_quant, b_quant, aw.Wp.p,
                            aw.colsum.as<int>(), aw.pb.as<float>(), st));
  aw.w.Wp = aw.Wp.p;
  aw.w.colsum = aw.colsum.as<int>();
  aw.w.cp4 = aw.colsum.as<int>() + epi_pair_offset_ints(N);
  aw.w.pb = aw.pb.as<float>();
  aw.w.u = 1.0f / (a_quant * b_quant);  // Intgemm.inl.cc:146
  aw.w.a_quant = a_quant;
  aw.w.b_quant = b_quant;
  aw.w.K = K;
  aw.w.N = N;
  aw.w.n_tiles = n_tiles;
  return 0;
}

int affine_common(const float *x, size_t M, size_t K, const int8_t *W_nk, size_t N,
                  const float *bias, float a_quant, float b_quant, const uint32_t *idx,
                  size_t n_idx, float *y, int32_t *acc) {
  if (!x || !W_nk || (!y && !acc)) return fail(-1, "null argument");
  if (K == 0 || K % 64 != 0 || K > 4096) return fail(-1, "K=%zu must be a multiple of 64, <= 4096", K);
  if (M == 0 || N == 0) return fail(-1, "empty operand");
  if (idx && n_idx == 0) return fail(-1, "empty index list");
  hipStream_t st = nullptr;
  TmpAffine t;
  const size_t Nout = idx ? n_idx : N;
  HIPCHK(t.x.reserve(M * K * sizeof(float)));
  HIPCHK(t.W.reserve(N * K));
  HIPCHK(hipMemcpyAsync(t.x.p, x, M * K * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.W.p, W_nk, N * K, hipMemcpyHostToDevice, st));
  if (bias) {
    HIPCHK(t.bias.reserve(N * sizeof(float)));
    HIPCHK(hipMemcpyAsync(t.bias.p, bias, N * sizeof(float), hipMemcpyHostToDevice, st));
  }
  if (idx) {
    for (size_t i = 0; i < n_idx; ++i)
      if (idx[i] >= N) return fail(-1, "index %u out of range (N=%zu)", idx[i], N);
    HIPCHK(t.idx.reserve(n_idx * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(t.idx.p, idx, n_idx * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  RCCHK(prepare_affine(t.aw, t.W.as<int8_t>(), (int)K, (int)Nout, idx ? t.idx.as<uint32_t>() : nullptr,
                       bias ? t.bias.as<float>() : nullptr, a_quant, b_quant, st));
  GemmArgs g;
  g.x_f32 = t.x.as<float>();
  g.lda = (int)K;
  g.M = (int)M;
  g.w = t.aw.w;
  if (acc) {
    HIPCHK(t.y.reserve(M * Nout * sizeof(int32_t)));
    g.acc_out = t.y.as<int32_t>();
    HIPCHK(launch_gemm(g, EPI_ACC, M >= 64 ? 64 : 16, st));
    HIPCHK(hipMemcpyAsync(acc, t.y.p, M * Nout * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  } else {
    HIPCHK(t.y.reserve(M * Nout * sizeof(float)));
    g.y = t.y.as<float>();
    g.ldy = (int)Nout;
    // many rows: the 128-row tiling (rows_per_block 0 asks for it where it applies)
    HIPCHK(launch_gemm(g, EPI_PLAIN, M >= 1024 ? 0 : (M >= 64 ? 64 : 16), st));
    HIPCHK(hipMemcpyAsync(y, t.y.p, M * Nout * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

}  // namespace

extern "C" int slimt_hip_affine(const float *x, size_t M, size_t K, const int8_t *W_nk, size_t N,
                                const float *bias, float a_quant, float b_quant, float *y) {
  return affine_common(x, M, K, W_nk, N, bias, a_quant, b_quant, nullptr, 0, y, nullptr);
}

extern "C" int slimt_hip_affine_select(const float *x, size_t M, size_t K, const int8_t *W_nk,
                                       size_t N, const float *bias, float a_quant, float b_quant,
                                       const uint32_t *idx, size_t n_idx, float *y) {
  if (!idx) return fail(-1, "idx is NULL");
  return affine_common(x, M, K, W_nk, N, bias, a_quant, b_quant, idx, n_idx, y, nullptr);
}

extern "C" int slimt_hip_affine_acc_i32(const float *x, size_t M, size_t K, const int8_t *W_nk,
                                        size_t N, float a_quant, int32_t *accS) {
  return affine_common(x, M, K, W_nk, N, nullptr, a_quant, 1.0f, nullptr, 0, nullptr, accS);
}

namespace {
struct Tmp3 {
  DevBuf a, b, c, d, e, f;
  ~Tmp3() { a.release(); b.release(); c.release(); d.release(); e.release(); f.release(); }
};
}  // namespace

extern "C" int slimt_hip_layer_norm(const float *x, const float *scale, const float *bias,
                                    float eps, size_t rows, size_t cols, float *y) {
  if (!x || !scale || !bias || !y || !rows || !cols) return fail(-1, "bad argument");
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(rows * cols * 4));
  HIPCHK(t.b.reserve(cols * 4));
  HIPCHK(t.c.reserve(cols * 4));
  HIPCHK(t.d.reserve(rows * cols * 4));
  HIPCHK(hipMemcpyAsync(t.a.p, x, rows * cols * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.b.p, scale, cols * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.c.p, bias, cols * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_layer_norm(t.a.as<float>(), t.b.as<float>(), t.c.as<float>(), eps, (int)rows,
                           (int)cols, t.d.as<float>(), st));
  HIPCHK(hipMemcpyAsync(y, t.d.p, rows * cols * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_softmax(const float *x, size_t rows, size_t cols, float *y) {
  if (!x || !y || !rows || !cols) return fail(-1, "bad argument");
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(rows * cols * 4));
  HIPCHK(t.b.reserve(rows * cols * 4));
  HIPCHK(hipMemcpyAsync(t.a.p, x, rows * cols * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_softmax(t.a.as<float>(), (int)rows, (int)cols, t.b.as<float>(), st));
  HIPCHK(hipMemcpyAsync(y, t.b.p, rows * cols * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_sample_truncated(const float *logits, size_t M, size_t N, const uint32_t *ids, float temperature,
                                          uint32_t top_k, float top_p, const uint64_t *keys, const uint32_t *steps,
                                          uint32_t *columns, float *thresholds, uint32_t *kept, float *scores) {
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return fail(-1, "sampling: temperature %g is not finite and > 0", (double)temperature);
  const float inv_T = 1.0f / temperature;
  if (!(inv_T > 0.0f) || !std::isfinite(inv_T)) return fail(-1, "sampling: 1 / temperature %g is not finite and > 0", (double)temperature);
  if (!(top_p > 0.0f && top_p <= 1.0f)) return fail(-1, "sampling truncation: top_p %g is not in (0, 1]", (double)top_p);
  if (!logits || !columns || !thresholds || !kept || !scores || !M || !N) return fail(-1, "bad argument");
  if (M > 0x7fffffffu || N > (size_t)kSampleTruncMaxN) return fail(-1, "sample_truncated: more than %d rows or %d columns", 0x7fffffff, kSampleTruncMaxN);
  std::vector<uint32_t> seeds(2 * M);  // the rows' hash words (sampling.h), as decode_begin_step_sm_kernel writes them
  for (size_t r = 0; r < M; ++r) {
    const uint64_t w = slimt_hip::sm_step_words(keys ? keys[r] : (uint64_t)r, steps ? steps[r] : 0u);
    seeds[r] = (uint32_t)w;
    seeds[M + r] = (uint32_t)(w >> 32);
  }
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(M * N * 4));
  HIPCHK(t.b.reserve(N * 4));
  HIPCHK(t.c.reserve(2 * M * 4));
  HIPCHK(t.d.reserve(7 * M * 4));
  HIPCHK(hipMemcpyAsync(t.a.p, logits, M * N * 4, hipMemcpyHostToDevice, st));
  if (ids) HIPCHK(hipMemcpyAsync(t.b.p, ids, N * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.c.p, seeds.data(), 2 * M * 4, hipMemcpyHostToDevice, st));
  SampleTruncArgs a;
  a.logits = t.a.as<float>();
  a.B = (int)M;
  a.N = (int)N;
  a.inv_T = inv_T;
  a.top_k = top_k;
  a.top_p = top_p;
  a.seeds = t.c.as<uint32_t>();
  a.shortlist = ids ? t.b.as<uint32_t>() : nullptr;
  float *o = t.d.as<float>();
  a.part_val = o;
  a.part_idx = reinterpret_cast<int *>(o + M);
  a.part_sum = o + 2 * M;
  a.part_mz = o + 3 * M;
  a.part_zw = o + 4 * M;
  a.thresholds = o + 5 * M;
  a.kept = reinterpret_cast<uint32_t *>(o + 6 * M);
  HIPCHK(launch_sample_truncated(a, st));
  std::vector<float> h(7 * M);
  HIPCHK(hipMemcpyAsync(h.data(), t.d.p, 7 * M * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t r = 0; r < M; ++r) {
    int col;
    memcpy(&col, &h[M + r], 4);
    // the "none" rule of decode_begin_step_sm_kernel: no key beat the start value, or logit 0 is NaN -- class 0, score NaN
    const bool none = col == 0x7fffffff || logits[r * N] != logits[r * N];
    columns[r] = none ? 0u : (uint32_t)col;
    scores[r] = slimt_hip::forced_score(h[2 * M + r], h[4 * M + r] - h[3 * M + r], none);
    thresholds[r] = h[5 * M + r];
    memcpy(&kept[r], &h[6 * M + r], 4);
  }
  return 0;
}

extern "C" int slimt_hip_highway(const float *x, const float *y, const float *g, size_t n,
                                 float *out) {
  if (!x || !y || !g || !out || !n) return fail(-1, "bad argument");
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(n * 4));
  HIPCHK(t.b.reserve(n * 4));
  HIPCHK(t.c.reserve(n * 4));
  HIPCHK(t.d.reserve(n * 4));
  HIPCHK(hipMemcpyAsync(t.a.p, x, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.b.p, y, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.c.p, g, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_highway(t.a.as<float>(), t.b.as<float>(), t.c.as<float>(), n, t.d.as<float>(), st));
  HIPCHK(hipMemcpyAsync(out, t.d.p, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_sdpa(const float *q, const float *k, const float *v, const float *mask,
                              size_t B, size_t H, size_t Tq, size_t S, size_t dh, float *out,
                              float *attn) {
  if (!q || !k || !v || !mask || !out) return fail(-1, "null argument");
  if (S < 1 || S > 128 || dh < 1 || dh > 64) return fail(-1, "unsupported S=%zu dh=%zu", S, dh);
  Tmp3 t;
  DevBuf qj, kj, vj, oj, ob;
  struct G { DevBuf *b[5]; ~G() { for (auto *x : b) x->release(); } } guard{{&qj, &kj, &vj, &oj, &ob}};
  hipStream_t st = nullptr;
  const size_t D = H * dh;
  const size_t nq = B * Tq * D * 4, nk = B * S * D * 4;
  HIPCHK(t.a.reserve(nq)); HIPCHK(t.b.reserve(nk)); HIPCHK(t.c.reserve(nk));
  HIPCHK(t.d.reserve(B * S * 4));
  HIPCHK(qj.reserve(nq)); HIPCHK(kj.reserve(nk)); HIPCHK(vj.reserve(nk));
  HIPCHK(oj.reserve(nq)); HIPCHK(ob.reserve(nq));
  HIPCHK(hipMemcpyAsync(t.a.p, q, nq, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.b.p, k, nk, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.c.p, v, nk, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.d.p, mask, B * S * 4, hipMemcpyHostToDevice, st));
  // [B,H,T,dh] -> joined [B,T,H*dh] (the engine's native layout)
  HIPCHK(launch_transpose_heads(t.a.as<float>(), (int)B, (int)H, (int)Tq, (int)dh, qj.as<float>(), st));
  HIPCHK(launch_transpose_heads(t.b.as<float>(), (int)B, (int)H, (int)S, (int)dh, kj.as<float>(), st));
  HIPCHK(launch_transpose_heads(t.c.as<float>(), (int)B, (int)H, (int)S, (int)dh, vj.as<float>(), st));
  if (attn) HIPCHK(t.e.reserve(B * H * Tq * S * 4));
  AttnArgs a;
  a.q = qj.as<float>(); a.k = kj.as<float>(); a.v = vj.as<float>();
  a.ldq = a.ldk = a.ldv = a.ldo = (int)D;
  a.mask = t.d.as<float>();
  a.B = (int)B; a.H = (int)H; a.Tq = (int)Tq; a.S = (int)S; a.dh = (int)dh;
  a.alpha = 1.0f / std::sqrt((float)dh);  // Modules.cc:43
  a.out = oj.as<float>();
  a.attn = attn ? t.e.as<float>() : nullptr;
  HIPCHK(launch_attention(a, st));
  HIPCHK(launch_transpose_heads(oj.as<float>(), (int)B, (int)Tq, (int)H, (int)dh, ob.as<float>(), st));
  HIPCHK(hipMemcpyAsync(out, ob.p, nq, hipMemcpyDeviceToHost, st));
  if (attn) HIPCHK(hipMemcpyAsync(attn, t.e.p, B * H * Tq * S * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
namespace {

struct ParamTable {
  std::map<std::string, const slimt_hip_param *> by_name;
  const slimt_hip_param *get(const std::string &n) const {
    auto it = by_name.find(n);
    return it == by_name.end() ? nullptr : it->second;
  }
};

int upload_f32(DevBuf &dst, const ParamTable &t, const std::string &name, size_t expect) {
  const slimt_hip_param *p = t.get(name);
  if (!p) return fail(-1, "missing parameter %s", name.c_str());
  if (p->type != 0 || (size_t)p->rows * p->cols != expect)
    return fail(-1, "parameter %s: expected f32 with %zu elements", name.c_str(), expect);
  HIPCHK(dst.reserve(expect * 4));
  HIPCHK(hipMemcpy(dst.p, p->data, expect * 4, hipMemcpyHostToDevice));
  return 0;
}

int scalar_f32(const ParamTable &t, const std::string &name, float *out) {
  const slimt_hip_param *p = t.get(name);
  if (!p) return fail(-1, "missing parameter %s", name.c_str());
  if (p->type != 0) return fail(-1, "parameter %s must be f32", name.c_str());
  *out = *reinterpret_cast<const float *>(p->data);
  return 0;
}

// Affine{W,b,quant} / Linear{W,quant} binding (Modules.cc:145-180,361-400)
int load_affine(AffineW &aw, const ParamTable &t, const std::string &wname,
                const std::string &bname /* may be empty */, int K, int N, DevBuf &scratch) {
  const slimt_hip_param *W = t.get(wname);
  if (!W) return fail(-1, "missing parameter %s", wname.c_str());
  if (W->type != 1 || W->rows != K || W->cols != N)
    return fail(-1, "parameter %s: expected intgemm8 [%d,%d], got type %d [%d,%d]", wname.c_str(),
                K, N, W->type, W->rows, W->cols);
  float a_quant = 0.f, b_quant = 0.f;
  RCCHK(scalar_f32(t, wname + "_QuantMultA", &a_quant));
  // b_quant sits right after the int8 payload (Modules.cc:18-22)
  memcpy(&b_quant, reinterpret_cast<const int8_t *>(W->data) + (size_t)K * N, sizeof(float));
  DevBuf bias;
  if (!bname.empty()) {
    int rc = upload_f32(bias, t, bname, (size_t)N);
    if (rc) return rc;
  }
  HIPCHK(scratch.reserve((size_t)K * N));
  // qmm::prepare_weight_quantized_transposed (Io.cc:234) is the identity for
  // this backend: the file layout [N][K] is the canonical layout.
  HIPCHK(hipMemcpy(scratch.p, W->data, (size_t)K * N, hipMemcpyHostToDevice));
  int rc = prepare_affine(aw, scratch.as<int8_t>(), K, N, nullptr,
                          bname.empty() ? nullptr : bias.as<float>(), a_quant, b_quant, nullptr);
  hipError_t e = hipDeviceSynchronize();
  bias.release();
  if (rc) return rc;
  HIPCHK(e);
  return 0;
}

int load_ln(LnW &ln, const ParamTable &t, const std::string &prefix, int D) {
  RCCHK(upload_f32(ln.scale, t, prefix + "_ln_scale", (size_t)D));
  RCCHK(upload_f32(ln.bias, t, prefix + "_ln_bias", (size_t)D));
  return 0;
}

int load_attn(AttnW &a, const ParamTable &t, const std::string &prefix, int D, DevBuf &scratch) {
  RCCHK(load_affine(a.q, t, prefix + "Wq", prefix + "bq", D, D, scratch));
  RCCHK(load_affine(a.k, t, prefix + "Wk", prefix + "bk", D, D, scratch));
  RCCHK(load_affine(a.v, t, prefix + "Wv", prefix + "bv", D, D, scratch));
  RCCHK(load_affine(a.o, t, prefix + "Wo", prefix + "bo", D, D, scratch));
  RCCHK(load_ln(a.ln, t, prefix + "Wo", D));
  return 0;
}

void free_affine(AffineW &a) {
  a.Wp.release();
  a.colsum.release();
  a.pb.release();
}
void free_ln(LnW &l) {
  l.scale.release();
  l.bias.release();
}
void free_attn(AttnW &a) {
  free_affine(a.q); free_affine(a.k); free_affine(a.v); free_affine(a.o);
  free_ln(a.ln);
}

void model_free(slimt_hip_model *m) {
  for (auto &L : m->enc) {
    free_attn(L.attn); free_affine(L.ffn1); free_affine(L.ffn2); free_ln(L.ffn_ln);
  }
  for (auto &L : m->dec) {
    free_affine(L.rnn_f); free_affine(L.rnn_w); free_ln(L.rnn_ln);
    free_attn(L.attn); free_affine(L.ffn1); free_affine(L.ffn2); free_ln(L.ffn_ln);
  }
  m->wemb.release(); m->out_raw.release(); m->out_bias.release();
  free_affine(m->out_full);
  for (hipEvent_t ev : m->gate_ev) (void)hipEventDestroy(ev);
  m->gate_ev.clear();
}

int model_build(slimt_hip_model *m, const slimt_hip_param *params, size_t n,
                const slimt_hip_dims *dims) {
  ParamTable t;
  for (size_t i = 0; i < n; ++i) {
    const slimt_hip_param &p = params[i];
    if (!p.name || !p.data) continue;
    if (p.type != 0 && p.type != 1) return fail(-1, "parameter %s: unknown type %d", p.name, p.type);
    if (p.rows <= 0 || p.cols <= 0)
      return fail(-1, "parameter %s: bad shape [%d,%d]", p.name, p.rows, p.cols);
    // a truncated or malformed file must not make the uploads below read past its mapping
    const uint64_t need = (uint64_t)p.rows * (uint64_t)p.cols * (p.type == 0 ? 4u : 1u) + (p.type == 1 ? 4u : 0u);
    if (p.bytes && p.bytes < need)
      return fail(-1, "parameter %s: %llu bytes, its shape [%d,%d] needs %llu", p.name,
                  (unsigned long long)p.bytes, p.rows, p.cols, (unsigned long long)need);
    t.by_name[p.name] = &p;
  }
  const slimt_hip_param *wemb = t.get("Wemb");
  if (!wemb) return fail(-1, "missing parameter Wemb");
  if (wemb->type != 1) return fail(-1, "Wemb must be intgemm8");
  m->V = wemb->rows;
  m->D = wemb->cols;
  m->H = dims->num_heads;
  m->Le = dims->encoder_layers;
  m->Ld = dims->decoder_layers;
  const int D = m->D, V = m->V;
  // What the per-stage kernels -- the path every model must be able to take (decode mode 1, slimt_hip_decode_step) -- are
  // instantiated for (the tilings are template arguments: further instantiations would widen the family again):
  //  D: the encoder's LayerNorm epilogue owns whole rows in 1, 2, 4 or 8 column tiles of 64 (kernels.hip, EPI_RES_LN)
  if (D != 64 && D != 128 && D != 256 && D != 512)
    return fail(-1, "unsupported embedding size %d (64, 128, 256 or 512)", D);
  //  D / H: the decoder's cross-attention exists for 16, 32 and 64, at D = 512 for 32 and 64 (decode_kernels.hip, dqattn_kernel)
  if (m->H <= 0 || D % m->H != 0) return fail(-1, "unsupported head count %d for embedding size %d", m->H, D);
  {
    const int dh = D / m->H;
    if ((dh != 16 && dh != 32 && dh != 64) || (D == 512 && dh == 16))
      return fail(-1, "unsupported head count %d: head size %d (16, 32 or 64; 32 or 64 at embedding size 512)", m->H, dh);
  }
  const slimt_hip_param *w1 = t.get("encoder_l1_ffn_W1");
  if (!w1) return fail(-1, "missing parameter encoder_l1_ffn_W1");
  m->F = w1->cols;
  //  F: the decoder's FFN2 keeps its 16 int8 input rows in LDS, up to K = 2048 (decode_kernels.hip, launch_dgemm)
  if (m->F % 64 != 0 || m->F <= 0 || m->F > 2048)
    return fail(-1, "unsupported ffn size %d (a multiple of 64, at most 2048)", m->F);
  const int F = m->F;
  const size_t VD = (size_t)V * D;

  // Wemb (Io.cc:182-224): keep the int8 table for lookups (E = q * (1/m)),
  // and re-quantise the dequantised table for the tied output layer exactly
  // as io::load_items does through qmm::prepare_weight_transposed.
  const int8_t *wq = reinterpret_cast<const int8_t *>(wemb->data);
  memcpy(&m->wemb_mult, wq + VD, sizeof(float));
  HIPCHK(m->wemb.reserve(VD));
  HIPCHK(hipMemcpy(m->wemb.p, wq, VD, hipMemcpyHostToDevice));
  {
    std::vector<float> E(VD);
    const float inv = 1 / m->wemb_mult;  // Io.cc:280-281
    for (size_t i = 0; i < VD; ++i) E[i] = static_cast<float>(wq[i]) * inv;
    std::vector<int8_t> prepared(VD);
    RCCHK(slimt_hip_prepare_weight_transposed(E.data(), prepared.data(), m->wemb_mult, (size_t)D,
                                              (size_t)V));
    HIPCHK(m->out_raw.reserve(VD));
    HIPCHK(hipMemcpy(m->out_raw.p, prepared.data(), VD, hipMemcpyHostToDevice));
    m->out_tied_exact = memcmp(prepared.data(), wq, VD) == 0;  // (both [V][D]: the preparation keeps the layout)
  }
  RCCHK(scalar_f32(t, "none_QuantMultA", &m->out_a_quant));
  RCCHK(upload_f32(m->out_bias, t, "decoder_ff_logit_out_b", (size_t)V));
  RCCHK(prepare_affine(m->out_full, m->out_raw.as<int8_t>(), D, V, nullptr,
                       m->out_bias.as<float>(), m->out_a_quant, m->wemb_mult, nullptr));
  HIPCHK(hipDeviceSynchronize());

  DevBuf scratch;
  struct G { DevBuf *b; ~G() { b->release(); } } guard{&scratch};
  m->enc.resize((size_t)m->Le);
  m->dec.resize((size_t)m->Ld);
  for (int i = 0; i < m->Le; ++i) {
    const std::string L = "encoder_l" + std::to_string(i + 1);
    auto &E = m->enc[(size_t)i];
    RCCHK(load_attn(E.attn, t, L + "_self_", D, scratch));
    RCCHK(load_affine(E.ffn1, t, L + "_ffn_W1", L + "_ffn_b1", D, F, scratch));
    RCCHK(load_affine(E.ffn2, t, L + "_ffn_W2", L + "_ffn_b2", F, D, scratch));
    RCCHK(load_ln(E.ffn_ln, t, L + "_ffn_ffn", D));
  }
  for (int i = 0; i < m->Ld; ++i) {
    const std::string L = "decoder_l" + std::to_string(i + 1);
    auto &Dl = m->dec[(size_t)i];
    RCCHK(load_affine(Dl.rnn_w, t, L + "_rnn_W", "", D, D, scratch));
    RCCHK(load_affine(Dl.rnn_f, t, L + "_rnn_Wf", L + "_rnn_bf", D, D, scratch));
    RCCHK(load_ln(Dl.rnn_ln, t, L + "_rnn_ffn", D));
    RCCHK(load_attn(Dl.attn, t, L + "_context_", D, scratch));
    RCCHK(load_affine(Dl.ffn1, t, L + "_ffn_W1", L + "_ffn_b1", D, F, scratch));
    RCCHK(load_affine(Dl.ffn2, t, L + "_ffn_W2", L + "_ffn_b2", F, D, scratch));
    RCCHK(load_ln(Dl.ffn_ln, t, L + "_ffn_ffn", D));
  }
  return 0;
}

}  // namespace

extern "C" int slimt_hip_model_create(const slimt_hip_param *params, size_t n_params,
                                      const slimt_hip_dims *dims, int device,
                                      slimt_hip_model **out) {
  if (!params || !dims || !out) return fail(-1, "null argument");
  *out = nullptr;
  int count = 0;
  RCCHK(slimt_hip_device_count(&count));
  if (count <= 0) return fail(-1, "no HIP device available (this backend has no CPU fallback)");
  if (device < 0 || device >= count) return fail(-1, "device %d out of range (%d devices)", device, count);
  HIPCHK(hipSetDevice(device));
  auto *m = new slimt_hip_model();
  m->device = device;
  {  // default decoder admission: three quarters of the CUs (measured optimum)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->decoder_budget = 7 * prop.multiProcessorCount / 8;
  }
  // the hardware queues the runtime started with: it has read GPU_MAX_HW_QUEUES by now (slimt_hip_device_count
  // initialised it), and this library only ever reads the variable here (slimt_hip_request_hw_queues aside)
  m->hw_queues = slimt_hip_hw_queues() > 0 ? slimt_hip_hw_queues() : 4;
  int rc = model_build(m, params, n_params, dims);
  if (rc) {
    model_free(m);
    delete m;
    return rc;
  }
  *out = m;
  return 0;
}

// The Marian .bin container (slimt/Io.cc:114-161): version, item count, headers, names, shapes,
// padding to a 256-byte boundary, payloads. Only views are taken; every read is bounds-checked.
extern "C" int slimt_hip_model_create_from_bin(const void *bin, size_t size, const slimt_hip_dims *dims,
                                               int device, slimt_hip_model **out) {
  if (!bin || !dims || !out) return fail(-1, "null argument");
  *out = nullptr;
  const char *p = static_cast<const char *>(bin), *const end = p + size;
  auto take = [&](size_t n) -> const char * {
    if ((size_t)(end - p) < n) return nullptr;
    const char *q = p;
    p += n;
    return q;
  };
  auto u64 = [&](uint64_t *v) -> bool {
    const char *q = take(8);
    if (q) memcpy(v, q, 8);
    return q != nullptr;
  };
  uint64_t version = 0, n = 0;
  if (!u64(&version) || !u64(&n)) return fail(-1, "truncated Marian .bin");
  if (version != 1) return fail(-1, "Marian .bin version %llu != 1", (unsigned long long)version);
  if (n > (1u << 20)) return fail(-1, "implausible item count %llu", (unsigned long long)n);
  struct Header { uint64_t name_length, type, shape_length, data_length; };  // slimt/Io.hh:24-29
  std::vector<Header> headers((size_t)n);
  for (Header &h : headers) {
    const char *q = take(sizeof(Header));
    if (!q) return fail(-1, "truncated Marian .bin");
    memcpy(&h, q, sizeof(Header));
  }
  std::vector<std::string> names((size_t)n);
  for (size_t i = 0; i < n; ++i) {
    const char *q = take(headers[i].name_length);
    if (!q) return fail(-1, "truncated Marian .bin");
    names[i].assign(q, headers[i].name_length ? headers[i].name_length - 1 : 0);
  }
  std::vector<slimt_hip_param> params;
  params.reserve((size_t)n);
  std::vector<size_t> which;
  for (size_t i = 0; i < n; ++i) {
    if (headers[i].shape_length > 8) return fail(-1, "item %s: %llu dimensions", names[i].c_str(), (unsigned long long)headers[i].shape_length);
    int32_t rows = 1, cols = 1;
    for (uint64_t d = 0; d < headers[i].shape_length; ++d) {
      const char *q = take(4);
      if (!q) return fail(-1, "truncated Marian .bin");
      int32_t v;
      memcpy(&v, q, 4);
      if (d + 2 == headers[i].shape_length) rows = v;
      if (d + 1 == headers[i].shape_length) cols = v;
    }
    const int type = headers[i].type == 0x0404 ? 0 : headers[i].type == 0x4101 ? 1 : -1;  // f32 / intgemm8 (Io.cc:37-84)
    if (type < 0) continue;  // e.g. special:model.yml
    slimt_hip_param q;
    q.name = names[i].c_str();
    q.type = type;
    q.rows = rows;
    q.cols = cols;
    q.data = nullptr;
    q.bytes = headers[i].data_length;
    params.push_back(q);
    which.push_back(i);
  }
  uint64_t pad = 0;
  if (!u64(&pad) || !take(pad)) return fail(-1, "truncated Marian .bin");  // Io.cc:151-153
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    const char *q = take(headers[i].data_length);
    if (!q) return fail(-1, "truncated Marian .bin (payload of %s)", names[i].c_str());
    if (k < which.size() && which[k] == i) params[k++].data = q;
  }
  return slimt_hip_model_create(params.data(), params.size(), dims, device, out);  // checks shapes against bytes
}

extern "C" int slimt_hip_model_destroy(slimt_hip_model *model) {
  if (!model) return 0;
  timing_report();
  (void)hipSetDevice(model->device);
  model_free(model);
  if (model->kv_wide_count) (void)hipHostFree(model->kv_wide_count);
  for (auto &b : model->kv_centre) b.release();
  model->kv_centre_sums.release();
  if (model->kv_centre_ev) (void)hipEventDestroy(model->kv_centre_ev);
  delete model;
  return 0;
}

extern "C" int slimt_hip_model_set_decoder_budget(slimt_hip_model *model, int workgroups) {
  if (!model) return fail(-1, "model is NULL");
  if (workgroups < 0) return fail(-1, "decoder budget %d < 0", workgroups);
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->decoder_budget = workgroups;
  return 0;
}

extern "C" int slimt_hip_model_set_kv_cache_policy(slimt_hip_model *model, int policy) {
  if (!model) return fail(-1, "model is NULL");
  if (policy < 0 || policy > 2) return fail(-1, "K/V cache policy %d not in 0..2", policy);
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->kv_policy = policy;
  return 0;
}

extern "C" int slimt_hip_model_set_xcd_affinity(slimt_hip_model *model, int xcds) {
  if (!model) return fail(-1, "model is NULL");
  if (xcds != 0 && xcds != 1 && xcds != 2 && xcds != 4) return fail(-1, "XCD affinity %d not in {0, 1, 2, 4}", xcds);
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->xcd_affinity = xcds;
  return 0;
}

extern "C" int slimt_hip_model_set_adaptive_decoder_rows(slimt_hip_model *model, int on) {
  if (!model) return fail(-1, "model is NULL");
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->adaptive_rows = on != 0;
  return 0;
}

extern "C" int slimt_hip_model_set_kv_cache_format(slimt_hip_model *model, int format) {
  if (!model) return fail(-1, "model is NULL");
  if (format < 0 || format > 3) return fail(-1, "K/V cache format %d not in 0..3", format);
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->kv_format = format;
  kv_watch_restart(model);  // choosing a format starts format 0's watches afresh (engine.h, kv_auto_wide)
  return 0;
}

extern "C" int slimt_hip_debug_kv_watch(slimt_hip_model *model, int *switched_to_24_bit, uint64_t *wide, uint64_t *submitted) {
  if (!model) return fail(-1, "model is NULL");
  if (switched_to_24_bit) *switched_to_24_bit = model->kv_auto_wide.load(std::memory_order_relaxed) ? 1 : 0;
  if (wide) *wide = model->kv_wide_count ? *static_cast<volatile unsigned long long *>(model->kv_wide_count) : 0;
  if (submitted) *submitted = model->kv_layers_submitted.load(std::memory_order_relaxed);
  return 0;
}

extern "C" int slimt_hip_debug_cross_attention(slimt_hip_ctx *ctx, int layer, int literal, const float *yq, float *joined,
                                               float *attn) {
  if (!ctx || !yq || !joined) return fail(-1, "null argument");
  const slimt_hip_model *m = ctx->model;
  if (layer < 0 || layer >= m->Ld) return fail(-1, "decoder layer %d not in 0..%d", layer, m->Ld - 1);
  if (!ctx->decode_ready || !ctx->kv_ready)
    return fail(-1, "no f32 K/V cache: call slimt_hip_decode_begin (or _begin_from) for the batch first");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  const int B = ctx->B, S = ctx->S, D = m->D, M = B * S;
  const DecLayerW &L = m->dec[(size_t)layer];
  HIPCHK(ctx->dout.reserve((size_t)B * D * 4));
  HIPCHK(ctx->dh.reserve((size_t)B * D * 4));
  HIPCHK(ctx->attn_dbg.reserve((size_t)B * m->H * S * 4));
  HIPCHK(hipMemcpyAsync(ctx->dh.p, yq, (size_t)B * D * 4, hipMemcpyHostToDevice, st));
  DQAttnArgs a;
  a.B = B; a.D = D; a.H = m->H; a.S = S;
  a.x.x = ctx->dh.as<float>();  // (unused rows: the queries are given)
  a.wq = L.attn.q.w;
  a.q_given = ctx->dh.as<float>();
  a.literal = literal != 0;
  const float *kv = ctx->kv.as<float>();
  a.k = kv + (size_t)(2 * layer) * M * D;
  a.v = kv + (size_t)(2 * layer + 1) * M * D;
  a.ldv = D;
  a.uk = L.attn.k.w.u;
  a.uv = L.attn.v.w.u;
  a.pbk = L.attn.k.w.pb;
  a.pbv = L.attn.v.w.pb;
  a.lengths = ctx->lengths.as<uint32_t>();
  a.alpha = 1.0f / std::sqrt(static_cast<float>(D / m->H));
  a.out_f32 = ctx->dout.as<float>();
  a.attn = ctx->attn_dbg.as<float>();
  HIPCHK(launch_dqattn(a, st));
  HIPCHK(hipMemcpyAsync(joined, ctx->dout.p, (size_t)B * D * 4, hipMemcpyDeviceToHost, st));
  if (attn) HIPCHK(hipMemcpyAsync(attn, ctx->attn_dbg.p, (size_t)B * m->H * S * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_debug_break_shortlist_handoff(slimt_hip_ctx *ctx, int broken, unsigned poll_limit) {
  if (!ctx) return fail(-1, "ctx is NULL");
  if (poll_limit == 0 || poll_limit > (1u << 24)) return fail(-1, "poll limit %u not in 1..2^24", poll_limit);
  ctx->gen_break = broken != 0;
  ctx->gen_spin_limit = poll_limit;
  return 0;
}

extern "C" int slimt_hip_debug_ctx_set_counters(slimt_hip_ctx *ctx, uint32_t value) {
  if (!ctx) return fail(-1, "ctx is NULL");
  if (!ctx->ticket.p) return fail(-1, "the context has no ticket counters");
  HIPCHK(hipSetDevice(ctx->model->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // the device words (engine.cpp, slimt_hip_ctx_create): [0] decoder, [1] fused encoder, [2..3] the two halves of the claim word
  const uint32_t words[4] = {value, value, value, value};
  HIPCHK(hipMemcpy(ctx->ticket.p, words, sizeof(words), hipMemcpyHostToDevice));
  ctx->ticket_base = ctx->enc_ticket_base = ctx->xarr_base = ctx->xclaim_base = value;
  // (an epoch of 0xffffffff is never carried from one launch to the next: encode_device turns it into 0 when it is used)
  ctx->gen_epoch = value == 0xffffffffu ? 0u : value;
  if (ctx->gen_flag.p) HIPCHK(hipMemset(ctx->gen_flag.p, 0, 64));
  return 0;
}

extern "C" int slimt_hip_debug_ctx_shortlists(slimt_hip_ctx *ctx, size_t n_batches, uint32_t *ids, size_t capacity, uint32_t *counts) {
  if (!ctx || !ids || !counts) return fail(-1, "null argument");
  if (n_batches == 0 || n_batches > (size_t)kMaxMerge) return fail(-1, "%zu shortlists not in 1..%d", n_batches, kMaxMerge);
  const size_t V = (size_t)ctx->model->V;
  // sub-batch j's ids at j * V, its count at n_sl_dev[j] (translate_many_generated); only what the context has reserved
  if (!ctx->n_sl_dev.p || ctx->n_sl_dev.bytes < n_batches * 4)
    return fail(-1, "shortlists: the context holds %zu counts, %zu asked for (no *_generated call yet?)", ctx->n_sl_dev.bytes / 4, n_batches);
  if (!ctx->shortlist.p || ctx->shortlist.bytes < n_batches * V * 4)
    return fail(-1, "shortlists: the context holds room for %zu lists of %zu ids, %zu asked for", ctx->shortlist.bytes / (V * 4), V, n_batches);
  HIPCHK(hipSetDevice(ctx->model->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(counts, ctx->n_sl_dev.p, n_batches * 4, hipMemcpyDeviceToHost));
  for (size_t j = 0; j < n_batches; ++j) {
    const size_t n = std::min(std::min((size_t)counts[j], capacity), V);  // (a count above V is reported as it is, never followed)
    if (n) HIPCHK(hipMemcpy(ids + j * capacity, ctx->shortlist.as<uint32_t>() + j * V, n * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int slimt_hip_debug_out_tied_exact(slimt_hip_model *model, int *exact) {
  if (!model || !exact) return fail(-1, "null argument");
  *exact = model->out_tied_exact ? 1 : 0;
  return 0;
}

// The proof model_build runs on a model's Wemb, on the caller's table [rows][cols] alone (no device): the table
// dequantised, re-quantised by its own multiplier, compared byte for byte.
extern "C" int slimt_hip_debug_tied_output_proof(const int8_t *wemb, size_t rows, size_t cols, float multiplier, int *exact) {
  if (!wemb || !exact) return fail(-1, "null argument");
  const size_t n = rows * cols;
  std::vector<float> E(n);
  const float inv = 1 / multiplier;
  for (size_t i = 0; i < n; ++i) E[i] = static_cast<float>(wemb[i]) * inv;
  std::vector<int8_t> prepared(n);
  RCCHK(slimt_hip_prepare_weight_transposed(E.data(), prepared.data(), multiplier, cols, rows));
  *exact = memcmp(prepared.data(), wemb, n) == 0 ? 1 : 0;
  return 0;
}

// The fused decoder's dynamic LDS as its launcher asks for it (kernels.h, fused_decode_launch_lds_bytes) for a shape, the
// sentences per workgroup (32 / 16 / 8 / 4), a sentence-length class (mid), the cache form (tight) and what else picks the
// instantiation (flags: bit 0 merged, 1 non-temporal cache loads, 2 scored, 3 forced, 4 sampled): host code, needs no device.
extern "C" int slimt_hip_debug_fused_decode_lds_bytes(int D, int F, int Ld, int sentences_per_wg, int kv24, int mid, int tight,
                                                      unsigned flags, size_t *bytes, int *ln_in_lds, int *epi_in_lds) {
  if (!bytes || !ln_in_lds || !epi_in_lds) return fail(-1, "null argument");
  bool ln = false, epi = false;
  *bytes = fused_decode_launch_lds_bytes(D, F, Ld, sentences_per_wg, kv24 != 0, mid, tight != 0, (flags & 4u) != 0, (flags & 8u) != 0,
                                         (flags & 16u) != 0, (flags & 1u) != 0, (flags & 2u) != 0, mid ? nullptr : &ln, &epi);
  *ln_in_lds = ln ? 1 : 0;
  *epi_in_lds = epi ? 1 : 0;
  return 0;
}

extern "C" int slimt_hip_debug_kv_narrow_limit(slimt_hip_model *model, int limit) {
  if (!model) return fail(-1, "model is NULL");
  if (limit < 1 || limit > (1 << 19)) return fail(-1, "narrow-form limit %d not in 1..2^19 (20 bits hold [-2^19, 2^19))", limit);
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->kv_narrow_limit = limit;
  kv_watch_restart(model);  // (a new limit: the watch starts afresh)
  return 0;
}

extern "C" int slimt_hip_debug_kv_tight_limit(slimt_hip_model *model, int limit) {
  if (!model) return fail(-1, "model is NULL");
  if (limit < 0 || limit > (1 << 15)) return fail(-1, "tight-form limit %d not in 0..2^15 (int16 holds [-2^15, 2^15); 0 = never tried)", limit);
  std::lock_guard<std::mutex> lock(model->gate_mu);
  model->kv_tight_limit = limit;
  kv_watch_restart(model);
  return 0;
}

extern "C" int slimt_hip_debug_kv_centres(slimt_hip_model *model, int32_t *out, size_t n, int *ready) {
  if (!model || !ready) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(model->device));
  *ready = kv_centres_ready(model) ? 1 : 0;
  if (!*ready || !out) return 0;
  const size_t have = (size_t)model->Ld * 2 * (size_t)model->D;
  if (n < have) return fail(-1, "kv centres: room for %zu values, the model has %zu", n, have);
  HIPCHK(hipMemcpy(out, model->kv_centre[model->kv_gen.load(std::memory_order_relaxed)].p, have * 4, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int slimt_hip_debug_kv_recalibrations(slimt_hip_model *model, int *generations_started, int max_recalibrations) {
  if (!model) return fail(-1, "model is NULL");
  if (max_recalibrations >= 0) model->kv_recal_max = std::min(max_recalibrations, slimt_hip_model::kKvGens - 1);
  if (generations_started) *generations_started = model->kv_gen.load(std::memory_order_relaxed);
  return 0;
}

extern "C" int slimt_hip_model_set_kv_centres(slimt_hip_model *model, const int32_t *centres, size_t n) {
  if (!model || !centres) return fail(-1, "null argument");
  const size_t have = (size_t)model->Ld * 2 * (size_t)model->D;
  if (n != have) return fail(-1, "kv centres: %zu values given, the model takes Ld * 2 * D = %zu", n, have);
  for (size_t i = 0; i < n; ++i)
    if (centres[i] <= -(1 << 24) || centres[i] >= (1 << 24)) return fail(-1, "kv centre %zu = %d not within (-2^24, 2^24)", i, centres[i]);
  HIPCHK(hipSetDevice(model->device));
  //  serialised against translate calls: they read the generation, its state and its buffer under these locks
  std::lock_guard<std::mutex> submit(model->submit_mu);
  std::lock_guard<std::mutex> gate(model->gate_mu);
  const int gen = model->kv_gen.load(std::memory_order_relaxed);
  const bool was_claimed = model->kv_centre_claimed.exchange(true, std::memory_order_acq_rel);
  if (was_claimed && model->kv_centre_state.load(std::memory_order_acquire) != 2 && !kv_centres_ready(model))
    return fail(-1, "kv centres: a calibration batch is in flight");
  // whatever fails below gives the claim back (a claim without centres would keep every batch from calibrating: the form
  // would silently never be used)
  struct Unclaim {
    slimt_hip_model *m;
    bool armed;
    ~Unclaim() {
      if (armed) m->kv_centre_claimed.store(false, std::memory_order_release);
    }
  } unclaim{model, !was_claimed};
  hipError_t e = model->kv_centre[gen].reserve(have * 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // (the caller promises no batch in flight; make the copy safe against a finished one's tail)
  if (e == hipSuccess) e = hipMemcpy(model->kv_centre[gen].p, centres, have * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail((int)e, "kv centres: %s", hipGetErrorString(e));
  unclaim.armed = false;
  model->kv_centre_state.store(2, std::memory_order_release);
  // layers switched off under the centres before, and the counters they were judged by, start over with these
  model->kv_tight_off.store(0, std::memory_order_relaxed);
  for (auto &c : model->kv_tight_submitted) c.store(0, std::memory_order_relaxed);
  if (model->kv_wide_count)
    for (int l = 0; l < 4; ++l) static_cast<volatile unsigned long long *>(model->kv_wide_count)[1 + 4 * gen + l] = 0;
  return 0;
}

extern "C" int slimt_hip_debug_kv_tight_watch(slimt_hip_model *model, unsigned *layers_off, uint64_t *missed, uint64_t *submitted) {
  if (!model) return fail(-1, "model is NULL");
  if (layers_off) *layers_off = model->kv_tight_off.load(std::memory_order_relaxed);
  for (int l = 0; l < 4; ++l) {
    if (missed)
      missed[l] = model->kv_wide_count ? static_cast<volatile unsigned long long *>(
                                              model->kv_wide_count)[1 + 4 * model->kv_gen.load(std::memory_order_relaxed) + l] : 0;
    if (submitted) submitted[l] = model->kv_tight_submitted[l].load(std::memory_order_relaxed);
  }
  return 0;
}

extern "C" int slimt_hip_debug_decoder_plan(slimt_hip_ctx *ctx, int out[6]) {
  if (!ctx || !out) return fail(-1, "null argument");
  for (int i = 0; i < 6; ++i) out[i] = ctx->plan_last[i];
  return 0;
}

extern "C" int slimt_hip_debug_kv_formats(slimt_hip_ctx *ctx, uint8_t *out, size_t n, size_t *batch) {
  if (!ctx || !out || !batch) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(ctx->model->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *batch = 0;
  if (!ctx->kv_fmt_valid) return 0;  // the last batch's caches are all in one form (24-bit or f32)
  const size_t have = (size_t)ctx->model->Ld * (size_t)ctx->kv_fmt_B;
  if (n < have) return fail(-1, "kv formats: %zu bytes for %zu", n, have);
  HIPCHK(hipMemcpy(out, ctx->kv_fmt.p, have, hipMemcpyDeviceToHost));
  *batch = (size_t)ctx->kv_fmt_B;
  return 0;
}

extern "C" int slimt_hip_model_device(const slimt_hip_model *model) { return model ? model->device : -1; }

extern "C" int slimt_hip_model_info(const slimt_hip_model *model, int32_t *dim_emb,
                                    int32_t *dim_ffn, int32_t *vocab, int32_t *heads) {
  if (!model) return fail(-1, "model is NULL");
  if (dim_emb) *dim_emb = model->D;
  if (dim_ffn) *dim_ffn = model->F;
  if (vocab) *vocab = model->V;
  if (heads) *heads = model->H;
  return 0;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
namespace {

// sinusoidal_signal (TensorOps.cc:245-265): host libm, like the reference.
void sinusoid_table(int S, int D, std::vector<float> &out) {
  out.assign((size_t)S * D, 0.f);
  float num_timescales = static_cast<float>(D) / 2;
  // std::log(10000.0F), written as its correctly rounded f32 value so that no
  // compiler's constant folding can differ from another's.
  const float log_10000 = 9.210340371976184f;
  float log_timescale_increment = log_10000 / (num_timescales - 1.0F);
  for (size_t p = 0; p < (size_t)S; ++p) {
    for (int i = 0; i < num_timescales; ++i) {
      float v = p * std::exp(i * -log_timescale_increment);
      size_t offset = p * (size_t)D + (size_t)i;
      out[offset] = std::sin(v);
      out[offset + static_cast<int>(num_timescales)] = std::cos(v);
    }
  }
}

void ctx_free(slimt_hip_ctx *c) {
  DevBuf *bufs[] = {&c->pos, &c->ids, &c->lengths, &c->x0, &c->x1, &c->q, &c->k, &c->v, &c->att,
                    &c->h8, &c->a8, &c->ticket, &c->kv, &c->kv_fmt, &c->cl_act, &c->cl_part, &c->cl_sync, &c->dx, &c->dx_pre, &c->dh, &c->datt8, &c->dout, &c->df8,
                    &c->state, &c->part_val, &c->part_idx, &c->part_sum, &c->sc_stage, &c->fp_stage, &c->fp_scratch, &c->fp_col, &c->fp_part_y, &c->sm_stage, &c->sm_seeds, &c->sm_part_mz, &c->sm_part_zw, &c->tr_logits, &c->prev, &c->out_ids, &c->out_len,
                    &c->finished, &c->n_finished, &c->align, &c->shortlist, &c->logits,
                    &c->attn_dbg, &c->stamps, &c->dbg_embed, &c->dbg_layers, &c->sl_scratch, &c->n_sl_dev, &c->gen_flag,
                    &c->score_ws, &c->score_io, &c->alt_stage, &c->cand_align, &c->cand_rank, &c->fo_stage, &c->cs_stage, &c->bm_state, &c->bm_slots, &c->bm_hist, &c->bm_align, &c->bm_stage};
  for (auto *b : bufs) b->release();
  free_affine(c->out_sl);
  if (c->n_finished_host) (void)hipHostFree(c->n_finished_host);
  for (auto &e : c->prof_events) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  if (c->sync_event) (void)hipEventDestroy(c->sync_event);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
}

int ctx_alloc(slimt_hip_ctx *c) {
  const slimt_hip_model *m = c->model;
  const size_t B = c->max_B, S = c->max_S, M = c->max_M;
  const size_t D = (size_t)m->D, F = (size_t)m->F, V = (size_t)m->V;
  std::vector<float> pos;
  sinusoid_table((int)S, (int)D, pos);
  HIPCHK(c->pos.reserve(pos.size() * 4));
  HIPCHK(hipMemcpy(c->pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(c->ids.reserve(M * 4));
  HIPCHK(c->lengths.reserve(B * 4));
  HIPCHK(c->x0.reserve(M * D * 4));
  HIPCHK(c->x1.reserve(M * D * 4));
  HIPCHK(c->q.reserve(M * D * 4));
  HIPCHK(c->k.reserve(M * D * 4));
  HIPCHK(c->v.reserve(M * D * 4));
  HIPCHK(c->att.reserve(M * D * 4));
  HIPCHK(c->h8.reserve(M * F));
  HIPCHK(c->a8.reserve(M * D));
  HIPCHK(c->ticket.reserve(16));  // [0] decoder, [1] fused encoder, [2..3] XCD-affine claim state (64 bits)
  HIPCHK(hipMemset(c->ticket.p, 0, 16));
  HIPCHK(c->kv.reserve((size_t)m->Ld * 2 * M * D * 4));
  HIPCHK(c->dx.reserve(B * D * 4));
  HIPCHK(c->dx_pre.reserve(B * D * 4));
  HIPCHK(c->dh.reserve(B * D * 4));
  HIPCHK(c->datt8.reserve(B * D));
  HIPCHK(c->dout.reserve(B * D * 4));
  HIPCHK(c->df8.reserve(B * F));
  HIPCHK(c->state.reserve((size_t)m->Ld * B * D * 4));
  const size_t max_parts = (V + 63) / 64;
  HIPCHK(c->part_val.reserve(B * max_parts * 4));
  HIPCHK(c->part_idx.reserve(B * max_parts * 4));
  HIPCHK(c->prev.reserve(B * 4));
  HIPCHK(c->out_len.reserve(B * 4));
  HIPCHK(c->finished.reserve(B));
  HIPCHK(c->n_finished.reserve(16));
  HIPCHK(c->shortlist.reserve(V * 4));
  HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&c->n_finished_host), 16, hipHostMallocDefault));
  std::memset(c->n_finished_host, 0, 16);  // [0] early-exit read-back, [1] size of the last generated shortlist
  return 0;
}

struct ProfScope {  // HIP events around one launch of the selected kernel family
  slimt_hip_ctx *c;
  bool on;
  ProfScope(slimt_hip_ctx *ctx, int family, double macs, double bytes)
      : c(ctx), on(ctx->prof_kernel == family) {
    if (!on) return;
    if (c->prof_used == c->prof_events.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        on = false;
        return;
      }
      c->prof_events.emplace_back(a, b);
    }
    c->prof_macs += macs;
    c->prof_bytes += bytes;
    (void)hipEventRecord(c->prof_events[c->prof_used].first, c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(c->prof_events[c->prof_used].second, c->stream);
    c->prof_used++;
  }
};

double gemm_macs(int M, const PreparedWeight &w) { return (double)M * w.K * w.N; }
double gemm_bytes(const PreparedWeight &w) { return (double)w.K * w.n_tiles * 16; }

}  // namespace

// Contexts alive per device in this process. Every context is a stream, and past ~22 of them the device's
// hardware queues are time-sliced whatever GPU_MAX_HW_QUEUES says: 21 / 22 workers 32.5 / 32.1 M tok/s, 24 workers
// 23.8 M, 32 workers 20.4 M (profiles/archive/r04_v1_budget_workers_sweep.txt). Said once, on stderr, when it happens
// (SLIMT_HIP_QUIET=1: not said); slimt_hip_contexts_on_device reports the count.
static constexpr int kMaxDevices = 64;
static constexpr int kContextCliff = 22;
static std::atomic<int> g_live_ctx[kMaxDevices];

static void count_context(int device, int delta) {
  if (device < 0 || device >= kMaxDevices) return;
  const int now = g_live_ctx[device].fetch_add(delta, std::memory_order_relaxed) + delta;
  if (delta > 0 && now > kContextCliff) {
    static std::atomic<bool> warned{false};
    if (!env().quiet && !warned.exchange(true))
      std::fprintf(stderr,
                   "slimt_hip: %d contexts on device %d in one process: past %d the device's hardware queues are "
                   "time-sliced (24 contexts measured 30 %% below 20); use fewer workers with larger batches, or one "
                   "process per device\n",
                   now, device, kContextCliff);
  }
}

extern "C" int slimt_hip_contexts_on_device(int device, int *count) {
  if (!count) return fail(-1, "null argument");
  if (device < 0 || device >= kMaxDevices) return fail(-1, "device %d out of range", device);
  *count = g_live_ctx[device].load(std::memory_order_relaxed);
  return 0;
}

// Contexts per hardware queue. The runtime gives a new stream a hardware queue of its own while fewer than
// GPU_MAX_HW_QUEUES exist, and afterwards the queue that the fewest streams hold -- the null stream counted like any
// other, although it carries nothing once the model is uploaded, and ties broken the runtime's way. With the default
// four queues the headline's twenty context streams landed 4 / 5 / 5 / 6 (the null stream's queue four, a tie lost on
// another six; tools/queue_ledger.py), and kernels that share a queue run one after the other: the step lasted as long
// as the queue with six, the others ran nothing for 17 % of it. So before a device's first context stream is made,
// every queue but the null stream's is given one stream that stays idle as well: all queues then start level, and
// "the fewest streams" spreads the contexts evenly whichever way ties go (20 contexts: 5 / 5 / 5 / 5). Only where
// sharing is the rule (up to 8 queues: past that a context usually has a queue to itself, and a hardware queue is not
// free). The streams live as long as the process. SLIMT_IDLE_STREAMS=0: none (A/B).
static void level_hardware_queues(int device, int queues) {
  static std::mutex mu;
  static bool done[kMaxDevices];
  static std::vector<hipStream_t> idle;  // (never destroyed: a destroyed one would tilt the queues again)
  if (!env().idle_streams || device < 0 || device >= kMaxDevices || queues < 2 || queues > 8) return;
  std::lock_guard<std::mutex> lock(mu);
  if (done[device]) return;
  done[device] = true;
  if (g_live_ctx[device].load(std::memory_order_relaxed) > 0) return;  // (contexts on streams of the caller's: left alone)
  (void)hipStreamQuery(nullptr);  // the null stream takes its queue first, if it has none yet
  for (int q = 1; q < queues; ++q) {
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();  // (no harm: the contexts spread as they did before)
      return;
    }
    idle.push_back(s);
  }
}

extern "C" int slimt_hip_ctx_create(slimt_hip_model *model, size_t max_batch,
                                    size_t max_source_length, void *stream, slimt_hip_ctx **out) {
  return slimt_hip_ctx_create_budget(model, max_batch, max_source_length,
                                     max_batch * max_source_length, stream, out);
}

extern "C" int slimt_hip_ctx_create_budget(slimt_hip_model *model, size_t max_batch,
                                           size_t max_source_length, size_t max_tokens,
                                           void *stream, slimt_hip_ctx **out) {
  if (!model || !out) return fail(-1, "null argument");
  *out = nullptr;
  if (max_batch == 0 || max_source_length == 0 || max_tokens == 0) return fail(-1, "empty workspace");
  if (max_source_length > 128)
    return fail(-1, "max_source_length %zu > 128 (slimt wraps at 128, Frontend.hh:27)", max_source_length);
  HIPCHK(hipSetDevice(model->device));
  auto *c = new slimt_hip_ctx();
  c->model = model;
  c->max_B = max_batch;
  c->max_S = max_source_length;
  c->max_M = std::min(max_batch * max_source_length, max_tokens);
  if (stream) {
    c->stream = reinterpret_cast<hipStream_t>(stream);
  } else {
    level_hardware_queues(model->device, model->hw_queues);
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      return fail((int)e, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->own_stream = true;
  }
  int rc = ctx_alloc(c);
  if (rc) {
    ctx_free(c);
    delete c;
    return rc;
  }
  count_context(model->device, +1);
  *out = c;
  return 0;
}

extern "C" int slimt_hip_ctx_destroy(slimt_hip_ctx *ctx) {
  if (!ctx) return 0;
  count_context(ctx->model->device, -1);
  (void)hipSetDevice(ctx->model->device);
  (void)hipStreamSynchronize(ctx->stream);
  {
    std::lock_guard<std::mutex> lock(ctx->model->gate_mu);
    auto &v = ctx->model->gate_ctx;
    for (size_t i = 0; i < v.size();)
      if (v[i].ctx == ctx) v.erase(v.begin() + (long)i); else ++i;
  }
  ctx_free(ctx);
  delete ctx;
  return 0;
}

extern "C" int slimt_hip_ctx_stream(slimt_hip_ctx *ctx, void **stream) {
  if (!ctx || !stream) return fail(-1, "null argument");
  *stream = reinterpret_cast<void *>(ctx->stream);
  return 0;
}

extern "C" int slimt_hip_ctx_set_decode_mode(slimt_hip_ctx *ctx, int mode) {
  if (!ctx) return fail(-1, "ctx is NULL");
  if (mode < 0 || mode > 6) return fail(-1, "bad decode mode %d", mode);
  ctx->decode_mode = mode;
  return 0;
}

extern "C" int slimt_hip_ctx_set_scores(slimt_hip_ctx *ctx, float *const *scores, size_t n) {
  if (!ctx) return fail(-1, "null argument");
  if (!scores && n) return fail(-1, "scores is NULL");
  ctx->armed.scores.assign(scores, scores + n);  // (checked by the call that takes them, CallOptions; n = 0: nothing armed)
  return 0;
}

extern "C" int slimt_hip_ctx_set_target_prefix(slimt_hip_ctx *ctx, const uint32_t *const *prefix_ids,
                                               const uint32_t *const *prefix_len, size_t n) {
  if (!ctx) return fail(-1, "null argument");
  if ((!prefix_ids || !prefix_len) && n) return fail(-1, "target prefix arrays are NULL");
  ctx->armed.prefix_ids.assign(prefix_ids, prefix_ids + n);  // (checked by the call that takes them; n = 0: nothing armed)
  ctx->armed.prefix_len.assign(prefix_len, prefix_len + n);
  return 0;
}

extern "C" uint64_t slimt_hip_sampling_key(uint64_t seed, uint64_t index) { return slimt_hip::sm_sentence_key(seed, index); }

extern "C" int slimt_hip_ctx_set_sampling(slimt_hip_ctx *ctx, float temperature, const uint64_t *const *keys, size_t n) {
  // (the value first: a bad temperature is refused whatever else is wrong with the call)
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return fail(-1, "sampling: temperature %g is not finite and > 0", (double)temperature);
  const float inv_T = 1.0f / temperature;
  if (!(inv_T > 0.0f) || !std::isfinite(inv_T)) return fail(-1, "sampling: 1 / temperature %g is not finite and > 0", (double)temperature);
  if (!ctx) return fail(-1, "null argument");
  if (keys)
    ctx->armed.keys.assign(keys, keys + n);  // (the count is checked by the call that takes them; n = 0: nothing armed)
  else
    ctx->armed.keys.assign(n, nullptr);
  ctx->armed.inv_T = inv_T;
  return 0;
}

extern "C" int slimt_hip_ctx_set_sampling_truncation(slimt_hip_ctx *ctx, uint32_t top_k, float top_p) {
  // (the value first, like the temperature)
  if (!(top_p > 0.0f && top_p <= 1.0f)) return fail(-1, "sampling truncation: top_p %g is not in (0, 1]", (double)top_p);
  if (!ctx) return fail(-1, "null argument");
  ctx->armed.top_k = top_k;  // (both off: nothing armed, the call is a plain sampled call)
  ctx->armed.top_p = top_p;
  return 0;
}

extern "C" int slimt_hip_ctx_set_fanout_consensus(slimt_hip_ctx *ctx, int max_order, int beta2, uint32_t *best, double *utility) {
  // (the values first, like the temperature)
  if (max_order == 0 && (best || utility)) return fail(-1, "consensus: max_order 0 disarms and takes no arrays");
  if (max_order < 0 || max_order > SLIMT_HIP_CONSENSUS_MAX_ORDER)
    return fail(-1, "consensus: max_order %d is not in 1..%d", max_order, SLIMT_HIP_CONSENSUS_MAX_ORDER);
  if (max_order && (beta2 < 1 || beta2 > SLIMT_HIP_CONSENSUS_MAX_BETA2))
    return fail(-1, "consensus: beta2 %d is not in 1..%d", beta2, SLIMT_HIP_CONSENSUS_MAX_BETA2);
  if (max_order && (!best || !utility)) return fail(-1, "consensus: best or utility is NULL");
  if (!ctx) return fail(-1, "null argument");
  ctx->armed.cs_order = max_order;  // (0: nothing armed)
  ctx->armed.cs_beta2 = beta2;
  ctx->armed.cs_best = best;
  ctx->armed.cs_util = utility;
  return 0;
}

extern "C" int slimt_hip_ctx_set_score_alternatives(slimt_hip_ctx *ctx, uint32_t k, uint32_t *alt_ids, float *alt_scores,
                                                    uint32_t *rank) {
  // (the value first, like the temperature)
  if (k > SLIMT_HIP_MAX_ALTERNATIVES)
    return fail(-1, "score alternatives: k %u exceeds SLIMT_HIP_MAX_ALTERNATIVES (%d)", k, SLIMT_HIP_MAX_ALTERNATIVES);
  if (!ctx) return fail(-1, "null argument");
  if (k && !alt_ids) return fail(-1, "score alternatives: alt_ids is NULL");
  ctx->alt_next_k = k;  // (k = 0: nothing armed)
  ctx->alt_next_ids = k ? alt_ids : nullptr;
  ctx->alt_next_scores = k ? alt_scores : nullptr;
  ctx->alt_next_rank = k ? rank : nullptr;
  return 0;
}

extern "C" int slimt_hip_ctx_set_encode_rows(slimt_hip_ctx *ctx, int rows) {
  if (!ctx) return fail(-1, "ctx is NULL");
  if (rows != 0 && rows != 32 && rows != 64) return fail(-1, "encoder rows per workgroup %d not in {0, 32, 64}", rows);
  ctx->encode_rows = rows;
  return 0;
}

extern "C" int slimt_hip_ctx_plan(const slimt_hip_ctx *ctx, size_t S, int *encoder_fused,
                                  int *decoder_fused) {
  if (!ctx) return fail(-1, "ctx is NULL");
  const slimt_hip_model *m = ctx->model;
  const bool fused = fused_decoder_allowed(ctx);
  if (encoder_fused)
    *encoder_fused = fused && (fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S) ||
                               long_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S));
  if (decoder_fused) *decoder_fused = fused && fused_decode_supported(m->D, m->F, m->H, m->Ld);
  return 0;
}

// A word of pinned host memory per context that kernels set when one of their bounded waits ran out (a member of a
// logits cluster that never arrived: 2; the in-launch shortlist's publisher never published: 1). Read where the host
// waits for the context's stream; the word is cleared and the call fails -- the batch's results are not to be used.
static unsigned *dev_error_word(slimt_hip_ctx *ctx) { return reinterpret_cast<unsigned *>(ctx->n_finished_host) + 2; }
static unsigned *dev_error_device_view(slimt_hip_ctx *ctx) {
  void *p = nullptr;
  if (!ctx->n_finished_host || hipHostGetDevicePointer(&p, dev_error_word(ctx), 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return static_cast<unsigned *>(p);
}
static int check_dev_error(slimt_hip_ctx *ctx) {
  if (!ctx->n_finished_host) return 0;
  volatile unsigned *w = dev_error_word(ctx);
  const unsigned e = *w;
  if (!e) return 0;
  *w = 0;
  return fail(-1, e == 1 ? "the batch's shortlist was never published inside the encoder launch (bounded wait ran out): results discarded"
                         : "a workgroup of a logits cluster never arrived (bounded wait ran out): results discarded");
}

extern "C" int slimt_hip_ctx_synchronize(slimt_hip_ctx *ctx) {
  if (!ctx) return fail(-1, "ctx is NULL");
  // A blocking-sync event, not hipStreamSynchronize: that one spins, and a host pipeline has one
  // thread per context waiting here for milliseconds -- a dozen spinning threads take the cores
  // the runtime's own threads and the batch builders need (the Service with 8 workers: 11.7 ->
  // 13.3 M tok/s once the waiters sleep).
  HIPCHK(hipSetDevice(ctx->model->device));  // the event is created and recorded on the context's device, whatever the caller's is
  if (!ctx->sync_event) HIPCHK(hipEventCreateWithFlags(&ctx->sync_event, hipEventBlockingSync | hipEventDisableTiming));
  HIPCHK(hipEventRecord(ctx->sync_event, ctx->stream));
  HIPCHK(hipEventSynchronize(ctx->sync_event));
  return check_dev_error(ctx);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
namespace {

EmbedArgs embed_args(const slimt_hip_ctx *c) {
  const slimt_hip_model *m = c->model;
  EmbedArgs e;
  e.wemb = m->wemb.as<int8_t>();
  e.inv_mult = 1 / m->wemb_mult;             // Io.cc:280-281
  e.sqrt_d = std::sqrt(static_cast<float>(m->D));  // Transformer.cc:34
  e.pos = c->pos.as<float>();
  e.D = m->D;
  e.V = m->V;
  return e;
}

// affine on M rows, f32 in -> f32 out
int run_affine_f32(slimt_hip_ctx *c, int family, const AffineW &w, const float *x, int M, float *y,
                   int rows_per_block, int kc_S = 0, int kc_dh = 0, bool raw_acc = false) {
  GemmArgs g;
  g.kc_S = kc_S;
  g.kc_dh = kc_dh;
  g.raw_acc = raw_acc;
  g.x_f32 = x;
  g.lda = w.w.K;
  g.M = M;
  g.w = w.w;
  g.y = y;
  g.ldy = w.w.N;
  ProfScope p(c, family, gemm_macs(M, w.w), gemm_bytes(w.w));
  HIPCHK(launch_gemm(g, EPI_PLAIN, rows_per_block, c->stream));
  return 0;
}

int run_affine_res_ln(slimt_hip_ctx *c, int family, const AffineW &w, const float *x_f32,
                      const int8_t *x_i8, int M, const float *res, const LnW &ln, float *y,
                      int rows_per_block) {
  GemmArgs g;
  g.x_f32 = x_f32;
  g.x_i8 = x_i8;
  g.lda = w.w.K;
  g.M = M;
  g.w = w.w;
  g.y = y;
  g.ldy = w.w.N;
  g.res = res;
  g.ldres = w.w.N;
  g.ln_scale = ln.scale.as<float>();
  g.ln_bias = ln.bias.as<float>();
  g.eps = 1e-6f;  // TensorOps.hh:67-68
  ProfScope p(c, family, gemm_macs(M, w.w), gemm_bytes(w.w));
  HIPCHK(launch_gemm(g, EPI_RES_LN, rows_per_block, c->stream));
  return 0;
}

// affine + residual on M rows (f32 or int8 in) -> f32 pre-LayerNorm sum
int run_affine_res(slimt_hip_ctx *c, int family, const AffineW &w, const float *x_f32,
                   const int8_t *x_i8, int M, const float *res, float *y, int rows_per_block) {
  GemmArgs g;
  g.x_f32 = x_f32;
  g.x_i8 = x_i8;
  g.lda = w.w.K;
  g.M = M;
  g.w = w.w;
  g.y = y;
  g.ldy = w.w.N;
  g.res = res;
  g.ldres = w.w.N;
  ProfScope p(c, family, gemm_macs(M, w.w), gemm_bytes(w.w));
  HIPCHK(launch_gemm(g, EPI_PLAIN, rows_per_block, c->stream));
  return 0;
}

int run_affine_relu_q(slimt_hip_ctx *c, int family, const AffineW &w, const float *x,
                      const int8_t *x_i8, int M, float a_quant_next, int8_t *y8,
                      int rows_per_block) {
  GemmArgs g;
  g.x_f32 = x;
  g.x_i8 = x_i8;
  g.lda = w.w.K;
  g.M = M;
  g.w = w.w;
  g.y_i8 = y8;
  g.ldy8 = w.w.N;
  g.a_quant_out = a_quant_next;
  ProfScope p(c, family, gemm_macs(M, w.w), gemm_bytes(w.w));
  HIPCHK(launch_gemm(g, EPI_RELU_Q, rows_per_block, c->stream));
  return 0;
}

int check_batch(const slimt_hip_ctx *c, size_t B, size_t S) {
  if (B == 0 || S == 0) return fail(-1, "empty batch");
  if (B > c->max_B || S > c->max_S || B * S > c->max_M)
    return fail(-1, "batch %zux%zu exceeds the context workspace %zux%zu (%zu padded tokens)", B, S,
                c->max_B, c->max_S, c->max_M);
  return 0;
}

// Model.cc:195-201: embedding + Encoder::forward. d_ids/d_len already in
// ctx->ids / ctx->lengths. Result in ctx->x0.
// embedded: ctx->x0 already holds the transformed embedding [B,S,D] (Encoder::forward's
// argument, Transformer.cc:57): the stage kernels run from there.
// D = 256: 64-row tiles (encode_tall.hip: the O projection's and the FFN's weights cross the
// CU's L2 path once per 64 rows) from 32 of them on: with other batches in flight they win
// already there (B = 128: 23.3 -> 26.2 M tok/s, B = 64: level), a lone batch of that size pays
// ~0.1 ms of latency; below that twice as many 32-row workgroups (and less padding) are better
bool tall_encoder_chosen(const slimt_hip_ctx *c, int B, int S) {
  const slimt_hip_model *m = c->model;
  const bool tall_mid = S > 32 && c->encode_rows != 32 && tall_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S);
  if (c->decode_mode == 1 || !(tall_mid || fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S))) return false;
  return tall_mid || (tall_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S) &&
                      (c->encode_rows == 64 || (c->encode_rows == 0 && tall_encode_grid(B, S, false) >= 32)));
}

// the encoders with a writer for the tight K/V form: every fused one for S <= 32 (64- and 32-row tiles at D = 256, the D = 512
// one), the 64-row one with a sentence of 33..64 tokens per workgroup, the per-sentence one for 65..128 tokens
static bool kv_tight_writer(const slimt_hip_ctx *c, int B, int S) {
  const slimt_hip_model *m = c->model;
  if (S > 64) return c->decode_mode != 1 && long_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S);
  if (S > 32) return tall_encoder_chosen(c, B, S);
  return c->decode_mode != 1 && fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S);
}

// embedding + every encoder layer + the decoder's K/V cache in one launch of encode_tall / encode_fused / encode_wide
bool fused_encoder_chosen(const slimt_hip_ctx *c, int B, int S) {
  (void)B;
  const slimt_hip_model *m = c->model;
  const bool tall_mid = S > 32 && c->encode_rows != 32 && tall_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S);
  return c->decode_mode != 1 && (tall_mid || fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S));
}

// One merged launch pair (kernels.h, MergeIn / MergeOut / MergePack): the sub-batches' tables as the kernels take them, and
// the packing jobs of the launch -- one per distinct shortlist, their buffers job strides apart in ctx->out_sl.
struct MergePlan {
  int n = 0;
  MergeIn in[kMaxMerge];
  MergeOut out[kMaxMerge];
  int n_jobs = 0;
  MergePack jobs[kMaxMerge];
  int max_N = 0;  // columns of the widest job
  size_t stride_wp = 0, stride_cs = 0, stride_pb = 0;
  bool dense = false;  // one output layer for all sub-batches: no holes between them (kernels.h, FusedDecodeArgs::sub_dense)
  BatchOptions opt[kMaxMerge];  // sub-batch j's options as the kernels address them (FusedDecodeArgs::sub_scores / sub_prefix_* / sub_keys)
};

// What a translate entry point opens with. Whatever the slimt_hip_ctx_set_* functions armed on the context is moved out of
// ctx->armed here -- consumed whether or not the call then succeeds -- checked against the call's n batches, and becomes
// ctx->call, the record every inner function reads; `user` holds the per-batch arrays as the caller gave them, one entry per
// batch, for the entry point to hand on: as they are where they are device memory (options_in_place), through
// stage_options where they are host memory. The checks run scores -> prefix -> sampling -> truncation -> consensus and the
// first refusal is the call's (rc); a truncated call must be sampled, so the truncation is looked at behind the sampling.
// While call.truncated or call.fanout is set fused_decoder_allowed() is false: the call decodes with the per-stage kernels
// and is never merged; the context's decode mode is not touched and still chooses the encoder. Consensus is for the
// fan-out entry points (fanout) only: any other call that finds it armed is refused. The destructor empties ctx->call.
// The score entry points (slimt_hip_score*) open no CallOptions: they neither read nor consume what was armed.
struct CallOptions {
  slimt_hip_ctx *c;
  std::vector<BatchOptions> user;
  int rc = 0;
  CallOptions(slimt_hip_ctx *ctx, size_t n, bool fanout = false) : c(ctx), user(n) {
    if (!c) return;
    const ArmedOptions a = std::move(c->armed);
    c->armed = {};
    c->call = {};
    rc = take(a, n, fanout);
    if (rc) c->call = {};
  }
  ~CallOptions() {
    if (c) c->call = {};
  }
  // A fan-out call (slimt_hip_translate_fanout*): N decoder rows over the call's B sources, opened behind the options, whose
  // arrays then count N rows; decoder_rows() is N from here on. N is bounded by max_batch, which sizes the per-row workspaces.
  int open_fanout(size_t N) {
    if (!c) return 0;
    if (N == 0) return fail(-1, "fan-out: no rows (N = 0)");
    if (N > c->max_B) return fail(-1, "fan-out: %zu rows exceed the context's max_batch %zu", N, c->max_B);
    c->call.fanout = true;
    c->call.rows = (int)N;
    return 0;
  }
  // A beam call (slimt_hip_translate_beam*): a fan-out call of B beam rows, source-major, row_src[r] = r / beam. It keeps
  // its own token scores and selects by them: whatever else was armed is a refusal (and consumed, as always).
  int open_beam(size_t B, int beam, int mode) {
    if (!c) return 0;
    const CallState &call = c->call;
    if (call.scored) return fail(-1, "beam: scores are armed (slimt_hip_ctx_set_scores); a beam call returns its own token scores");
    if (call.forced) return fail(-1, "beam: a target prefix is armed (slimt_hip_ctx_set_target_prefix); prefix-constrained beams are not supported");
    if (call.sampled) return fail(-1, "beam: sampling is armed (slimt_hip_ctx_set_sampling); a beam call is not sampled");
    if (B * (size_t)beam > c->max_B)
      return fail(-1, "beam: %zu sources of beam %d exceed the context's max_batch %zu", B, beam, c->max_B);
    if (B == 0) return fail(-1, "empty batch");
    RCCHK(open_fanout(B * (size_t)beam));
    c->call.beam = beam;
    c->call.beam_mode = mode;
    c->bm_row_src.resize(B * (size_t)beam);
    for (size_t r = 0; r < c->bm_row_src.size(); ++r) c->bm_row_src[r] = (uint32_t)(r / (size_t)beam);
    return 0;
  }

 private:
  int take(const ArmedOptions &a, size_t n, bool fanout) {
    CallState &call = c->call;
    if (!a.scores.empty()) {
      if (a.scores.size() != n) return fail(-1, "scores: %zu destinations armed, the call has %zu batches", a.scores.size(), n);
      for (size_t j = 0; j < n; ++j) {
        if (!a.scores[j]) return fail(-1, "scores: destination %zu is NULL", j);
        user[j].scores = a.scores[j];
      }
      call.scored = true;
    }
    if (!a.prefix_ids.empty()) {
      if (a.prefix_ids.size() != n) return fail(-1, "target prefix: %zu batches armed, the call has %zu", a.prefix_ids.size(), n);
      for (size_t j = 0; j < n; ++j) {
        if (!a.prefix_ids[j] || !a.prefix_len[j]) return fail(-1, "target prefix: batch %zu has a NULL array", j);
        user[j].prefix_ids = a.prefix_ids[j];
        user[j].prefix_len = a.prefix_len[j];
      }
      call.forced = true;
    }
    if (!a.keys.empty()) {  // (keys[j] may be NULL: batch j's keys are its row indices)
      if (a.keys.size() != n) return fail(-1, "sampling: %zu batches armed, the call has %zu", a.keys.size(), n);
      for (size_t j = 0; j < n; ++j) user[j].keys = a.keys[j];
      call.sampled = true;
      call.inv_T = a.inv_T;
    }
    if (a.top_k != 0 || a.top_p != 1.0f) {
      if (!call.sampled) return fail(-1, "sampling truncation: armed without sampling (slimt_hip_ctx_set_sampling)");
      call.truncated = true;
      call.top_k = a.top_k;
      call.top_p = a.top_p;
    }
    if (a.cs_order > 0) {
      if (!fanout) return fail(-1, "consensus: armed on a translate call that is not a fan-out call (slimt_hip_translate_fanout*)");
      call.consensus = true;
      call.cs_order = a.cs_order;
      call.cs_beta2 = a.cs_beta2;
      call.cs_best = a.cs_best;
      call.cs_util = a.cs_util;
    }
    return 0;
  }
};

// A batch whose options are device memory (the _device entry points): the kernels address them where they are.
void options_in_place(slimt_hip_ctx *c, const BatchOptions &user) { c->call.dev = user; }

// the device view of a pinned host allocation (hipHostMalloc / slimt_hip_host_alloc), else nullptr
void *host_device_view(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}

// A host prefix of B sentences with rows Tmax apart: every length <= Tmax, every id of the prefix < V.
int prefix_check(const slimt_hip_ctx *c, const uint32_t *ids, const uint32_t *len, size_t B, size_t Tmax) {
  for (size_t b = 0; b < B; ++b) {
    if (len[b] > Tmax) return fail(-1, "target prefix: length %u of sentence %zu > Tmax %zu", len[b], b, Tmax);
    for (size_t t = 0; t < len[b]; ++t)
      if (ids[b * Tmax + t] >= (uint32_t)c->model->V)
        return fail(-1, "target prefix: id %u of sentence %zu out of range", ids[b * Tmax + t], b);
  }
  return 0;
}

// Host prefixes and keys -> addresses the kernels read: n batches' user[j] of rows[j] rows with prefix rows Tmax[j] apart, to
// dev[j].prefix_* / dev[j].keys (dev[j].scores is not touched: a host call's scores have a copy-back, translate_host). Pinned
// arrays (hipHostMalloc / slimt_hip_host_alloc) are read in place, like the pinned inputs of the asynchronous calls
// (translate_host: no copy queued behind other streams' kernels); a pageable batch's prefix (ids, then lengths) and keys
// are staged in device memory with one asynchronous copy each on the context's stream; NULL keys stay NULL. Every prefix is
// checked first: nothing is queued for an invalid one.
int stage_options(slimt_hip_ctx *c, size_t n, const BatchOptions *user, const size_t *rows, const size_t *Tmax, BatchOptions *dev) {
  for (size_t j = 0; j < n; ++j)
    if (user[j].prefix_ids) RCCHK(prefix_check(c, user[j].prefix_ids, user[j].prefix_len, rows[j], Tmax[j]));
  size_t fp_words = 0, sm_words = 0;
  for (size_t j = 0; j < n; ++j) {
    const BatchOptions &u = user[j];
    BatchOptions &d = dev[j];
    d.prefix_ids = u.prefix_ids ? static_cast<const uint32_t *>(host_device_view(u.prefix_ids)) : nullptr;
    d.prefix_len = u.prefix_ids ? static_cast<const uint32_t *>(host_device_view(u.prefix_len)) : nullptr;
    if (!d.prefix_ids || !d.prefix_len) d.prefix_ids = d.prefix_len = nullptr;  // (both in place, or both staged)
    d.keys = u.keys ? static_cast<const uint64_t *>(host_device_view(u.keys)) : nullptr;
    if (u.prefix_ids && !d.prefix_ids) fp_words += rows[j] * Tmax[j] + rows[j];
    if (u.keys && !d.keys) sm_words += rows[j];
  }
  if (fp_words) HIPCHK(c->fp_stage.reserve(fp_words * 4));
  if (sm_words) HIPCHK(c->sm_stage.reserve(sm_words * 8));
  uint32_t *p = c->fp_stage.as<uint32_t>();
  uint64_t *q = c->sm_stage.as<uint64_t>();
  for (size_t j = 0; j < n; ++j) {
    const BatchOptions &u = user[j];
    BatchOptions &d = dev[j];
    const size_t ids = rows[j] * Tmax[j];
    if (u.prefix_ids && !d.prefix_ids) {
      HIPCHK(hipMemcpyAsync(p, u.prefix_ids, ids * 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(p + ids, u.prefix_len, rows[j] * 4, hipMemcpyHostToDevice, c->stream));
      d.prefix_ids = p;
      d.prefix_len = p + ids;
      p += ids + rows[j];
    }
    if (u.keys && !d.keys) {
      HIPCHK(hipMemcpyAsync(q, u.keys, rows[j] * 8, hipMemcpyHostToDevice, c->stream));
      d.keys = q;
      q += rows[j];
    }
  }
  return 0;
}

// ... for the batches of a host _many_ call (n <= kMaxMerge): batch j of B_j sentences padded to S_j tokens
int stage_options(slimt_hip_ctx *c, const slimt_hip_batch *batches, size_t n, size_t S, float limit_factor, const BatchOptions *user,
                  BatchOptions *dev) {
  size_t rows[kMaxMerge], Tmax[kMaxMerge];
  for (size_t j = 0; j < n; ++j) {
    rows[j] = batches[j].B;
    Tmax[j] = std::max<size_t>(1, (size_t)(limit_factor * (float)(batches[j].S ? batches[j].S : S)));
  }
  return stage_options(c, n, user, rows, Tmax, dev);
}

// every encoder layer's weights, and the decoder layers' K / V projections the persistent encoders cache
void fill_encoder_layers(const slimt_hip_model *m, FusedEncodeArgs &f) {
  for (int l = 0; l < m->Le; ++l) {
    const EncLayerW &L = m->enc[(size_t)l];
    FusedEncLayerW &fl = f.L[l];
    fl.q = L.attn.q.w; fl.k = L.attn.k.w; fl.v = L.attn.v.w; fl.o = L.attn.o.w;
    fl.ffn1 = L.ffn1.w; fl.ffn2 = L.ffn2.w;
    fl.attn_ln_s = L.attn.ln.scale.as<float>(); fl.attn_ln_b = L.attn.ln.bias.as<float>();
    fl.ffn_ln_s = L.ffn_ln.scale.as<float>(); fl.ffn_ln_b = L.ffn_ln.bias.as<float>();
  }
  for (int l = 0; l < m->Ld; ++l) {
    f.dec_k[l] = m->dec[(size_t)l].attn.k.w;
    f.dec_v[l] = m->dec[(size_t)l].attn.v.w;
  }
}

// The narrow (20-bit) form of a batch's packed cache where `narrow` allows it (launch_choice.h, kv_narrow_shape, behind a
// kv24 launch) and the model's watch still wants it -- the forms are then recorded in ctx->kv_fmt -- and below it the tight
// (16-bit) form for the decoder layers that try it. The watches' counters (kv_layers_submitted, kv_tight_submitted) take
// this batch here, once, before its launch.
int arm_kv_forms(slimt_hip_ctx *c, FusedEncodeArgs &f, int B, int S, bool narrow) {
  const slimt_hip_model *m = c->model;
  c->kv_fmt_valid = narrow && kv_narrow_wanted(c->model, &f.kv_wide_count);
#ifdef SLIMT_EXP_NO_KV20  // A/B builds: the 24-bit form only
  c->kv_fmt_valid = false;
#endif
  if (!c->kv_fmt_valid) return 0;
  HIPCHK(c->kv_fmt.reserve((size_t)m->Ld * c->max_B));
  f.kv_fmt = c->kv_fmt.as<unsigned char>();
  f.kv_narrow_limit = std::min(m->kv_narrow_limit, 1 << 19);
  c->kv_fmt_B = B;
  c->model->kv_layers_submitted.fetch_add((unsigned long long)B * m->Ld, std::memory_order_relaxed);
  f.kv_tight_layers = kv_tight_wanted(c, S, kv_tight_writer(c, B, S), &f.kv_not16_count);
  if (f.kv_tight_layers) {
    f.kv_tight_limit = std::min(m->kv_tight_limit, 1 << 15);
    for (int l = 0; l < m->Ld; ++l)
      for (int p = 0; p < 2; ++p) f.kv_centre[l][p] = m->kv_centre_of(c->kv_gen, l, p);
    c->kv_tight = true;
    for (int l = 0; l < m->Ld; ++l)
      if ((f.kv_tight_layers >> l) & 1u) c->model->kv_tight_submitted[l].fetch_add((unsigned long long)B, std::memory_order_relaxed);
  }
  return 0;
}

// gen (nullable; only where fused_encoder_chosen): the batch's shortlist is generated inside the encoder launch
// (kernels.h, FusedEncodeArgs::gen) -- its ids / count are pack->idx / pack->n_dev.
int encode_device(slimt_hip_ctx *c, int B, int S, float *h_embed, float *h_layers,
                  const uint32_t *d_ids = nullptr, const uint32_t *d_lengths = nullptr,
                  const PackArgs *pack = nullptr, bool embedded = false, bool keep_out = true,
                  bool kv24 = false, const ShortlistArgs *gen = nullptr, bool kv_store_nt = false,
                  const MergePlan *mp = nullptr) {
  // kv24 (translate_device only: the caller decodes with the persistent kernel's packed-cache
  // variant right behind this launch): the fused encoder leaves the 24-bit K/V cache
  // keep_out = false (the translate path): the persistent encoder leaves the decoder its K/V
  // cache only -- the encoder output itself (B S D f32, 8 MB at the headline size) is not written
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  const int M = B * S, D = m->D;
  const size_t nbytes = (size_t)M * D * 4;
  c->kv_fmt_valid = false;  // set by arm_kv_forms, where a persistent encoder records the forms of a packed cache
  c->kv_tight = false;
  c->B = B;
  c->S = S;
  c->have_encoder_out = false;
  c->decode_ready = false;
  c->kv_ready = false;
  // sentences of 33..64 tokens: the 64-row D = 256 encoder takes one per workgroup (else the
  // per-sentence kernel below)
  const bool tall_mid = S > 32 && c->encode_rows != 32 && tall_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S);
  if (!embedded && c->decode_mode != 1 && (tall_mid || fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S))) {
    // embedding + every encoder layer + the decoder's K/V cache in one launch
    FusedEncodeArgs f;
    f.B = B; f.S = S; f.Le = m->Le; f.Ld = m->Ld;
    fill_encoder_layers(m, f);
    f.emb = embed_args(c);
    f.ids = d_ids ? d_ids : c->ids.as<uint32_t>();
    f.lengths = d_lengths ? d_lengths : c->lengths.as<uint32_t>();
    f.alpha = 1.0f / std::sqrt(static_cast<float>(m->D / m->H));
    f.kv = c->kv.as<float>();
    f.kv24 = kv24;
    f.kv_store_nt = kv_store_nt;
    if (kv24 && (size_t)M * D * 3 >= (1u << 31)) return fail(-1, "packed K/V cache: %d rows exceed a 2 GB plane", M);
    // the narrow (20-bit) form where the writer and the reader have it -- D = 256 or 512, S <= 32 -- and where a
    // sentence's V block (groups of eight keys) fits the slot of its 24-bit form (groups of four): not S = 1..4, 9..12
    // (... and S = 33..64 at D = 256: the 64-row encoder with one sentence per workgroup, attention_packed64 with Form20)
    RCCHK(arm_kv_forms(c, f, B, S, kv24 && kv_narrow_shape(D, S, /*long_encoder=*/false)));
    f.enc_out = keep_out ? c->x0.as<float>() : nullptr;
    if (pack) {
      f.pack = *pack;
      f.pack_tiles = (pack->N + 15) / 16;
    }
    if (mp) {  // a merged launch: the sub-batches' inputs, and one packing job per distinct shortlist
      f.n_sub = mp->n;
      for (int j = 0; j < mp->n; ++j) f.sub[j] = mp->in[j];
      if (pack) {
        f.n_pack = mp->n_jobs;
        for (int j = 0; j < mp->n_jobs; ++j) f.pjob[j] = mp->jobs[j];
        f.pack_tiles = (mp->max_N + 15) / 16;
        f.pack_stride_wp = mp->stride_wp;
        f.pack_stride_cs = mp->stride_cs;
        f.pack_stride_pb = mp->stride_pb;
      }
    }
    if (h_embed) {
      HIPCHK(c->dbg_embed.reserve(nbytes));
      f.embed_out = c->dbg_embed.as<float>();
    }
    if (h_layers) {
      HIPCHK(c->dbg_layers.reserve(nbytes * (size_t)m->Le));
      f.layer_out = c->dbg_layers.as<float>();
    }
    f.trace = g_occ_trace;
    if (c->stamp_step >= 0 && c->stamps.p) {  // encoder stamps live in slots 48..55
      f.stamps = c->stamps.as<unsigned long long>() + 48;
      f.stamp_layer = c->stamp_step < m->Le ? c->stamp_step : m->Le - 1;
    }
    f.ticket = c->ticket.as<unsigned>() + 1;  // over-subscribed launch, tiles claimed by ticket
    f.ticket_base = c->enc_ticket_base;
    const bool tall = tall_encoder_chosen(c, B, S);
    if (gen) {
      if (!pack) return fail(-1, "in-launch shortlist generation needs a packing job");
      HIPCHK(c->gen_flag.reserve(64));
      if (c->gen_epoch == 0) HIPCHK(hipMemsetAsync(c->gen_flag.p, 0, 64, st));
      f.gen = *gen;
      f.gen_flag = c->gen_flag.as<unsigned>();
      f.gen_epoch = ++c->gen_epoch;
      f.dev_error = dev_error_device_view(c);
      f.gen_spin_limit = c->gen_spin_limit;
      if (c->gen_break) f.gen_wait_xor = 0x40000000u;  // (debug: the waiters look for an epoch nobody publishes)
      if (c->gen_epoch == 0xffffffffu) c->gen_epoch = 0;  // (the flag is cleared again before epoch 1 is reused)
    }
    {
      const double macs = (double)M * (m->Le * (4.0 * D * D + 2.0 * D * m->F) + m->Ld * 2.0 * D * D);
      ProfScope p(c, SLIMT_HIP_K_ENCODE_FUSED, macs, 0);
      if (tall)
        HIPCHK(launch_encode_tall(f, m->F, st));
      else
        HIPCHK(launch_encode_fused(f, m->D, m->F, m->H, st));
    }
    c->enc_ticket_base += (unsigned)(tall ? tall_encode_grid(B, S, true) : fused_encode_grid(B, S, true));
    if (h_embed) HIPCHK(hipMemcpyAsync(h_embed, c->dbg_embed.p, nbytes, hipMemcpyDeviceToHost, st));
    if (h_layers)
      HIPCHK(hipMemcpyAsync(h_layers, c->dbg_layers.p, nbytes * (size_t)m->Le, hipMemcpyDeviceToHost, st));
    c->have_encoder_out = keep_out;
    c->kv_ready = !kv24;  // the step-wise decoder reads the f32 form only
    return 0;
  }
  if (mp) return fail(-1, "merged launch: no persistent encoder for this shape");
  if (!embedded && c->decode_mode != 1 && long_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, S)) {
    // 32 < S <= 128: one persistent workgroup per sentence (kernels.hip, encode_long_kernel)
    LongEncodeArgs a;
    FusedEncodeArgs &f = a.f;
    f.B = B; f.S = S; f.Le = m->Le; f.Ld = m->Ld;
    fill_encoder_layers(m, f);
    f.emb = embed_args(c);
    f.ids = d_ids ? d_ids : c->ids.as<uint32_t>();
    f.lengths = d_lengths ? d_lengths : c->lengths.as<uint32_t>();
    f.alpha = 1.0f / std::sqrt(static_cast<float>(m->D / m->H));
    f.kv = c->kv.as<float>();
    f.kv24 = kv24;
    // (the narrow form of the packed cache: the first path above has the note; here every S up to 128)
    RCCHK(arm_kv_forms(c, f, B, S, kv24 && kv_narrow_shape(D, S, /*long_encoder=*/true)));
    f.enc_out = c->x0.as<float>();
    if (pack) {
      f.pack = *pack;
      f.pack_tiles = (pack->N + 15) / 16;
    }
    if (h_embed) {
      HIPCHK(c->dbg_embed.reserve(nbytes));
      f.embed_out = c->dbg_embed.as<float>();
    }
    if (h_layers) {
      HIPCHK(c->dbg_layers.reserve(nbytes * (size_t)m->Le));
      f.layer_out = c->dbg_layers.as<float>();
    }
    a.H = m->H; a.D = m->D; a.F = m->F;
    a.x = c->x0.as<float>(); a.y = c->x1.as<float>();
    a.q = c->q.as<float>(); a.k = c->k.as<float>(); a.v = c->v.as<float>();
    a.att = c->att.as<float>();
    a.h8 = c->h8.as<int8_t>();
    {
      const double macs = (double)M * (m->Le * (4.0 * D * D + 2.0 * D * m->F) + m->Ld * 2.0 * D * D);
      ProfScope p(c, SLIMT_HIP_K_ENCODE_FUSED, macs, 0);
      HIPCHK(launch_encode_long(a, st));
    }
    if (h_embed) HIPCHK(hipMemcpyAsync(h_embed, c->dbg_embed.p, nbytes, hipMemcpyDeviceToHost, st));
    if (h_layers)
      HIPCHK(hipMemcpyAsync(h_layers, c->dbg_layers.p, nbytes * (size_t)m->Le, hipMemcpyDeviceToHost, st));
    c->have_encoder_out = true;
    c->kv_ready = !kv24;  // the step-wise decoder reads the f32 form only
    return 0;
  }
  float *x = c->x0.as<float>(), *y = c->x1.as<float>();
  if (!embedded) HIPCHK(launch_embed_encoder(embed_args(c), c->ids.as<uint32_t>(), B, S, x, st));
  if (h_embed) HIPCHK(hipMemcpyAsync(h_embed, x, nbytes, hipMemcpyDeviceToHost, st));
  const int rpb = M >= 2048 ? 64 : (M >= 512 ? 32 : 16);
  const int rpb_ln = M >= 4096 ? 32 : 16;
  // measured at M = 8192, K = N = 512 (base): 64-row blocks 20.9 us, 32-row blocks
  // 14.5 us (twice the blocks in flight); FFN1 (N = 2048) prefers 64 rows
  const int rpb_n = M >= 2048 ? 32 : rpb;
  const bool big = M >= 2048 && (D == 64 || D == 128 || D == 256 || D == 512);
  for (int l = 0; l < m->Le; ++l) {
    const EncLayerW &L = m->enc[(size_t)l];
    // Attention::forward (Modules.cc:287-319)
    RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_ENC, L.attn.q, x, M, c->q.as<float>(), rpb_n));
    RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_ENC, L.attn.k, x, M, c->k.as<float>(), rpb_n));
    RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_ENC, L.attn.v, x, M, c->v.as<float>(), rpb_n));
    AttnArgs a;
    a.q = c->q.as<float>(); a.k = c->k.as<float>(); a.v = c->v.as<float>();
    a.ldq = a.ldk = a.ldv = a.ldo = D;
    a.lengths = c->lengths.as<uint32_t>();
    a.B = B; a.H = m->H; a.Tq = S; a.S = S; a.dh = D / m->H;
    a.alpha = 1.0f / std::sqrt(static_cast<float>(a.dh));
    a.out = c->att.as<float>();
    {
      ProfScope p(c, SLIMT_HIP_K_ATTN_ENC, 0, 0);
      HIPCHK(launch_attention(a, st));
    }
    if (big) {
      // many rows: residual sums from narrow GEMM blocks (no block has to own whole
      // rows), LayerNorm as a pass of its own that also writes FFN1's int8 operand
      RCCHK(run_affine_res(c, SLIMT_HIP_K_GEMM_ENC, L.attn.o, c->att.as<float>(), nullptr, M, x, y, rpb_n));
      HIPCHK(launch_layer_norm_q(y, L.attn.ln.scale.as<float>(), L.attn.ln.bias.as<float>(), 1e-6f, M, D,
                                 y, c->a8.as<int8_t>(), L.ffn1.w.a_quant, st));
      RCCHK(run_affine_relu_q(c, SLIMT_HIP_K_GEMM_ENC, L.ffn1, nullptr, c->a8.as<int8_t>(), M,
                              L.ffn2.w.a_quant, c->h8.as<int8_t>(), rpb));
      RCCHK(run_affine_res(c, SLIMT_HIP_K_GEMM_ENC, L.ffn2, nullptr, c->h8.as<int8_t>(), M, y, x, rpb_n));
      HIPCHK(launch_layer_norm_q(x, L.ffn_ln.scale.as<float>(), L.ffn_ln.bias.as<float>(), 1e-6f, M, D, x,
                                 nullptr, 0.0f, st));
    } else {
      RCCHK(run_affine_res_ln(c, SLIMT_HIP_K_GEMM_ENC, L.attn.o, c->att.as<float>(), nullptr, M, x,
                              L.attn.ln, y, rpb_ln));
      // FFN (Modules.cc:326-331): y -> x
      RCCHK(run_affine_relu_q(c, SLIMT_HIP_K_GEMM_ENC, L.ffn1, y, nullptr, M, L.ffn2.w.a_quant,
                              c->h8.as<int8_t>(), rpb));
      RCCHK(run_affine_res_ln(c, SLIMT_HIP_K_GEMM_ENC, L.ffn2, nullptr, c->h8.as<int8_t>(), M, y,
                              L.ffn_ln, x, rpb_ln));
    }
    if (h_layers)
      HIPCHK(hipMemcpyAsync(h_layers + (size_t)l * M * D, x, nbytes, hipMemcpyDeviceToHost, st));
  }
  c->have_encoder_out = true;
  return 0;
}

// per-batch decoder setup: cross-attention K/V of the encoder output (computed
// ONCE instead of every step, Modules.cc:248), shortlist gather, start states
// (Transformer.cc:78-85).
int decode_setup(slimt_hip_ctx *c, size_t n_sl) {
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  const int B = c->B, S = c->S, M = B * S, D = m->D;
  if (!c->have_encoder_out) return fail(-1, "decode before encode");
  const int rpb = M >= 512 ? 32 : 16;
  float *kv = c->kv.as<float>();
  for (int l = 0; l < m->Ld && !c->kv_ready; ++l) {
    const DecLayerW &L = m->dec[(size_t)l];
    // K in the coalescing-friendly cache layout [sentence][head][d/4][key][4]; both as float(accS): the
    // attention applies the projections' u and pb after its sums (kernels.h, kv24)
    RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_ENC, L.attn.k, c->x0.as<float>(), M,
                         kv + (size_t)(2 * l) * M * D, rpb, S, D / m->H, true));
    RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_ENC, L.attn.v, c->x0.as<float>(), M,
                         kv + (size_t)(2 * l + 1) * M * D, rpb, 0, 0, true));
  }
  c->n_sl = (int)n_sl;
  if (n_sl) {
    // affine_with_select's SelectColumnsB + bias gather (Intgemm.inl.cc:48-69),
    // hoisted out of the step loop: the shortlist is fixed per batch (Model.cc:117-120)
    RCCHK(prepare_affine(c->out_sl, m->out_raw.as<int8_t>(), D, (int)n_sl,
                         c->shortlist.as<uint32_t>(), m->out_bias.as<float>(), m->out_a_quant,
                         m->wemb_mult, st));
  }
  HIPCHK(hipMemsetAsync(c->state.p, 0, (size_t)m->Ld * decoder_rows(c) * D * 4, st));  // (one state per decoder row)
  c->decode_ready = true;
  return 0;
}

const AffineW &output_layer(const slimt_hip_ctx *c) {
  return c->n_sl ? c->out_sl : c->model->out_full;
}

// The last decoder LayerNorm is applied by the consumer of ctx->dx_pre (the
// logits GEMM, or the next layer's SSRU): rows of the final decoder state.
RowSrc decoder_out_rows(const slimt_hip_ctx *c) {
  const DecLayerW &L = c->model->dec.back();
  RowSrc r;
  r.x = c->dx_pre.as<float>();
  r.ln_scale = L.ffn_ln.scale.as<float>();
  r.ln_bias = L.ffn_ln.bias.as<float>();
  return r;
}

// DecoderLayer::forward x Ld (Modules.cc:237-259). Input: the step's target
// embedding in ctx->dx; output: pre-LayerNorm rows in ctx->dx_pre.
int decoder_layers(slimt_hip_ctx *c, float *d_align, int Tmax, const uint32_t *d_out_len,
                   float *d_attn_dbg) {
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  // B sources, N decoder rows (N = B but in a fan-out call): the K / V planes are M = B S positions apart and, with the
  // lengths, indexed by the source -- in the cross-attention only; everything else is row-wise
  const int B = c->B, N = decoder_rows(c), S = c->S, M = B * S, D = m->D;
  float *kv = c->kv.as<float>();
  for (int l = 0; l < m->Ld; ++l) {
    const DecLayerW &L = m->dec[(size_t)l];
    // layer input rows: embedding (layer 0) or LN(previous layer's pre-LN rows)
    RowSrc xin;
    if (l == 0) {
      xin.x = c->dx.as<float>();
    } else {
      const DecLayerW &P = m->dec[(size_t)l - 1];
      xin.x = c->dx_pre.as<float>();
      xin.ln_scale = P.ffn_ln.scale.as<float>();
      xin.ln_bias = P.ffn_ln.bias.as<float>();
    }
    DSsruArgs s;
    s.B = N; s.D = D;
    s.x = xin;
    s.wf = L.rnn_f.w; s.w = L.rnn_w.w;
    s.state = (c->call.bm_state_cur ? c->call.bm_state_cur : c->state.as<float>()) + (size_t)l * N * D;  // (a beam call: the step's block)
    s.h_pre = c->dh.as<float>();
    {
      ProfScope p(c, SLIMT_HIP_K_SSRU, 2.0 * N * D * D, 2.0 * D * D);
      HIPCHK(launch_dssru(s, st));
    }
    RowSrc h;  // LN(x + relu(c')), Modules.cc:230
    h.x = c->dh.as<float>();
    h.ln_scale = L.rnn_ln.scale.as<float>();
    h.ln_bias = L.rnn_ln.bias.as<float>();
    // Attention::forward (Modules.cc:287-319): Q projection + SDPA over the cached K/V
    DQAttnArgs a;
    a.B = B; a.D = D; a.H = m->H; a.S = S;
    a.x = h;
    a.wq = L.attn.q.w;
    a.k = kv + (size_t)(2 * l) * M * D;
    a.v = kv + (size_t)(2 * l + 1) * M * D;
    a.ldv = D;
    a.uk = L.attn.k.w.u;
    a.uv = L.attn.v.w.u;
    a.pbk = L.attn.k.w.pb;
    a.pbv = L.attn.v.w.pb;
    a.lengths = c->lengths.as<uint32_t>();
    a.alpha = 1.0f / std::sqrt(static_cast<float>(D / m->H));
    a.literal = m->kv_format == 3;
    a.out_i8 = c->datt8.as<int8_t>();
    a.a_quant_out = L.attn.o.w.a_quant;
    if (l + 1 == m->Ld) {  // alignment = last layer (Transformer.cc:165-174)
      a.attn = d_attn_dbg;
      if (d_align) {
        a.align = d_align;
        a.out_len = d_out_len;
        a.finished = c->finished.as<uint8_t>();
        a.Tmax = Tmax;
      }
    }
    {
      ProfScope p(c, SLIMT_HIP_K_ATTN_DEC, (double)N * D * D, (double)D * D);
      if (c->call.fanout) {  // rows that share sources: a source's K / V staged once per run of its rows (decode_fanout.hip)
        a.rows = N;
        a.row_src = c->call.row_src;
        HIPCHK(launch_dqattn_fanout(a, st));
      } else {
        HIPCHK(launch_dqattn(a, st));
      }
    }
    // O projection + residual h (Modules.cc:308-314) -> pre-LN rows
    DGemmArgs o;
    o.B = N; o.D = D;
    o.a_i8 = c->datt8.as<int8_t>();
    o.w = L.attn.o.w;
    o.res = h;
    o.y = c->dout.as<float>();
    o.ldy = D;
    {
      ProfScope p(c, SLIMT_HIP_K_GEMM_DEC, gemm_macs(N, o.w), gemm_bytes(o.w));
      HIPCHK(launch_dgemm(o, EPI_PLAIN, st));
    }
    RowSrc ao;  // LN(h + O(...)), Modules.cc:316
    ao.x = c->dout.as<float>();
    ao.ln_scale = L.attn.ln.scale.as<float>();
    ao.ln_bias = L.attn.ln.bias.as<float>();
    // FFN (Modules.cc:251-257)
    DGemmArgs f1;
    f1.B = N; f1.D = D;
    f1.a = ao;
    f1.w = L.ffn1.w;
    f1.y_i8 = c->df8.as<int8_t>();
    f1.ldy8 = m->F;
    f1.a_quant_out = L.ffn2.w.a_quant;
    {
      ProfScope p(c, SLIMT_HIP_K_GEMM_DEC, gemm_macs(N, f1.w), gemm_bytes(f1.w));
      HIPCHK(launch_dgemm(f1, EPI_RELU_Q, st));
    }
    DGemmArgs f2;
    f2.B = N; f2.D = D;
    f2.a_i8 = c->df8.as<int8_t>();
    f2.w = L.ffn2.w;
    f2.res = ao;
    f2.y = c->dx_pre.as<float>();
    f2.ldy = D;
    {
      ProfScope p(c, SLIMT_HIP_K_GEMM_DEC, gemm_macs(N, f2.w), gemm_bytes(f2.w));
      HIPCHK(launch_dgemm(f2, EPI_PLAIN, st));
    }
  }
  return 0;
}

// The steps of a beam call (include/slimt_hip.h, slimt_hip_translate_beam*) behind translate_device's
// encoder and decode_setup: R = B beam rows, source-major, whose sources call.row_src names. A step is decoder_layers with
// the fan-out attention, the logits gemm with EPI_PLAIN into tr_logits, and ONE launch of beam_select.hip's kernel, which
// also gathers the SSRU states by parent from the step's block into the other and embeds the next tokens. The attention
// writes its alignment rows into a history [R][Tmax][S] at the rows' step word; the finish kernel behind the last step
// orders the hypotheses and collects tokens, scores and alignment rows along the back-pointers.
int beam_steps(slimt_hip_ctx *c, size_t B, size_t S, size_t Tmax, uint32_t eos_id, const uint32_t *d_shortlist, uint32_t *d_out_ids,
               uint32_t *d_out_len, float *d_align, int steps_hint) {
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  CallState &call = c->call;
  const size_t k = (size_t)call.beam, R = B * k;
  const AffineW &out = output_layer(c);
  if (!call.fanout || (size_t)call.rows != R || !call.row_src || !call.bm_dev_totals) return fail(-1, "beam: not a beam call");
  if ((uint32_t)out.w.N >= kBeamMaxN) return fail(-1, "beam: an output layer of %d columns (2^20 or more)", out.w.N);
  const size_t T = std::min(Tmax, steps_hint > 0 ? (size_t)steps_hint : Tmax);
  HIPCHK(c->tr_logits.reserve(R * (size_t)out.w.N * 4));
  HIPCHK(c->bm_state.reserve((size_t)m->Ld * R * m->D * 4));
  HIPCHK(c->bm_slots.reserve((4 * R + B) * 4));
  HIPCHK(c->bm_hist.reserve(3 * T * R * 4));
  if (d_align) HIPCHK(c->bm_align.reserve(R * Tmax * S * 4));
  float *const totals = c->bm_slots.as<float>();
  uint32_t *const flags = c->bm_slots.as<uint32_t>() + R, *const len = flags + R, *const step_word = len + R, *const done = step_word + R;
  uint32_t *const h_parent = c->bm_hist.as<uint32_t>(), *const h_token = h_parent + T * R;
  float *const h_score = reinterpret_cast<float *>(h_token + T * R);
  float *const blocks[2] = {c->state.as<float>(), c->bm_state.as<float>()};
  BeamSelectArgs sa;
  sa.logits = c->tr_logits.as<float>();
  sa.B = (int)B; sa.k = (int)k; sa.N = out.w.N;
  sa.ids = d_shortlist;
  sa.eos = eos_id;
  sa.totals_in = sa.totals_out = totals;
  sa.flags_in = sa.flags_out = flags;
  sa.len_in = sa.len_out = len;
  sa.step_word = step_word;
  sa.Ld = m->Ld;
  sa.emb = embed_args(c);
  sa.dx = c->dx.as<float>();
  sa.done = done;
  sa.n_finished = c->n_finished.as<int>();
  {
    BeamSelectArgs ia = sa;  // the start state: slot 0 live at +0, the zero embedding (decode_setup zeroed block 0's states)
    ia.init = 1;
    const hipError_t he = launch_beam_select(ia, st);
    if (he != hipSuccess) return fail((int)he, "beam start: %s", hipGetErrorString(he));
  }
  size_t t = 0;
  for (; t < T; ++t) {
    if (steps_hint <= 0 && t > 0 && (t % 8) == 0) {  // stop as soon as every source is done
      HIPCHK(hipMemcpyAsync(c->n_finished_host, c->n_finished.p, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (*c->n_finished_host >= (int)B) break;
    }
    call.bm_state_cur = blocks[t & 1];
    RCCHK(decoder_layers(c, d_align ? c->bm_align.as<float>() : nullptr, (int)Tmax, step_word, nullptr));
    DGemmArgs g;
    g.B = (int)R;
    g.D = m->D;
    g.a = decoder_out_rows(c);
    g.w = out.w;
    g.y = c->tr_logits.as<float>();
    g.ldy = out.w.N;
    {
      ProfScope p(c, SLIMT_HIP_K_LOGITS, gemm_macs((int)R, out.w), gemm_bytes(out.w));
      HIPCHK(launch_dgemm(g, EPI_PLAIN, st));
    }
    sa.t = (int)t;
    sa.parent = h_parent + t * R;
    sa.token = h_token + t * R;
    sa.token_score = h_score + t * R;
    sa.state_src = blocks[t & 1];
    sa.state_dst = blocks[(t + 1) & 1];
    const hipError_t he = launch_beam_select(sa, st);
    if (he != hipSuccess) return fail((int)he, "beam selection: %s", hipGetErrorString(he));
  }
  BeamFinishArgs fa;
  fa.B = (int)B; fa.k = (int)k; fa.T = (int)t; fa.Tmax = (int)Tmax; fa.S = (int)S; fa.mode = call.beam_mode;
  fa.parent = h_parent; fa.token = h_token; fa.token_score = h_score;
  fa.totals = totals; fa.flags = flags; fa.len = len;
  fa.align_hist = d_align ? c->bm_align.as<float>() : nullptr;
  fa.lengths = c->lengths.as<uint32_t>();
  fa.out_ids = d_out_ids; fa.out_len = d_out_len;
  fa.out_totals = call.bm_dev_totals; fa.out_scores = call.bm_dev_scores; fa.out_align = d_align;
  const hipError_t he = launch_beam_finish(fa, st);
  if (he != hipSuccess) return fail((int)he, "beam finish: %s", hipGetErrorString(he));
  return 0;
}

// The slot a lean translate call draws when it starts, and the k (kept launches of every 8) of the admission before it: the
// K/V cache policy of THIS call, known to its encoder before its decoder is admitted (launch_choice.h, kv_launch_eighths).
struct KvCallSlot {
  unsigned long long slot = 0;
  int k = 8;
};
// The persistent decoder's launch in three steps (translate_device): the tiling asked for, the arguments, the admission.
struct FusedTiling {
  bool tight = false, clusters = false;
  int rows_per_wg = 0;
};

// ---- the persistent decoder: the whole greedy loop in one launch (decode_fused.hip) ---------------------------------
// The tiling a launch asks for (launch_choice.h), from what the call and this context's last encoder left.
FusedTiling choose_fused_tiling(slimt_hip_ctx *c, size_t B, size_t S, bool kv24, bool scored, bool merged, size_t n_expected) {
  const slimt_hip_model *m = c->model;
  // 32 sentences per workgroup (where the kernel has it) once the output layer dominates the
  // weights a step streams: with the full 32k vocabulary it is 8 of 10 MB per workgroup and step, and
  // halving it per sentence beats the longer attention chain (B = 512, full vocabulary: 20.4 -> 23-24 M
  // tok/s; at 16k columns the two are level, below that 16 rows win)
  // ... and 8 or 4 (decode_fused.hip, SPW) when the decoders in flight would leave most of the chip idle:
  // decided in admit_and_launch_fused, under the admission lock, from the contexts that have a decoder pending
  // Round 5: where the kernel has it, output layers that wide are SHARED by clusters of four 16-sentence workgroups
  // instead (decode_fused.hip, CL: each member streams a quarter of the columns for all 64 sentences) -- under the
  // decoder admission only: the members wait for each other, and the admission is what guarantees every admitted
  // workgroup a CU without waiting for another decoder (decode mode 6 forces clusters, 3 the 32-sentence tiling)
  // Measured on config 4 (B = 512, 32,000 columns, 20 workers; profiles/r05_cluster_logits.txt): clusters 23.4 M tok/s,
  // the 32-sentence tiling 24.9 M, the 16-sentence one 22.0 M -- a member's quarter of the columns takes 27 us + 14 us of
  // skew between its waves + 6 us of hand-overs where the whole layer took 70, but the 32-sentence tiling's per-sentence
  // cost is lower still: the phase is bound by the arg-max epilogue's issue slots and the address path's load
  // instructions (six per column tile here, four and a half there), not by the bytes the split saves. So: on request only.
  // a batch whose encoder was allowed the tight cache form: the tilings with its reader, whatever is asked for now (the
  // encoder is only allowed it when this context's decoders take those: kv_tight_wanted; a mode changed between the two
  // calls, or a first large output layer, ends up here)
  // (scored calls: the 16-sentence tilings without clusters, the only ones with the scored twin -- decode modes 2-6 and
  // the adaptive rows are "16 rows" for them)
  FusedTiling t;
  t.tight = kv_tight_launch(kv24, c->kv_tight, c->kv_fmt_valid, c->kv_fmt_B, (int)B);
  t.clusters = clusters_chosen(cluster_ok(kv24, m->D, m->F, S, m->decoder_budget), c->decode_mode, t.tight, merged, scored);
  c->expect_large_output = n_expected > 16384;
  t.rows_per_wg = fused_rows_requested(t.clusters, scored, c->decode_mode, n_expected, t.tight, S,
                                       fused_decode_tight_rows32_supported(m->D, m->F, m->H, m->Ld), merged);
  return t;
}

// Weights, K/V constants, the call's options and a merged launch's tables. No lock, no decision: those are
// choose_fused_tiling before it and admit_and_launch_fused behind it. d_shortlist: nullptr for the full vocabulary.
int fill_fused_decode_args(slimt_hip_ctx *c, FusedDecodeArgs &f, const FusedTiling &tiling, size_t B, size_t S, size_t Tmax,
                           int steps_hint, const uint32_t *d_lengths, const uint32_t *d_shortlist, const uint32_t *d_n_sl,
                           uint32_t eos_id, uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align, float *align_out,
                           float *d_scores, bool kv24, const MergePlan *mp) {
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  const CallState &call = c->call;
  const bool forced = call.forced, sampled = call.sampled, scored = call.scored || forced || sampled;
  const AffineW &out = output_layer(c);
  f.B = (int)B; f.S = (int)S; f.Ld = m->Ld;
  f.max_steps = steps_hint > 0 ? steps_hint : (int)(Tmax > 1 ? Tmax : 1);
  f.Tmax = (int)Tmax;
  f.kv_tight = tiling.tight;
  f.rows_per_wg = tiling.rows_per_wg;
  if (tiling.clusters) {
    const size_t tiles = (B + 15) / 16, n_clusters = (tiles + 3) / 4;
    HIPCHK(c->cl_act.reserve(tiles * 16 * (size_t)m->D));
    HIPCHK(c->cl_part.reserve(tiles * (16 * 4 + 1) * 8));
    HIPCHK(c->cl_sync.reserve(n_clusters * 4));
    HIPCHK(hipMemsetAsync(c->cl_sync.p, 0, n_clusters * 4, st));
    f.cluster = 4;
    f.cl_act = c->cl_act.as<unsigned char>();
    f.cl_part = c->cl_part.as<int>();
    f.cl_sync = c->cl_sync.as<unsigned>();
    f.dev_error = dev_error_device_view(c);
  }
  for (int l = 0; l < m->Ld; ++l) {
    const DecLayerW &L = m->dec[(size_t)l];
    FusedLayerW &fl = f.L[l];
    fl.rnn_f = L.rnn_f.w; fl.rnn_w = L.rnn_w.w; fl.q = L.attn.q.w; fl.o = L.attn.o.w;
    fl.ffn1 = L.ffn1.w; fl.ffn2 = L.ffn2.w;
    fl.rnn_ln_s = L.rnn_ln.scale.as<float>(); fl.rnn_ln_b = L.rnn_ln.bias.as<float>();
    fl.attn_ln_s = L.attn.ln.scale.as<float>(); fl.attn_ln_b = L.attn.ln.bias.as<float>();
    fl.ffn_ln_s = L.ffn_ln.scale.as<float>(); fl.ffn_ln_b = L.ffn_ln.bias.as<float>();
  }
  f.out = out.w;
  f.out_n_dev = d_n_sl;
  f.shortlist = d_shortlist;
  f.emb = embed_args(c);
  f.out_tied_exact = m->out_tied_exact;
  f.kv = c->kv.as<float>();
  f.kv24 = kv24;
  if (kv24 && c->kv_fmt_valid && c->kv_fmt_B == (int)B) f.kv_fmt = c->kv_fmt.as<unsigned char>();
  for (int l = 0; l < m->Ld; ++l) {  // the projections' constants, applied after the attention's sums (kernels.h, kv24)
    const AffineW &wk = m->dec[(size_t)l].attn.k, &wv = m->dec[(size_t)l].attn.v;
    f.kv_pb[l][0] = wk.w.pb;
    f.kv_pb[l][1] = wv.w.pb;
    f.kv_cs[l][0] = wk.w.colsum;
    f.kv_cs[l][1] = wv.w.colsum;
    f.kv_u[l][0] = wk.w.u;
    f.kv_u[l][1] = wv.w.u;
    f.kv_u256[l][0] = wk.w.u * (1.0f / 256.0f);  // exact scalings: the packed integers come back
    f.kv_u256[l][1] = wv.w.u * (1.0f / 256.0f);  // as accS * 256 (decode_fused.hip, unpack24f)
    f.kv_centre[l][0] = m->kv_centre_of(c->kv_gen, l, 0);  // (the tight form, the generation this batch's encoder wrote
    f.kv_centre[l][1] = m->kv_centre_of(c->kv_gen, l, 1);  //  it against; null until calibrated, not read then)
    f.kv_u4096[l][0] = wk.w.u * (1.0f / 4096.0f);  // ... as accS * 4096 from the narrow form (unpack20)
    f.kv_u4096[l][1] = wv.w.u * (1.0f / 4096.0f);
  }
  f.scores = d_scores;
  if (sampled) {
    f.inv_T = call.inv_T;
    f.keys = mp ? nullptr : call.dev.keys;
    for (int j = 0; mp && j < mp->n; ++j) f.sub_keys[j] = mp->opt[j].keys;
  }
  if (forced && !mp) {
    f.prefix_ids = call.dev.prefix_ids;
    f.prefix_len = call.dev.prefix_len;
  }
  if (mp) {
    f.n_sub = mp->n;
    f.sub_dense = mp->dense ? 1 : 0;
    for (int j = 0; j < mp->n; ++j) f.sub[j] = mp->out[j];
    for (int j = 0; scored && j < mp->n; ++j) f.sub_scores[j] = mp->opt[j].scores;
    for (int j = 0; forced && j < mp->n; ++j) {
      f.sub_prefix_ids[j] = mp->opt[j].prefix_ids;
      f.sub_prefix_len[j] = mp->opt[j].prefix_len;
    }
    f.out_stride_wp = mp->stride_wp;
    f.out_stride_cs = mp->stride_cs;
    f.out_stride_pb = mp->stride_pb;
    f.shortlist = nullptr;
  }
  f.cells = c->state.as<float>();
  f.lengths = d_lengths;
  f.alpha = 1.0f / std::sqrt(static_cast<float>(m->D / m->H));
  f.eos = eos_id;
  f.out_ids = d_out_ids;
  f.out_len = d_out_len;
  f.align = d_align;
  f.align_out = d_align ? align_out : nullptr;
  f.trace = g_occ_trace;
  f.ticket = c->ticket.as<unsigned>();
  f.ticket_base = c->ticket_base;  // advanced by admit_and_launch_fused, once the launch is in the stream
  if (c->stamp_step >= 0 && c->stamps.p) {
    f.stamps = c->stamps.as<unsigned long long>();
    f.stamp_step = c->stamp_step;
  }
  return 0;
}

// The launch: everything the model's contexts decide together, under gate_mu -- the pending contexts, the plan
// (decoder_plan.h), the K/V temporal policy, the XCD homes, the admission wait, the launch and the gate event -- or, without
// a decoder budget, the launch alone.
int admit_and_launch_fused(slimt_hip_ctx *c, FusedDecodeArgs &f, size_t B, size_t S, bool kv24, const KvCallSlot &drawn,
                           StageClock &clk) {
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  int rows = fused_decode_rows(m->D, m->F, m->H, m->Ld, (int)S, (int)B, f.rows_per_wg, kv24);
  unsigned tickets = (unsigned)fused_decode_grid((int)B, true, rows);
  const double macs = (double)B * f.max_steps *
                      (m->Ld * (4.0 * m->D * m->D + 2.0 * m->D * m->F) + (double)m->D * f.out.N);
  double wbytes = (double)f.max_steps * ((B + rows - 1) / rows) *
                  (m->Ld * (4.0 * m->D * m->D + 2.0 * m->D * m->F) + (double)m->D * f.out.n_tiles * 16);
  slimt_hip_model *gm = c->model;
  int wgs = ((int)B + rows - 1) / rows;
  if (gm->decoder_budget > 0) {
    // decoder admission (engine.h): launch k waits for launch k - n on its own stream
    constexpr size_t kRing = 64;
    clk.lap(7);
    std::lock_guard<std::mutex> lock(gm->gate_mu);
    clk.lap(2);
    while (gm->gate_ev.size() < kRing) {
      hipEvent_t ev;
      HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      gm->gate_ev.push_back(ev);
    }
    // K/V cache policy (decode_fused.hip, KV_AUX). The caches that are being read at any
    // moment are those of the decoders that run: at most one per context (a context is a
    // stream), one per hardware queue and n by admission. While they fit the 256 MB Infinity Cache every
    // step re-reads them from there and non-temporal loads only lose that; beyond it the
    // cache streams from HBM anyway and non-temporal loads keep it from displacing the
    // weights. In between, the first layers' caches stay temporal (they then fit) and the
    // rest stream: t_layers = as many of the Ld per-layer caches as 300 MB cover.
    // Measured (tok/s, t_layers 0 / 1 / 2, Ld = 2): B=256, S=32 at 8 workers 17.1 / - /
    // 18.8 M, 12: 21.9 / 22.5 / 22.1, 16: 23.6 / 24.2 / 22.6, 20: 23.9 / 24.5 / 23.5;
    // B=512 full vocabulary 16.7 / 17.1 / 15.8; B=128, S=64 9.0 / 8.5 / 7.9; B=64, S=32
    // 11.9 / - / 13.6; base 6.4 / 5.9 / 5.7.
    // Which contexts have a decoder pending is judged from when they launched last (a translate
    // call takes a few milliseconds), not by asking the runtime: one hipEventQuery per context
    // under this lock made every launch O(contexts) runtime calls, and with a dozen worker threads
    // the launches queued behind each other (Service, 16 workers: 9.9 ms per launch call).
    // (the narrow form is what the model's sentences are expected to take where the kernels have it: 2.5 bytes per value)
    const double kv_bytes = (double)m->Ld * 2.0 * (double)B * (double)S * m->D * kv_bytes_per_value(f.kv_tight, f.kv_fmt != nullptr, kv24);
    const auto now = std::chrono::steady_clock::now();
    double pending = kv_bytes;
    size_t contexts = 1;
    bool known = false;
    for (auto &g : gm->gate_ctx) {
      if (g.ctx == c) {
        g.seq = gm->gate_seq;
        g.kv_bytes = kv_bytes;
        g.when = now;
        known = true;
      } else if (gm->gate_seq - g.seq < kRing && now - g.when < std::chrono::milliseconds(25)) {
        pending += g.kv_bytes;
        contexts += 1;
      }
    }
    if (!known) gm->gate_ctx.push_back({c, gm->gate_seq, kv_bytes, now});
    // The plan (decoder_plan.h): sentences per workgroup (decode mode 0: the fewest of 16 / 8 / 4 with which the
    // decoders in flight still fit the budget -- one batch of 256 alone runs on 64 CUs instead of 16; a workgroup of
    // fewer sentences streams the same weights for them: worth it only for CUs that would idle; results do not depend
    // on it), the admission depth n and the K/V policy below. Decoders in flight = min(pending contexts, hardware
    // queues): with GPU_MAX_HW_QUEUES = 32 the headline's twenty contexts are twenty decoders and stay at 16
    // sentences, n = 14; with the runtime's default four queues only four run, and they take the 8-sentence tiling
    // (4 x 32 workgroups) with no admission waits ("queue-bound").
    // (SLIMT_ROWS_OVERSUB loosens "fit the budget")
    // ... the K/V caches in eighths of a layer's caches (kernels.h, kv_temporal_eighths): SLIMT_KV_BUDGET_MB /
    // SLIMT_KV_GRAIN tune the rule (defaults: 300 MB in whole layers, the measured optimum above)
    // Round 4: WHICH caches stay temporal. "Layer 0 of every decoder" (the rule above) makes every workgroup pay one
    // cached and one streamed attention per step; keeping BOTH layers of k of every 8 launches (by admission order)
    // and streaming both layers of the others holds the same bytes but lets the kept decoders run their whole step
    // at the cached speed (and finish together, so no CU idles inside a launch): 32.35 -> 33.05-33.26 M tok/s at
    // k = 6, 32.5-32.9 at k = 5, 32.3-32.6 at k = 7, 31.7 all temporal (profiles/archive/r04_v3_kv_by_launch.txt).
    // k = as many eighths of the pending decoders as SLIMT_KV_LAUNCH_BUDGET_MB covers (round 4: 270, the 24-bit form;
    // round 5: 300 -- with the narrow form the headline's decoders hold 232 MB, k = 6 / 7 / 8 measure the same
    // (35.8 / 35.7 / 35.6 M tok/s, profiles/r05_kv_keep_sweep.txt), and every launch then runs the kept instantiation);
    // SLIMT_KV_BY_LAUNCH: 0 = the per-layer rule, 1..8 = that k.
    // (sentences of up to 32 tokens; longer ones measured 2-3 % slower this way and keep the per-layer rule:
    // S = 64 18.5 -> 17.9 M, S = 128 8.2 -> 8.0 M)
    // ... and launches of which at least four fit the budget: ONE batch of 4096 holds 400 MB by itself, and keeping
    // "all of it" thrashes where "its layer 0" fits (29.8 -> 27.2 M tok/s). With four queues the four decoders in
    // flight hold 4 x 13-17 MB at the headline: every launch stays temporal.
    DecoderPlanIn pin;
    pin.B = (int)B; pin.S = (int)S; pin.Ld = m->Ld;
    pin.rows = rows;
    pin.adaptive = c->decode_mode == 0 && f.rows_per_wg == 0 && gm->adaptive_rows;
    pin.narrow_ok = fused_decode_rows(m->D, m->F, m->H, m->Ld, (int)S, (int)B, 4, kv24) == 4 &&
                    fused_decode_rows(m->D, m->F, m->H, m->Ld, (int)S, (int)B, 8, kv24) == 8;
    pin.kv_bytes = kv_bytes;
    pin.pending_kv = pending;
    pin.contexts = contexts;
    pin.queues = gm->hw_queues;
    pin.budget = gm->decoder_budget;
    pin.kv_policy = gm->kv_policy;
    pin.ring = kRing;
    pin.rows_oversub = env().rows_oversub;
    pin.kv_budget = env().kv_budget;
    pin.kv_grain = env().kv_grain;
    pin.by_launch = env().kv_by_launch;
    pin.launch_budget = env().kv_launch_budget;
    const DecoderPlan plan = decoder_plan(pin);
    if (plan.rows != rows) {
      f.rows_per_wg = plan.rows;
      rows = plan.rows;
      tickets = (unsigned)fused_decode_grid((int)B, true, rows);
      wgs = plan.wgs;
      wbytes = (double)f.max_steps * wgs *
               (m->Ld * (4.0 * m->D * m->D + 2.0 * m->D * m->F) + (double)m->D * f.out.n_tiles * 16);
    }
    const size_t n = plan.n;
    const int all = 8 * m->Ld;
    // (the slot was drawn when the call started, with the k of the admission before it: the encoder of a call
    // whose cache will be streamed can then write it non-temporally, SLIMT_KV_STORE_NT=1)
    const int eighths = kv_launch_eighths(plan.by_launch, plan.eighths, plan.k, drawn.slot, drawn.k, env().kv_store_nt, all);
    gm->kv_k_last.store(plan.by_launch ? plan.k : 8, std::memory_order_relaxed);
    f.kv_nt = eighths < all;
    f.kv_temporal_eighths = eighths;
    c->plan_last[0] = rows;
    c->plan_last[1] = (int)contexts;
    c->plan_last[2] = (int)plan.in_flight;
    c->plan_last[3] = plan.wait ? (int)n : 0;
    c->plan_last[4] = eighths;
    c->plan_last[5] = gm->hw_queues;
    if (plan.wait && gm->gate_seq >= n) HIPCHK(hipStreamWaitEvent(st, gm->gate_ev[(gm->gate_seq - n) % kRing], 0));
    clk.lap(3);
    const int n_home = gm->xcd_affinity;
    const bool affine = n_home > 0 && rows == 16 && wgs <= 16 * n_home;
    if (affine) {
      if (gm->gate_home.size() < kRing) gm->gate_home.assign(kRing, 0u);
      unsigned mask = gm->gate_seq >= n ? gm->gate_home[(gm->gate_seq - n) % kRing] : 0u;
      if (!mask || __builtin_popcount(mask) != n_home) {
        const unsigned slot = (unsigned)(gm->gate_seq % (size_t)(8 / n_home));
        mask = n_home == 1 ? 1u << slot : n_home == 2 ? 3u << (2 * slot) : 0xfu << (4 * (slot & 1));
      }
      gm->gate_home[gm->gate_seq % kRing] = mask;
      f.home_mask = mask;
      f.xstate = reinterpret_cast<unsigned long long *>(c->ticket.as<unsigned>() + 2);
      f.xarr_base = c->xarr_base;
      f.xclaim_base = c->xclaim_base;
      f.xgrid = 8u * (unsigned)((wgs + n_home - 1) / n_home);
    } else if (!gm->gate_home.empty()) {
      gm->gate_home[gm->gate_seq % kRing] = 0u;
    }
    {
      ProfScope p(c, SLIMT_HIP_K_DECODE_FUSED, macs, wbytes);
      HIPCHK(launch_decode_fused(f, m->D, m->F, m->H, st));
    }
    clk.lap(4);
    if (affine) {
      c->xarr_base += f.xgrid;
      c->xclaim_base += (unsigned)wgs;
    } else {
      c->ticket_base += tickets;
    }
    HIPCHK(hipEventRecord(gm->gate_ev[gm->gate_seq % kRing], st));
    clk.lap(5);
    gm->gate_seq += 1;
    return 0;
  }
  ProfScope p(c, SLIMT_HIP_K_DECODE_FUSED, macs, wbytes);
  HIPCHK(launch_decode_fused(f, m->D, m->F, m->H, st));
  c->ticket_base += tickets;
  return 0;
}

// ---- the step-wise loop: every call the persistent decoder refuses (truncated, fan-out, beam, consensus; decode mode 1,
// K/V format 3, shapes without the kernel) ----------------------------------------------------------------------------
int decode_stepwise(slimt_hip_ctx *c, size_t B, size_t S, size_t R, size_t Tmax, const uint32_t *d_shortlist, uint32_t eos_id,
                    uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align, float *d_scores, int steps_hint, bool merged) {
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  const CallState &call = c->call;
  const bool forced = call.forced, sampled = call.sampled;
  const AffineW &out = output_layer(c);
  DecodeState ds;
  ds.prev = c->prev.as<uint32_t>();
  ds.out_ids = d_out_ids;
  ds.out_len = d_out_len;
  ds.finished = c->finished.as<uint8_t>();
  ds.n_finished = c->n_finished.as<int>();
  ds.Tmax = (int)Tmax;
  ds.eos = eos_id;
  ds.shortlist = d_shortlist;
  ds.pb0 = out.w.pb;
  ds.u_out = out.w.u;
  if (call.beam) return beam_steps(c, B, S, Tmax, eos_id, ds.shortlist, d_out_ids, d_out_len, d_align, steps_hint);
  // a truncated call stores each step's logits and selects over them: one partial per row (sample_truncate.hip)
  const bool truncated = sampled && call.truncated;
  if (call.truncated && !truncated) return fail(-1, "sampling truncation: the call is not sampled");
  const int n_parts = truncated ? 1 : dgemm_col_blocks(out.w.K, out.w.N, (int)R);
  if (truncated) HIPCHK(c->tr_logits.reserve(R * (size_t)out.w.N * 4));
  const EmbedArgs e = embed_args(c);
  if (d_scores) HIPCHK(c->part_sum.reserve(R * (size_t)n_parts * 4));
  float *const part_sum = d_scores ? c->part_sum.as<float>() : nullptr;
  if (forced && merged) return fail(-1, "target prefix: merged launches decode with the persistent kernels only");
  if (sampled && merged) return fail(-1, "sampling: merged launches decode with the persistent kernels only");
  SampledStep ss;  // (sampled: the keys, the steps' hash words and the partials beside the arg-max's, kernels.h)
  if (sampled) {
    HIPCHK(c->sm_seeds.reserve(2 * R * 4));
    HIPCHK(c->sm_part_mz.reserve(R * (size_t)n_parts * 4));
    HIPCHK(c->sm_part_zw.reserve(R * (size_t)n_parts * 4));
    ss.inv_T = call.inv_T;
    ss.keys = call.dev.keys;
    ss.seeds = c->sm_seeds.as<uint32_t>();
    ss.part_mz = c->sm_part_mz.as<float>();
    ss.part_zw = c->sm_part_zw.as<float>();
  }
  ForcedStep fs;  // (forced: the prefix's tokens and their columns, kernels.h)
  if (forced) {
    HIPCHK(c->fp_col.reserve(R * 4));
    HIPCHK(c->fp_part_y.reserve(R * (size_t)n_parts * 4));
    fs.ids = call.dev.prefix_ids;
    fs.len = call.dev.prefix_len;
    fs.sl = ds.shortlist;
    fs.N = out.w.N;
    fs.fcol = c->fp_col.as<int>();
    fs.part_y = c->fp_part_y.as<float>();
  }
  const size_t max_steps = steps_hint > 0 ? (size_t)steps_hint : (Tmax > 1 ? Tmax : 1);
  int rc = 0;
  size_t t = 0;
  bool all_done = false;
  for (; t < max_steps && !rc; ++t) {
    hipError_t he = launch_decode_begin_step(e, ds, (int)R, t == 0, 1, c->part_val.as<float>(),
                                             c->part_idx.as<int>(), n_parts, c->dx.as<float>(), st, part_sum, d_scores, &fs, &ss);
    if (he != hipSuccess) { rc = fail((int)he, "decode_begin_step: %s", hipGetErrorString(he)); break; }
    if (steps_hint <= 0 && t > 0 && (t % 8) == 0) {
      // stop as soon as every sentence has emitted EOS (Model.cc:161)
      he = hipMemcpyAsync(c->n_finished_host, c->n_finished.p, sizeof(int), hipMemcpyDeviceToHost, st);
      if (he == hipSuccess) he = hipStreamSynchronize(st);
      if (he != hipSuccess) { rc = fail((int)he, "early-exit readback: %s", hipGetErrorString(he)); break; }
      if (*c->n_finished_host >= (int)R) { all_done = true; break; }
    }
    rc = decoder_layers(c, d_align, (int)Tmax, d_out_len, nullptr);
    if (rc) break;
    DGemmArgs g;
    g.B = (int)R;
    g.D = m->D;
    g.a = decoder_out_rows(c);
    g.w = out.w;
    g.part_val = c->part_val.as<float>();
    g.part_idx = c->part_idx.as<int>();
    g.n_parts = n_parts;
    g.part_sum = part_sum;
    g.fcol = fs.fcol;
    g.part_y = fs.ids ? c->fp_part_y.as<float>() : nullptr;
    if (sampled) {
      g.fcol = fs.ids ? fs.fcol : nullptr;
      g.inv_T = ss.inv_T;
      g.seeds = ss.seeds;
      g.sm_shortlist = ds.shortlist;
      g.part_mz = c->sm_part_mz.as<float>();
      g.part_zw = c->sm_part_zw.as<float>();
    }
    if (truncated) {
      g.y = c->tr_logits.as<float>();
      g.ldy = out.w.N;
    }
    {
      ProfScope p(c, SLIMT_HIP_K_LOGITS, gemm_macs((int)R, out.w), gemm_bytes(out.w));
      he = launch_dgemm(g, truncated ? EPI_PLAIN : sampled ? EPI_ARGMAX_SM : fs.ids ? EPI_ARGMAX_FP : d_scores ? EPI_ARGMAX_SC : EPI_ARGMAX, st);
    }
    if (he != hipSuccess) { rc = fail((int)he, "logits gemm: %s", hipGetErrorString(he)); break; }
    if (truncated) {
      SampleTruncArgs ta;
      ta.logits = c->tr_logits.as<float>();
      ta.B = (int)R;
      ta.N = out.w.N;
      ta.inv_T = ss.inv_T;
      ta.top_k = call.top_k;
      ta.top_p = call.top_p;
      ta.seeds = ss.seeds;
      ta.shortlist = ds.shortlist;
      ta.fcol = g.fcol;
      ta.part_val = g.part_val;
      ta.part_idx = g.part_idx;
      ta.part_sum = g.part_sum;
      ta.part_mz = g.part_mz;
      ta.part_zw = g.part_zw;
      ta.part_y = g.part_y;
      he = launch_sample_truncated(ta, st);
      if (he != hipSuccess) { rc = fail((int)he, "truncated sampling: %s", hipGetErrorString(he)); break; }
    }
  }
  if (!rc && !all_done) {
    hipError_t he = launch_decode_begin_step(e, ds, (int)R, 0, 0, c->part_val.as<float>(),
                                             c->part_idx.as<int>(), n_parts, c->dx.as<float>(), st, part_sum, d_scores, &fs, &ss);
    if (he != hipSuccess) rc = fail((int)he, "final record: %s", hipGetErrorString(he));
  }
  if (!rc && call.consensus) {  // the selection over the rows just written (consensus.hip): one launch behind the last step
    ConsensusArgs ca;
    ca.ids = d_out_ids;
    ca.len = d_out_len;
    ca.row_src = c->call.row_src;
    ca.N = (uint32_t)R;
    ca.T = (uint32_t)Tmax;
    ca.B = (uint32_t)B;
    ca.max_order = call.cs_order;
    ca.beta2 = call.cs_beta2;
    ca.utility = call.cs_dev_util;
    ca.best = call.cs_dev_best;
    ProfScope p(c, SLIMT_HIP_K_CONSENSUS, 0, 0);
    const hipError_t he = launch_consensus(ca, st);
    if (he != hipSuccess) rc = fail((int)he, "consensus: %s", hipGetErrorString(he));
  }
  return rc;
}

// The batch's options as the kernels address them (the entry points set them): call.dev, or in a merged launch each
// sub-batch's mp->opt[j].
// a scored call: each recorded token's log-probability goes beside it
// a forced call takes the scored kernels' forced twins: scored as well, into a context-owned scratch when the caller did
// not ask for scores (merged: sub-batch j's rows of it from its first sentence on, Tmax_j <= Tmax)
// a sampled call takes their sampled twins, with or without a prefix: scored in the same way
int check_call_destinations(slimt_hip_ctx *c, size_t R, size_t Tmax, MergePlan *mp, float **d_scores_out) {
  const CallState &call = c->call;
  const bool forced = call.forced;
  const bool sampled = call.sampled;
  const bool scored = call.scored || forced || sampled;
  if ((forced || sampled) && !call.scored) {
    HIPCHK(c->fp_scratch.reserve(R * Tmax * 4));
    for (int j = 0; mp && j < mp->n; ++j) mp->opt[j].scores = c->fp_scratch.as<float>() + (size_t)mp->out[j].first * Tmax;
  }
  float *const d_scores = scored && !mp ? (call.scored ? call.dev.scores : c->fp_scratch.as<float>()) : nullptr;
  if (scored && !mp && !d_scores) return fail(-1, "scores: no destination for this batch");
  for (int j = 0; scored && mp && j < mp->n; ++j)
    if (!mp->opt[j].scores) return fail(-1, "scores: no destination for batch %d", j);
  if (forced && !mp && !(call.dev.prefix_ids && call.dev.prefix_len)) return fail(-1, "target prefix: none for this batch");
  for (int j = 0; forced && mp && j < mp->n; ++j)
    if (!mp->opt[j].prefix_ids || !mp->opt[j].prefix_len) return fail(-1, "target prefix: none for batch %d", j);
  *d_scores_out = d_scores;
  return 0;
}

// The lean path's first launch: the output layer's packing job (one per distinct shortlist in a merged launch), the
// call's slot in the by-launch K/V policy, the persistent encoder, and -- for the batch that claimed it -- the centres'
// reduction behind it.
int encode_lean_for_translate(slimt_hip_ctx *c, const uint32_t *d_ids, const uint32_t *d_lengths, const uint32_t *d_shortlist,
                              size_t B, size_t S, size_t n_sl, const uint32_t *d_n_sl, const ShortlistArgs *gen, MergePlan *mp,
                              bool kv24, bool calibrate, KvCallSlot &slot) {
  const slimt_hip_model *m = c->model;
  PackArgs job;
  if (n_sl && mp) {
    // one allocation for the launch's jobs, job j at j strides (a stride holds the widest job)
    mp->stride_wp = (packed_weight_bytes(m->D, (int)n_sl) + 255) / 256 * 256;
    mp->stride_cs = (colsum_alloc_bytes((int)n_sl) + 255) / 256 * 256;
    mp->stride_pb = (((size_t)n_sl + 15) / 16 * 16 * sizeof(float) + 255) / 256 * 256;
    HIPCHK(c->out_sl.Wp.reserve(mp->stride_wp * mp->n_jobs));
    HIPCHK(c->out_sl.colsum.reserve(mp->stride_cs * mp->n_jobs));
    HIPCHK(c->out_sl.pb.reserve(mp->stride_pb * mp->n_jobs));
    RCCHK(prepare_affine_meta(c->out_sl, m->out_raw.as<int8_t>(), m->D, mp->jobs[0].N, mp->jobs[0].idx,
                              m->out_bias.as<float>(), m->out_a_quant, m->wemb_mult, job, m->V));
  } else if (n_sl) {
    RCCHK(prepare_affine_meta(c->out_sl, m->out_raw.as<int8_t>(), m->D, (int)n_sl, d_shortlist,
                              m->out_bias.as<float>(), m->out_a_quant, m->wemb_mult, job, m->V));
  }
  job.n_dev = d_n_sl;
  // the decoder's cache policy of THIS call (decided in admit_and_launch_fused, under the admission lock, from the same
  // two numbers): will its caches be kept in the Infinity Cache, or streamed? Streamed ones are also WRITTEN past it
  slot.slot = c->model->kv_call_seq.fetch_add(1, std::memory_order_relaxed);
  slot.k = c->model->kv_k_last.load(std::memory_order_relaxed);
  RCCHK(encode_device(c, (int)B, (int)S, nullptr, nullptr, d_ids, d_lengths, n_sl ? &job : nullptr, false, false, kv24, gen,
                      kv_store_streamed(env().kv_store_nt, kv24, slot.slot, slot.k), mp));
  c->n_sl = (int)n_sl;
  if (calibrate) queue_centre_reduction(c, (int)B, (int)S);
  return 0;
}

// The stage-wise path: the batch into the context's own buffers (d_lengths / d_shortlist then name those), the per-stage
// encoder, decode_setup, and the outputs cleared for R decoder rows.
int encode_stagewise_for_translate(slimt_hip_ctx *c, const uint32_t *d_ids, const uint32_t **d_lengths_io,
                                   const uint32_t **d_shortlist_io, size_t B, size_t S, size_t R, size_t Tmax, size_t n_sl,
                                   uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align) {
  hipStream_t st = c->stream;
  const uint32_t *d_lengths = *d_lengths_io, *d_shortlist = *d_shortlist_io;
  if (d_ids != c->ids.as<uint32_t>())
    HIPCHK(hipMemcpyAsync(c->ids.p, d_ids, B * S * 4, hipMemcpyDeviceToDevice, st));
  if (d_lengths != c->lengths.as<uint32_t>())
    HIPCHK(hipMemcpyAsync(c->lengths.p, d_lengths, B * 4, hipMemcpyDeviceToDevice, st));
  if (n_sl && d_shortlist != c->shortlist.as<uint32_t>()) {
    c->sl_host.clear();  // ctx->shortlist no longer holds what translate_host uploaded last
    HIPCHK(hipMemcpyAsync(c->shortlist.p, d_shortlist, n_sl * 4, hipMemcpyDeviceToDevice, st));
  }
  *d_lengths_io = c->lengths.as<uint32_t>();
  *d_shortlist_io = c->shortlist.as<uint32_t>();
  RCCHK(encode_device(c, (int)B, (int)S, nullptr, nullptr));
  RCCHK(decode_setup(c, n_sl));
  HIPCHK(hipMemsetAsync(d_out_ids, 0, R * (Tmax ? Tmax : 1) * 4, st));
  HIPCHK(hipMemsetAsync(d_out_len, 0, R * 4, st));
  HIPCHK(hipMemsetAsync(c->finished.p, 0, R, st));
  HIPCHK(hipMemsetAsync(c->n_finished.p, 0, 16, st));
  if (d_align) HIPCHK(hipMemsetAsync(d_align, 0, R * Tmax * S * 4, st));
  return 0;
}

// d_ids / d_lengths / d_shortlist: device pointers (the caller's, or the
// context's staging buffers). When both persistent kernels apply, a translate
// call is exactly two launches: [encoder + K/V cache + shortlist packing] and
// [decode loop]; nothing is copied or memset in between (small helper kernels
// queue behind the long-running decoders of the other workers).
int translate_device(slimt_hip_ctx *c, const uint32_t *d_ids, const uint32_t *d_lengths,
                     const uint32_t *d_shortlist, size_t B, size_t S, size_t n_sl,
                     float limit_factor, uint32_t eos_id, uint32_t *d_out_ids, uint32_t *d_out_len,
                     float *d_align, int steps_hint, const uint32_t *d_n_sl = nullptr,
                     float *align_out = nullptr, size_t n_sl_hint = 0, const ShortlistArgs *gen = nullptr,
                     MergePlan *mp = nullptr) {
  // mp (merged launch; lean path only, checked by the caller): B = the launch's global sentences, n_sl = the widest job's
  // columns (0 = full vocabulary for every sub-batch); d_ids / d_lengths / d_shortlist / d_out_* / d_align are not used
  // gen (with d_n_sl, lean path, 64-row encoder): the shortlist is generated inside the encoder launch
  // n_sl_hint (with d_n_sl): what the host expects the device-side shortlist size to be (the size of
  // this context's previous generated shortlist): tuning decisions only
  // align_out != nullptr (persistent decoder only): d_align is a staging buffer in device memory and
  // the decoder copies each sentence's rows from there to align_out when its loop ends (see
  // FusedDecodeArgs::align_out)
  // d_n_sl != nullptr: the shortlist was generated on this stream; its size is on
  // the device and n_sl is only the capacity of d_shortlist (persistent kernels only)
  const slimt_hip_model *m = c->model;
  // Model.cc:144-161: the first step is unconditional (one token is always recorded), the
  // loop then runs while i < (size_t)(limit_factor * S): at least one output column
  const size_t Tmax = std::max<size_t>(1, (size_t)(limit_factor * (float)S));
  const bool lean = persistent_path(c, S);
  // R decoder rows over the B sources: B, but in a fan-out call (never lean, never merged). The caller's outputs, the
  // per-call options and every decoder workspace are per row; ids, lengths, the encoder and the K / V per source.
  const CallState &call = c->call;
  const size_t R = call.fanout ? (size_t)call.rows : B;
  if (call.consensus) {  // (a fan-out call; the selection runs behind the last step, in decode_stepwise)
    if (!call.fanout || !call.cs_dev_best || !call.cs_dev_util) return fail(-1, "consensus: not a fan-out call");
    if (Tmax > (size_t)SLIMT_HIP_CONSENSUS_MAX_T)
      return fail(-1, "consensus: the call's Tmax %zu exceeds %d", Tmax, SLIMT_HIP_CONSENSUS_MAX_T);
  }
  // The K/V cache form (launch_choice.h, kv_cache_form): packed where the persistent pair has it for this shape and S.
  KvFormIn form;
  form.D = m->D; form.F = m->F; form.H = m->H;
  form.kv_format = m->kv_format;
  form.S = S;
  form.encode_rows = c->encode_rows;
  form.decode_mode = c->decode_mode;
  form.lean = lean;
  form.fused_encode_ok = fused_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S);
  form.tall_encode_ok = tall_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S);
  form.long_encode_ok = long_encode_supported(m->D, m->F, m->H, m->Le, m->Ld, (int)S);
  form.decode_packed_ok = fused_decode_packed_supported(m->D, m->F, m->H, m->Ld);
  form.decode_mid_ok = fused_decode_mid_supported(m->D, m->F, m->H, m->Ld);
  form.decode_long24_ok = fused_decode_long24_supported(m->D, m->F, m->H, m->Ld);
  const bool kv_packed = kv_cache_form(form).packed;
  // The tight form's centres (engine.h, kv_centre): the first batch of enough rows that could take the form is cached as
  // f32 instead, and its column means become the centres (behind the encoder, on this stream).
  ClaimGuard claim(c->model);
  if (kv_packed && c->model->kv_centre_state.load(std::memory_order_acquire) == 0 && kv_calibration_rows(B, S) &&
      kv_tight_shape(c, (int)S, kv_tight_writer(c, (int)B, (int)S)))
    claim.take();
  const bool calibrate = claim.armed;
  const bool kv24 = kv_packed && !calibrate;
  // One thread at a time queues a persistent translate (a few runtime calls, ~50 us): the runtime
  // serialises launches internally anyway, and a dozen worker threads contending inside it take
  // far longer per call than the same calls made one after the other (Service, 10 workers: 2.1 ms
  // per launch call against 0.05 ms with two).
  std::unique_lock<std::mutex> submit(c->model->submit_mu, std::defer_lock);
  StageClock clk;
  if (lean && env().submit_lock) submit.lock();
  clk.lap(2);
  if (env().host_timing) g_timing.calls += 1;
  float *d_scores = nullptr;
  RCCHK(check_call_destinations(c, R, Tmax, mp, &d_scores));
  KvCallSlot slot;
  if (lean) {
    RCCHK(encode_lean_for_translate(c, d_ids, d_lengths, d_shortlist, B, S, n_sl, d_n_sl, gen, mp, kv24, calibrate, slot));
    clk.lap(1);
  } else {
    RCCHK(encode_stagewise_for_translate(c, d_ids, &d_lengths, &d_shortlist, B, S, R, Tmax, n_sl, d_out_ids, d_out_len, d_align));
  }
  if (!n_sl) d_shortlist = nullptr;
  if (fused_decoder_allowed(c) && fused_decode_supported(m->D, m->F, m->H, m->Ld)) {
    const bool scored = call.scored || call.forced || call.sampled;
    const size_t n_expected = d_n_sl && n_sl_hint ? n_sl_hint : mp ? (size_t)(n_sl ? mp->max_N : m->V) : (size_t)output_layer(c).w.N;
    const FusedTiling tiling = choose_fused_tiling(c, B, S, kv24, scored, mp != nullptr, n_expected);
    FusedDecodeArgs f;
    RCCHK(fill_fused_decode_args(c, f, tiling, B, S, Tmax, steps_hint, d_lengths, d_shortlist, d_n_sl, eos_id, d_out_ids, d_out_len,
                                 d_align, align_out, d_scores, kv24, mp));
    return admit_and_launch_fused(c, f, B, S, kv24, slot, clk);
  }
  return decode_stepwise(c, B, S, R, Tmax, d_shortlist, eos_id, d_out_ids, d_out_len, d_align, d_scores, steps_hint, mp != nullptr);
}

}  // namespace

namespace {
// Staging for the alignment rows of a pinned asynchronous translate: sized ONCE for the largest batch
// the context takes at this limit factor (a buffer that grows batch by batch frees and allocates device
// memory under the other contexts' streams, and hipFree waits for the device).
size_t align_staging_bytes(const slimt_hip_ctx *ctx, size_t B, size_t S, size_t Tmax, float limit_factor) {
  const size_t t_max = (size_t)(limit_factor * (float)ctx->max_S) + 1;
  const size_t worst = ctx->max_M * t_max * 4;
  return std::max(worst <= ((size_t)256 << 20) ? worst : 0, B * Tmax * S * 4);
}

constexpr uint64_t kShortlistMagic = 0xF11A48D5013417F5ull;  // Shortlist.hh:40

// hash_combine over uint64 words from header.frequent on (Shortlist.cc:66-73,
// Utils.hh:47-67 with libstdc++'s identity std::hash<uint64_t>)
uint64_t shortlist_checksum(const unsigned char *blob, size_t size) {
  uint64_t seed = 0;
  for (size_t i = 16; i + 8 <= size; i += 8) {
    uint64_t v;
    std::memcpy(&v, blob + i, 8);
    seed ^= v + 0x9e3779b9ull + (seed << 6) + (seed >> 2);
  }
  return seed;
}

// bitmaps start zeroed and every generate call leaves them zeroed
int shortlist_scratch(DevBuf &buf, const slimt_hip_shortlist *sl, hipStream_t st) {
  const size_t need = shortlist_scratch_bytes((int)sl->source_vocab, (int)sl->target_vocab);
  if (buf.bytes < need) {
    HIPCHK(buf.reserve(need));
    HIPCHK(hipMemsetAsync(buf.p, 0, buf.bytes, st));
  }
  return 0;
}

void shortlist_args(const slimt_hip_shortlist *sl, const uint32_t *d_ids, const uint32_t *d_len,
                    size_t B, size_t S, uint32_t *d_out, uint32_t *d_n, ShortlistArgs &a) {
  a.w2o = sl->w2o.as<unsigned long long>();
  a.lists = sl->lists.as<uint32_t>();
  a.frequent = sl->frequent;
  a.shared = sl->shared ? 1 : 0;
  a.src_vocab = (int)sl->source_vocab;
  a.tgt_vocab = (int)sl->target_vocab;
  a.ids = d_ids;
  a.lengths = d_len;
  a.B = (int)B;
  a.S = (int)S;
  a.out = d_out;
  a.n_out = d_n;
}

// A caller's host shortlist of n ids in ctx->shortlist, where the kernels read it.
int upload_shortlist_if_changed(slimt_hip_ctx *ctx, const uint32_t *ids, size_t n) {
  if (!n || (ctx->sl_host.size() == n && std::memcmp(ctx->sl_host.data(), ids, n * 4) == 0)) return 0;
  hipStream_t st = ctx->stream;
  ctx->sl_host.clear();  // until the upload has succeeded the device copy is nobody's
  HIPCHK(hipMemcpyAsync(ctx->shortlist.p, ids, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));  // (the caller's array may be pageable: the copy is staged; done once per shortlist)
  ctx->sl_host.assign(ids, ids + n);
  return 0;
}

// The generator's arguments for the batch's list in ctx->shortlist, its count in ctx->n_sl_dev, on the context's scratch.
// n_lists > 1 (a merged launch, one list per sub-batch inside the encoder launch): that many counts, and no scratch -- the
// bitmaps in global memory are the two-kernel generator's. Launching and reading the count back are the caller's.
int generated_shortlist_args(slimt_hip_ctx *ctx, const slimt_hip_shortlist *sl, const uint32_t *d_ids, const uint32_t *d_len,
                             size_t B, size_t S, ShortlistArgs &a, size_t n_lists = 1) {
  ctx->sl_host.clear();  // ctx->shortlist no longer holds what translate_host uploaded last
  HIPCHK(ctx->n_sl_dev.reserve(4 * n_lists));
  if (n_lists == 1) RCCHK(shortlist_scratch(ctx->sl_scratch, sl, ctx->stream));
  shortlist_args(sl, d_ids, d_len, B, S, ctx->shortlist.as<uint32_t>(), ctx->n_sl_dev.as<uint32_t>(), a);
  if (n_lists == 1) a.scratch = ctx->sl_scratch.as<uint32_t>();
  return 0;
}

int check_generator(const slimt_hip_ctx *ctx, const slimt_hip_shortlist *sl) {
  const slimt_hip_model *m = ctx->model;
  if (sl->device != m->device) return fail(-1, "shortlist and context are on different devices");
  if (sl->target_vocab != (size_t)m->V)
    return fail(-1, "shortlist target vocabulary %zu != model vocabulary %d", sl->target_vocab, m->V);
  return 0;
}

// Model::forward's order (Model.cc:117-120): the batch's shortlist first -- generated on ctx's
// stream into ctx->shortlist -- then translate_device with it. Arrays the device can read.
int translate_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const uint32_t *d_src_ids,
                        const uint32_t *d_lengths, size_t B, size_t S, float limit_factor, uint32_t eos_id,
                        uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align, int steps_hint,
                        float *align_out) {
  const slimt_hip_model *m = ctx->model;
  hipStream_t st = ctx->stream;
  ShortlistArgs a;
  RCCHK(generated_shortlist_args(ctx, sl, d_src_ids, d_lengths, B, S, a));
  // the count also goes to a pinned word: what this context's PREVIOUS shortlist held is the host's
  // estimate of this one's size (a batch's shortlist is sized on the device; the host only picks
  // the decoder variant by it)
  uint32_t *hint = reinterpret_cast<uint32_t *>(ctx->n_finished_host) + 1;
  const size_t n_hint = *hint;
  void *hint_dev = nullptr;
  if (hipHostGetDevicePointer(&hint_dev, hint, 0) == hipSuccess) a.n_out_host = static_cast<uint32_t *>(hint_dev);
  const bool lean = persistent_path(ctx, S);
  // With the 64-row encoder the generator runs INSIDE the encoder launch, by the workgroup that starts first
  // (encode_tall.hip): as a launch of its own -- one workgroup -- it waited ~0.5 ms for a CU behind the
  // other batches' persistent kernels (47 us alone). Same ids, same count, same consumers.
  const bool fold = env().shortlist_fold;
  // (the persistent encoders of sentences up to 64 tokens: 64-row / 32-row tiles at D = 256, D = 512; the
  // per-sentence kernel for 65..128 tokens keeps the two-kernel generator)
  const bool in_launch = fold && lean && fused_encoder_chosen(ctx, (int)B, (int)S) &&
                         shortlist_in_launch_lds_bytes(a.src_vocab, a.tgt_vocab) <= 64 * 1024;
  if (!in_launch) HIPCHK(launch_shortlist_generate(a, st));
  if (lean)  // the size stays on the device: capacity V, actual count read by the kernels
    return translate_device(ctx, d_src_ids, d_lengths, ctx->shortlist.as<uint32_t>(), B, S,
                            (size_t)m->V, limit_factor, eos_id, d_out_ids, d_out_len, d_align,
                            steps_hint, ctx->n_sl_dev.as<uint32_t>(), align_out, n_hint, in_launch ? &a : nullptr);
  uint32_t n = 0;  // stage kernels are sized on the host: one 4-byte read-back
  HIPCHK(hipMemcpyAsync(&n, ctx->n_sl_dev.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return translate_device(ctx, d_src_ids, d_lengths, ctx->shortlist.as<uint32_t>(), B, S, n,
                          limit_factor, eos_id, d_out_ids, d_out_len, d_align, steps_hint);
}

// One batch with a listed shortlist, every array and option in device memory: slimt_hip_translate_device behind its guard,
// and a batch of slimt_hip_translate_many_device that goes on its own.
int translate_device_batch(slimt_hip_ctx *ctx, const BatchOptions &user, const uint32_t *d_src_ids, const uint32_t *d_lengths,
                           size_t B, size_t S, const uint32_t *d_shortlist, size_t n_shortlist, float limit_factor,
                           uint32_t eos_id, uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align, int steps_hint) {
  if (!ctx || !d_src_ids || !d_lengths || !d_out_ids || !d_out_len) return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  if (n_shortlist > (size_t)ctx->model->V) return fail(-1, "shortlist larger than the vocabulary");
  if (n_shortlist && !d_shortlist) return fail(-1, "shortlist is NULL");
  HIPCHK(hipSetDevice(ctx->model->device));
  options_in_place(ctx, user);
  return translate_device(ctx, d_src_ids, d_lengths, d_shortlist, B, S, n_shortlist, limit_factor,
                          eos_id, d_out_ids, d_out_len, d_align, steps_hint);
}
}  // namespace

extern "C" int slimt_hip_translate_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids,
                                          const uint32_t *d_lengths, size_t B, size_t S,
                                          const uint32_t *d_shortlist, size_t n_shortlist,
                                          float limit_factor, uint32_t eos_id,
                                          uint32_t *d_out_ids, uint32_t *d_out_len,
                                          float *d_align, int steps_hint) {
  CallOptions opt(ctx, 1);
  RCCHK(opt.rc);
  return translate_device_batch(ctx, opt.user[0], d_src_ids, d_lengths, B, S, d_shortlist, n_shortlist, limit_factor, eos_id,
                                d_out_ids, d_out_len, d_align, steps_hint);
}

namespace {
// Model::forward on host buffers: validate, queue H2D + kernels + D2H on the ctx stream.
// gen (nullable): the batch's lexical shortlist is generated on the device (Model.cc:117-120; shortlist / n_shortlist are
// then not used): no host shortlist, no upload, no synchronisation in the asynchronous form.
// user: the batch's options as the caller gave them, host memory: staged here into ctx->call.dev.
int translate_host(slimt_hip_ctx *ctx, slimt_hip_shortlist *gen, const BatchOptions &user, const uint32_t *src_ids,
                   const uint32_t *lengths, size_t B, size_t S, const uint32_t *shortlist, size_t n_shortlist, float limit_factor,
                   uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *align, bool wait,
                   const uint32_t *row_src = nullptr) {
  if (!ctx || !src_ids || !lengths || !out_ids || !out_len) return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  // a fan-out call (opened by the entry point): R = N rows named by row_src; every output, option and staging below is per
  // row, the ids and lengths per source
  CallState &call = ctx->call;
  const bool fanout = call.fanout;
  if (fanout && !row_src) return fail(-1, "null argument");
  const size_t R = fanout ? (size_t)call.rows : B;
  StageClock hclk;
  const slimt_hip_model *m = ctx->model;
  uint32_t vmax = (uint32_t)m->V;
  if (gen) {
    RCCHK(check_generator(ctx, gen));
    vmax = (uint32_t)std::min((size_t)m->V, gen->source_vocab);
  } else {
    if (n_shortlist > (size_t)m->V) return fail(-1, "shortlist larger than the vocabulary");
    if (n_shortlist && !shortlist) return fail(-1, "shortlist is NULL");
  }
  for (size_t i = 0; i < B * S; ++i)
    if (src_ids[i] >= vmax) return fail(-1, "token id %u out of range", src_ids[i]);
  for (size_t i = 0; !gen && i < n_shortlist; ++i)
    if (shortlist[i] >= (uint32_t)m->V) return fail(-1, "shortlist id %u out of range", shortlist[i]);
  for (size_t i = 0; i < B; ++i)
    if (lengths[i] > S) return fail(-1, "length %u > S", lengths[i]);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  const size_t Tmax = std::max<size_t>(1, (size_t)(limit_factor * (float)S));
  // the shortlist is read at random every step: it stays on the device, uploaded when it changes
  if (!gen) RCCHK(upload_shortlist_if_changed(ctx, shortlist, n_shortlist));
  // the kernels for either shortlist, on arrays the device can read; the alignment rows go to ctx->align and, where
  // align_out is given, from there to the caller's pinned array
  auto run = [&](const uint32_t *d_ids, const uint32_t *d_len, uint32_t *d_out, uint32_t *d_ol, int steps_hint,
                 float *align_out) {
    float *d_align = align ? ctx->align.as<float>() : nullptr;
    if (gen)
      return translate_generated(ctx, gen, d_ids, d_len, B, S, limit_factor, eos_id, d_out, d_ol, d_align, steps_hint,
                                 align_out);
    return translate_device(ctx, d_ids, d_len, ctx->shortlist.as<uint32_t>(), B, S, n_shortlist, limit_factor, eos_id, d_out,
                            d_ol, d_align, steps_hint, nullptr, align_out);
  };
  // Asynchronous callers with PINNED buffers (hipHostMalloc / slimt_hip_host_alloc): the persistent
  // kernels read the ids / lengths and write tokens, lengths and alignments in host memory themselves
  // -- no copy on either side. Copies are what a host pipeline stalls on: an asynchronous copy
  // of stream A sits in a DMA queue behind copies that wait for stream B's kernels (measured with the
  // Service: 12 contexts of equal batches ran strictly one after the other, 3.7 M tok/s).
  const bool persistent = persistent_path(ctx, S);
  hclk.lap(0);
  // (a forced call: the caller's host prefix, checked; it and a sampled call's host keys pinned in place or staged)
  call.dev = {};
  RCCHK(stage_options(ctx, 1, &user, &R, &Tmax, &call.dev));
  if (fanout) {  // (the rows' sources: a pinned array in place, a pageable one staged in device memory)
    call.row_src = static_cast<const uint32_t *>(host_device_view(row_src));
    if (!call.row_src) {
      HIPCHK(ctx->fo_stage.reserve(R * 4));
      HIPCHK(hipMemcpyAsync(ctx->fo_stage.p, row_src, R * 4, hipMemcpyHostToDevice, st));
      call.row_src = ctx->fo_stage.as<uint32_t>();
    }
  }
  if (call.consensus) {  // (a fan-out call with the selection armed: utility [R] f64, then best [B] u32, staged on the device)
    HIPCHK(ctx->cs_stage.reserve(R * 8 + B * 4));
    call.cs_dev_util = ctx->cs_stage.as<double>();
    call.cs_dev_best = reinterpret_cast<uint32_t *>(ctx->cs_stage.as<char>() + R * 8);
  }
  if (call.beam) {  // (a beam call: totals [R], then token scores [R][Tmax] where asked for, staged on the device)
    HIPCHK(ctx->bm_stage.reserve(R * 4 + (call.bm_scores ? R * Tmax * 4 : 0)));
    call.bm_dev_totals = ctx->bm_stage.as<float>();
    call.bm_dev_scores = call.bm_scores ? ctx->bm_stage.as<float>() + R : nullptr;
    if (call.bm_scores) HIPCHK(hipMemsetAsync(call.bm_dev_scores, 0, R * Tmax * 4, st));
  }
  float *const scores = user.scores;  // (a scored call: the caller's [B][Tmax] host array)
  if (!wait && persistent) {
    void *v_ids = host_device_view(src_ids), *v_len = host_device_view(lengths), *v_out = host_device_view(out_ids),
         *v_ol = host_device_view(out_len), *v_al = align ? host_device_view(align) : nullptr;
    void *v_sc = scores ? host_device_view(scores) : nullptr;
    hclk.lap(6);
    if (v_ids && v_len && v_out && v_ol && (!align || v_al) && (!scores || v_sc)) {
      call.dev.scores = static_cast<float *>(v_sc);
      // alignment rows (Model.cc:84-108) are staged in device memory and leave for the host once per
      // sentence, as whole 16-byte stores when its loop ends: written row by row across PCIe from
      // inside the step loop they cost the Service 28 % (12.9 against 17.9 M tok/s)
      if (align) HIPCHK(ctx->align.reserve(align_staging_bytes(ctx, B, S, Tmax, limit_factor)));
      return run(static_cast<const uint32_t *>(v_ids), static_cast<const uint32_t *>(v_len), static_cast<uint32_t *>(v_out),
                 static_cast<uint32_t *>(v_ol), (int)Tmax, static_cast<float *>(v_al));
    }
  }
  HIPCHK(ctx->out_ids.reserve(R * Tmax * 4));
  if (align) HIPCHK(ctx->align.reserve(R * Tmax * S * 4));
  if (scores) {
    HIPCHK(ctx->sc_stage.reserve(R * Tmax * 4));
    call.dev.scores = ctx->sc_stage.as<float>();
  }
  HIPCHK(hipMemcpyAsync(ctx->ids.p, src_ids, B * S * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->lengths.p, lengths, B * 4, hipMemcpyHostToDevice, st));
  // asynchronous callers never read back inside the loop: a fixed step budget (the persistent
  // decoder still leaves its loop as soon as every sentence has emitted EOS)
  RCCHK(run(ctx->ids.as<uint32_t>(), ctx->lengths.as<uint32_t>(), ctx->out_ids.as<uint32_t>(), ctx->out_len.as<uint32_t>(),
            wait ? 0 : (int)Tmax, nullptr));
  HIPCHK(hipMemcpyAsync(out_ids, ctx->out_ids.p, R * Tmax * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out_len, ctx->out_len.p, R * 4, hipMemcpyDeviceToHost, st));
  if (align) HIPCHK(hipMemcpyAsync(align, ctx->align.p, R * Tmax * S * 4, hipMemcpyDeviceToHost, st));
  if (scores) HIPCHK(hipMemcpyAsync(scores, ctx->sc_stage.p, R * Tmax * 4, hipMemcpyDeviceToHost, st));
  if (call.consensus) {
    HIPCHK(hipMemcpyAsync(call.cs_util, call.cs_dev_util, R * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(call.cs_best, call.cs_dev_best, B * 4, hipMemcpyDeviceToHost, st));
  }
  if (call.beam) {
    HIPCHK(hipMemcpyAsync(call.bm_totals, call.bm_dev_totals, R * 4, hipMemcpyDeviceToHost, st));
    if (call.bm_scores) HIPCHK(hipMemcpyAsync(call.bm_scores, call.bm_dev_scores, R * Tmax * 4, hipMemcpyDeviceToHost, st));
  }
  if (wait) RCCHK(slimt_hip_ctx_synchronize(ctx));  // sleeps on a blocking-sync event (a worker per context: no spinning)
  return 0;
}
}  // namespace

extern "C" int slimt_hip_translate(slimt_hip_ctx *ctx, const uint32_t *src_ids,
                                   const uint32_t *lengths, size_t B, size_t S,
                                   const uint32_t *shortlist, size_t n_shortlist,
                                   float limit_factor, uint32_t eos_id, uint32_t *out_ids,
                                   uint32_t *out_len, float *align) {
  CallOptions opt(ctx, 1);
  RCCHK(opt.rc);
  return translate_host(ctx, nullptr, opt.user[0], src_ids, lengths, B, S, shortlist, n_shortlist, limit_factor, eos_id,
                        out_ids, out_len, align, true);
}

extern "C" int slimt_hip_translate_async(slimt_hip_ctx *ctx, const uint32_t *src_ids,
                                         const uint32_t *lengths, size_t B, size_t S,
                                         const uint32_t *shortlist, size_t n_shortlist,
                                         float limit_factor, uint32_t eos_id, uint32_t *out_ids,
                                         uint32_t *out_len, float *align) {
  CallOptions opt(ctx, 1);
  RCCHK(opt.rc);
  return translate_host(ctx, nullptr, opt.user[0], src_ids, lengths, B, S, shortlist, n_shortlist, limit_factor, eos_id,
                        out_ids, out_len, align, false);
}

// ---- fan-out: N decoder rows over B sources encoded once (include/slimt_hip.h, slimt_hip_translate_fanout*) ------------
// translate_host / translate_device above with the outputs and options counted by row (CallOptions::open_fanout);
// decode_fanout.hip has the attention that looks a row's source up.
namespace {
int translate_fanout_host(slimt_hip_ctx *ctx, slimt_hip_shortlist *gen, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                          size_t S, const uint32_t *row_src, size_t N, const uint32_t *shortlist, size_t n_shortlist,
                          float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *align, bool wait) {
  CallOptions opt(ctx, 1, true);
  // (what needs no context is checked first: these refusals say what is wrong with the arguments, context or not)
  if (N == 0) return fail(-1, "fan-out: no rows (N = 0)");
  if (!row_src) return fail(-1, "null argument");
  for (size_t r = 0; r < N; ++r)
    if (row_src[r] >= B) return fail(-1, "fan-out: row %zu names source %u, the call has %zu", r, row_src[r], B);
  if (!ctx) return fail(-1, "null argument");
  RCCHK(opt.rc);
  RCCHK(opt.open_fanout(N));
  return translate_host(ctx, gen, opt.user[0], src_ids, lengths, B, S, shortlist, n_shortlist, limit_factor, eos_id, out_ids,
                        out_len, align, wait, row_src);
}
}  // namespace

extern "C" int slimt_hip_translate_fanout(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                          const uint32_t *row_src, size_t N, const uint32_t *shortlist, size_t n_shortlist,
                                          float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *align) {
  return translate_fanout_host(ctx, nullptr, src_ids, lengths, B, S, row_src, N, shortlist, n_shortlist, limit_factor, eos_id,
                               out_ids, out_len, align, true);
}

extern "C" int slimt_hip_translate_fanout_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                                size_t S, const uint32_t *row_src, size_t N, const uint32_t *shortlist,
                                                size_t n_shortlist, float limit_factor, uint32_t eos_id, uint32_t *out_ids,
                                                uint32_t *out_len, float *align) {
  return translate_fanout_host(ctx, nullptr, src_ids, lengths, B, S, row_src, N, shortlist, n_shortlist, limit_factor, eos_id,
                               out_ids, out_len, align, false);
}

extern "C" int slimt_hip_translate_fanout_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                                          const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                                          const uint32_t *row_src, size_t N, float limit_factor, uint32_t eos_id,
                                                          uint32_t *out_ids, uint32_t *out_len, float *align) {
  if (!shortlist) return fail(-1, "null argument");
  return translate_fanout_host(ctx, shortlist, src_ids, lengths, B, S, row_src, N, nullptr, 0, limit_factor, eos_id, out_ids,
                               out_len, align, false);
}

extern "C" int slimt_hip_translate_fanout_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths,
                                                 size_t B, size_t S, const uint32_t *d_row_src, size_t N,
                                                 const uint32_t *d_shortlist, size_t n_shortlist, float limit_factor,
                                                 uint32_t eos_id, uint32_t *d_out_ids, uint32_t *d_out_len, float *d_align,
                                                 int steps_hint) {
  CallOptions opt(ctx, 1, true);
  RCCHK(opt.rc);
  RCCHK(opt.open_fanout(N));
  if (!ctx || !d_src_ids || !d_lengths || !d_row_src || !d_out_ids || !d_out_len) return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  if (n_shortlist > (size_t)ctx->model->V) return fail(-1, "shortlist larger than the vocabulary");
  if (n_shortlist && !d_shortlist) return fail(-1, "shortlist is NULL");
  HIPCHK(hipSetDevice(ctx->model->device));
  ctx->call.row_src = d_row_src;
  ctx->call.cs_dev_best = ctx->call.cs_best;  // (device memory, like the other outputs: best [B], utility [N])
  ctx->call.cs_dev_util = ctx->call.cs_util;
  options_in_place(ctx, opt.user[0]);  // (scores [N][Tmax], prefix and keys by row)
  return translate_device(ctx, d_src_ids, d_lengths, d_shortlist, B, S, n_shortlist, limit_factor, eos_id, d_out_ids, d_out_len,
                          d_align, steps_hint);
}

// ---- beam search with n-best output (include/slimt_hip.h, slimt_hip_translate_beam*) --------------------
// A fan-out call of B beam rows whose steps end in beam_select.hip's selection (beam_steps above); the outputs count
// [B][beam] hypotheses, best first.
namespace {
int beam_arguments(int beam, int length_mode) {
  if (beam < 1 || beam > SLIMT_HIP_MAX_BEAM) return fail(-1, "beam: a beam of %d is not in 1..%d", beam, SLIMT_HIP_MAX_BEAM);
  if (length_mode != 0 && length_mode != 1) return fail(-1, "beam: length_mode %d is not 0 (sum) or 1 (mean per token)", length_mode);
  return 0;
}

int translate_beam_host(slimt_hip_ctx *ctx, slimt_hip_shortlist *gen, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                        size_t S, int beam, int length_mode, const uint32_t *shortlist, size_t n_shortlist, float limit_factor,
                        uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *totals, float *token_scores, float *align,
                        bool wait) {
  CallOptions opt(ctx, 1);
  // (what needs no context is checked first: these refusals say what is wrong with the arguments, context or not)
  RCCHK(beam_arguments(beam, length_mode));
  if (!ctx || !totals) return fail(-1, "null argument");
  RCCHK(opt.rc);
  RCCHK(opt.open_beam(B, beam, length_mode));
  ctx->call.bm_totals = totals;
  ctx->call.bm_scores = token_scores;
  return translate_host(ctx, gen, opt.user[0], src_ids, lengths, B, S, shortlist, n_shortlist, limit_factor, eos_id, out_ids,
                        out_len, align, wait, ctx->bm_row_src.data());
}
}  // namespace

extern "C" int slimt_hip_translate_beam(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                        int beam, int length_mode, const uint32_t *shortlist, size_t n_shortlist,
                                        float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *totals,
                                        float *token_scores, float *align) {
  return translate_beam_host(ctx, nullptr, src_ids, lengths, B, S, beam, length_mode, shortlist, n_shortlist, limit_factor, eos_id,
                             out_ids, out_len, totals, token_scores, align, true);
}

extern "C" int slimt_hip_translate_beam_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                              size_t S, int beam, int length_mode, const uint32_t *shortlist, size_t n_shortlist,
                                              float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len,
                                              float *totals, float *token_scores, float *align) {
  return translate_beam_host(ctx, nullptr, src_ids, lengths, B, S, beam, length_mode, shortlist, n_shortlist, limit_factor, eos_id,
                             out_ids, out_len, totals, token_scores, align, false);
}

extern "C" int slimt_hip_translate_beam_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist, const uint32_t *src_ids,
                                                        const uint32_t *lengths, size_t B, size_t S, int beam, int length_mode,
                                                        float limit_factor, uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len,
                                                        float *totals, float *token_scores, float *align) {
  if (!shortlist) return fail(-1, "null argument");
  return translate_beam_host(ctx, shortlist, src_ids, lengths, B, S, beam, length_mode, nullptr, 0, limit_factor, eos_id, out_ids,
                             out_len, totals, token_scores, align, false);
}

extern "C" int slimt_hip_translate_beam_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths, size_t B,
                                               size_t S, int beam, int length_mode, const uint32_t *d_shortlist, size_t n_shortlist,
                                               float limit_factor, uint32_t eos_id, uint32_t *d_out_ids, uint32_t *d_out_len,
                                               float *d_totals, float *d_token_scores, float *d_align, int steps_hint) {
  CallOptions opt(ctx, 1);
  RCCHK(beam_arguments(beam, length_mode));
  if (!ctx || !d_src_ids || !d_lengths || !d_out_ids || !d_out_len || !d_totals) return fail(-1, "null argument");
  RCCHK(opt.rc);
  RCCHK(opt.open_beam(B, beam, length_mode));
  RCCHK(check_batch(ctx, B, S));
  if (n_shortlist > (size_t)ctx->model->V) return fail(-1, "shortlist larger than the vocabulary");
  if (n_shortlist && !d_shortlist) return fail(-1, "shortlist is NULL");
  HIPCHK(hipSetDevice(ctx->model->device));
  const size_t R = B * (size_t)beam;
  HIPCHK(ctx->fo_stage.reserve(R * 4));  // (the rows' sources, written once)
  HIPCHK(hipMemcpyAsync(ctx->fo_stage.p, ctx->bm_row_src.data(), R * 4, hipMemcpyHostToDevice, ctx->stream));
  ctx->call.row_src = ctx->fo_stage.as<uint32_t>();
  ctx->call.bm_dev_totals = d_totals;
  ctx->call.bm_dev_scores = d_token_scores;
  return translate_device(ctx, d_src_ids, d_lengths, d_shortlist, B, S, n_shortlist, limit_factor, eos_id, d_out_ids, d_out_len,
                          d_align, steps_hint);
}

// One selection over the caller's arrays: host pointers, stateless, waits (like slimt_hip_sample_truncated).
extern "C" int slimt_hip_beam_step(const float *logits, size_t B, int beam, size_t N, const uint32_t *ids, const float *totals_in,
                                   const uint32_t *flags_in, uint32_t eos_id, uint32_t *parent, uint32_t *token, float *token_score,
                                   float *totals_out, uint32_t *flags_out) {
  RCCHK(beam_arguments(beam, 0));
  if (!logits || !totals_in || !flags_in || !parent || !token || !token_score || !totals_out || !flags_out || !B || !N)
    return fail(-1, "bad argument");
  if (N >= (size_t)slimt_hip::kBeamMaxN) return fail(-1, "beam: an output layer of %zu columns (2^20 or more)", N);
  const size_t R = B * (size_t)beam;
  if (B > 0x7fffffffu / (size_t)beam) return fail(-1, "beam_step: more than %d rows", 0x7fffffff);
  for (size_t r = 0; r < R; ++r) {
    if (flags_in[r] > slimt_hip::kBeamFinished) return fail(-1, "beam_step: flag %u of row %zu is not 0 (dead), 1 (live) or 2 (finished)", flags_in[r], r);
    if (flags_in[r] == slimt_hip::kBeamLive && !std::isfinite(totals_in[r])) return fail(-1, "beam_step: the total of live row %zu is not finite", r);
    if (flags_in[r] == slimt_hip::kBeamFinished && totals_in[r] != totals_in[r]) return fail(-1, "beam_step: the total of finished row %zu is NaN", r);
  }
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(R * N * 4));
  HIPCHK(t.b.reserve(N * 4));
  HIPCHK(t.c.reserve(2 * R * 4));
  HIPCHK(t.d.reserve(5 * R * 4));
  HIPCHK(hipMemcpyAsync(t.a.p, logits, R * N * 4, hipMemcpyHostToDevice, st));
  if (ids) HIPCHK(hipMemcpyAsync(t.b.p, ids, N * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.c.p, totals_in, R * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.c.as<char>() + R * 4, flags_in, R * 4, hipMemcpyHostToDevice, st));
  BeamSelectArgs a;
  a.logits = t.a.as<float>();
  a.B = (int)B;
  a.k = beam;
  a.N = (int)N;
  a.ids = ids ? t.b.as<uint32_t>() : nullptr;
  a.eos = eos_id;
  a.totals_in = t.c.as<float>();
  a.flags_in = t.c.as<uint32_t>() + R;
  uint32_t *o = t.d.as<uint32_t>();
  a.parent = o;
  a.token = o + R;
  a.token_score = reinterpret_cast<float *>(o + 2 * R);
  a.totals_out = reinterpret_cast<float *>(o + 3 * R);
  a.flags_out = o + 4 * R;
  HIPCHK(launch_beam_select(a, st));
  HIPCHK(hipMemcpyAsync(parent, o, R * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(token, o + R, R * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(token_score, o + 2 * R, R * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(totals_out, o + 3 * R, R * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(flags_out, o + 4 * R, R * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// ---- several batches in one launch pair (include/slimt_hip.h, slimt_hip_translate_many*) ----------------------------
namespace {
constexpr size_t kMergeAlign = 32;  // a sub-batch starts at a multiple of the widest decoder tile (kernels.h, MergeOut)

bool merge_supported(const slimt_hip_ctx *c, size_t rows, size_t S) {
  const slimt_hip_model *m = c->model;
  return fused_decoder_allowed(c) && c->decode_mode != 6 && fused_decode_supported(m->D, m->F, m->H, m->Ld) &&
         fused_encoder_chosen(c, (int)rows, (int)S);
}

// the sub-batches' tables. align_staging (nullable): the alignment rows are staged there (global sentence order) and
// each batch's `align` (a device view of the caller's pinned array) is where they go when a sentence ends
// align: sub-batches start at multiples of it -- the decoder's tile where every sub-batch has its own output layer; with
// ONE layer for all of them (one shortlist pointer and size, or the full vocabulary) they follow each other densely
// whatever it says
int build_merge_plan(const slimt_hip_ctx *c, const slimt_hip_batch *b, size_t n, size_t S, size_t Tmax, float limit_factor,
                     int steps_hint, float *align_staging, MergePlan &mp, size_t &rows, size_t align = kMergeAlign) {
  mp.n = (int)n;
  rows = 0;
  mp.dense = true;
  for (size_t j = 1; j < n; ++j)
    if (b[j].shortlist != b[0].shortlist || b[j].n_shortlist != b[0].n_shortlist) mp.dense = false;
  if (!env().merge_dense) mp.dense = false;  // A/B
  if (mp.dense) align = 1;
  size_t stage_at = 0;  // floats of alignment staging handed out so far (16-byte pieces: the decoder copies whole quads)
  for (size_t j = 0; j < n; ++j) {
    const size_t Sj = b[j].S ? b[j].S : S;
    if (Sj > S) return fail(-1, "batch %zu is padded to %zu tokens, the launch to %zu", j, Sj, S);
    const size_t Tj = std::max<size_t>(1, (size_t)(limit_factor * (float)Sj));  // Model.cc:159-161 on this batch's length
    if (!b[j].src_ids || !b[j].lengths || !b[j].out_ids || !b[j].out_len) return fail(-1, "batch %zu: null array", j);
    if (b[j].B == 0) return fail(-1, "batch %zu is empty", j);
    if (b[j].n_shortlist > (size_t)c->model->V) return fail(-1, "batch %zu: shortlist larger than the vocabulary", j);
    if (b[j].n_shortlist && !b[j].shortlist) return fail(-1, "batch %zu: shortlist is NULL", j);
    if ((b[j].n_shortlist != 0) != (b[0].n_shortlist != 0))
      return fail(-1, "merged batches: all with a shortlist or all with the full vocabulary");
    MergeIn &in = mp.in[j];
    MergeOut &o = mp.out[j];
    in.ids = b[j].src_ids;
    in.lengths = b[j].lengths;
    in.first = (int)rows;
    in.n = (int)b[j].B;
    in.S = (int)Sj;
    o.lengths = b[j].lengths;
    o.out_ids = b[j].out_ids;
    o.out_len = b[j].out_len;
    if (b[j].align && align_staging) {
      o.align = align_staging + stage_at;
      o.align_out = b[j].align;
      stage_at += (b[j].B * Tj * Sj + 3) / 4 * 4;
    } else {
      o.align = b[j].align;
      o.align_out = nullptr;
    }
    o.shortlist = b[j].n_shortlist ? b[j].shortlist : nullptr;
    o.first = (int)rows;
    o.n = (int)b[j].B;
    o.N = b[j].n_shortlist ? (int)b[j].n_shortlist : c->model->V;
    o.job = 0;
    o.S = (int)Sj;
    o.Tmax = (int)Tj;
    o.max_steps = steps_hint > 0 ? std::min(steps_hint, (int)Tj) : (int)Tj;
    if (b[j].n_shortlist) {  // one packing job per distinct (pointer, size)
      int job = -1;
      for (int q = 0; q < mp.n_jobs; ++q)
        if (mp.jobs[q].idx == b[j].shortlist && mp.jobs[q].N == (int)b[j].n_shortlist) job = q;
      if (job < 0) {
        job = mp.n_jobs++;
        mp.jobs[job].idx = b[j].shortlist;
        mp.jobs[job].N = (int)b[j].n_shortlist;
        mp.max_N = std::max(mp.max_N, (int)b[j].n_shortlist);
      }
      o.job = job;
    }
    rows += (b[j].B + align - 1) / align * align;
  }
  return 0;
}

// the decoder tile of a merged launch: always 16 sentences -- where an unmerged call would take the 32-sentence tiling (decode
// mode 3, or mode 0 with an output layer of more than 16k columns) a merged one runs the 16-sentence tiling instead
// (translate_device; decode_fused.hip compiles the merged paths into the 16-row tilings only)
constexpr size_t kMergeTile = 16;

// Batch j of a host _many_ call as its front checks it: the arrays, B, and the batch's padded length against the launch's;
// with `values` every id (< vmax) and every length as well.
int check_host_batch(const slimt_hip_batch &b, size_t j, size_t S, uint32_t vmax, bool values) {
  if (!b.src_ids || !b.lengths || !b.out_ids || !b.out_len || b.B == 0) return fail(-1, "batch %zu: null array or empty", j);
  const size_t Sj = b.S ? b.S : S;
  if (Sj > S) return fail(-1, "batch %zu is padded to %zu tokens, the launch to %zu", j, Sj, S);
  for (size_t i = 0; values && i < b.B * Sj; ++i)
    if (b.src_ids[i] >= vmax) return fail(-1, "batch %zu: token id %u out of range", j, b.src_ids[i]);
  for (size_t i = 0; values && i < b.B; ++i)
    if (b.lengths[i] > Sj) return fail(-1, "batch %zu: length %u > S", j, b.lengths[i]);
  return 0;
}

// A host batch as the kernels read and write it: dev = b with the device views of its pinned arrays (the shortlist stays
// the caller's). false: one of the arrays is pageable.
bool pinned_batch_view(const slimt_hip_batch &b, slimt_hip_batch &dev) {
  dev = b;
  dev.src_ids = static_cast<const uint32_t *>(host_device_view(b.src_ids));
  dev.lengths = static_cast<const uint32_t *>(host_device_view(b.lengths));
  dev.out_ids = static_cast<uint32_t *>(host_device_view(b.out_ids));
  dev.out_len = static_cast<uint32_t *>(host_device_view(b.out_len));
  dev.align = b.align ? static_cast<float *>(host_device_view(b.align)) : nullptr;
  return dev.src_ids && dev.lengths && dev.out_ids && dev.out_len && (!b.align || dev.align);
}
}  // namespace

extern "C" size_t slimt_hip_translate_many_rows(const size_t *B, size_t n_batches) {
  size_t rows = 0;
  for (size_t j = 0; B && j < n_batches; ++j) rows += (B[j] + kMergeAlign - 1) / kMergeAlign * kMergeAlign;
  return rows;
}

extern "C" int slimt_hip_translate_many_device(slimt_hip_ctx *ctx, const slimt_hip_batch *batches, size_t n_batches, size_t S,
                                               float limit_factor, uint32_t eos_id, int steps_hint) {
  CallOptions opt(ctx, n_batches);
  RCCHK(opt.rc);
  if (!ctx || !batches || n_batches == 0) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(ctx->model->device));
  const size_t Tmax = std::max<size_t>(1, (size_t)(limit_factor * (float)S));
  MergePlan mp;
  size_t rows = 0;
  const bool mergeable = n_batches > 1 && n_batches <= (size_t)kMaxMerge && !ctx->call.truncated;  // (truncated: batch by batch)
  if (mergeable)
    RCCHK(build_merge_plan(ctx, batches, n_batches, S, Tmax, limit_factor, steps_hint, nullptr, mp, rows, kMergeTile));
  for (size_t j = 0; mergeable && j < n_batches; ++j) mp.opt[j] = opt.user[j];  // (device memory: addressed where it is)
  if (mergeable && rows <= ctx->max_B && rows * S <= ctx->max_M && S <= ctx->max_S && merge_supported(ctx, rows, S))
    return translate_device(ctx, batches[0].src_ids, batches[0].lengths, batches[0].shortlist, rows, S, (size_t)mp.max_N,
                            limit_factor, eos_id, batches[0].out_ids, batches[0].out_len, batches[0].align, steps_hint, nullptr,
                            nullptr, 0, nullptr, &mp);
  for (size_t j = 0; j < n_batches; ++j) {  // batch by batch, in order, on the same stream
    const slimt_hip_batch &b = batches[j];
    // (a call that comes this way must give what a merged launch gives: the launch's step budget is the longest batch's,
    // and a shorter batch takes at most its own Tmax_j -- build_merge_plan's rule. With the budget as given, a sentence
    // of a shorter batch that had not ended by Tmax_j went on counting steps: out_len[b] > Tmax_j, past its row of out_ids.)
    const size_t Sj = b.S ? b.S : S, Tj = std::max<size_t>(1, (size_t)(limit_factor * (float)Sj));
    const int hint = steps_hint > 0 ? std::min(steps_hint, (int)Tj) : steps_hint;
    RCCHK(translate_device_batch(ctx, opt.user[j], b.src_ids, b.lengths, b.B, Sj, b.shortlist, b.n_shortlist, limit_factor,
                                 eos_id, b.out_ids, b.out_len, b.align, hint));
  }
  return 0;
}

extern "C" int slimt_hip_translate_many_async(slimt_hip_ctx *ctx, const slimt_hip_batch *batches, size_t n_batches, size_t S,
                                              float limit_factor, uint32_t eos_id) {
  CallOptions opt(ctx, n_batches);
  RCCHK(opt.rc);
  if (!ctx || !batches || n_batches == 0) return fail(-1, "null argument");
  const slimt_hip_model *m = ctx->model;
  HIPCHK(hipSetDevice(m->device));
  const size_t Tmax = std::max<size_t>(1, (size_t)(limit_factor * (float)S));
  bool merged = n_batches > 1 && n_batches <= (size_t)kMaxMerge && S <= ctx->max_S && !ctx->call.truncated;
  slimt_hip_batch dev[kMaxMerge];
  MergePlan mp;  // (its opt[j].scores: the device views of the pinned score arrays)
  bool any_align = false;
  size_t rows = 0;
  for (size_t j = 0; merged && j < n_batches; ++j) {
    const slimt_hip_batch &b = batches[j];
    if (b.shortlist != batches[0].shortlist || b.n_shortlist != batches[0].n_shortlist) merged = false;  // one host shortlist
    // (ids and lengths only while a merged launch is still possible: else each batch's translate_host checks its own)
    RCCHK(check_host_batch(b, j, S, (uint32_t)m->V, merged));
    if (!pinned_batch_view(b, dev[j])) merged = false;
    float *const sc = opt.user[j].scores;
    if (sc && !(mp.opt[j].scores = static_cast<float *>(host_device_view(sc)))) merged = false;
    any_align = any_align || b.align != nullptr;
    rows += b.B;  // (one shortlist for all: the sub-batches follow each other densely)
  }
  auto fits = [&](size_t r) { return r <= ctx->max_B && r * S <= ctx->max_M; };
  auto batch_by_batch = [&]() {
    for (size_t j = 0; j < n_batches; ++j) {
      const slimt_hip_batch &b = batches[j];
      RCCHK(translate_host(ctx, nullptr, opt.user[j], b.src_ids, b.lengths, b.B, b.S ? b.S : S, b.shortlist, b.n_shortlist,
                           limit_factor, eos_id, b.out_ids, b.out_len, b.align, false));
    }
    return 0;
  };
  merged = merged && fits(rows) && merge_supported(ctx, rows, S);
  if (!merged) return batch_by_batch();
  const size_t n_sl = batches[0].n_shortlist;
  const uint32_t *shortlist = batches[0].shortlist;
  if (n_sl > (size_t)m->V) return fail(-1, "shortlist larger than the vocabulary");
  if (n_sl && !shortlist) return fail(-1, "shortlist is NULL");
  for (size_t i = 0; i < n_sl; ++i)
    if (shortlist[i] >= (uint32_t)m->V) return fail(-1, "shortlist id %u out of range", shortlist[i]);
  RCCHK(upload_shortlist_if_changed(ctx, shortlist, n_sl));  // (translate_host: uploaded when it changes)
  if (any_align) HIPCHK(ctx->align.reserve(align_staging_bytes(ctx, rows, S, Tmax, limit_factor)));
  for (size_t j = 0; j < n_batches; ++j) {
    dev[j].shortlist = n_sl ? ctx->shortlist.as<uint32_t>() : nullptr;
    dev[j].n_shortlist = n_sl;
  }
  RCCHK(build_merge_plan(ctx, dev, n_batches, S, Tmax, limit_factor, 0, any_align ? ctx->align.as<float>() : nullptr, mp, rows));
  // (SLIMT_MERGE_DENSE=0: the plan counted its rows again, every sub-batch from a multiple of kMergeAlign -- more than the
  // dense sum checked above; a launch that no longer fits the workspace goes batch by batch, nothing of it is queued yet)
  if (!fits(rows) || !merge_supported(ctx, rows, S)) return batch_by_batch();
  RCCHK(stage_options(ctx, batches, n_batches, S, limit_factor, opt.user.data(), mp.opt));
  return translate_device(ctx, dev[0].src_ids, dev[0].lengths, dev[0].shortlist, rows, S, (size_t)mp.max_N, limit_factor, eos_id,
                          dev[0].out_ids, dev[0].out_len, any_align ? ctx->align.as<float>() : nullptr, (int)Tmax, nullptr,
                          any_align ? dev[0].align : nullptr, 0, nullptr, &mp);
}

extern "C" int slimt_hip_host_alloc(size_t bytes, void **out) {
  if (!out) return fail(-1, "null argument");
  *out = nullptr;
  g_hip_called.store(true, std::memory_order_relaxed);
  HIPCHK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return 0;
}

extern "C" int slimt_hip_host_free(void *p) {
  if (p) HIPCHK(hipHostFree(p));
  return 0;
}

extern "C" int slimt_hip_encode(slimt_hip_ctx *ctx, const uint32_t *src_ids,
                                const uint32_t *lengths, size_t B, size_t S, float *embed_out,
                                float *layer_out, float *enc_out) {
  if (!ctx || !src_ids || !lengths) return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  const slimt_hip_model *m = ctx->model;
  for (size_t i = 0; i < B * S; ++i)
    if (src_ids[i] >= (uint32_t)m->V) return fail(-1, "token id %u out of range", src_ids[i]);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->ids.p, src_ids, B * S * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->lengths.p, lengths, B * 4, hipMemcpyHostToDevice, st));
  RCCHK(encode_device(ctx, (int)B, (int)S, embed_out, layer_out));
  if (enc_out)
    HIPCHK(hipMemcpyAsync(enc_out, ctx->x0.p, B * S * (size_t)m->D * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_encode_embedded(slimt_hip_ctx *ctx, const float *embedding,
                                         const uint32_t *lengths, size_t B, size_t S, float *enc_out) {
  if (!ctx || !embedding || !lengths || !enc_out) return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  const slimt_hip_model *m = ctx->model;
  for (size_t i = 0; i < B; ++i)
    if (lengths[i] > S) return fail(-1, "length %u > S", lengths[i]);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  const size_t nbytes = B * S * (size_t)m->D * 4;
  HIPCHK(hipMemcpyAsync(ctx->x0.p, embedding, nbytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->lengths.p, lengths, B * 4, hipMemcpyHostToDevice, st));
  RCCHK(encode_device(ctx, (int)B, (int)S, nullptr, nullptr, nullptr, nullptr, nullptr, true));
  HIPCHK(hipMemcpyAsync(enc_out, ctx->x0.p, nbytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_decode_begin_from(slimt_hip_ctx *ctx, const float *encoder_out,
                                           const uint32_t *lengths, size_t B, size_t S,
                                           const uint32_t *shortlist, size_t n_shortlist) {
  if (!ctx || !encoder_out || !lengths) return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  const slimt_hip_model *m = ctx->model;
  for (size_t i = 0; i < B; ++i)
    if (lengths[i] > S) return fail(-1, "length %u > S", lengths[i]);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->x0.p, encoder_out, B * S * (size_t)m->D * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->lengths.p, lengths, B * 4, hipMemcpyHostToDevice, st));
  ctx->B = (int)B;
  ctx->S = (int)S;
  ctx->have_encoder_out = true;
  ctx->kv_ready = false;  // the cross-attention K/V of THIS encoder output are computed below
  ctx->decode_ready = false;
  return slimt_hip_decode_begin(ctx, shortlist, n_shortlist);
}

extern "C" int slimt_hip_decode_begin(slimt_hip_ctx *ctx, const uint32_t *shortlist,
                                      size_t n_shortlist) {
  if (!ctx) return fail(-1, "ctx is NULL");
  const slimt_hip_model *m = ctx->model;
  if (n_shortlist > (size_t)m->V) return fail(-1, "shortlist larger than the vocabulary");
  if (n_shortlist && !shortlist) return fail(-1, "shortlist is NULL");
  for (size_t i = 0; i < n_shortlist; ++i)
    if (shortlist[i] >= (uint32_t)m->V) return fail(-1, "shortlist id %u out of range", shortlist[i]);
  HIPCHK(hipSetDevice(m->device));
  if (n_shortlist) {
    ctx->sl_host.clear();  // ctx->shortlist no longer holds what translate_host uploaded last
    HIPCHK(hipMemcpyAsync(ctx->shortlist.p, shortlist, n_shortlist * 4, hipMemcpyHostToDevice,
                          ctx->stream));
  }
  RCCHK(decode_setup(ctx, n_shortlist));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

static int decode_step_impl(slimt_hip_ctx *ctx, const uint32_t *prev, const float *states_in,
                            float *logits, float *attn, float *states) {
  if (!ctx || !logits) return fail(-1, "null argument");
  if (!ctx->decode_ready) return fail(-1, "decode_step before decode_begin");
  const slimt_hip_model *m = ctx->model;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  const size_t B = (size_t)ctx->B, S = (size_t)ctx->S, D = (size_t)m->D;
  if (prev) {
    for (size_t i = 0; i < B; ++i)
      if (prev[i] >= (uint32_t)m->V) return fail(-1, "token id %u out of range", prev[i]);
    HIPCHK(hipMemcpyAsync(ctx->prev.p, prev, B * 4, hipMemcpyHostToDevice, st));
  }
  if (states_in)  // the caller's SSRU cells (Decoder::step's `states`, Transformer.cc:120-128)
    HIPCHK(hipMemcpyAsync(ctx->state.p, states_in, (size_t)m->Ld * B * D * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_embed_decoder(embed_args(ctx), ctx->prev.as<uint32_t>(), (int)B, prev == nullptr,
                              ctx->dx.as<float>(), st));
  if (attn) HIPCHK(ctx->attn_dbg.reserve(B * (size_t)m->H * S * 4));
  RCCHK(decoder_layers(ctx, nullptr, 0, nullptr, attn ? ctx->attn_dbg.as<float>() : nullptr));
  const AffineW &out = output_layer(ctx);
  const size_t N = (size_t)out.w.N;
  HIPCHK(ctx->logits.reserve(B * N * 4));
  DGemmArgs g;
  g.B = (int)B;
  g.D = m->D;
  g.a = decoder_out_rows(ctx);
  g.w = out.w;
  g.y = ctx->logits.as<float>();
  g.ldy = (int)N;
  HIPCHK(launch_dgemm(g, EPI_PLAIN, st));
  HIPCHK(hipMemcpyAsync(logits, ctx->logits.p, B * N * 4, hipMemcpyDeviceToHost, st));
  if (attn)
    HIPCHK(hipMemcpyAsync(attn, ctx->attn_dbg.p, B * (size_t)m->H * S * 4, hipMemcpyDeviceToHost, st));
  if (states)
    HIPCHK(hipMemcpyAsync(states, ctx->state.p, (size_t)m->Ld * B * D * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_decode_step(slimt_hip_ctx *ctx, const uint32_t *prev, float *logits,
                                     float *attn, float *states) {
  return decode_step_impl(ctx, prev, nullptr, logits, attn, states);
}

extern "C" int slimt_hip_decode_step_states(slimt_hip_ctx *ctx, const uint32_t *prev,
                                            const float *states_in, float *logits, float *attn,
                                            float *states_out) {
  if (!states_in) return fail(-1, "null argument");
  return decode_step_impl(ctx, prev, states_in, logits, attn, states_out);
}

// ---------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------
extern "C" int slimt_hip_profile_enable(slimt_hip_ctx *ctx, int kernel_id) {
  if (!ctx) return fail(-1, "ctx is NULL");
  if (kernel_id < 0 || kernel_id >= SLIMT_HIP_K_COUNT) return fail(-1, "bad kernel id %d", kernel_id);
  ctx->prof_kernel = kernel_id;
  return slimt_hip_profile_reset(ctx);
}

extern "C" int slimt_hip_profile_reset(slimt_hip_ctx *ctx) {
  if (!ctx) return fail(-1, "ctx is NULL");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->prof_used = 0;
  ctx->prof_macs = 0;
  ctx->prof_bytes = 0;
  return 0;
}

extern "C" int slimt_hip_profile_read(slimt_hip_ctx *ctx, uint64_t *launches, double *total_ms,
                                      double *int8_macs, double *weight_bytes) {
  if (!ctx) return fail(-1, "ctx is NULL");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  double ms = 0;
  for (size_t i = 0; i < ctx->prof_used; ++i) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, ctx->prof_events[i].first, ctx->prof_events[i].second));
    ms += t;
  }
  if (launches) *launches = ctx->prof_used;
  if (total_ms) *total_ms = ms;
  if (int8_macs) *int8_macs = ctx->prof_macs;
  if (weight_bytes) *weight_bytes = ctx->prof_bytes;
  return 0;
}

// Diagnostic occupancy trace of the persistent kernels (kernels.h, OccTrace)
extern "C" int slimt_hip_debug_occupancy_trace(void *device_buf, size_t capacity) {
  g_occ_trace.buf = static_cast<unsigned long long *>(device_buf);
  g_occ_trace.capacity = device_buf ? (unsigned)capacity : 0u;
  return 0;
}

// Diagnostic: wall-clock stamps (100 MHz ticks) at the phase boundaries of the
// persistent decoder, workgroup 0, decode step `step`. step < 0 disables.
extern "C" int slimt_hip_debug_decode_stamps(slimt_hip_ctx *ctx, int step, uint64_t *out,
                                             size_t n) {
  if (!ctx) return fail(-1, "ctx is NULL");
  HIPCHK(hipSetDevice(ctx->model->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (out && n && ctx->stamps.p) {
    if (n > 64) n = 64;
    HIPCHK(hipMemcpy(out, ctx->stamps.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  ctx->stamp_step = step;
  if (step >= 0) {
    HIPCHK(ctx->stamps.reserve(64 * sizeof(uint64_t)));
    HIPCHK(hipMemset(ctx->stamps.p, 0, 64 * sizeof(uint64_t)));
  }
  return 0;
}

// ---------------------------------------------------------------------------
// lexical shortlist (slimt/Shortlist.{hh,cc})
// ---------------------------------------------------------------------------
extern "C" int slimt_hip_shortlist_create(const void *blob, size_t blob_size, size_t source_vocab,
                                          size_t target_vocab, int shared, int check, int device,
                                          slimt_hip_shortlist **out) {
  if (!blob || !out) return fail(-1, "null argument");
  if (source_vocab == 0 || target_vocab == 0 || source_vocab > (1u << 22) || target_vocab > (1u << 22))
    return fail(-1, "bad vocabulary sizes %zu / %zu", source_vocab, target_vocab);
  if (shortlist_lds_bytes((int)source_vocab, (int)target_vocab) > 160 * 1024)
    return fail(-1, "vocabularies too large for the on-chip truth tables");
  uint64_t h[6];
  if (blob_size < sizeof(h))  // Shortlist.cc:49-51
    return fail(-1, "shortlist length too short to have a header: %zu", blob_size);
  const unsigned char *p = static_cast<const unsigned char *>(blob);
  std::memcpy(h, p, sizeof(h));
  if (h[0] != kShortlistMagic) return fail(-1, "incorrect magic in binary shortlist");  // :56
  const uint64_t n_off = h[4], n_ids = h[5];
  if (n_off > (1ull << 32) || n_ids > (1ull << 40)) return fail(-1, "implausible shortlist header");
  const uint64_t expected = sizeof(h) + n_off * 8 + n_ids * 4;  // :58-64
  if (expected != blob_size)
    return fail(-1, "shortlist header claims file size should be %llu but file is %zu",
                (unsigned long long)expected, blob_size);
  if (check && shortlist_checksum(p, blob_size) != h[1])  // :66-76
    return fail(-1, "checksum check failed: this binary shortlist is corrupted");
  if (n_off != source_vocab + 1)
    return fail(-1, "shortlist has %llu offsets, expected source vocabulary + 1 = %zu",
                (unsigned long long)n_off, source_vocab + 1);
  // content_check (Shortlist.cc:16-38), always: the kernel trusts these ranges
  const unsigned char *po = p + sizeof(h), *pl = po + n_off * 8;
  uint64_t prev = 0;
  for (uint64_t i = 0; i < n_off; ++i) {
    uint64_t v;
    std::memcpy(&v, po + 8 * i, 8);
    // the reference's check wants every offset but the last strictly inside (Shortlist.cc:18-21)
    if (v > n_ids || v < prev || (check && i + 1 < n_off && v >= n_ids))
      return fail(-1, "offset table not within shortlist size");
    prev = v;
  }
  if (prev != n_ids) return fail(-1, "word_to_offset != shortlist_size");
  for (uint64_t j = 0; j < n_ids; ++j) {
    uint32_t v;
    std::memcpy(&v, pl + 4 * j, 4);
    if (v >= target_vocab) return fail(-1, "shortlist indices are out of bounds");
  }
  HIPCHK(hipSetDevice(device));
  auto *sl = new slimt_hip_shortlist();
  sl->device = device;
  sl->frequent = h[2];
  sl->best = h[3];
  sl->source_vocab = source_vocab;
  sl->target_vocab = target_vocab;
  sl->shared = shared != 0;
  hipError_t e = sl->w2o.reserve(n_off * 8);
  if (e == hipSuccess) e = sl->lists.reserve(n_ids ? n_ids * 4 : 4);
  if (e == hipSuccess) e = sl->out.reserve(target_vocab * 4);
  if (e == hipSuccess) e = sl->n_out.reserve(4);
  if (e == hipSuccess) e = hipMemcpy(sl->w2o.p, po, n_off * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess && n_ids) e = hipMemcpy(sl->lists.p, pl, n_ids * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    slimt_hip_shortlist_destroy(sl);
    return fail((int)e, "shortlist upload: %s", hipGetErrorString(e));
  }
  *out = sl;
  return 0;
}

extern "C" int slimt_hip_shortlist_destroy(slimt_hip_shortlist *sl) {
  if (!sl) return 0;
  (void)hipSetDevice(sl->device);
  for (DevBuf *b : {&sl->w2o, &sl->lists, &sl->ids, &sl->lengths, &sl->out, &sl->n_out, &sl->scratch})
    b->release();
  delete sl;
  return 0;
}

extern "C" int slimt_hip_shortlist_info(const slimt_hip_shortlist *sl, uint64_t *frequent,
                                        uint64_t *best) {
  if (!sl) return fail(-1, "shortlist is NULL");
  if (frequent) *frequent = sl->frequent;
  if (best) *best = sl->best;
  return 0;
}

extern "C" int slimt_hip_shortlist_generate(slimt_hip_shortlist *sl, const uint32_t *src_ids,
                                            const uint32_t *lengths, size_t B, size_t S,
                                            uint32_t *out_ids, size_t *n_out) {
  if (!sl || !src_ids || !lengths || !out_ids || !n_out) return fail(-1, "null argument");
  if (B == 0 || S == 0) return fail(-1, "empty batch");
  if (B * S > (1u << 28)) return fail(-1, "batch too large");
  for (size_t b = 0; b < B; ++b) {
    if (lengths[b] > S) return fail(-1, "length %u > S", lengths[b]);
    for (size_t j = 0; j < lengths[b]; ++j)
      if (src_ids[b * S + j] >= sl->source_vocab)
        return fail(-1, "token id %u out of range", src_ids[b * S + j]);
  }
  // ShortlistGenerator::generate is const and is called by every Async worker on ONE shared
  // generator (Model.cc:117-120); this entry point stages through per-handle buffers, so
  // concurrent callers take turns (the _device variants use the caller's context instead)
  std::lock_guard<std::mutex> lock(sl->mu);
  HIPCHK(hipSetDevice(sl->device));
  HIPCHK(sl->ids.reserve(B * S * 4));
  HIPCHK(sl->lengths.reserve(B * 4));
  HIPCHK(hipMemcpy(sl->ids.p, src_ids, B * S * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(sl->lengths.p, lengths, B * 4, hipMemcpyHostToDevice));
  RCCHK(shortlist_scratch(sl->scratch, sl, nullptr));
  ShortlistArgs a;
  shortlist_args(sl, sl->ids.as<uint32_t>(), sl->lengths.as<uint32_t>(), B, S,
                 sl->out.as<uint32_t>(), sl->n_out.as<uint32_t>(), a);
  a.scratch = sl->scratch.as<uint32_t>();
  HIPCHK(launch_shortlist_generate(a, nullptr));
  uint32_t n = 0;
  HIPCHK(hipMemcpy(&n, sl->n_out.p, 4, hipMemcpyDeviceToHost));
  if (n > sl->target_vocab) return fail(-1, "shortlist kernel returned %u ids", n);
  if (n) HIPCHK(hipMemcpy(out_ids, sl->out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  *n_out = n;
  return 0;
}

extern "C" int slimt_hip_shortlist_generate_device(slimt_hip_shortlist *sl, slimt_hip_ctx *ctx,
                                                   const uint32_t *d_src_ids,
                                                   const uint32_t *d_lengths, size_t B, size_t S,
                                                   uint32_t *d_out_ids, uint32_t *d_n_out) {
  if (!sl || !ctx || !d_src_ids || !d_lengths || !d_out_ids || !d_n_out)
    return fail(-1, "null argument");
  if (B == 0 || S == 0) return fail(-1, "empty batch");
  if (sl->device != ctx->model->device) return fail(-1, "shortlist and context are on different devices");
  HIPCHK(hipSetDevice(sl->device));
  RCCHK(shortlist_scratch(ctx->sl_scratch, sl, ctx->stream));
  ShortlistArgs a;
  shortlist_args(sl, d_src_ids, d_lengths, B, S, d_out_ids, d_n_out, a);
  a.scratch = ctx->sl_scratch.as<uint32_t>();
  HIPCHK(launch_shortlist_generate(a, ctx->stream));
  return 0;
}

extern "C" int slimt_hip_translate_device_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl,
                                                    const uint32_t *d_src_ids,
                                                    const uint32_t *d_lengths, size_t B, size_t S,
                                                    float limit_factor, uint32_t eos_id,
                                                    uint32_t *d_out_ids, uint32_t *d_out_len,
                                                    float *d_align, int steps_hint) {
  CallOptions opt(ctx, 1);
  RCCHK(opt.rc);
  if (!ctx || !sl || !d_src_ids || !d_lengths || !d_out_ids || !d_out_len)
    return fail(-1, "null argument");
  RCCHK(check_batch(ctx, B, S));
  RCCHK(check_generator(ctx, sl));
  HIPCHK(hipSetDevice(ctx->model->device));
  options_in_place(ctx, opt.user[0]);
  return translate_generated(ctx, sl, d_src_ids, d_lengths, B, S, limit_factor, eos_id, d_out_ids, d_out_len,
                             d_align, steps_hint, nullptr);
}

// ---- merged launches whose batches each get THEIR lexical shortlist, generated inside the encoder launch ---------------
namespace {
// What a translate_many_generated call has beside its batches. dev[j]: batch j's options as the kernels address them (device
// memory, or the device views of pinned arrays; for the prefixes and keys also staged copies).
struct ManyGenerated {
  const BatchOptions *dev = nullptr;
  // the asynchronous entry point: the same batches with the caller's HOST pointers, and host[j], their options as the caller
  // gave them -- what the batch-by-batch fallback hands to translate_host, which knows when the kernels can use pinned
  // arrays in place
  const slimt_hip_batch *host_batches = nullptr;
  const BatchOptions *host = nullptr;
  bool stage_align = false;  // the alignment rows are staged in ctx->align (the batches' `align` are pinned views)
  int steps_hint = 0;
};

// dev: the batches with arrays the device can read (device memory, or the device views of pinned arrays); the merged launch
// when it is possible, else batch by batch through translate_generated
int translate_many_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const slimt_hip_batch *dev, size_t n, size_t S,
                             float limit_factor, uint32_t eos_id, const ManyGenerated &o) {
  const slimt_hip_model *m = ctx->model;
  const size_t Tmax = std::max<size_t>(1, (size_t)(limit_factor * (float)S));
  const size_t V = (size_t)m->V;
  const int steps_hint = o.steps_hint;
  const bool stage_align = o.stage_align;
  size_t rows = 0;
  bool any_align = false;
  uint32_t *hint = reinterpret_cast<uint32_t *>(ctx->n_finished_host) + 1;  // (translate_generated: the previous shortlist's size)
  const size_t n_hint = *hint;
  for (size_t j = 0; j < n; ++j) {
    rows += (dev[j].B + kMergeTile - 1) / kMergeTile * kMergeTile;
    any_align = any_align || dev[j].align != nullptr;
  }
  const bool fold = env().shortlist_fold;
  const bool merged = n > 1 && n <= (size_t)kMaxMerge && !ctx->call.truncated && S <= ctx->max_S && rows <= ctx->max_B && rows * S <= ctx->max_M &&
                      merge_supported(ctx, rows, S) && fold &&
                      shortlist_in_launch_lds_bytes((int)sl->source_vocab, (int)sl->target_vocab) <= 64 * 1024;
  if (!merged && o.host_batches) {
    for (size_t j = 0; j < n; ++j) {
      const slimt_hip_batch &b = o.host_batches[j];
      RCCHK(translate_host(ctx, sl, o.host[j], b.src_ids, b.lengths, b.B, b.S ? b.S : S, nullptr, 0, limit_factor, eos_id,
                           b.out_ids, b.out_len, b.align, false));
    }
    return 0;
  }
  if (!merged) {
    for (size_t j = 0; j < n; ++j) {
      const slimt_hip_batch &b = dev[j];
      const size_t Sj = b.S ? b.S : S, Tj = std::max<size_t>(1, (size_t)(limit_factor * (float)Sj));
      float *staging = nullptr;
      if (b.align && stage_align) {
        HIPCHK(ctx->align.reserve(align_staging_bytes(ctx, b.B, Sj, Tj, limit_factor)));
        staging = ctx->align.as<float>();
      }
      RCCHK(check_batch(ctx, b.B, Sj));
      options_in_place(ctx, o.dev[j]);
      RCCHK(translate_generated(ctx, sl, b.src_ids, b.lengths, b.B, Sj, limit_factor, eos_id, b.out_ids, b.out_len,
                                staging ? staging : b.align, steps_hint > 0 ? std::min(steps_hint, (int)Tj) : (stage_align ? (int)Tj : 0),
                                staging ? b.align : nullptr));
    }
    return 0;
  }
  ctx->sl_host.clear();  // ctx->shortlist no longer holds what translate_host uploaded last
  HIPCHK(ctx->shortlist.reserve(n * V * 4));  // job j's ids at j * V, its count at n_sl_dev[j]
  ShortlistArgs a;
  RCCHK(generated_shortlist_args(ctx, sl, dev[0].src_ids, dev[0].lengths, dev[0].B, S, a, (size_t)kMaxMerge));
  slimt_hip_batch plan[kMaxMerge];
  for (size_t j = 0; j < n; ++j) {
    plan[j] = dev[j];
    plan[j].shortlist = ctx->shortlist.as<uint32_t>() + j * V;
    plan[j].n_shortlist = V;  // the capacity; the kernels read the count
  }
  if (any_align && stage_align) HIPCHK(ctx->align.reserve(align_staging_bytes(ctx, rows, S, Tmax, limit_factor)));
  MergePlan mp;
  RCCHK(build_merge_plan(ctx, plan, n, S, Tmax, limit_factor, steps_hint, any_align && stage_align ? ctx->align.as<float>() : nullptr, mp, rows, kMergeTile));
  for (size_t j = 0; j < n; ++j) mp.opt[j] = o.dev[j];
  void *hint_dev = nullptr;
  if (hipHostGetDevicePointer(&hint_dev, hint, 0) == hipSuccess) a.n_out_host = static_cast<uint32_t *>(hint_dev);
  return translate_device(ctx, plan[0].src_ids, plan[0].lengths, ctx->shortlist.as<uint32_t>(), rows, S, V, limit_factor, eos_id,
                          plan[0].out_ids, plan[0].out_len, any_align ? (stage_align ? ctx->align.as<float>() : plan[0].align) : nullptr,
                          steps_hint > 0 ? steps_hint : (int)Tmax, ctx->n_sl_dev.as<uint32_t>(),
                          any_align && stage_align ? plan[0].align : nullptr, n_hint, &a, &mp);
}
}  // namespace

extern "C" int slimt_hip_translate_many_device_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const slimt_hip_batch *batches,
                                                         size_t n_batches, size_t S, float limit_factor, uint32_t eos_id,
                                                         int steps_hint) {
  CallOptions opt(ctx, n_batches);
  RCCHK(opt.rc);
  if (!ctx || !sl || !batches || n_batches == 0) return fail(-1, "null argument");
  RCCHK(check_generator(ctx, sl));
  for (size_t j = 0; j < n_batches; ++j) {
    const slimt_hip_batch &b = batches[j];
    if (!b.src_ids || !b.lengths || !b.out_ids || !b.out_len || b.B == 0) return fail(-1, "batch %zu: null array or empty", j);
    if ((b.S ? b.S : S) > S) return fail(-1, "batch %zu is padded to %zu tokens, the launch to %zu", j, b.S, S);
  }
  HIPCHK(hipSetDevice(ctx->model->device));
  ManyGenerated o;
  o.steps_hint = steps_hint;
  o.dev = opt.user.data();  // (device memory: addressed where it is)
  return translate_many_generated(ctx, sl, batches, n_batches, S, limit_factor, eos_id, o);
}

extern "C" int slimt_hip_translate_many_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const slimt_hip_batch *batches,
                                                        size_t n_batches, size_t S, float limit_factor, uint32_t eos_id) {
  CallOptions opt(ctx, n_batches);
  RCCHK(opt.rc);
  if (!ctx || !sl || !batches || n_batches == 0) return fail(-1, "null argument");
  RCCHK(check_generator(ctx, sl));
  const slimt_hip_model *m = ctx->model;
  HIPCHK(hipSetDevice(m->device));
  const uint32_t vmax = (uint32_t)std::min((size_t)m->V, sl->source_vocab);
  slimt_hip_batch dev[kMaxMerge];
  BatchOptions dev_opt[kMaxMerge];  // (scores: the device views of the pinned arrays; prefixes and keys: those, or staged copies)
  bool pinned = n_batches <= (size_t)kMaxMerge;
  for (size_t j = 0; j < n_batches; ++j) {  // (every batch in full before anything is queued)
    RCCHK(check_host_batch(batches[j], j, S, vmax, true));
    if (!pinned) continue;
    if (!pinned_batch_view(batches[j], dev[j])) pinned = false;
    float *const sc = opt.user[j].scores;
    if (sc && !(dev_opt[j].scores = static_cast<float *>(host_device_view(sc)))) pinned = false;
  }
  if (pinned) {
    RCCHK(stage_options(ctx, batches, n_batches, S, limit_factor, opt.user.data(), dev_opt));
    ManyGenerated o;
    o.host_batches = batches;
    o.host = opt.user.data();
    o.dev = dev_opt;
    o.stage_align = true;
    return translate_many_generated(ctx, sl, dev, n_batches, S, limit_factor, eos_id, o);
  }
  for (size_t j = 0; j < n_batches; ++j) {  // pageable arrays, or too many batches: one by one through the copying path
    const slimt_hip_batch &b = batches[j];
    RCCHK(translate_host(ctx, sl, opt.user[j], b.src_ids, b.lengths, b.B, b.S ? b.S : S, nullptr, 0, limit_factor, eos_id,
                         b.out_ids, b.out_len, b.align, false));
  }
  return 0;
}

extern "C" int slimt_hip_translate_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl, const uint32_t *src_ids,
                                             const uint32_t *lengths, size_t B, size_t S, float limit_factor,
                                             uint32_t eos_id, uint32_t *out_ids, uint32_t *out_len, float *align) {
  CallOptions opt(ctx, 1);
  RCCHK(opt.rc);
  if (!sl) return fail(-1, "null argument");
  return translate_host(ctx, sl, opt.user[0], src_ids, lengths, B, S, nullptr, 0, limit_factor, eos_id, out_ids, out_len, align,
                        true);
}

extern "C" int slimt_hip_translate_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *sl,
                                                   const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                                   size_t S, float limit_factor, uint32_t eos_id,
                                                   uint32_t *out_ids, uint32_t *out_len, float *align) {
  CallOptions opt(ctx, 1);
  RCCHK(opt.rc);
  if (!sl) return fail(-1, "null argument");
  return translate_host(ctx, sl, opt.user[0], src_ids, lengths, B, S, nullptr, 0, limit_factor, eos_id, out_ids, out_len, align,
                        false);
}

// ---- teacher-forced scoring: every target position in one tall pass (include/slimt_hip.h, slimt_hip_score*) -----------
// score_tall.hip has the kernels and the reasoning. Here: the context's encoder for the batch with the f32 float(accS) K/V
// cache of the stage path (encode_device / decode_setup), then per chunk of whole sentences the decoder layers as tall
// GEMMs (launch_gemm: 128-row tiles from 1024 rows on, bit-identical to the step-wise dgemm) around the scan, the
// attention and the scoring output layer. None of it reads or consumes what set_scores / set_target_prefix / set_sampling
// armed: these entry points open no CallOptions.
namespace {
constexpr size_t kScoreChunkRows = 8192;         // rows of a chunk (whole sentences; a single sentence may exceed it)
constexpr size_t kScoreMaxT = 65536;             // longest target
constexpr size_t kScoreMaxRows = (size_t)1 << 24;  // largest B * T of a call

// a buffer a queued kernel may still read: the context is synchronised before the old block is freed
int score_reserve(slimt_hip_ctx *c, DevBuf &buf, size_t bytes) {
  if (bytes <= buf.bytes && buf.p) return 0;
  if (buf.p) HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(buf.reserve(bytes));
  return 0;
}

// NR: the target rows of the call -- its B sentences, or the N candidates of a candidate call
int score_check(const slimt_hip_ctx *c, size_t B, size_t S, size_t n_sl, size_t T, size_t NR) {
  RCCHK(check_batch(c, B, S));
  const slimt_hip_model *m = c->model;
  if (T == 0) return fail(-1, "score: T is 0 (a target row needs at least one column)");
  if (T > kScoreMaxT || NR > kScoreMaxRows || NR * T > kScoreMaxRows)
    return fail(-1, "score: %zu x %zu target positions exceed the limits (T <= %zu, B * T <= %zu)", NR, T, kScoreMaxT, kScoreMaxRows);
  if (n_sl > (size_t)m->V) return fail(-1, "shortlist larger than the vocabulary");
  if (m->kv_format == 3)
    return fail(-1, "score: the model is set to K/V cache format 3 (the literal cross-attention order); the scoring pass "
                    "has the hoisted order only");
  if (!score_supported(m->D, m->H) || S > 128)
    return fail(-1, "score: no scoring kernels for D = %d with %d heads, S = %zu", m->D, m->H, S);
  return 0;
}

// The alternatives armed on a context (slimt_hip_ctx_set_score_alternatives) are taken by the score entry point that comes
// next, whether it succeeds or not; translate calls construct none of these.
struct AltCall {
  ScoreAltArgs a;  // k = 0: the call is not armed
  explicit AltCall(slimt_hip_ctx *ctx) {
    if (!ctx || !ctx->alt_next_k) return;
    a.k = (int)ctx->alt_next_k;
    a.ids = ctx->alt_next_ids;
    a.scores = ctx->alt_next_scores;
    a.rank = ctx->alt_next_rank;
    ctx->alt_next_k = 0;
    ctx->alt_next_ids = nullptr;
    ctx->alt_next_scores = nullptr;
    ctx->alt_next_rank = nullptr;
  }
};

// memory a kernel can write: device, managed or pinned host memory as the runtime knows it
bool device_visible(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged;
}

// the alternatives of a _device call (k = 0: unarmed): each array given is memory the kernels can write
int alternatives_device_visible(const ScoreAltArgs &alt) {
  if (!alt.k) return 0;
  const void *arr[3] = {alt.ids, alt.scores, alt.rank};
  const char *name[3] = {"alt_ids", "alt_scores", "rank"};
  for (int i = 0; i < 3; ++i)
    if (arr[i] && !device_visible(arr[i]))
      return fail(-1, "score alternatives: %s is not memory the device can write (the arrays are of the kind of scores)", name[i]);
  return 0;
}

// alt (k = 0: unarmed): ids / scores / rank are addresses the kernels write
// d_cand (nullable): a candidate call -- the targets, scores, alignment and alternatives are those of N candidates, candidate
// c over source d_cand[c]; the B sources are encoded once. nullptr: target row b belongs to source b (N is not read)
int score_device(slimt_hip_ctx *c, const uint32_t *d_ids, const uint32_t *d_lengths, size_t B, size_t S,
                 const uint32_t *d_shortlist, size_t n_sl, const uint32_t *d_tgt, const uint32_t *d_tlen, size_t T,
                 float *d_scores, float *d_align, const ScoreAltArgs &alt, const uint32_t *d_cand = nullptr, size_t N = 0) {
  const size_t NR = d_cand ? N : B;  // target sentences
  const slimt_hip_model *m = c->model;
  hipStream_t st = c->stream;
  const size_t D = (size_t)m->D, F = (size_t)m->F;
  // the batch through the context's encoder; K / V as the stage path caches them (decode_setup), the output layer packed
  if (d_ids != c->ids.as<uint32_t>()) HIPCHK(hipMemcpyAsync(c->ids.p, d_ids, B * S * 4, hipMemcpyDefault, st));
  if (d_lengths != c->lengths.as<uint32_t>())
    HIPCHK(hipMemcpyAsync(c->lengths.p, d_lengths, B * 4, hipMemcpyDefault, st));
  if (n_sl && d_shortlist != c->shortlist.as<uint32_t>()) {
    c->sl_host.clear();  // ctx->shortlist no longer holds what a host call uploaded last
    HIPCHK(hipMemcpyAsync(c->shortlist.p, d_shortlist, n_sl * 4, hipMemcpyDefault, st));
  }
  RCCHK(encode_device(c, (int)B, (int)S, nullptr, nullptr));
  RCCHK(decode_setup(c, n_sl));
  c->decode_ready = false;  // (the step-wise API starts from its own decode_begin)
  const AffineW &out = output_layer(c);
  // workspace of one chunk: four f32 row buffers, two int8 ones, FFN1's int8 output, the target columns
  const size_t spc = std::max<size_t>(1, kScoreChunkRows / T);  // sentences per chunk
  const size_t ws_rows = std::min(NR, spc) * T;
  auto up = [](size_t n) { return (n + 255) / 256 * 256; };
  const size_t b_f32 = up(ws_rows * D * 4), b_i8 = up(ws_rows * D), b_f8 = up(ws_rows * F), b_col = up(ws_rows * 4);
  RCCHK(score_reserve(c, c->score_ws, 4 * b_f32 + 2 * b_i8 + b_f8 + b_col));
  char *p = c->score_ws.as<char>();
  float *x = reinterpret_cast<float *>(p);
  float *f = reinterpret_cast<float *>(p + b_f32);
  float *wx = reinterpret_cast<float *>(p + 2 * b_f32);
  float *h = reinterpret_cast<float *>(p + 3 * b_f32);
  int8_t *att8 = reinterpret_cast<int8_t *>(p + 4 * b_f32);
  int8_t *y8 = att8 + b_i8;
  int8_t *f8 = y8 + b_i8;
  int *tcol = reinterpret_cast<int *>(f8 + b_f8);
  const float *kv = c->kv.as<float>();
  const size_t M = B * S;
  for (size_t b0 = 0; b0 < NR; b0 += spc) {
    ScoreRows rows;
    rows.b0 = (int)b0;
    rows.nb = (int)std::min(spc, NR - b0);
    rows.T = (int)T;
    rows.tgt_ids = d_tgt;
    rows.tgt_len = d_tlen;
    const int R = rows.nb * rows.T;
    HIPCHK(launch_score_embed(embed_args(c), rows, n_sl ? c->shortlist.as<uint32_t>() : nullptr, out.w.N, x, tcol, st));
    for (int l = 0; l < m->Ld; ++l) {
      const DecLayerW &L = m->dec[(size_t)l];
      // SSRU (Modules.cc:190-235): both gate GEMMs over all rows, then the scan
      RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_DEC, L.rnn_f, x, R, f, 0));
      RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_DEC, L.rnn_w, x, R, wx, 0));
      {
        ProfScope ps(c, SLIMT_HIP_K_SSRU, 0, 0);
        HIPCHK(launch_score_scan(rows, m->D, x, f, wx, L.rnn_ln.scale.as<float>(), L.rnn_ln.bias.as<float>(), 1e-6f, h, st));
      }
      // Attention::forward (Modules.cc:287-319): Q projection, then every query row of a sentence over its cached K / V
      RCCHK(run_affine_f32(c, SLIMT_HIP_K_GEMM_DEC, L.attn.q, h, R, f, 0));
      ScoreAttnArgs a;
      a.rows = rows;
      a.D = m->D; a.H = m->H; a.S = (int)S;
      a.q = f;
      a.k = kv + (size_t)(2 * l) * M * D;
      a.v = kv + (size_t)(2 * l + 1) * M * D;
      a.ldv = m->D;
      a.uk = L.attn.k.w.u;
      a.uv = L.attn.v.w.u;
      a.pbk = L.attn.k.w.pb;
      a.pbv = L.attn.v.w.pb;
      a.lengths = c->lengths.as<uint32_t>();
      a.alpha = 1.0f / std::sqrt(static_cast<float>(m->D / m->H));
      a.out_i8 = att8;
      a.a_quant_out = L.attn.o.w.a_quant;
      a.align = l + 1 == m->Ld ? d_align : nullptr;  // alignment = last layer (Transformer.cc:165-174)
      {
        ProfScope ps(c, SLIMT_HIP_K_ATTN_DEC, 0, 0);
        if (d_cand) {
          ScoreCandAttnArgs ca;
          ca.a = a;
          ca.cand_src = d_cand;
          ca.B = (int)B;
          HIPCHK(launch_score_candidates_attention(ca, st));
        } else {
          HIPCHK(launch_score_attention(a, st));
        }
      }
      // O projection + residual, LayerNorm (Modules.cc:308-316); FFN (Modules.cc:251-257)
      RCCHK(run_affine_res(c, SLIMT_HIP_K_GEMM_DEC, L.attn.o, nullptr, att8, R, h, wx, 0));
      HIPCHK(launch_layer_norm_q(wx, L.attn.ln.scale.as<float>(), L.attn.ln.bias.as<float>(), 1e-6f, R, m->D, wx, y8,
                                 L.ffn1.w.a_quant, st));
      RCCHK(run_affine_relu_q(c, SLIMT_HIP_K_GEMM_DEC, L.ffn1, nullptr, y8, R, L.ffn2.w.a_quant, f8, 0));
      RCCHK(run_affine_res(c, SLIMT_HIP_K_GEMM_DEC, L.ffn2, nullptr, f8, R, wx, x, 0));
      const bool last = l + 1 == m->Ld;  // the last layer's rows leave quantised for the output layer as well
      HIPCHK(launch_layer_norm_q(x, L.ffn_ln.scale.as<float>(), L.ffn_ln.bias.as<float>(), 1e-6f, R, m->D, x,
                                 last ? y8 : nullptr, last ? out.w.a_quant : 0.0f, st));
    }
    ScoreOutArgs o;
    o.rows = rows;
    o.a_i8 = y8;
    o.w = out.w;
    o.tcol = tcol;
    o.scores = d_scores;
    {
      ProfScope ps(c, SLIMT_HIP_K_LOGITS, (double)R * out.w.K * out.w.N, gemm_bytes(out.w));
      if (alt.k) {
        ScoreAltArgs al = alt;
        al.sl = n_sl ? c->shortlist.as<uint32_t>() : nullptr;
        HIPCHK(launch_score_alternatives(o, al, st));
      } else {
        HIPCHK(launch_score_output(o, st));
      }
    }
  }
  return 0;
}

// Host buffers: validated, then read / written in place where pinned, else bracketed by copies on the context's stream.
// gen (nullable): the batch's lexical shortlist is generated on the device first (shortlist / n_sl are then not used).
// candidates: a candidate call (slimt_hip_score_candidates*) -- tgt_ids, tgt_len, scores, align and the alternatives are
// those of N candidates, cand_src [N] their sources. Otherwise target row b belongs to source b (cand_src / N are not read).
int score_host(slimt_hip_ctx *ctx, slimt_hip_shortlist *gen, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
               size_t S, const uint32_t *shortlist, size_t n_sl, const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T,
               float *scores, float *align, bool wait, bool candidates = false, const uint32_t *cand_src = nullptr,
               size_t N = 0) {
  AltCall ac(ctx);
  if (ctx && T == 0) return fail(-1, "score: T is 0 (a target row needs at least one column)");
  if (!ctx || !src_ids || !lengths || !tgt_ids || !tgt_len || !scores || (candidates && !cand_src))
    return fail(-1, "null argument");
  const size_t NR = candidates ? N : B;  // target sentences
  RCCHK(score_check(ctx, B, S, n_sl, T, NR));
  ScoreAltArgs alt = ac.a;
  if (alt.k) {  // the three arrays are of the kind of scores: all pinned (written in place) or all pageable (staged)
    const bool pinned = host_device_view(scores) != nullptr;
    const void *arr[3] = {alt.ids, alt.scores, alt.rank};
    const char *name[3] = {"alt_ids", "alt_scores", "rank"};
    for (int i = 0; i < 3; ++i)
      if (arr[i] && (host_device_view(arr[i]) != nullptr) != pinned)
        return fail(-1, "score alternatives: %s is %s memory, scores is %s: the arrays are of the kind of scores", name[i],
                    pinned ? "pageable" : "pinned", pinned ? "pinned" : "pageable");
  }
  const slimt_hip_model *m = ctx->model;
  uint32_t vmax = (uint32_t)m->V;
  if (gen) {
    RCCHK(check_generator(ctx, gen));
    vmax = (uint32_t)std::min((size_t)m->V, gen->source_vocab);
  } else if (n_sl && !shortlist) {
    return fail(-1, "shortlist is NULL");
  }
  for (size_t i = 0; i < B * S; ++i)
    if (src_ids[i] >= vmax) return fail(-1, "token id %u out of range", src_ids[i]);
  for (size_t i = 0; !gen && i < n_sl; ++i)
    if (shortlist[i] >= (uint32_t)m->V) return fail(-1, "shortlist id %u out of range", shortlist[i]);
  for (size_t b = 0; b < B; ++b)
    if (lengths[b] > S) return fail(-1, "length %u > S", lengths[b]);
  for (size_t b = 0; b < NR; ++b) {
    if (candidates && cand_src[b] >= B)
      return fail(-1, "score: candidate %zu names source %u, the batch has %zu", b, cand_src[b], B);
    if (tgt_len[b] > T) return fail(-1, "score: target length %u of sentence %zu > T %zu", tgt_len[b], b, T);
    for (size_t t = 0; t < tgt_len[b]; ++t)
      if (tgt_ids[b * T + t] >= (uint32_t)m->V)
        return fail(-1, "score: target id %u of sentence %zu out of range", tgt_ids[b * T + t], b);
  }
  if (NR == 0) return 0;  // (a candidate call without candidates: nothing to write)
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = ctx->stream;
  // (translate_host: the shortlist stays on the device, uploaded when it changes)
  if (!gen) RCCHK(upload_shortlist_if_changed(ctx, shortlist, n_sl));
  // inputs: pinned arrays in place, others staged; [tgt_ids NR T][tgt_len NR][cand_src NR][scores NR T] in score_io
  const uint32_t *d_ids = static_cast<const uint32_t *>(host_device_view(src_ids));
  const uint32_t *d_len = static_cast<const uint32_t *>(host_device_view(lengths));
  const uint32_t *d_tgt = static_cast<const uint32_t *>(host_device_view(tgt_ids));
  const uint32_t *d_tlen = static_cast<const uint32_t *>(host_device_view(tgt_len));
  float *d_scores = static_cast<float *>(host_device_view(scores));
  const uint32_t *d_cand = candidates ? static_cast<const uint32_t *>(host_device_view(cand_src)) : nullptr;
  RCCHK(score_reserve(ctx, ctx->score_io, (2 * NR * T + 2 * NR) * 4));
  DevBuf &al_stage = candidates ? ctx->cand_align : ctx->align;  // (ctx->align is the context's, sized for max_batch)
  if (align) RCCHK(score_reserve(ctx, al_stage, NR * T * S * 4));
  if (!d_ids) {
    HIPCHK(hipMemcpyAsync(ctx->ids.p, src_ids, B * S * 4, hipMemcpyHostToDevice, st));
    d_ids = ctx->ids.as<uint32_t>();
  }
  if (!d_len) {
    HIPCHK(hipMemcpyAsync(ctx->lengths.p, lengths, B * 4, hipMemcpyHostToDevice, st));
    d_len = ctx->lengths.as<uint32_t>();
  }
  uint32_t *io = ctx->score_io.as<uint32_t>();
  if (!d_tgt) {
    HIPCHK(hipMemcpyAsync(io, tgt_ids, NR * T * 4, hipMemcpyHostToDevice, st));
    d_tgt = io;
  }
  if (!d_tlen) {
    HIPCHK(hipMemcpyAsync(io + NR * T, tgt_len, NR * 4, hipMemcpyHostToDevice, st));
    d_tlen = io + NR * T;
  }
  if (candidates && !d_cand) {
    HIPCHK(hipMemcpyAsync(io + NR * T + NR, cand_src, NR * 4, hipMemcpyHostToDevice, st));
    d_cand = io + NR * T + NR;
  }
  // outputs that are copied back go down first: the copy back then restores every entry the pass does not write
  float *stage_sc = nullptr;
  if (!d_scores) {
    stage_sc = reinterpret_cast<float *>(io + NR * T + 2 * NR);
    HIPCHK(hipMemcpyAsync(stage_sc, scores, NR * T * 4, hipMemcpyHostToDevice, st));
    d_scores = stage_sc;
  }
  if (align) HIPCHK(hipMemcpyAsync(al_stage.p, align, NR * T * S * 4, hipMemcpyHostToDevice, st));
  // the alternatives likewise: pinned arrays in place, pageable ones as [ids B T k][scores B T k][rank B T] in alt_stage
  ScoreAltArgs user_alt = alt;
  const size_t n_alt = NR * T * (size_t)alt.k;
  bool stage_alt = false;
  if (alt.k) {
    if (void *v = host_device_view(alt.ids)) {
      alt.ids = static_cast<uint32_t *>(v);
      alt.scores = alt.scores ? static_cast<float *>(host_device_view(alt.scores)) : nullptr;
      alt.rank = alt.rank ? static_cast<uint32_t *>(host_device_view(alt.rank)) : nullptr;
    } else {
      stage_alt = true;
      RCCHK(score_reserve(ctx, ctx->alt_stage, (2 * n_alt + NR * T) * 4));
      uint32_t *sa = ctx->alt_stage.as<uint32_t>();
      alt.ids = sa;
      HIPCHK(hipMemcpyAsync(alt.ids, user_alt.ids, n_alt * 4, hipMemcpyHostToDevice, st));
      if (user_alt.scores) {
        alt.scores = reinterpret_cast<float *>(sa + n_alt);
        HIPCHK(hipMemcpyAsync(alt.scores, user_alt.scores, n_alt * 4, hipMemcpyHostToDevice, st));
      }
      if (user_alt.rank) {
        alt.rank = sa + 2 * n_alt;
        HIPCHK(hipMemcpyAsync(alt.rank, user_alt.rank, NR * T * 4, hipMemcpyHostToDevice, st));
      }
    }
  }
  const uint32_t *d_sl = ctx->shortlist.as<uint32_t>();
  if (gen) {  // Model.cc:117-120: the batch's shortlist, generated on this stream into ctx->shortlist
    ShortlistArgs a;
    RCCHK(generated_shortlist_args(ctx, gen, d_ids, d_len, B, S, a));
    HIPCHK(launch_shortlist_generate(a, st));
    uint32_t n = 0;  // the tall kernels are sized on the host: one 4-byte read-back
    HIPCHK(hipMemcpyAsync(&n, ctx->n_sl_dev.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    n_sl = n;
  }
  RCCHK(score_device(ctx, d_ids, d_len, B, S, d_sl, n_sl, d_tgt, d_tlen, T, d_scores, align ? al_stage.as<float>() : nullptr,
                     alt, d_cand, NR));
  if (stage_sc) HIPCHK(hipMemcpyAsync(scores, stage_sc, NR * T * 4, hipMemcpyDeviceToHost, st));
  if (stage_alt) {
    HIPCHK(hipMemcpyAsync(user_alt.ids, alt.ids, n_alt * 4, hipMemcpyDeviceToHost, st));
    if (user_alt.scores) HIPCHK(hipMemcpyAsync(user_alt.scores, alt.scores, n_alt * 4, hipMemcpyDeviceToHost, st));
    if (user_alt.rank) HIPCHK(hipMemcpyAsync(user_alt.rank, alt.rank, NR * T * 4, hipMemcpyDeviceToHost, st));
  }
  if (align) HIPCHK(hipMemcpyAsync(align, al_stage.p, NR * T * S * 4, hipMemcpyDeviceToHost, st));
  if (wait) RCCHK(slimt_hip_ctx_synchronize(ctx));
  return 0;
}
}  // namespace

extern "C" int slimt_hip_score(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                               const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                               const uint32_t *tgt_len, size_t T, float *scores, float *align) {
  return score_host(ctx, nullptr, src_ids, lengths, B, S, shortlist, n_shortlist, tgt_ids, tgt_len, T, scores, align, true);
}

extern "C" int slimt_hip_score_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                     const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                                     const uint32_t *tgt_len, size_t T, float *scores, float *align) {
  return score_host(ctx, nullptr, src_ids, lengths, B, S, shortlist, n_shortlist, tgt_ids, tgt_len, T, scores, align, false);
}

extern "C" int slimt_hip_score_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist, const uint32_t *src_ids,
                                               const uint32_t *lengths, size_t B, size_t S, const uint32_t *tgt_ids,
                                               const uint32_t *tgt_len, size_t T, float *scores, float *align) {
  if (!shortlist) {
    AltCall ac(ctx);  // (taken whatever the outcome)
    return fail(-1, "null argument");
  }
  return score_host(ctx, shortlist, src_ids, lengths, B, S, nullptr, 0, tgt_ids, tgt_len, T, scores, align, false);
}

extern "C" int slimt_hip_score_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths, size_t B,
                                      size_t S, const uint32_t *d_shortlist, size_t n_shortlist, const uint32_t *d_tgt_ids,
                                      const uint32_t *d_tgt_len, size_t T, float *d_scores, float *d_align) {
  AltCall ac(ctx);
  if (ctx && T == 0) return fail(-1, "score: T is 0 (a target row needs at least one column)");
  if (!ctx || !d_src_ids || !d_lengths || !d_tgt_ids || !d_tgt_len || !d_scores) return fail(-1, "null argument");
  RCCHK(score_check(ctx, B, S, n_shortlist, T, B));
  if (n_shortlist && !d_shortlist) return fail(-1, "shortlist is NULL");
  HIPCHK(hipSetDevice(ctx->model->device));
  RCCHK(alternatives_device_visible(ac.a));
  return score_device(ctx, d_src_ids, d_lengths, B, S, d_shortlist, n_shortlist, d_tgt_ids, d_tgt_len, T, d_scores, d_align,
                      ac.a);
}

// ---- candidates: N target rows over B sources encoded once (include/slimt_hip.h, slimt_hip_score_candidates*) ----------
// score_host / score_device above with the targets counted by candidate; score_candidates.hip has the attention that
// knows each candidate's source, and the ranking.
static_assert(slimt_hip::kScoreCandidateRun == SLIMT_HIP_CANDIDATE_RUN, "the run length the header documents");

extern "C" int slimt_hip_score_candidates(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                          const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                                          const uint32_t *tgt_len, size_t T, const uint32_t *cand_src, size_t N, float *scores,
                                          float *align) {
  return score_host(ctx, nullptr, src_ids, lengths, B, S, shortlist, n_shortlist, tgt_ids, tgt_len, T, scores, align, true, true,
                    cand_src, N);
}

extern "C" int slimt_hip_score_candidates_async(slimt_hip_ctx *ctx, const uint32_t *src_ids, const uint32_t *lengths, size_t B,
                                                size_t S, const uint32_t *shortlist, size_t n_shortlist, const uint32_t *tgt_ids,
                                                const uint32_t *tgt_len, size_t T, const uint32_t *cand_src, size_t N,
                                                float *scores, float *align) {
  return score_host(ctx, nullptr, src_ids, lengths, B, S, shortlist, n_shortlist, tgt_ids, tgt_len, T, scores, align, false, true,
                    cand_src, N);
}

extern "C" int slimt_hip_score_candidates_async_generated(slimt_hip_ctx *ctx, slimt_hip_shortlist *shortlist,
                                                          const uint32_t *src_ids, const uint32_t *lengths, size_t B, size_t S,
                                                          const uint32_t *tgt_ids, const uint32_t *tgt_len, size_t T,
                                                          const uint32_t *cand_src, size_t N, float *scores, float *align) {
  if (!shortlist) {
    AltCall ac(ctx);  // (taken whatever the outcome)
    return fail(-1, "null argument");
  }
  return score_host(ctx, shortlist, src_ids, lengths, B, S, nullptr, 0, tgt_ids, tgt_len, T, scores, align, false, true, cand_src,
                    N);
}

extern "C" int slimt_hip_score_candidates_device(slimt_hip_ctx *ctx, const uint32_t *d_src_ids, const uint32_t *d_lengths,
                                                 size_t B, size_t S, const uint32_t *d_shortlist, size_t n_shortlist,
                                                 const uint32_t *d_tgt_ids, const uint32_t *d_tgt_len, size_t T,
                                                 const uint32_t *d_cand_src, size_t N, float *d_scores, float *d_align) {
  AltCall ac(ctx);
  if (ctx && T == 0) return fail(-1, "score: T is 0 (a target row needs at least one column)");
  if (!ctx || !d_src_ids || !d_lengths || !d_tgt_ids || !d_tgt_len || !d_cand_src || !d_scores) return fail(-1, "null argument");
  RCCHK(score_check(ctx, B, S, n_shortlist, T, N));
  if (n_shortlist && !d_shortlist) return fail(-1, "shortlist is NULL");
  if (N == 0) return 0;
  HIPCHK(hipSetDevice(ctx->model->device));
  RCCHK(alternatives_device_visible(ac.a));
  return score_device(ctx, d_src_ids, d_lengths, B, S, d_shortlist, n_shortlist, d_tgt_ids, d_tgt_len, T, d_scores, d_align, ac.a,
                      d_cand_src, N);
}

namespace {
int candidates_rank_check(const void *scores, const void *tgt_len, const void *cand_src, size_t N, size_t T, size_t B, int mode,
                          const void *totals, const void *best) {
  if (!scores || !tgt_len || !cand_src || !totals || !best) return fail(-1, "null argument");
  if (mode != 0 && mode != 1) return fail(-1, "candidates rank: mode %d is neither 0 (sum) nor 1 (mean per token)", mode);
  if (B == 0 || B > 0xffffffffu) return fail(-1, "candidates rank: %zu sources", B);
  if (T == 0 || T > kScoreMaxT || N > kScoreMaxRows || N * T > kScoreMaxRows)
    return fail(-1, "candidates rank: %zu x %zu scores exceed the limits (1 <= T <= %zu, N * T <= %zu)", N, T, kScoreMaxT,
                kScoreMaxRows);
  return 0;
}

CandRankArgs candidates_rank_args(const float *scores, const uint32_t *tgt_len, const uint32_t *cand_src, size_t N, size_t T,
                                  size_t B, int mode, float *totals, uint32_t *best, unsigned long long *entries) {
  CandRankArgs a;
  a.scores = scores;
  a.tgt_len = tgt_len;
  a.cand_src = cand_src;
  a.N = N;
  a.T = (uint32_t)T;
  a.B = (uint32_t)B;
  a.mode = mode;
  a.totals = totals;
  a.best = best;
  a.entries = entries;
  return a;
}
}  // namespace

extern "C" int slimt_hip_candidates_rank(const float *scores, const uint32_t *tgt_len, const uint32_t *cand_src, size_t N, size_t T,
                                         size_t B, int mode, float *totals, uint32_t *best) {
  RCCHK(candidates_rank_check(scores, tgt_len, cand_src, N, T, B, mode, totals, best));
  for (size_t c = 0; c < N; ++c) {
    if (cand_src[c] >= B) return fail(-1, "candidates rank: candidate %zu names source %u of %zu", c, cand_src[c], B);
    if (tgt_len[c] > T) return fail(-1, "candidates rank: length %u of candidate %zu > T %zu", tgt_len[c], c, T);
  }
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(std::max<size_t>(1, N * T) * 4));
  HIPCHK(t.b.reserve(std::max<size_t>(1, N) * 4));
  HIPCHK(t.c.reserve(std::max<size_t>(1, N) * 4));
  HIPCHK(t.d.reserve(std::max<size_t>(1, N) * 4));
  HIPCHK(t.e.reserve(B * 4));
  HIPCHK(t.f.reserve(B * 8));
  if (N) {
    HIPCHK(hipMemcpyAsync(t.a.p, scores, N * T * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t.b.p, tgt_len, N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t.c.p, cand_src, N * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(launch_candidates_rank(candidates_rank_args(t.a.as<float>(), t.b.as<uint32_t>(), t.c.as<uint32_t>(), N, T, B, mode,
                                                     t.d.as<float>(), t.e.as<uint32_t>(), t.f.as<unsigned long long>()), st));
  if (N) HIPCHK(hipMemcpyAsync(totals, t.d.p, N * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(best, t.e.p, B * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_candidates_rank_device(slimt_hip_ctx *ctx, const float *d_scores, const uint32_t *d_tgt_len,
                                                const uint32_t *d_cand_src, size_t N, size_t T, size_t B, int mode,
                                                float *d_totals, uint32_t *d_best) {
  if (!ctx) return fail(-1, "null argument");
  RCCHK(candidates_rank_check(d_scores, d_tgt_len, d_cand_src, N, T, B, mode, d_totals, d_best));
  HIPCHK(hipSetDevice(ctx->model->device));
  RCCHK(score_reserve(ctx, ctx->cand_rank, B * 8));
  HIPCHK(launch_candidates_rank(candidates_rank_args(d_scores, d_tgt_len, d_cand_src, N, T, B, mode, d_totals, d_best,
                                                     ctx->cand_rank.as<unsigned long long>()), ctx->stream));
  return 0;
}

// ---- consensus selection among each source's rows (include/slimt_hip.h, slimt_hip_consensus_select*; consensus.hip) --------
static_assert(kConsensusMaxOrder == SLIMT_HIP_CONSENSUS_MAX_ORDER && kConsensusMaxRows == SLIMT_HIP_CONSENSUS_MAX_ROWS &&
                  kConsensusMaxT == SLIMT_HIP_CONSENSUS_MAX_T && kConsensusMaxBeta2 == SLIMT_HIP_CONSENSUS_MAX_BETA2,
              "include/slimt_hip.h and kernels.h disagree on the consensus limits");
namespace {
int consensus_check(const void *ids, const void *len, const void *row_src, size_t N, size_t T, size_t B, int max_order, int beta2,
                    const void *utility, const void *best) {
  if (max_order < 1 || max_order > SLIMT_HIP_CONSENSUS_MAX_ORDER)
    return fail(-1, "consensus: max_order %d is not in 1..%d", max_order, SLIMT_HIP_CONSENSUS_MAX_ORDER);
  if (beta2 < 1 || beta2 > SLIMT_HIP_CONSENSUS_MAX_BETA2)
    return fail(-1, "consensus: beta2 %d is not in 1..%d", beta2, SLIMT_HIP_CONSENSUS_MAX_BETA2);
  if (!best || (N && (!ids || !len || !row_src || !utility))) return fail(-1, "null argument");
  if (B == 0 || B > 0x7fffffffu) return fail(-1, "consensus: %zu sources", B);
  if (T == 0 || T > (size_t)SLIMT_HIP_CONSENSUS_MAX_T || N > kConsensusMaxN)
    return fail(-1, "consensus: %zu rows of %zu tokens exceed the limits (1 <= T <= %d, N <= %u)", N, T,
                SLIMT_HIP_CONSENSUS_MAX_T, kConsensusMaxN);
  return 0;
}

ConsensusArgs consensus_args(const uint32_t *ids, const uint32_t *len, const uint32_t *row_src, size_t N, size_t T, size_t B,
                             int max_order, int beta2, double *utility, uint32_t *best) {
  ConsensusArgs a;
  a.ids = ids;
  a.len = len;
  a.row_src = row_src;
  a.N = (uint32_t)N;
  a.T = (uint32_t)T;
  a.B = (uint32_t)B;
  a.max_order = max_order;
  a.beta2 = beta2;
  a.utility = utility;
  a.best = best;
  return a;
}
}  // namespace

extern "C" int slimt_hip_consensus_select(const uint32_t *ids, const uint32_t *len, const uint32_t *row_src, size_t N, size_t T,
                                          size_t B, int max_order, int beta2, double *utility, uint32_t *best) {
  RCCHK(consensus_check(ids, len, row_src, N, T, B, max_order, beta2, utility, best));
  {
    std::map<uint32_t, uint32_t> rows;  // (N <= 65536 entries, whatever B)
    for (size_t c = 0; c < N; ++c) {
      if (row_src[c] >= B) return fail(-1, "consensus: row %zu names source %u of %zu", c, row_src[c], B);
      if (len[c] > T) return fail(-1, "consensus: length %u of row %zu > T %zu", len[c], c, T);
      if (++rows[row_src[c]] > (uint32_t)SLIMT_HIP_CONSENSUS_MAX_ROWS)
        return fail(-1, "consensus: source %u has more than %d rows", row_src[c], SLIMT_HIP_CONSENSUS_MAX_ROWS);
    }
  }
  Tmp3 t;
  hipStream_t st = nullptr;
  HIPCHK(t.a.reserve(std::max<size_t>(1, N * T) * 4));
  HIPCHK(t.b.reserve(std::max<size_t>(1, N) * 4));
  HIPCHK(t.c.reserve(std::max<size_t>(1, N) * 4));
  HIPCHK(t.d.reserve(std::max<size_t>(1, N) * 8));
  HIPCHK(t.e.reserve(B * 4));
  if (N) {
    HIPCHK(hipMemcpyAsync(t.a.p, ids, N * T * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t.b.p, len, N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t.c.p, row_src, N * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(launch_consensus(consensus_args(t.a.as<uint32_t>(), t.b.as<uint32_t>(), t.c.as<uint32_t>(), N, T, B, max_order, beta2,
                                         t.d.as<double>(), t.e.as<uint32_t>()), st));
  if (N) HIPCHK(hipMemcpyAsync(utility, t.d.p, N * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(best, t.e.p, B * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int slimt_hip_consensus_select_device(slimt_hip_ctx *ctx, const uint32_t *d_ids, const uint32_t *d_len,
                                                 const uint32_t *d_row_src, size_t N, size_t T, size_t B, int max_order,
                                                 int beta2, double *d_utility, uint32_t *d_best) {
  RCCHK(consensus_check(d_ids, d_len, d_row_src, N, T, B, max_order, beta2, d_utility, d_best));
  if (!ctx) return fail(-1, "null argument");
  HIPCHK(hipSetDevice(ctx->model->device));
  ProfScope p(ctx, SLIMT_HIP_K_CONSENSUS, 0, 0);
  HIPCHK(launch_consensus(consensus_args(d_ids, d_len, d_row_src, N, T, B, max_order, beta2, d_utility, d_best), ctx->stream));
  return 0;
}
