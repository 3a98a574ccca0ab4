// extern "C" surface of libmodsgpu.so (include/mods_hip.h): context management, timing,
// detector entry points and introspection for the parity tests.
#include "common.hpp"
#include "u8_strips.hpp"
#include "detmath.hpp"
#include "ransac_host.hpp"
#include "f_laf.hpp"
#include "h_laf.hpp"
#include "../../include/mods_degensac.h"
#include <cstdarg>
#include <memory>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>
#include <time.h>
#include <sys/prctl.h>

namespace mods {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// How a pipeline thread waits for a stream.  hipStreamQuery on a stream that is not done makes the runtime put a marker behind the
// stream's work and has the runtime's OWN thread spin until that marker completes: tools/ubench/rt_thread_probe.hip - a 5 ms kernel
// polled with hipStreamQuery every 50 us keeps that thread at 98.5 % of a core for the whole 5 ms, the same kernel behind a recorded
// event polled with hipEventQuery at 0.0 % (a word in pinned memory written by a kernel: 0.0 % as well).  That spinning was the "one
// core per process" of rounds 4 and 5 (1.1 ms per pair at 900 pairs/s).  So: record an event of the calling thread behind the work
// and poll THAT, sleeping in between.
// (A first attempt this round - a one-thread kernel that stores a sequence number to pinned memory - showed no gain only because
// other waits of the process still used hipStreamQuery; one pending query-marker is enough to keep the runtime's thread spinning.)
// Events / streams a thread borrows for as long as it lives: handed back to a process-wide list when the thread ends (no runtime call
// in a thread's exit path - the runtime may be shutting down by then -, and a pipeline that is created and destroyed again and again
// reuses the same few objects)
template <class T> struct HandlePool {
  std::mutex mu;
  std::vector<T> free_[16];
  T take(int dev, T (*make)()) {
    { std::lock_guard<std::mutex> lk(mu); if (!free_[dev].empty()) { T h = free_[dev].back(); free_[dev].pop_back(); return h; } }
    return make();
  }
  void give(int dev, T h) { std::lock_guard<std::mutex> lk(mu); free_[dev].push_back(h); }
};
template <class T> struct Borrowed {
  HandlePool<T> *pool; T h[16] = {};
  explicit Borrowed(HandlePool<T> *p) : pool(p) {}
  ~Borrowed() { for (int d = 0; d < 16; d++) if (h[d]) pool->give(d, h[d]); }
};
static HandlePool<hipEvent_t> *event_pool() { static HandlePool<hipEvent_t> *p = new HandlePool<hipEvent_t>(); return p; }     // (never destroyed: threads may outlive statics)
static HandlePool<hipStream_t> *stream_pool() { static HandlePool<hipStream_t> *p = new HandlePool<hipStream_t>(); return p; }
// the thread's event on the device that OWNS stream s (an event can only be recorded on a stream of its own device, and a polling
// thread may wait for a stream of another device than its current one: the plane getters, the multi-device helpers); the event is
// created with that device current, and the caller's device is put back
static hipEvent_t thread_event(hipStream_t s) {
  static thread_local Borrowed<hipEvent_t> t(event_pool());
  int cur = 0, dev = 0;
  if (hipGetDevice(&cur) != hipSuccess) return nullptr;
  dev = cur;
  if (s && hipStreamGetDevice(s, &dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (dev < 0 || dev >= 16) return nullptr;
  if (!t.h[dev]) {
    if (dev != cur && hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    t.h[dev] = t.pool->take(dev, +[]() -> hipEvent_t { hipEvent_t e = nullptr; return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? e : nullptr; });
    if (dev != cur) (void)hipSetDevice(cur);
  }
  return t.h[dev];
}
hipError_t stream_wait(hipStream_t s) {
  const long ns = tl_wait_sleep_ns;
  if (ns <= 0) return hipStreamSynchronize(s);
  hipEvent_t ev = thread_event(s);
  if (!ev) return hipStreamSynchronize(s);
  hipError_t e = hipEventRecord(ev, s);
  if (e != hipSuccess) { (void)hipGetLastError(); return hipStreamSynchronize(s); }   // (the runtime's own wait works from any current device)
  e = hipEventQuery(ev);
  for (int i = 0; i < tl_wait_spin_polls && e == hipErrorNotReady; i++) e = hipEventQuery(ev);
  // every poll is a runtime call and a wake-up of this thread (~4 us of CPU): the sleep grows by half per poll up to its bound, so a
  // batch's 10 ms cost a GPU worker ~45 polls instead of 200 and a scoring round a verify thread ~6 instead of 25 (process CPU per
  // pair 2.35 -> ~2.0 ms at the same rate, profiles/r05_wait_interval_sweep.log); the wait overshoots by at most a third of itself
  long cur = ns;
  const long cap = std::max(ns, tl_wait_sleep_max_ns);
  while (e == hipErrorNotReady) {
    const timespec ts = {0, cur};
    nanosleep(&ts, nullptr);
    e = hipEventQuery(ev);
    cur = std::min(cap, cur + cur / 2);
  }
  // a "not ready" answer may have been left as the thread's last error: it is not one
  const hipError_t last = hipGetLastError();
  if (e == hipSuccess && last != hipSuccess && last != hipErrorNotReady) return last;
  return e;
}

// (a blocking copy / fill inside a stream capture would be recorded as a node and then waited for - which a capture forbids: refused
// here, so that no upload can end up inside a recorded detect + describe graph)
static bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
  return st != hipStreamCaptureStatusNone;
}
hipError_t copy_wait(hipStream_t s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  if (!bytes) return hipSuccess;
  if (capturing(s)) return hipErrorStreamCaptureUnsupported;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  return e != hipSuccess ? e : stream_wait(s);
}
hipError_t fill_wait(hipStream_t s, void *dst, int value, size_t bytes) {
  if (!bytes) return hipSuccess;
  if (capturing(s)) return hipErrorStreamCaptureUnsupported;
  const hipError_t e = hipMemsetAsync(dst, value, bytes, s);
  return e != hipSuccess ? e : stream_wait(s);
}
hipStream_t thread_stream(int dev) {
  static thread_local Borrowed<hipStream_t> t(stream_pool());
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return nullptr;                             // (nullptr = the legacy stream: what the call used before)
  if (dev < 0) dev = cur;
  if (dev >= 16) return nullptr;
  if (!t.h[dev]) {
    if (dev != cur && hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    t.h[dev] = t.pool->take(dev, +[]() -> hipStream_t { hipStream_t q = nullptr; return hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess ? q : nullptr; });
    if (dev != cur) (void)hipSetDevice(cur);
  }
  return t.h[dev];
}
// the device a device pointer lives on (-1: not a device pointer the runtime knows - the calling thread's current device then)
int device_of_pointer(const void *p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

void wait_mode_for_worker(long default_sleep_ns) {
  long ns = default_sleep_ns, cap = 250000;
  if (const char *m = getenv("MODS_SYNC")) {
    if (!strncmp(m, "spin", 4)) ns = 0;
    else if (!strncmp(m, "sleep", 5)) { if (m[5] == ':') { ns = std::max(1l, atol(m + 6)) * 1000; cap = ns; } }   // a given interval is kept as it is
    else fprintf(stderr, "mods: MODS_SYNC=%s not understood (spin | sleep[:microseconds]); keeping the default\n", m);
  }
  tl_wait_sleep_ns = ns;
  tl_wait_sleep_max_ns = cap;
  if (ns > 0) prctl(PR_SET_TIMERSLACK, 1000ul, 0, 0, 0);   // default slack 50 us: a 30 us sleep would take 80
}

StageScope::StageScope(mods_ctx *c, int s, double bytes) : ctx(c), stage(s) {
  on = (c->timing_mask >> s) & 1;
  if (!on) return;
  StageTimer &t = c->timers[s];
  auto get = [&]() {
    hipEvent_t e;
    if (!t.pool.empty()) { e = t.pool.back(); t.pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
  };
  e0 = get(); e1 = get();
  t.bytes += bytes;
  (void)hipEventRecord(e0, c->stream);
}
StageScope::~StageScope() {
  if (!on) return;
  (void)hipEventRecord(e1, ctx->stream);
  ctx->timers[stage].pending.emplace_back(e0, e1);
}

}  // namespace mods

using namespace mods;

namespace mods { int ransac_failed(); }   // ransac.hip: the calling thread's last exp_ransac*custom hit a device failure

extern "C" {

const char *mods_last_error(void) { return g_err; }

int mods_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int ctx_create_impl(int device, int max_w, int max_h, int batch, unsigned stream_flags, mods_ctx **out);

int mods_ctx_create(int device, int max_w, int max_h, int batch, mods_ctx **out) {
  // default: a stream that orders itself after the legacy default stream, so that images produced by
  // another library on the default stream (e.g. a torch .cuda() copy) are complete when kernels read them
  return ctx_create_impl(device, max_w, max_h, batch, hipStreamDefault, out);
}

// flags bit 0: non-blocking stream (no implicit ordering with the default stream; the caller guarantees
// that inputs are complete).  Needed for several contexts to overlap on one GPU.
int mods_ctx_create_ex(int device, int max_w, int max_h, int batch, int flags, mods_ctx **out) {
  return ctx_create_impl(device, max_w, max_h, batch, (flags & 1) ? hipStreamNonBlocking : hipStreamDefault, out);
}

static int ctx_create_impl(int device, int max_w, int max_h, int batch, unsigned stream_flags, mods_ctx **out) {
  if (!out || max_w <= 0 || max_h <= 0 || batch <= 0) { set_error("mods_ctx_create: bad arguments"); return MODS_E_ARG; }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n) {
    set_error("no HIP device available (count=%d, requested %d): libmodsgpu has no CPU path", n, device);
    return MODS_E_NODEVICE;
  }
  MODS_HIP_CHECK(hipSetDevice(device));
  std::unique_ptr<mods_ctx> c(new mods_ctx());   // a failed creation releases what it made
  c->device = device; c->max_w = max_w; c->max_h = max_h; c->batch = batch;
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->n_cu = cus; }
  MODS_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, stream_flags));
  const size_t px = (size_t)max_w * max_h;
  size_t mc = px / 8;
  mc = std::max<size_t>(mc, 1u << 16);
  mc = std::min<size_t>(mc, 1u << 22);
  c->max_cand = (int)mc;
  MODS_HIP_CHECK(c->pyr_dev.reserve(1));
  MODS_HIP_CHECK(c->input_dev.reserve(px * batch));
  MODS_HIP_CHECK(c->tmp_dev.reserve(px * batch));
  MODS_HIP_CHECK(c->gauss_taps_dev.reserve(16 * 64));
  MODS_HIP_CHECK(c->smm_mask_dev.reserve(32 * 32));
  MODS_HIP_CHECK(c->cand.reserve(mc * batch));
  MODS_HIP_CHECK(c->cand_count.reserve(3 * (size_t)batch));
  MODS_HIP_CHECK(c->keys_dev.reserve(mc * batch));
  MODS_HIP_CHECK(c->sort_keys.reserve(mc * batch));
  MODS_HIP_CHECK(c->sort_idx.reserve(2 * mc * batch));
  MODS_HIP_CHECK(c->rank_dev.reserve(mc * batch));
  MODS_HIP_CHECK(c->nms_mask.reserve((px / 64 + (size_t)max_h + 64) * kMaxLevels * batch));
  MODS_HIP_CHECK(c->host_counts.reserve(5 * (size_t)batch + 4));   // cand / acc / key / region / inside counts, error flag
  MODS_HIP_CHECK(c->ori_dev.reserve(48 * mc * batch));
  MODS_HIP_CHECK(c->regions_dev.reserve(mc * batch));
  MODS_HIP_CHECK(c->region_count.reserve(3 * (size_t)batch));   // regions, then 2 tier counts per image
  MODS_HIP_CHECK(c->inside_count.reserve((size_t)batch));
  MODS_HIP_CHECK(mods::fill_wait(c->stream, c->inside_count, 0, sizeof(int) * batch));
  *out = c.release();
  return MODS_OK;
}

static void dd_graph_drop(mods_ctx *c) {
  for (auto &e : c->dd_cache) (void)hipGraphExecDestroy(e.second);
  c->dd_cache.clear();
}

}  // extern "C"

// what is not memory; the buffers (members, MserState, helper_stage) free themselves after this
mods_ctx::~mods_ctx() {
  for (auto &t : timers) {
    for (auto &p : t.pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &e : t.pool) (void)hipEventDestroy(e);
  }
  mser_release(this);
  distractor_release(this);
  for (mods_ctx *h : helpers) if (h) mods_ctx_destroy(h);
  (void)hipSetDevice(device);
  dd_graph_drop(this);
  if (stream2) (void)hipStreamDestroy(stream2);
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (ev_join) (void)hipEventDestroy(ev_join);
  if (stream) (void)hipStreamDestroy(stream);
}

extern "C" {

void mods_ctx_destroy(mods_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)mods::stream_wait(c->stream);
  delete c;
}

int mods_ctx_sync(mods_ctx *c) { MODS_HIP_CHECK(mods::stream_wait(c->stream)); return MODS_OK; }
void *mods_ctx_stream(mods_ctx *c) { return (void *)c->stream; }

int mods_ctx_timing_enable(mods_ctx *c, int stage_mask) { c->timing_mask = stage_mask; return MODS_OK; }
int mods_ctx_pyramid_streams(mods_ctx *c, int n) {
  if (!c || n < 1 || n > 2) { set_error("pyramid streams: 1 or 2"); return MODS_E_ARG; }
  c->pyr_streams = n;
  return MODS_OK;
}

static int resolve_timers(mods_ctx *c) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  for (auto &t : c->timers) {
    for (auto &p : t.pending) {
      float ms = 0;
      MODS_HIP_CHECK(hipEventElapsedTime(&ms, p.first, p.second));
      t.total_ms += ms;
      t.launches++;
      t.pool.push_back(p.first); t.pool.push_back(p.second);
    }
    t.pending.clear();
  }
  return MODS_OK;
}

int mods_ctx_timing_read(mods_ctx *c, int stage, double *total_ms, int *launches, double *bytes) {
  if (stage < 0 || stage >= MODS_STAGE_COUNT) return MODS_E_ARG;
  int rc = resolve_timers(c);
  if (rc) return rc;
  if (total_ms) *total_ms = c->timers[stage].total_ms;
  if (launches) *launches = c->timers[stage].launches;
  if (bytes) *bytes = c->timers[stage].bytes;
  return MODS_OK;
}

int mods_ctx_timing_reset(mods_ctx *c) {
  int rc = resolve_timers(c);
  if (rc) return rc;
  for (auto &t : c->timers) { t.total_ms = 0; t.launches = 0; t.bytes = 0; }
  return MODS_OK;
}

// ---- detector -----------------------------------------------------------------------------
static int detect_common(mods_ctx *c, const float *img_dev, int n_img, int w, int h, int stride,
                         const mods_hessaff_params *par, mods_affkey *out_host, int max_out, int *n_out_host) {
  if (!c || !img_dev || !par || !n_out_host) { set_error("detect: null argument"); return MODS_E_ARG; }
  if (w <= 0 || h <= 0 || (size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  if (stride < w) { set_error("detect: stride %d < width %d", stride, w); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc;
  if ((rc = detect_any(c, img_dev, n_img, w, h, stride, par, 1.0, 1.0))) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(c->host_counts, c->cand_count, sizeof(int) * 3 * c->batch, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  for (int b = 0; b < n_img; b++) {
    if (c->host_counts[b] > c->max_cand) { set_error("NMS hit list overflow: %d > %d", c->host_counts[b], c->max_cand); return MODS_E_CAPACITY; }
    const int n = c->host_counts[2 * c->batch + b];
    n_out_host[b] = n;
    if (out_host) {
      if (n > max_out) { set_error("keypoint output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
      MODS_HIP_CHECK(mods::copy_wait(c->stream, out_host + (size_t)b * max_out, c->keys_dev + (size_t)b * c->max_cand, sizeof(mods_affkey) * n, hipMemcpyDeviceToHost));
    }
  }
  return MODS_OK;
}

int mods_detect_hessian_affine_dev(mods_ctx *c, const float *img_dev, int n_img, int w, int h, int stride,
                                   const mods_hessaff_params *par, mods_affkey *out_host, int max_out, int *n_out_host) {
  return detect_common(c, img_dev, n_img, w, h, stride, par, out_host, max_out, n_out_host);
}

int mods_detect_hessian_affine(mods_ctx *c, const float *img, int w, int h, int stride, const mods_hessaff_params *par,
                               mods_affkey *out, int max_out, int *n_out) {
  if (!c || !img) { set_error("detect: null argument"); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(hipMemcpy2DAsync(c->input_dev, sizeof(float) * w, img, sizeof(float) * stride, sizeof(float) * w, h,
                                  hipMemcpyHostToDevice, c->stream));
  return detect_common(c, c->input_dev, 1, w, h, w, par, out, max_out, n_out);
}

int mods_pyramid_octaves(mods_ctx *c) { return c->pyr.n_oct; }
int mods_pyramid_dims(mods_ctx *c, int o, int *w, int *h) {
  if (o < 0 || o >= c->pyr.n_oct) return MODS_E_ARG;
  *w = c->pyr.oct[o].w; *h = c->pyr.oct[o].h;
  return MODS_OK;
}
int mods_pyramid_plane(mods_ctx *c, int img, int o, int level, int kind, float *dst) {
  if (o < 0 || o >= c->pyr.n_oct || level < 0 || level >= c->pyr.n_levels || img < 0 || img >= c->last_n_img) return MODS_E_ARG;
  const OctaveDev &oc = c->pyr.oct[o];
  const float *p = (kind ? oc.resp[level] : oc.blur[level]) + (size_t)oc.w * oc.h * img;
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  MODS_HIP_CHECK(mods::copy_wait(c->stream, dst, p, sizeof(float) * (size_t)oc.w * oc.h, hipMemcpyDeviceToHost));
  return MODS_OK;
}
// accepted (post-dedup) localisation records of image `img`, in list (arbitrary) order
int mods_pyramid_candidates(mods_ctx *c, int img, mods_candidate *out, int max_out, int *n_out) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int count = 0;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, &count, c->cand_count + img, sizeof(int), hipMemcpyDeviceToHost));
  int n = std::min(count, c->max_cand);
  std::vector<CandDev> v(n);
  MODS_HIP_CHECK(mods::copy_wait(c->stream, v.data(), c->cand + (size_t)img * c->max_cand, sizeof(CandDev) * n, hipMemcpyDeviceToHost));
  // state: 2 accepted (claimed its octaveMap cell), 3 Baumberg converged, 4 Baumberg rejected
  int m = 0;
  for (auto &cd : v) {
    if (!(cd.state == 2 || cd.state == 3 || cd.state == 4)) continue;
    if (m < max_out) {
      mods_candidate &o = out[m];
      o.octave = cd.octave; o.level = cd.level; o.r0 = cd.r0; o.c0 = cd.c0; o.r = cd.r; o.c = cd.c;
      o.x = cd.x; o.y = cd.y; o.s = cd.s; o.pixelDistance = cd.pixelDistance; o.response = cd.response; o.type = cd.type;
    }
    m++;
  }
  *n_out = m;
  return m > max_out ? MODS_E_CAPACITY : MODS_OK;
}
// raw NMS hit records of image `img` in list (arbitrary) order, whatever localisation made of them: (octave, level, r0, c0) of the
// first min(count, max_cand) records; *n_out = the device's count, which exceeds max_cand after an overflowing detection
int mods_pyramid_nms_hits(mods_ctx *c, int img, int *out4, int max_out, int *n_out) {
  if (!c || !n_out || img < 0 || img >= c->batch || (max_out > 0 && !out4)) { set_error("pyramid_nms_hits: bad argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int count = 0;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, &count, c->cand_count + img, sizeof(int), hipMemcpyDeviceToHost));
  *n_out = count;
  const int n = std::max(0, std::min(count, c->max_cand));
  if (n > max_out) { set_error("NMS hit output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
  std::vector<CandDev> v(n);
  MODS_HIP_CHECK(mods::copy_wait(c->stream, v.data(), c->cand + (size_t)img * c->max_cand, sizeof(CandDev) * n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    out4[4 * i] = v[i].octave; out4[4 * i + 1] = v[i].level; out4[4 * i + 2] = v[i].r0; out4[4 * i + 3] = v[i].c0;
  }
  return MODS_OK;
}

// ---- orientation + description ----------------------------------------------------------------
static int check_desc_err(mods_ctx *c) {
  int e = 0;
  MODS_HIP_CHECK(hipMemcpyAsync(&e, c->desc_err_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  if (e) {
    MODS_HIP_CHECK(hipMemsetAsync(c->desc_err_dev, 0, sizeof(int), c->stream));
    set_error("measurement region larger than the descriptor scratch (P2 > 3*max(w,h) or > 4096 blur taps)");
    return MODS_E_CAPACITY;
  }
  return MODS_OK;
}

// The launches of one detect + describe call: scale space, NMS, localisation, Baumberg, order, orientation, extraction, SIFT and the
// read-back of the batch's counters (pinned host words) - ~70 dispatches for a 1080p batch, no host round trip between them.
static int dd_enqueue(mods_ctx *c, const PixelSources &img, int n_img, int w, int h, int stride, const mods_hessaff_params *det,
                      const mods_describe_params *desc) {
  int rc;
  if ((rc = detect_any(c, img.f32, n_img, w, h, stride, det, 1.0, 1.0))) return rc;
  PixelSources planes = img;
  if (stride != w) planes.f32 = c->tmp_dev;   // pyramid_build repacked the batch there (such a call has no 8-bit source)
  if ((rc = describe_run(c, planes, n_img, w, h, desc))) return rc;
  // every count and the error flag of the batch in one round trip (pinned host words)
  int *hc = c->host_counts;
  MODS_HIP_CHECK(hipMemcpyAsync(hc, c->cand_count, sizeof(int) * 3 * c->batch, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(hc + 3 * c->batch, c->region_count, sizeof(int) * c->batch, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(hc + 4 * c->batch, c->inside_count, sizeof(int) * n_img, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(hc + 5 * c->batch, c->desc_err_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  return MODS_OK;
}

static unsigned long long fnv1a(const void *p, size_t n, unsigned long long h) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

// Replay instead of re-issue (mods_ctx_graphs).  A pipeline worker calls this with the same arguments batch after batch: every kernel
// argument is either a pointer into the context's pools or a parameter, every data-dependent quantity lives on the device, so the
// sequence of launches is the same each time.  The first call with a set of arguments runs eagerly (it may allocate pools, upload tap
// tables, set kernel attributes); the second one is recorded with hipStreamBeginCapture (both streams of the forked pyramid end up in
// the graph through their fork / join events) and launched; later ones are one hipGraphLaunch.  A recording that fails - a call in
// the chain that cannot be captured - switches the context back to eager launches for good.  Off while stage timers are on (their
// events belong to single launches), with external hooks (host round trips) and for the MSER detector (host threads).
// Only recordings with TWO branches (the forked scale space of a large batch) are replayed.  A recording that is one linear chain
// of launches faults on replay with this runtime (ROCm 7.0.2, HIP 7.0.51831: "illegal memory access" in the first replay, 12 of 12
// linear configurations of tools/exp_graph.py, while all 16 - linear and forked - replay bit-identically with
// DEBUG_CLR_GRAPH_PACKET_CAPTURE=0, the switch for the runtime's replay of pre-built AQL packets, which linear kernel chains
// take; profiles/r05_graph_replay_matrix*.log).  That switch is read when the runtime starts, out of a library's reach, so calls
// whose scale space does not fork (small images, small batches, mods_ctx_pyramid_streams(1)) stay eager.
static int dd_run(mods_ctx *c, const PixelSources &img, int n_img, int w, int h, int stride, const mods_hessaff_params *det,
                  const mods_describe_params *desc) {
  // (domain-size pooling: the chain runs eagerly - K extractions are K times the launches, and no recording of it has been tried)
  const bool can = c->dd_graphs && c->timing_mask == 0 && !mods::has_hooks(c) && !mods::has_nets(c) && det->detectorType != MODS_DET_MSER &&
                   c->dsp_scales < 2;
  if (!can) { mods::dev_state_changed(c); return dd_enqueue(c, img, n_img, w, h, stride, det, desc); }
  mods_ctx::DdKey key;
  key.img = img; key.n_img = n_img; key.w = w; key.h = h; key.stride = stride;
  key.par_hash = fnv1a(desc, sizeof(*desc), fnv1a(det, sizeof(*det), 1469598103934665603ull)) ^ (unsigned long long)c->pyr_streams;
  key.epoch = c->dev_state_epoch;
  // A recording is made, and replayed, only right behind a call with the SAME arguments: tables that live on the device and are
  // refreshed from the host when the arguments change (the octave table, tap slots, masks) are then exactly what the recorded
  // launches expect, and no such refresh can end up inside a recording.  A worker's steady state - full batches of one geometry -
  // is a run of identical calls; a change of batch size or geometry costs one eager call.
  if (c->dd_stale) { dd_graph_drop(c); c->dd_linear.clear(); c->dd_stale = false; }
  const bool repeat = key == c->dd_prev;
  c->dd_prev = key;
  if (!repeat) return dd_enqueue(c, img, n_img, w, h, stride, det, desc);
  for (auto &e : c->dd_cache)
    if (e.first == key) {
      MODS_HIP_CHECK(hipGraphLaunch(e.second, c->stream));
      c->dd_replays++;
      return MODS_OK;
    }
  for (const auto &k2 : c->dd_linear)
    if (k2 == key) return dd_enqueue(c, img, n_img, w, h, stride, det, desc);
  hipStream_t s = c->stream;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    c->dd_graphs = false;
    return dd_enqueue(c, img, n_img, w, h, stride, det, desc);
  }
  const int rc = dd_enqueue(c, img, n_img, w, h, stride, det, desc);
  hipGraph_t g = nullptr;
  const hipError_t e_end = hipStreamEndCapture(s, &g);
  hipGraphExec_t ex = nullptr;
  if (rc == MODS_OK && e_end == hipSuccess && g && !c->pyr_forked) {      // a linear recording: not replayed (above); nothing has run yet
    (void)hipGraphDestroy(g);
    if (c->dd_linear.size() >= 16) c->dd_linear.erase(c->dd_linear.begin());
    c->dd_linear.push_back(key);
    return dd_enqueue(c, img, n_img, w, h, stride, det, desc);
  }
  if (rc == MODS_OK && e_end == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
    (void)hipGraphDestroy(g);
    if (c->dd_cache.size() >= 8) { (void)hipGraphExecDestroy(c->dd_cache.front().second); c->dd_cache.erase(c->dd_cache.begin()); }
    c->dd_cache.emplace_back(key, ex);
    MODS_HIP_CHECK(hipGraphLaunch(ex, c->stream));
    c->dd_replays++;
    return MODS_OK;
  }
  // not capturable here (or the chain itself failed): nothing has run - clean up and issue the launches directly
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  c->pyr_side = false;                    // (a fork recorded into the dead capture)
  c->dd_graphs = false;
  c->omap_dirty = true;
  return dd_enqueue(c, img, n_img, w, h, stride, det, desc);
}

int mods_ctx_graphs(mods_ctx *c, int on) {
  if (!c) return MODS_E_ARG;
  c->dd_graphs = on != 0;
  if (!on) { dd_graph_drop(c); c->dd_linear.clear(); }
  mods::dev_state_changed(c);
  return MODS_OK;
}
long mods_ctx_graph_replays(const mods_ctx *c) { return c ? c->dd_replays : 0; }
long mods_ctx_u8_source_calls(const mods_ctx *c) { return c ? c->u8_source_calls : 0; }
long mods_ctx_u8_strip_calls(const mods_ctx *c) { return c ? c->u8_strip_calls : 0; }
int mods_ctx_u8_kernels(mods_ctx *c, int mask) {
  if (!c || mask > 255) { set_error("u8_kernels: bad argument"); return MODS_E_ARG; }
  c->u8_kernels = mask < 0 ? -1 : mask;
  mods::dev_state_changed(c);            // (a recorded detect + describe graph holds the other form's launches)
  return MODS_OK;
}

// the call behind both detect + describe entry points
static int dd_call(mods_ctx *c, const PixelSources &img, int n_img, int w, int h, int stride, const mods_hessaff_params *det,
                   const mods_describe_params *desc, int *n_detected_host, int *n_regions_host) {
  int rc;
  if ((rc = mods::dsp_check(c, desc))) return rc;      // (before the detector's launches)
  if ((rc = dd_run(c, img, n_img, w, h, stride, det, desc))) return rc;
  int *hc = c->host_counts;
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  for (int b = 0; b < n_img; b++) {
    if (hc[b] > c->max_cand) { set_error("NMS hit list overflow: %d > %d", hc[b], c->max_cand); return MODS_E_CAPACITY; }
    if (n_detected_host) n_detected_host[b] = hc[2 * c->batch + b];
    if (hc[3 * c->batch + b] > std::min(c->max_cand, 1 << 17)) { set_error("region list overflow: %d", hc[3 * c->batch + b]); return MODS_E_CAPACITY; }
    if (n_regions_host) n_regions_host[b] = hc[3 * c->batch + b];
  }
  c->last_region_counts.assign(hc + 3 * c->batch, hc + 3 * c->batch + n_img);
  c->last_inside_counts.assign(hc + 4 * c->batch, hc + 4 * c->batch + n_img);
  if (hc[5 * c->batch]) {
    MODS_HIP_CHECK(hipMemsetAsync(c->desc_err_dev, 0, sizeof(int), c->stream));
    set_error("measurement region larger than the descriptor scratch (P2 > 3*max(w,h) or > 4096 blur taps)");
    return MODS_E_CAPACITY;
  }
  return MODS_OK;
}

int mods_detect_describe_dev(mods_ctx *c, const float *img_dev, int n_img, int w, int h, int stride,
                             const mods_hessaff_params *det, const mods_describe_params *desc, int *n_detected_host,
                             int *n_regions_host) {
  if (!c || !img_dev || !det || !desc) { set_error("detect_describe: null argument"); return MODS_E_ARG; }
  if (w <= 0 || h <= 0 || (size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("detect_describe: image larger than the context"); return MODS_E_ARG; }
  if (n_img < 1 || n_img > c->batch) { set_error("detect_describe: %d images, context batch %d", n_img, c->batch); return MODS_E_ARG; }
  if (stride < w) { set_error("detect_describe: stride %d < width %d", stride, w); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  return dd_call(c, {img_dev}, n_img, w, h, stride, det, desc, n_detected_host, n_regions_host);
}

// 8-bit grey in HBM: converted (exactly) into input_dev, from which the scale space is built and the keypoints are detected as in
// mods_detect_describe_dev; orientation and description sample from the 8-bit images themselves in the kernels whose mask bit is on
// (pixel_sources.hpp) - (float)u8 at the load gives the fp32 copy's values, so the regions are the same to the bit.
// Rows that are not packed (stride != w) and the MSER detector take the fp32 copy throughout.
int mods_detect_describe_dev_u8(mods_ctx *c, const unsigned char *img_u8, int n_img, int w, int h, int stride,
                                const mods_hessaff_params *det, const mods_describe_params *desc, int *n_detected_host,
                                int *n_regions_host) {
  if (!c || !img_u8 || !det || !desc) { set_error("detect_describe_u8: null argument"); return MODS_E_ARG; }
  if (w <= 0 || h <= 0 || (size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("detect_describe_u8: image larger than the context"); return MODS_E_ARG; }
  if (n_img < 1 || n_img > c->batch) { set_error("detect_describe_u8: %d images, context batch %d", n_img, c->batch); return MODS_E_ARG; }
  if (stride < w) { set_error("detect_describe_u8: stride %d < width %d", stride, w); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  PixelSources img;
  const int rc = mods::u8_sources_launch(c, img_u8, n_img, w, h, stride, det->detectorType != MODS_DET_MSER, &img);
  if (rc) return rc;
  return dd_call(c, img, n_img, w, h, w, det, desc, n_detected_host, n_regions_host);
}

// ---- the strip layout of the 8-bit twin, for the tests: the header's functions as they are (no device), and the twin of a batch as the
// conversion launch makes it
int mods_u8_strips_layout(int w, int h, unsigned *max_width, unsigned *n_strips, unsigned *pitch, size_t *image_bytes) {
  if (max_width) *max_width = mods::kStripMaxW;
  if (!mods::strip_layout_ok(w, h)) { set_error("u8_strips_layout: %d x %d is outside the layout", w, h); return MODS_E_ARG; }
  if (n_strips) *n_strips = mods::strip_count(w);
  if (pitch) *pitch = mods::strip_pitch(h);
  if (image_bytes) *image_bytes = mods::strip_image_bytes(w, h);
  return MODS_OK;
}
// strip_of(x) for x = 0 .. n - 1
void mods_u8_strips_strip_of(unsigned n, unsigned *out) { for (unsigned x = 0; x < n; x++) out[x] = mods::strip_of(x); }
// strip_offset of every pair start of a w x h image: out[(h - 1)][(w - 1)], x <= w - 2, y <= h - 2
int mods_u8_strips_offsets(int w, int h, unsigned *out) {
  if (!out || !mods::strip_layout_ok(w, h)) { set_error("u8_strips_offsets: bad argument"); return MODS_E_ARG; }
  const unsigned pitch = mods::strip_pitch(h);
  for (int y = 0; y <= h - 2; y++)
    for (int x = 0; x <= w - 2; x++) out[(size_t)y * (w - 1) + x] = mods::strip_offset((unsigned)x, (unsigned)y, pitch);
  return MODS_OK;
}
// the batch [n_img][h][w] is staged `src_offset` (0 .. 15) bytes into the context's staging area, converted, and the twin that the
// conversion launch made is copied to out (n_img * strip_image_bytes)
int mods_u8_strips_fetch(mods_ctx *c, const unsigned char *img_u8_host, int n_img, int w, int h, int src_offset, unsigned char *out) {
  if (!c || !img_u8_host || !out) { set_error("u8_strips_fetch: null argument"); return MODS_E_ARG; }
  if (n_img < 1 || n_img > c->batch || src_offset < 0 || src_offset > 15) { set_error("u8_strips_fetch: bad argument"); return MODS_E_ARG; }
  if (w <= 0 || h <= 0 || (size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("u8_strips_fetch: image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc;
  if ((rc = mods::u8_stage_ensure(c))) return rc;
  const size_t n = (size_t)n_img * w * h;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, c->u8_stage_dev + src_offset, img_u8_host, n, hipMemcpyHostToDevice));
  if ((rc = mods::u8_to_f32_launch(c, c->u8_stage_dev + src_offset, n_img, w, h, w, c->input_dev, true))) return rc;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, out, c->u8_strip_dev.get(), mods::strip_image_bytes(w, h) * n_img, hipMemcpyDeviceToHost));
  return MODS_OK;
}

// Route the description of every following call through `fn` (NULL: back to the built-in RootSIFT).  The patches are
// ExtractPatchesColumn's (synth-detection.cpp:38-132; fp32, no photometric normalisation): patchSize x patchSize at mrSize.
int mods_ctx_set_external_descriptor(mods_ctx *c, mods_descriptor_fn fn, void *user, double mrSize, int patchSize) {
  if (!c) return MODS_E_ARG;
  c->ext_fn = fn; c->ext_user = user; c->ext_mr = mrSize; c->ext_ps = patchSize;
  c->ext_net = nullptr;                  // a slot holds a callback or a built-in network (nets.hip), never both
  return MODS_OK;
}

int mods_ctx_set_external_shape(mods_ctx *c, mods_descriptor_fn fn, void *user, double mrSize, int patchSize) {
  if (!c) return MODS_E_ARG;
  if (fn && (patchSize < 8 || patchSize > 63)) { set_error("external shape: patch size %d unsupported", patchSize); return MODS_E_ARG; }
  c->shape_fn = fn; c->shape_user = user; c->shape_mr = mrSize; c->shape_ps = patchSize;
  c->shape_net = nullptr;
  return MODS_OK;
}

int mods_ctx_set_external_orientation(mods_ctx *c, mods_descriptor_fn fn, void *user, double mrSize, int patchSize) {
  if (!c) return MODS_E_ARG;
  if (fn && (patchSize < 8 || patchSize > 63)) { set_error("external orientation: patch size %d unsupported", patchSize); return MODS_E_ARG; }
  c->ori_fn = fn; c->ori_user = user; c->ori_mr = mrSize; c->ori_ps = patchSize;
  c->ori_net = nullptr;
  return MODS_OK;
}
// host copy of the patches the describe stage extracted for image slot img in its last call ([n][ps][ps] fp32)
int mods_patches_fetch(mods_ctx *c, int img, int ps, float *out, int max_regions, int *n_out) {
  if (!c || !out || !n_out || img < 0 || img >= c->batch || !c->desc_scratch) { set_error("patches_fetch: nothing described"); return MODS_E_ARG; }
  const int reg_cap = std::min(c->max_cand, 1 << 17);
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int n = 0;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, &n, c->region_count + img, sizeof(int), hipMemcpyDeviceToHost));
  if (n > reg_cap) n = reg_cap;
  if (n > max_regions) { set_error("patch output overflow: %d > %d", n, max_regions); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(mods::copy_wait(c->stream, out, c->desc_scratch + (size_t)img * reg_cap * ps * ps, sizeof(float) * (size_t)n * ps * ps, hipMemcpyDeviceToHost));
  *n_out = n;
  return MODS_OK;
}

// size of the reference's unoriented ("None") region list of image slot img after the last describe call:
// detections whose centre, in the original frame, lies inside the image (imagerepresentation.cpp:867, 939)
// Baumberg work of image slot img, accumulated since mods_baumberg_stats_enable(ctx, 1): keypoints that entered the iteration and
// iterations run (each = one smmWindowSize^2 window of bilinear taps, affine.cpp:26-158).  Off by default: two atomics per keypoint.
int mods_baumberg_stats_enable(mods_ctx *c, int on) {
  if (!c) return MODS_E_ARG;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  c->baum_stats_dev.release();
  mods::dev_pool_reallocated(c);         // (a recorded detect + describe graph holds the old pointer)
  if (on) {
    const size_t n = 2 * 64 * (size_t)c->batch;
    MODS_HIP_CHECK(c->baum_stats_dev.reserve(n));
    MODS_HIP_CHECK(mods::fill_wait(c->stream, c->baum_stats_dev, 0, sizeof(unsigned long long) * n));
  }
  return MODS_OK;
}
int mods_baumberg_stats(mods_ctx *c, int img, unsigned long long *keypoints, unsigned long long *iterations) {
  if (!c || img < 0 || img >= c->batch || !c->baum_stats_dev) return MODS_E_ARG;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  unsigned long long v[2 * 64], kp = 0, it = 0;   // 64 slots per image (the kernel spreads its adds)
  MODS_HIP_CHECK(mods::copy_wait(c->stream, v, c->baum_stats_dev + 2 * 64 * (size_t)img, sizeof(v), hipMemcpyDeviceToHost));
  for (int q = 0; q < 64; q++) { kp += v[2 * q]; it += v[2 * q + 1]; }
  if (keypoints) *keypoints = kp;
  if (iterations) *iterations = it;
  return MODS_OK;
}

// ---- detection masks (detection_mask.hpp; the gate: detect.hip) ---------------------------------------------------------------
// Every change goes through dev_state_changed: a recorded detect + describe call holds the launches of the mask set it was recorded
// with (with or without the gate) and is not replayed across a change.  The mask's BYTES are read when the gate runs, so new
// contents behind an unchanged pointer need nothing.
static int detection_mask_set(mods_ctx *c, int image, const unsigned char *dev, int w, int h, int stride) {
  if ((int)c->det_masks.size() < c->batch) c->det_masks.resize((size_t)c->batch, mods::DetMaskDev{nullptr, 0, 0, 0, 0});
  if (dev) {     // the gate's table and counters, here and not in the first masked call: that call then changes no pool
    MODS_HIP_CHECK(hipSetDevice(c->device));
    MODS_HIP_CHECK(mods::reserve_pool(c, c->gate_tab_dev, (size_t)c->batch, (size_t)c->batch));
    MODS_HIP_CHECK(mods::reserve_pool(c, c->gate_counts_dev, 2 * (size_t)c->batch, 2 * (size_t)c->batch));
  }
  c->det_masks[image] = dev ? mods::DetMaskDev{dev, w, h, stride, 0} : mods::DetMaskDev{nullptr, 0, 0, 0, 0};
  mods::dev_state_changed(c);
  return MODS_OK;
}
static int detection_mask_args(mods_ctx *c, int image, const void *mask, int w, int h, int stride, const char *who) {
  if (!c) { set_error("%s: null context", who); return MODS_E_ARG; }
  if (image < 0 || image >= c->batch) { set_error("%s: image %d, context batch %d", who, image, c->batch); return MODS_E_ARG; }
  if (mask && (w <= 0 || h <= 0 || stride < w)) { set_error("%s: a mask of %d x %d with row stride %d", who, w, h, stride); return MODS_E_ARG; }
  return MODS_OK;
}
int mods_ctx_detection_mask_dev(mods_ctx *c, int image, const unsigned char *mask_dev, int w, int h, int stride) {
  const int rc = detection_mask_args(c, image, mask_dev, w, h, stride, "detection_mask_dev");
  if (rc) return rc;
  return detection_mask_set(c, image, mask_dev, w, h, stride);
}
int mods_ctx_detection_mask(mods_ctx *c, int image, const unsigned char *mask_host, int w, int h, int stride) {
  const int rc = detection_mask_args(c, image, mask_host, w, h, stride, "detection_mask");
  if (rc) return rc;
  if (!mask_host) return detection_mask_set(c, image, nullptr, 0, 0, 0);
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((int)c->det_mask_own.size() < c->batch) c->det_mask_own.resize((size_t)c->batch);
  mods::Buf<unsigned char> &own = c->det_mask_own[image];
  const size_t bytes = (size_t)w * h;
  MODS_HIP_CHECK(mods::reserve_pool(c, own, bytes, bytes));
  // the context's copy is dense; ordered on the stream behind whatever still reads the previous contents
  MODS_HIP_CHECK(hipMemcpy2DAsync(own, (size_t)w, mask_host, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return detection_mask_set(c, image, own, w, h, w);
}
int mods_ctx_detection_masks_clear(mods_ctx *c) {
  if (!c) { set_error("detection_masks_clear: null context"); return MODS_E_ARG; }
  for (auto &m : c->det_masks) m = mods::DetMaskDev{nullptr, 0, 0, 0, 0};
  mods::dev_state_changed(c);
  return MODS_OK;
}
int mods_ctx_detection_mask_counts(mods_ctx *c, int image, int *n_accepted, int *n_kept) {
  if (!c || image < 0 || image >= c->batch) { set_error("detection_mask_counts: bad argument"); return MODS_E_ARG; }
  int v[2] = {-1, -1};
  if (c->gate_ladder_last) {
    if (image < 2 && image < (int)c->det_masks.size() && c->det_masks[image].mask) { v[0] = (int)c->gate_ladder[2 * image]; v[1] = (int)c->gate_ladder[2 * image + 1]; }
  } else if (image < (int)c->gate_had_mask.size() && c->gate_had_mask[image] && c->gate_counts_dev) {
    MODS_HIP_CHECK(hipSetDevice(c->device));
    MODS_HIP_CHECK(mods::stream_wait(c->stream));
    MODS_HIP_CHECK(mods::copy_wait(c->stream, v, c->gate_counts_dev + 2 * (size_t)image, sizeof(v), hipMemcpyDeviceToHost));
  }
  if (n_accepted) *n_accepted = v[0];
  if (n_kept) *n_kept = v[1];
  return MODS_OK;
}
int mods_detection_mask_test(const unsigned char *mask, int w, int h, int stride, double x, double y) {
  if (!mask || w <= 0 || h <= 0 || stride < w) return 0;
  return mods::detection_mask_on(mask, w, h, stride, x, y) ? 1 : 0;
}

int mods_unoriented_count(mods_ctx *c, int img) {
  if (!c || img < 0 || img >= (int)c->last_inside_counts.size()) return 0;
  return c->last_inside_counts[img];
}

int mods_regions_fetch(mods_ctx *c, int img, mods_region *out, int max_out, int *n_out) {
  if (!c || img < 0 || img >= c->batch || !n_out) return MODS_E_ARG;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int n = 0;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, &n, c->region_count + img, sizeof(int), hipMemcpyDeviceToHost));
  *n_out = n;
  if (out) {
    if (n > max_out) { set_error("region output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
    MODS_HIP_CHECK(mods::copy_wait(c->stream, out, c->regions_dev + (size_t)img * c->max_cand, sizeof(mods_region) * n, hipMemcpyDeviceToHost));
  }
  return MODS_OK;
}

int mods_regions_fetch_half(mods_ctx *c, int img, mods_region *out, int max_out, int *n_out) {
  if (!c || img < 0 || img >= c->batch || !n_out) return MODS_E_ARG;
  if (!c->have_half || !c->regions_half_dev) { set_error("no HalfRootSIFT descriptors: the last describe call did not ask for them"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int n = 0;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, &n, c->region_count + img, sizeof(int), hipMemcpyDeviceToHost));
  *n_out = n;
  if (out) {
    if (n > max_out) { set_error("region output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
    MODS_HIP_CHECK(mods::copy_wait(c->stream, out, c->regions_half_dev + (size_t)img * c->max_cand, sizeof(mods_region) * n, hipMemcpyDeviceToHost));
  }
  return MODS_OK;
}
const mods_region *mods_regions_half_dev(mods_ctx *c, int img) {
  return (c && c->have_half && c->regions_half_dev) ? c->regions_half_dev + (size_t)img * c->max_cand : nullptr;
}

int mods_orient_describe(mods_ctx *c, const float *img, int w, int h, int stride, const mods_affkey *keys, int n_keys,
                         const mods_describe_params *par, mods_region *out, int max_out, int *n_out) {
  if (!c || !img || !par || !n_out || (n_keys > 0 && !keys)) { set_error("orient_describe: null argument"); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  if (n_keys > c->max_cand) { set_error("too many keypoints for the context: %d > %d", n_keys, c->max_cand); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(hipMemcpy2DAsync(c->input_dev, sizeof(float) * w, img, sizeof(float) * stride, sizeof(float) * w, h,
                                  hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(c->keys_dev, keys, sizeof(mods_affkey) * n_keys, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(c->cand_count + 2 * c->batch, &n_keys, sizeof(int), hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));   // n_keys is a stack variable
  int rc = describe_run(c, {c->input_dev}, 1, w, h, par);
  if (rc) return rc;
  if ((rc = mods_regions_fetch(c, 0, out, max_out, n_out))) return rc;
  return check_desc_err(c);
}

// mods_orient_describe for an 8-bit grey host image: staged packed in u8_stage_dev, converted (exactly) into input_dev, and the 8-bit
// copy is the call's sampling source in the kernels whose mask bit is on (mods_ctx_u8_kernels) - the given keypoints reach every size
// class of those kernels, which the detector's own keypoints on an affordable image do not.  Everything that does not need the
// context is checked first, so that a bad call is refused without a device.
int mods_orient_describe_u8(mods_ctx *c, const unsigned char *img_u8, int w, int h, int stride, const mods_affkey *keys, int n_keys,
                            const mods_describe_params *par, mods_region *out, int max_out, int *n_out) {
  if (!img_u8 || !par || !n_out || (n_keys > 0 && !keys)) { set_error("orient_describe_u8: null argument"); return MODS_E_ARG; }
  if (w < 1 || h < 1) { set_error("orient_describe_u8: image size %d x %d", w, h); return MODS_E_ARG; }
  if (stride < w) { set_error("orient_describe_u8: stride %d < width %d", stride, w); return MODS_E_ARG; }
  if (n_keys < 0) { set_error("orient_describe_u8: %d keypoints", n_keys); return MODS_E_ARG; }
  if (!c) { set_error("orient_describe_u8: null context"); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("orient_describe_u8: image %d x %d larger than the context", w, h); return MODS_E_ARG; }
  if (n_keys > c->max_cand) { set_error("orient_describe_u8: too many keypoints for the context: %d > %d", n_keys, c->max_cand); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc;
  if ((rc = mods::u8_stage_ensure(c))) return rc;
  MODS_HIP_CHECK(hipMemcpy2DAsync(c->u8_stage_dev, w, img_u8, stride, w, h, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(c->keys_dev, keys, sizeof(mods_affkey) * n_keys, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(c->cand_count + 2 * c->batch, &n_keys, sizeof(int), hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));   // n_keys is a stack variable
  PixelSources img;
  if ((rc = mods::u8_sources_launch(c, c->u8_stage_dev, 1, w, h, w, true, &img))) return rc;
  if ((rc = describe_run(c, img, 1, w, h, par))) return rc;
  if ((rc = mods_regions_fetch(c, 0, out, max_out, n_out))) return rc;
  return check_desc_err(c);
}

int mods_dominant_angle(mods_ctx *c, const float *patch, int ps, double th, float *angle, int *found) {
  mods_describe_params dp = {5.1962, ps, 1, th, 5.1962, c->desc_ps ? c->desc_ps : 41, 1, 1, 0.2};
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc = describe_configure(c, &dp);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, patch, sizeof(float) * ps * ps, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_dominant_angle_test(c, c->input_dev, ps, th, c->tmp_dev))) return rc;
  float res[2];
  MODS_HIP_CHECK(hipMemcpyAsync(res, c->tmp_dev, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  *found = res[0] != 0.f;
  *angle = res[1];
  return MODS_OK;
}

int mods_selftest_fast_sqrt(mods_ctx *c, unsigned long long *out5) {
  if (!c || !out5) { set_error("selftest: null argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  return launch_fast_sqrt_selftest(c, out5);
}

int mods_sift_patch(mods_ctx *c, const float *patch, int ps, int rootsift, double maxBinValue, uint8_t *out128) {
  mods_describe_params dp = {5.1962, c->desc_ori_ps ? c->desc_ori_ps : 32, 1, 0.8, 5.1962, ps, 1, rootsift, maxBinValue};
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc = describe_configure(c, &dp);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, patch, sizeof(float) * ps * ps, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_sift_patch_test(c, c->input_dev, ps, rootsift, maxBinValue, (uint8_t *)c->tmp_dev.get()))) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(out128, c->tmp_dev, 128, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

// ---- domain-size pooling of the SIFT descriptor (contract in include/mods_hip.h) ----------------
static int dsp_args(const char *who, int K, double a, double b) {
  if (K == 0 || K == 1) return MODS_OK;
  if (K < 0 || K > 8) { set_error("%s: numScales %d (0 or 1: off; 2 .. 8)", who, K); return MODS_E_ARG; }
  if (!std::isfinite(a) || !(a > 0)) { set_error("%s: startCoef %g (finite, > 0)", who, a); return MODS_E_ARG; }
  if (!std::isfinite(b) || !(b > a) || b > 4) { set_error("%s: endCoef %g (finite, startCoef < endCoef <= 4)", who, b); return MODS_E_ARG; }
  return MODS_OK;
}
int mods_ctx_domain_pooling(mods_ctx *c, int numScales, double startCoef, double endCoef) {
  const int rc = dsp_args("domain_pooling", numScales, startCoef, endCoef);
  if (rc) return rc;
  if (!c) { set_error("domain_pooling: null context"); return MODS_E_ARG; }
  const bool on = numScales >= 2;
  c->dsp_scales = on ? numScales : 0;
  c->dsp_start = on ? startCoef : 0;
  c->dsp_end = on ? endCoef : 0;
  mods::dev_state_changed(c);        // (recorded launch chains are not replayed across the change)
  return MODS_OK;
}
int mods_ctx_domain_pooling_get(const mods_ctx *c, int *numScales, double *startCoef, double *endCoef) {
  if (!c) { set_error("domain_pooling_get: null context"); return MODS_E_ARG; }
  if (numScales) *numScales = c->dsp_scales;
  if (startCoef) *startCoef = c->dsp_start;
  if (endCoef) *endCoef = c->dsp_end;
  return MODS_OK;
}
// the pooled twin of mods_sift_patch: K host patches [K][ps][ps] of one region through the accumulate and finish kernels
int mods_test_sift_pooled(mods_ctx *c, const float *patches, int K, int ps, int rootsift, int half, int photoNorm, double maxBinValue,
                          uint8_t *out128) {
  if (!c || !patches || !out128) { set_error("test_sift_pooled: null argument"); return MODS_E_ARG; }
  if (K < 1 || K > 8) { set_error("test_sift_pooled: %d patches (1 .. 8)", K); return MODS_E_ARG; }
  if ((size_t)K * ps * ps > (size_t)c->max_w * c->max_h * c->batch) { set_error("test_sift_pooled: the patches do not fit the context's input buffer"); return MODS_E_ARG; }
  mods_describe_params dp = {5.1962, c->desc_ori_ps ? c->desc_ori_ps : 32, 1, 0.8, 5.1962, ps, photoNorm, rootsift, maxBinValue};
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc = describe_configure(c, &dp);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, patches, sizeof(float) * (size_t)K * ps * ps, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_sift_pooled_test(c, c->input_dev, K, ps, rootsift, half, photoNorm, maxBinValue, (uint8_t *)c->tmp_dev.get()))) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(out128, c->tmp_dev, 128, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

// ---- matching ----------------------------------------------------------------------------------
// The packed output of the last search (n tentatives | correspondences | frames, common.hpp) in ONE device-to-host copy,
// split into the caller's arrays (any of them may be null).  Synchronises the context's stream.
int mods_match_copy_out(mods_ctx *c, int n, mods_tentative *tent, double *u6, double *laf) {
  if (n <= 0) return MODS_OK;
  static thread_local std::vector<char> stage;
  stage.resize(tent_bytes((size_t)n));
  MODS_HIP_CHECK(hipMemcpyAsync(stage.data(), c->m_tent, stage.size(), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  tent_unpack(stage.data(), (size_t)n, tent, u6, laf);
  return MODS_OK;
}

int mods_match_fetch_internal(mods_ctx *c, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  const int n = read_slot(c->m_count, count_slot());
  *n_out = n;
  if (n > max_out) { set_error("tentative output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
  return mods_match_copy_out(c, n, out, u6_out, laf_out);
}

// what the two searches over host lists share: the argument checks and the upload into the context's staging lists
static int match_upload(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, const int *n_out) {
  if (!c || !n_out || (n_q > 0 && !q) || (n_t > 0 && !t)) { set_error("match: null argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc = match_ensure_buffers(c);
  if (rc) return rc;
  if (n_q > c->max_cand || n_t > c->max_cand) { set_error("match: list larger than the context capacity"); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipMemcpyAsync(c->m_regs, q, sizeof(mods_region) * n_q, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(c->m_regs + c->max_cand, t, sizeof(mods_region) * n_t, hipMemcpyHostToDevice, c->stream));
  return MODS_OK;
}

int mods_match_fginn(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, double ratio,
                     double contradDist, int nn, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out) {
  int rc = match_upload(c, q, n_q, t, n_t, n_out);
  if (rc || (rc = match_run(c, c->m_regs, n_q, c->m_regs + c->max_cand, n_t, ratio, contradDist, nn))) return rc;
  return mods_match_fetch_internal(c, out, u6_out, laf_out, max_out, n_out);
}

// MatchFLANNDistance (matching.cpp:572-633): nearest neighbour by Hamming distance over the descriptor bytes, kept when the
// distance is at most (int)(float)threshold; exact search
int mods_match_distance(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, double threshold,
                        mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out) {
  int rc = match_upload(c, q, n_q, t, n_t, n_out);
  if (rc || (rc = match_run_distance(c, c->m_regs, n_q, c->m_regs + c->max_cand, n_t, threshold))) return rc;
  return mods_match_fetch_internal(c, out, u6_out, laf_out, max_out, n_out);
}

int mods_match_dev(mods_ctx *c, int img_q, int img_t, double ratio, double contradDist, int nn, mods_tentative *out,
                   double *u6_out, double *laf_out, int max_out, int *n_out) {
  if (!c || !n_out) { set_error("match: null argument"); return MODS_E_ARG; }
  const int nb = (int)c->last_region_counts.size();
  if (img_q < 0 || img_q >= nb || img_t < 0 || img_t >= nb) { set_error("match: image index outside the last described batch"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc = match_run(c, c->regions_dev + (size_t)img_q * c->max_cand, c->last_region_counts[img_q],
                     c->regions_dev + (size_t)img_t * c->max_cand, c->last_region_counts[img_t], ratio, contradDist, nn);
  if (rc) return rc;
  return mods_match_fetch_internal(c, out, u6_out, laf_out, max_out, n_out);
}

// The k nearest trains of every query (knn.hip), host lists staged as mods_match_fginn stages them.  The matcher's scratch and its
// "last search" are not touched: the search packs into buffers of its own
int mods_match_knn(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, int k, int *idx_out, int *d2_out) {
  if (!c || (n_q > 0 && !q) || (n_t > 0 && !t)) { set_error("match_knn: null argument"); return MODS_E_ARG; }
  if (n_q < 0 || n_t < 0) { set_error("match_knn: negative count (%d queries, %d trains)", n_q, n_t); return MODS_E_ARG; }
  int rc = knn_check("match_knn", k, idx_out, d2_out);
  if (rc) return rc;
  if (n_q > c->max_cand || n_t > c->max_cand) { set_error("match_knn: list larger than the context capacity"); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if (n_q > 0 && n_t > 0) {
    MODS_HIP_CHECK(mods::reserve_scratch(c, c->m_regs, 2 * (size_t)c->max_cand, 2 * (size_t)c->max_cand));
    MODS_HIP_CHECK(hipMemcpyAsync(c->m_regs, q, sizeof(mods_region) * n_q, hipMemcpyHostToDevice, c->stream));
    MODS_HIP_CHECK(hipMemcpyAsync(c->m_regs + c->max_cand, t, sizeof(mods_region) * n_t, hipMemcpyHostToDevice, c->stream));
  }
  return knn_search(c, "match_knn", c->m_regs, n_q, c->m_regs + c->max_cand, n_t, k, idx_out, d2_out);
}

int mods_match_knn_dev(mods_ctx *c, int img_q, int img_t, int k, int *idx_out, int *d2_out) {
  if (!c) { set_error("match_knn_dev: null context"); return MODS_E_ARG; }
  int rc = knn_check("match_knn_dev", k, idx_out, d2_out);
  if (rc) return rc;
  const int nb = (int)c->last_region_counts.size();
  if (img_q < 0 || img_q >= nb || img_t < 0 || img_t >= nb) { set_error("match_knn_dev: image index outside the last described batch"); return MODS_E_ARG; }
  if (c->last_region_counts[img_q] > c->max_cand || c->last_region_counts[img_t] > c->max_cand) { set_error("match_knn_dev: list larger than the context capacity"); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  return knn_search(c, "match_knn_dev", c->regions_dev + (size_t)img_q * c->max_cand, c->last_region_counts[img_q],
                    c->regions_dev + (size_t)img_t * c->max_cand, c->last_region_counts[img_t], k, idx_out, d2_out);
}

// DuplicateFiltering, matching.cpp:2615-2679: optional stable sort, then the first correspondence
// (in list order) of every group whose two endpoints lie within r of each other survives.  A uniform
// grid over the first-image points (cell = r) bounds the candidates to the 3x3 neighbourhood; the
// accept/reject sequence is the reference's.
int mods_duplicate_filter(mods_tentative *tent, double *u6, double *laf, int n, double r, int mode, int *n_out) {
  if (!n_out || (n > 0 && (!tent || !u6))) { set_error("duplicate_filter: null argument"); return MODS_E_ARG; }
  *n_out = n;
  if (r <= 0 || n <= 0) return MODS_OK;
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  if (mode >= 1 && mode <= 3) {
    // (key, index) pairs sorted by value: the order of a stable sort by key, without a random access per comparison
    if (mode == 3 && !laf) { set_error("duplicate_filter: biggerRegion needs the local affine frames"); return MODS_E_ARG; }   // CompareCorrespondenceByScale, matching.cpp:74
    std::vector<std::pair<double, int>> keyed(n);
    for (int i = 0; i < n; i++)
      keyed[i] = {mode == 1 ? std::fabs(tent[i].ratio) : mode == 2 ? std::fabs((double)tent[i].d1) : std::fabs(laf[(size_t)i * 14 + 6]), i};
    std::sort(keyed.begin(), keyed.end());
    for (int i = 0; i < n; i++) order[i] = keyed[i].second;
  }
  std::vector<mods_tentative> ts(n);
  std::vector<double> us((size_t)n * 6), ls(laf ? (size_t)n * 14 : 0);
  for (int i = 0; i < n; i++) {
    ts[i] = tent[order[i]];
    memcpy(&us[(size_t)i * 6], &u6[(size_t)order[i] * 6], 6 * sizeof(double));
    if (laf) memcpy(&ls[(size_t)i * 14], &laf[(size_t)order[i] * 14], 14 * sizeof(double));
  }
  const double r_sq = r * r;
  // hash grid of the kept correspondences, keyed by the first-image cell: chained buckets in two flat arrays (which
  // kept correspondence is met first inside a cell does not matter, only whether one is met)
  // ~8 buckets per correspondence: a probe of an empty neighbour cell then rarely walks a chain of unrelated entries (with a fixed
  // 16 k buckets the 24 k correspondences of a 4096^2 pair cost ~13 useless distance tests each: 8 of the pair's 43 ms)
  size_t kBuckets = 1 << 14;
  while (kBuckets < (size_t)n * 8) kBuckets <<= 1;
  std::vector<int> head(kBuckets, -1), next(n);
  auto cell_of = [&](double v) { return (long long)std::floor(v / r); };
  auto hash = [&](long long cx, long long cy) { return (size_t)(((unsigned long long)cx * 73856093ull) ^ ((unsigned long long)cy * 19349663ull)) & (kBuckets - 1); };
  std::vector<char> keep(n, 0);
  int m = 0;
  for (int j = 0; j < n; j++) {
    const double x1 = us[(size_t)j * 6], y1 = us[(size_t)j * 6 + 1], x2 = us[(size_t)j * 6 + 3], y2 = us[(size_t)j * 6 + 4];
    const long long cx = cell_of(x1), cy = cell_of(y1);
    bool dup = false;
    for (long long dy = -1; dy <= 1 && !dup; dy++)
      for (long long dx = -1; dx <= 1 && !dup; dx++)
        for (int i = head[hash(cx + dx, cy + dy)]; i >= 0; i = next[i]) {
          double ex = us[(size_t)i * 6] - x1, ey = us[(size_t)i * 6 + 1] - y1;
          if (ex * ex + ey * ey > r_sq) continue;
          ex = us[(size_t)i * 6 + 3] - x2; ey = us[(size_t)i * 6 + 4] - y2;
          if (ex * ex + ey * ey <= r_sq) { dup = true; break; }
        }
    if (!dup) { keep[j] = 1; const size_t b = hash(cx, cy); next[j] = head[b]; head[b] = j; }
  }
  for (int j = 0; j < n; j++)
    if (keep[j]) {
      tent[m] = ts[j];
      memcpy(&u6[(size_t)m * 6], &us[(size_t)j * 6], 6 * sizeof(double));
      if (laf) memcpy(&laf[(size_t)m * 14], &ls[(size_t)j * 14], 14 * sizeof(double));
      m++;
    }
  *n_out = m;
  return MODS_OK;
}

// ---- verification ----------------------------------------------------------------------------------
// cv::invert(3x3, DECOMP_LU) as OpenCV evaluates small matrices: determinant and cofactors in
// double (OpenCV is not in the image: closed form assumed; result 0 when the determinant is 0).
static bool invert3(const double *S, double *t) {
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  if (d == 0) { for (int i = 0; i < 9; i++) t[i] = 0; return false; }
  d = 1. / d;
  t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
  t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
  t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
  t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
  t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
  t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
  t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
  return true;
}

}  // extern "C"

namespace mods {
// H_LAF_check (matching.cpp:250-308), shared by mods_loransac_h and mods_orsa_h: correspondence i of cur survives when the
// symmetric transfer errors (HDsSymMax) of its centre and of the two frame points k_sigma along the local affine frame's axes sum
// to at most bound^2.  H21: the model from image 2 to image 1, row-major (its inverse is taken here, as the error function takes
// it); laf: n x 14 frames; bound <= 0 or laf == NULL: nothing is checked.  ops = the host SIMD table, evaluated lanes-wide over
// structure-of-arrays copies (every lane does the scalar code's operations in its order: the same bits); nullptr: the scalar
// statement.
void h_laf_check(const double *laf, const double *H21, double bound, const rs::SimdOps *ops, std::vector<int> &cur) {
  if (!(bound > 0) || !laf) return;
  const double ks = 3.0;   // matching.cpp:171
  const double Hd[9] = {H21[0], H21[3], H21[6], H21[1], H21[4], H21[7], H21[2], H21[5], H21[8]};   // degensac's layout
  if (ops) {
    const int m = (int)cur.size();
    if (m == 0) return;
    const int m_pad = (m + rs::SIMD_PAD - 1) / rs::SIMD_PAD * rs::SIMD_PAD;
    std::vector<double> buf((size_t)7 * m_pad);
    double *c0 = buf.data(), *c1 = c0 + m_pad, *c2 = c1 + m_pad, *c3 = c2 + m_pad, *e0 = c3 + m_pad, *e1 = e0 + m_pad, *e2 = e1 + m_pad;
    const double *soa[5] = {c0, c1, c2, c3, c3};
    rs::SymH sh;
    rs::sym_prepare(Hd, &sh);
    // the centre pair is the correspondence itself (u[0..1], u[3..4] = f[0..1], f[7..8]); then the two frame points
    for (int k = 0; k < m_pad; k++) { const double *f = laf + (size_t)cur[k < m ? k : m - 1] * 14; c0[k] = f[0]; c1[k] = f[1]; c2[k] = f[7]; c3[k] = f[8]; }
    ops->hsym_all(soa, m_pad, sh.H1, sh.Hinv, 1, e0);
    for (int k = 0; k < m_pad; k++) {
      const double *f = laf + (size_t)cur[k < m ? k : m - 1] * 14;
      c0[k] = f[0] + ks * f[3] * f[6]; c1[k] = f[1] + ks * f[5] * f[6]; c2[k] = f[7] + ks * f[10] * f[13]; c3[k] = f[8] + ks * f[12] * f[13];
    }
    ops->hsym_all(soa, m_pad, sh.H1, sh.Hinv, 1, e1);
    for (int k = 0; k < m_pad; k++) {
      const double *f = laf + (size_t)cur[k < m ? k : m - 1] * 14;
      c0[k] = f[0] + ks * f[2] * f[6]; c1[k] = f[1] + ks * f[4] * f[6]; c2[k] = f[7] + ks * f[9] * f[13]; c3[k] = f[8] + ks * f[11] * f[13];
    }
    ops->hsym_all(soa, m_pad, sh.H1, sh.Hinv, 1, e2);
    int kept = 0;
    for (int k = 0; k < m; k++) {
      const double sumErr = std::sqrt(e0[k] + e1[k] + e2[k]);
      if (!(sumErr > bound)) cur[kept++] = cur[k];
    }
    cur.resize(kept);
    return;
  }
  std::vector<int> good;
  for (int i : cur) {
    const double *f = laf + (size_t)i * 14;
    double u[18], err[3];
    u[0] = f[0]; u[1] = f[1]; u[2] = 1.0;
    u[3] = f[7]; u[4] = f[8]; u[5] = 1.0;
    u[6] = u[0] + ks * f[3] * f[6]; u[7] = u[1] + ks * f[5] * f[6]; u[8] = 1.0;
    u[9] = u[3] + ks * f[10] * f[13]; u[10] = u[4] + ks * f[12] * f[13]; u[11] = 1.0;
    u[12] = u[0] + ks * f[2] * f[6]; u[13] = u[1] + ks * f[4] * f[6]; u[14] = 1.0;
    u[15] = u[3] + ks * f[9] * f[13]; u[16] = u[4] + ks * f[11] * f[13]; u[17] = 1.0;
    HDsSymMax(nullptr, u, Hd, err, 3);
    const double sumErr = std::sqrt(err[0] + err[1] + err[2]);
    if (!(sumErr > bound)) good.push_back(i);
  }
  cur.swap(good);
}

// cv::invert of a 3 x 3 matrix as the homography branch takes it, for the other verifiers
bool invert3x3(const double *S, double *t) { return invert3(S, t); }
}  // namespace mods

extern "C" {

// What LORANSACFiltering does with the model of the homography branch (matching.cpp:745-805): H -> row-major img1->img2 by inv(H^T),
// NaiveHCheck (10 px, :1014-1043) over the RANSAC inliers, H_LAF_check (:250-308: HDsSymMax on the three frame points).  mask[i] = 1
// for the correspondences that survive; returns their number.  ops = the host SIMD table (ransac_simd.hpp): both checks are the
// symmetric transfer error of point pairs, evaluated lanes-wide over structure-of-arrays copies of the inliers (every lane does the
// scalar code's operations in its order: the same bits); ops = nullptr runs the scalar statement (kept for the self-test).
static int h_post_checks(const double *u6, const double *laf, int n, const unsigned char *inl2, const double *Hloran,
                         const mods_ransac_params *par, const mods::rs::SimdOps *ops, unsigned char *mask, double *H_out) {
  const int MIN_POINTS = 8;
  // H: inv(Hloran^T); reading the column-major h as a row-major matrix is H^T, its transpose is h read column-wise
  const double Ht[9] = {Hloran[0], Hloran[3], Hloran[6], Hloran[1], Hloran[4], Hloran[7], Hloran[2], Hloran[5], Hloran[8]};
  double Hinv[9];
  invert3(Ht, Hinv);
  bool nonzero = false;
  for (int i = 0; i < 9; i++) nonzero = nonzero || (Hinv[i] != 0.0);
  if (!nonzero) return 0;
  for (int i = 0; i < 9; i++) H_out[i] = Hinv[i];
  std::vector<int> cur;
  for (int i = 0; i < n; i++) if (inl2[i]) cur.push_back(i);
  const double affineFerror = 3.0 * par->HLAFCoef * par->err_threshold;
  const double err_sq = 10.0 * 10.0;
  double Hi[9];
  invert3(Hinv, Hi);
  if (ops) {
    const int m = (int)cur.size();
    if (m == 0) return 0;
    const int m_pad = (m + mods::rs::SIMD_PAD - 1) / mods::rs::SIMD_PAD * mods::rs::SIMD_PAD;
    std::vector<double> buf((size_t)6 * m_pad);
    double *c0 = buf.data(), *c1 = c0 + m_pad, *c2 = c1 + m_pad, *c3 = c2 + m_pad, *e0 = c3 + m_pad, *e1 = e0 + m_pad;
    const double *soa[5] = {c0, c1, c2, c3, c3};
    for (int k = 0; k < m_pad; k++) {
      const double *p = u6 + (size_t)cur[k < m ? k : m - 1] * 6;
      c0[k] = p[0]; c1[k] = p[1]; c2[k] = p[3]; c3[k] = p[4];
    }
    ops->hsym_both_all(soa, m_pad, Hinv, Hi, e0, e1);
    int ok = 0;
    for (int k = 0; k < m; k++) if ((e0[k] <= err_sq) && (e1[k] <= err_sq)) ok++;
    if (ok < MIN_POINTS) return 0;
    mods::h_laf_check(laf, Ht, affineFerror, ops, cur);
  } else {
    // NaiveHCheck over the RANSAC inliers
    {
      int ok = 0;
      for (int i : cur) {
        const double *p = u6 + (size_t)i * 6;
        const double *Hm = Hinv;
        double xa = (Hm[0] * p[0] + Hm[1] * p[1] + Hm[2]) / (Hm[6] * p[0] + Hm[7] * p[1] + Hm[8]);
        double ya = (Hm[3] * p[0] + Hm[4] * p[1] + Hm[5]) / (Hm[6] * p[0] + Hm[7] * p[1] + Hm[8]);
        const double d1 = (p[3] - xa) * (p[3] - xa) + (p[4] - ya) * (p[4] - ya);
        xa = (Hi[0] * p[3] + Hi[1] * p[4] + Hi[2]) / (Hi[6] * p[3] + Hi[7] * p[4] + Hi[8]);
        ya = (Hi[3] * p[3] + Hi[4] * p[4] + Hi[5]) / (Hi[6] * p[3] + Hi[7] * p[4] + Hi[8]);
        const double d2 = (p[0] - xa) * (p[0] - xa) + (p[1] - ya) * (p[1] - ya);
        if ((d1 <= err_sq) && (d2 <= err_sq)) ok++;
      }
      if (ok < MIN_POINTS) cur.clear();
    }
    mods::h_laf_check(laf, Ht, affineFerror, nullptr, cur);
  }
  if ((int)cur.size() < MIN_POINTS) cur.clear();
  for (int i : cur) mask[i] = 1;
  return (int)cur.size();
}

// LORANSACFiltering for the homography branch (useF = 0), matching.cpp:637-805: degensac LO-RANSAC,
// H -> row-major img1->img2 by inv(H^T), NaiveHCheck (10 px, :1014-1043), H_LAF_check (:250-308).
// mask[i] = 1 for the correspondences that survive every check.
// clock of the MODS_RANSAC_PROF lines: wall time, or the calling thread's CPU time with MODS_RANSAC_PROF=cpu (ransac.hip: rs_now_us)
static double prof_ms() {
  if (ransac_profile_mode() == 2) { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
  return now_ms();
}

int mods_loransac_h(const double *u6, const double *laf, int n, const mods_ransac_params *par, unsigned char *mask, double *H_out,
                    int *n_inliers, int *stats3) {
  const double t_enter = prof_ms();
  if (!par || !mask || !H_out || !n_inliers || (n > 0 && !u6)) { set_error("loransac_h: null argument"); return MODS_E_ARG; }
  *n_inliers = 0;
  for (int i = 0; i < 9; i++) H_out[i] = -1;   // TentativeCorrespListExt(): H[i] = -1 (matching.hpp:92-99)
  for (int i = 0; i < n; i++) mask[i] = 0;
  if (stats3) { stats3[0] = stats3[1] = stats3[2] = 0; }
  const int MIN_POINTS = 8;
  if (n < MIN_POINTS) return MODS_OK;
  int max_samples = par->max_samples;
  if (n <= 20) max_samples = 1000;
  std::vector<double> u2(u6, u6 + (size_t)n * 6);
  std::vector<unsigned char> inl2(n);
  std::vector<int> data_out(18);   // (the reference sizes it 18 n, matching.cpp:700; three counters are written)
  double Hloran[9];
  void (*f0)(const double *, const double *, const double *, double *, int);
  void (*f1)(const double *, const double *, const double *, double *, int, int *, int);
  void (*f2)(const double *, const double *, const double *, double *, int, int *, int);
  if (par->errorType == 0) { f0 = &HDs; f1 = &HDsi; f2 = &HDsidx; }
  else if (par->errorType == 1) { f0 = &HDsSymMax; f1 = &HDsiSymMax; f2 = &HDsSymidxMax; }
  else { f0 = &HDsSym; f1 = &HDsiSym; f2 = &HDsSymidx; }
  exp_ransacHcustom(u2.data(), n, par->err_threshold * par->err_threshold, par->confidence, max_samples, Hloran, inl2.data(), 4,
                    data_out.data(), 1, 0, nullptr, f0, f1, f2, par->doSymmCheck);   // (no residual rows: nobody reads them here)
  if (mods::ransac_failed()) return MODS_E_HIP;   // device failure inside the control loop; mods_last_error() says which
  const double t_post0 = prof_ms();
  if (stats3) { stats3[0] = data_out[0]; stats3[1] = data_out[1]; stats3[2] = data_out[2]; }
  *n_inliers = h_post_checks(u6, laf, n, inl2.data(), Hloran, par, mods::rs::simd_ops(), mask, H_out);
  if (ransac_profile_on()) fprintf(stderr, "loransac_h prof: whole %.0f us, checks after RANSAC %.0f us\n", 1e3 * (prof_ms() - t_enter), 1e3 * (prof_ms() - t_post0));
  return MODS_OK;
}

int mods_test_host_hchecks(const double *u6, const double *laf14, int n, const unsigned char *inl, const double *Hloran,
                           const mods_ransac_params *par, int lanes, unsigned char *mask, double *H_out) {
  if (!u6 || !inl || !Hloran || !par || !mask || !H_out || n < 0) return MODS_E_ARG;
  const mods::rs::SimdOps *ops = lanes ? mods::rs::simd_ops_lanes(lanes) : nullptr;
  if (lanes && !ops) return MODS_E_ARG;
  for (int i = 0; i < 9; i++) H_out[i] = -1;
  for (int i = 0; i < n; i++) mask[i] = 0;
  return h_post_checks(u6, laf14, n, inl, Hloran, par, ops, mask, H_out);
}

// useF branch of LORANSACFiltering (matching.cpp:711-726, 804-816): DEGENSAC + F_LAF_check (:192-249)
int mods_loransac_f(const double *u6, const double *laf, int n, const mods_ransac_params *par, unsigned char *mask, double *F_out,
                    int *n_inliers, int *stats3) {
  if (!par || !mask || !F_out || !n_inliers || (n > 0 && !u6)) { set_error("loransac_f: null argument"); return MODS_E_ARG; }
  *n_inliers = 0;
  for (int i = 0; i < 9; i++) F_out[i] = -1;
  for (int i = 0; i < n; i++) mask[i] = 0;
  if (stats3) { stats3[0] = stats3[1] = stats3[2] = 0; }
  const int MIN_POINTS = 8;
  if (n < MIN_POINTS) return MODS_OK;
  std::vector<double> u2(u6, u6 + (size_t)n * 6);
  std::vector<unsigned char> inl2(n);
  std::vector<int> data_out((size_t)n * 18, 0);
  double Floran[9], HinF[9];
  double *resids = nullptr;
  int I_H = 0;
  void (*fds)(const double *, const double *, double *, int) = par->errorType == 0 ? &FDs : &FDsSym;
  void (*exfds)(const double *, const double *, double *, double *, int) = par->errorType == 0 ? &exFDs : &exFDsSym;
  exp_ransacFcustom(u2.data(), n, par->err_threshold * par->err_threshold, par->confidence, par->max_samples, Floran, inl2.data(),
                    data_out.data(), par->localOptimization, 0, &resids, HinF, &I_H, exfds, fds, par->doSymmCheck);
  free(resids);
  if (mods::ransac_failed()) return MODS_E_HIP;
  if (stats3) { stats3[0] = data_out[0]; stats3[1] = data_out[1]; stats3[2] = I_H; }
  std::vector<int> cur;
  for (int i = 0; i < n; i++) if (inl2[i]) cur.push_back(i);
  f_laf_check(laf, Floran, par->LAFCoef * par->err_threshold, fds, cur);
  if ((int)cur.size() < MIN_POINTS) cur.clear();
  for (int i : cur) mask[i] = 1;
  *n_inliers = (int)cur.size();
  for (int i = 0; i < 9; i++) F_out[i] = Floran[i];     // ransac_corresp.H[i] = Hloran[i], matching.cpp:814-815
  return MODS_OK;
}

// ---- single primitives -------------------------------------------------------------------
int mods_gauss_blur(mods_ctx *c, const float *src, int w, int h, float sigma, float *dst) {
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, src, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  int rc = launch_gauss_blur(c, c->input_dev, c->tmp_dev, w, h, 1, sigma);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(dst, c->tmp_dev, sizeof(float) * (size_t)w * h, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

int mods_upscale2x(mods_ctx *c, const float *src, int w, int h, float *dst) {
  if (!c || !src || !dst || w <= 0 || h <= 0) { set_error("upscale2x: bad argument"); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  MODS_HIP_CHECK(mods::reserve_pool(c, c->up_tmp, 4 * n, 4 * n));
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, src, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  int rc = launch_upscale2x(c, c->input_dev, c->up_tmp, w, h, 1);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(dst, c->up_tmp, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

// A doubled first octave for the scale-space detectors of this context (pyramid.hip: pyramid_configure, pyramid_build_levels)
int mods_ctx_upscale_input(mods_ctx *c, int mode) {
  if (!c) { set_error("upscale_input: null context"); return MODS_E_ARG; }
  if (mode < 0 || mode > 2) { set_error("upscale_input: mode %d (0 off, 1 on, 2 on with the unfused first level)", mode); return MODS_E_ARG; }
  if (c->upscale_mode != mode) {
    c->upscale_mode = mode;
    mods::dev_state_changed(c);              // (recorded launch chains are not replayed across the change)
  }
  return MODS_OK;
}

int mods_ctx_upscale_input_get(const mods_ctx *c, int *mode) {
  if (!c || !mode) { set_error("upscale_input_get: null argument"); return MODS_E_ARG; }
  *mode = c->upscale_mode;
  return MODS_OK;
}

int mods_hessian_response(mods_ctx *c, const float *src, int w, int h, float norm, float *dst) {
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, src, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  int rc = launch_hessian_response(c, c->input_dev, c->tmp_dev, w, h, 1, norm);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(dst, c->tmp_dev, sizeof(float) * (size_t)w * h, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

int mods_resize_half(mods_ctx *c, const float *src, int w, int h, float *dst, int *dw, int *dh) {
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  resize_half_dims(w, h, dw, dh);
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, src, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice, c->stream));
  int rc = launch_resize_half(c, c->input_dev, c->tmp_dev, w, h, *dw, *dh, 1);
  if (rc) return rc;
  MODS_HIP_CHECK(hipMemcpyAsync(dst, c->tmp_dev, sizeof(float) * (size_t)(*dw) * (*dh), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

}  // extern "C"

namespace {
// memory policy of mods_test_buffer_growth: counts, fails on a chosen call, and knows which pointers are live
struct FakeMem {
  static inline int allocs = 0, frees = 0, bad_frees = 0, fail_at = -1;   // fail_at: the allocation (counted from 0) that fails
  static inline std::vector<void *> live;
  static void reset() { allocs = frees = bad_frees = 0; fail_at = -1; }
  static hipError_t alloc(void **p, size_t bytes) {
    if (allocs++ == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    live.push_back(*p);
    return hipSuccess;
  }
  static hipError_t free(void *p) {
    frees++;
    auto it = std::find(live.begin(), live.end(), p);
    if (it == live.end()) { bad_frees++; return hipErrorInvalidValue; }   // freed twice, or never allocated
    live.erase(it);
    ::free(p);
    return hipSuccess;
  }
};
}  // namespace

extern "C" int mods_test_buffer_growth(int *report, int n) {
  using B = mods::Buf<double, FakeMem>;
  constexpr int kReport = 16, kGroup = 4;
  if (!report || n < kReport) return MODS_E_ARG;
  for (int i = 0; i < kReport; i++) report[i] = -1;
  FakeMem::reset();
  int successful = 0;   // allocations that returned memory
  {
    B a;
    bool ok = a.reserve(100, 150) == hipSuccess && a.capacity() == 150;
    successful++;
    int a0 = FakeMem::allocs, f0 = FakeMem::frees;
    bool moved = false;
    ok = ok && a.reserve(120, 180, &moved) == hipSuccess && !moved && a.capacity() == 150;
    report[0] = (FakeMem::allocs - a0) + (FakeMem::frees - f0);                 // a reserve below the capacity: 0 calls
    ok = ok && a.reserve(151, 300, &moved) == hipSuccess && moved && a.capacity() == 300;
    successful++;
    report[1] = FakeMem::frees - f0; report[2] = FakeMem::allocs - a0;          // a growth: 1 free, 1 allocation
    a0 = FakeMem::allocs; f0 = FakeMem::frees;
    FakeMem::fail_at = FakeMem::allocs;
    report[3] = a.reserve(301, 600) != hipSuccess && a.get() == nullptr;        // a failed growth: empty
    report[4] = (int)a.capacity();
    report[5] = FakeMem::frees - f0;                                            // ... and the old allocation freed once
    FakeMem::fail_at = -1;
    a0 = FakeMem::allocs;
    ok = ok && a.reserve(10, 10) == hipSuccess && a.get() && a.capacity() == 10;
    successful++;
    report[6] = FakeMem::allocs - a0;                                           // the reserve after it allocates again: 1
    // moves, swap, detach
    B b(std::move(a));
    ok = ok && !a.get() && a.capacity() == 0 && b.capacity() == 10;
    B c; ok = ok && c.reserve(5, 5) == hipSuccess; successful++;
    c = std::move(b);                                                           // onto a non-empty buffer: its allocation is freed
    ok = ok && c.capacity() == 10 && !b.get();
    B d; ok = ok && d.reserve(7, 7) == hipSuccess; successful++;
    c.swap(d);
    ok = ok && c.capacity() == 7 && d.capacity() == 10;
    double *raw = d.detach();
    ok = ok && raw && !d.get() && d.capacity() == 0;
    B e; ok = ok && e.reserve(3, 3) == hipSuccess; successful++;
    (void)FakeMem::free(raw);                                                   // the detached allocation is the caller's
    FakeMem::fail_at = FakeMem::allocs;
    ok = ok && e.reserve(4, 4) != hipSuccess && !e.get();
    FakeMem::fail_at = -1;
    report[7] = ok;
    // the group rule: allocation j of kGroup fails -> all empty; without a failure all hold their elements
    B g[kGroup];
    int left = 0;
    for (int j = 0; j < kGroup; j++) {
      for (int q = 0; q < kGroup; q++) if (g[q].reserve(2, 2) == hipSuccess) successful++;   // a non-empty group to start from
      const int before = FakeMem::allocs;
      FakeMem::fail_at = FakeMem::allocs + j;
      if (mods::reserve_group(g[0], 8 + j, g[1], 16 + j, g[2], 24 + j, g[3], 32 + j) == hipSuccess) left += 100;
      successful += FakeMem::allocs - before - 1;
      FakeMem::fail_at = -1;
      for (const B &x : g) left += x.get() != nullptr || x.capacity() != 0;
    }
    report[8] = left;                                                           // 0
    const int before = FakeMem::allocs;
    report[9] = mods::reserve_group(g[0], 8, g[1], 16, g[2], 24, g[3], 32) == hipSuccess;
    successful += FakeMem::allocs - before;
    report[10] = (g[0].capacity() == 8) + (g[1].capacity() == 16) + (g[2].capacity() == 24) + (g[3].capacity() == 32);   // kGroup
  }
  report[11] = FakeMem::bad_frees;                                              // 0: nothing freed twice
  report[12] = (int)FakeMem::live.size();                                       // 0: everything freed by now
  report[13] = successful;
  report[14] = FakeMem::frees;                                                  // == report[13]: each allocation freed exactly once
  report[15] = kGroup;
  return kReport;
}
