// ORSA a-contrario fundamental-matrix verification (orsa.cpp:371-678, called by ORSAFiltering, matching.cpp:824-914): GPU
// scoring of the hypotheses + host control loop.
//
// Structure (as ransac_f.hip).  orsa() draws one 7-point sample per iteration from glibc's rand() (7 raw values per iteration,
// whatever the state), solves it into 1..3 candidate F (orsa_host.hpp) and scores each candidate by sorting its n symmetric
// epipolar errors and scanning the n NFA values of the sorted prefixes.  The sequential decisions are cheap: a new record, the
// switch to the optimisation phase (which narrows the sampling to the record's inliers).  So the host draws the raw values of a
// block of iterations ahead, maps them to samples with the current (nid, id) and solves them on the host pool, the device scores
// every candidate of the block in one launch - errors, sort, NFA terms, first argmin - and the host replays the reference's
// decisions in order.  A trigger of the optimisation changes how the later samples of the block map to indices: those are
// discarded, re-mapped from the same raw values and re-solved (a rewind).  The sorted index prefix a record needs comes from
// the host (matcherrorn with glibc's qsort) for record-setting models only; models whose errors hold a NaN are scored on the
// host altogether (compf is not a strict weak order then).
//
//   orsa_score_kernel : a workgroup holds G models; model g's error keys (float bits: non-negative floats order as uint32) sit in
//                       a P = 2^k slot segment, padded with 0xffffffff, in LDS (P <= ORSA_LDS_KEYS) or, above that, one model per
//                       workgroup in a global scratch segment (the HBM tier).  A bitonic network of segment size P sorts every
//                       segment at once; every thread then evaluates the NFA terms of its slots and a 64-bit LDS atomicMin over
//                       (ordered nfa, position) gives the first argmin.
//
// The same kernel body scores ORSA-H, the a-contrario homography verifier (mods_orsa_h, useF = 3; contract in mods_hip.h, parity
// with the IPOL code unpinned), through a second model policy: 4-point samples, the transfer error, its NFA.  Its models arrive
// as sample indices and are solved in the workgroup's first phase (orsa_h_host.hpp: solve_h4, shared with the host path).
#include "common.hpp"
#include "f_laf.hpp"
#include "h_laf.hpp"
#include "orsa_h_host.hpp"
#include "orsa_host.hpp"
#include "ransac_gpu.hpp"
#include "ransac_pool.hpp"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstring>
#include <mutex>
#include <ctime>
#include <functional>

#include "../../include/mods_degensac.h"

namespace mods {

constexpr int ORSA_LDS_KEYS = 32768;   // 128 KiB of keys: the largest power-of-two segment a workgroup's LDS holds
constexpr int ORSA_MAX_PACK = 256;
// key slots a workgroup packs small models into by default: 1024 was fastest at every fixture size in the 1024 / 4096 / 16384 /
// 32768 sweep (profiles/orsa_pack_sweep.txt) - more, smaller workgroups spread a block's models over more CUs
constexpr int ORSA_WG_KEYS = 1024;     // models per workgroup at most (their minima and flags: 3 KiB of LDS)

struct OrsaOut { float nfa; int imin; float logalpha; int nan; };

struct OrsaConst {
  const float4 *pts;     // (p1x, p1y, p2x, p2y) normalised, n entries
  const float *logcn, *logck;   // logcombi(i, n) and the model's second table, logcombi(S, i): n + 1 entries each
  int n, P, G, n_models;
  float logalpha0, loge0;
};

__device__ __forceinline__ unsigned err_key(const float *F, float4 p) {
#pragma clang fp contract(off)
  const double x1 = p.x, y1 = p.y, x2 = p.z, y2 = p.w;
  const double F11 = F[0], F12 = F[1], F13 = F[2], F21 = F[3], F22 = F[4], F23 = F[5], F31 = F[6], F32 = F[7], F33 = F[8];
  const double rxc = F11 * x2 + F21 * y2 + F31;
  const double ryc = F12 * x2 + F22 * y2 + F32;
  const double rwc = F13 * x2 + F23 * y2 + F33;
  const double r = (rxc * x1 + ryc * y1 + rwc);
  const double rx = F11 * x1 + F12 * y1 + F13;
  const double ry = F21 * x1 + F22 * y1 + F23;
  const double a = rxc * rxc + ryc * ryc;
  const double b = rx * rx + ry * ry;
  return __float_as_uint((float)(r * r * (a + b) / (a * b)));
}

// (float)log10((double)e): ocml's double log10 rounded to float; equal to glibc's for every non-negative float
// (tools/orsa_log10_sweep.py, profiles/orsa_log10_sweep.txt)
__device__ __forceinline__ float log10_ref_dev(float e) { return (float)log10((double)e); }

// What orsa_score_kernel takes from the model it scores: the sample size S (the scan starts at sorted position S, the exponent of
// position i is i - (S - 1), the second table is logcombi(S, .)), the error key of a correspondence, the log of the probability
// of that error, and whether a workgroup keeps its models in LDS - solved there from sample indices, or copied from given
// matrices - and counts a model with a NaN error as invalid (nfa 10000, imin 0) instead of handing it to the host.
struct ModelF {   // fundamental matrix, symmetric epipolar line error: alpha = alpha0 sqrt(e)
  static constexpr int S = 7;
  static constexpr bool LDS_MODELS = false;
  static __device__ __forceinline__ unsigned key(const float *F, float4 p) { return err_key(F, p); }
  static __device__ __forceinline__ float logalpha(float logalpha0, float e) {
#pragma clang fp contract(off)
    return logalpha0 + 0.5 * (double)log10_ref_dev(e);
  }
};
struct ModelH {   // homography, squared transfer error in image 2: alpha = alpha0 e, an exact zero error clamped to FLT_MIN
  static constexpr int S = 4;
  static constexpr bool LDS_MODELS = true;
  static __device__ __forceinline__ unsigned key(const float *H, float4 p) {
    return __float_as_uint(orsa_h::h_error(H, p.x, p.y, p.z, p.w));
  }
  static __device__ __forceinline__ float logalpha(float logalpha0, float e) {
#pragma clang fp contract(off)
    return logalpha0 + log10_ref_dev(e < FLT_MIN ? FLT_MIN : e);
  }
};

template <class M> __device__ __forceinline__ float nfa_term_dev(const OrsaConst &k, float e, int i, float *la_out) {
#pragma clang fp contract(off)
  const float la = M::logalpha(k.logalpha0, e);
  *la_out = la;
  return k.loge0 + la * (float)(i - (M::S - 1)) + k.logcn[i + 1] + k.logck[i + 1];
}

__device__ __forceinline__ unsigned long long nfa_order(float nfa, int i) {
  unsigned u = __float_as_uint(nfa == 0.0f ? 0.0f : nfa);   // -0 and +0 compare equal in the scan
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned)i;
}

// bytes of LDS ahead of the keys: G minima, G flags, and the G models of an LDS_MODELS policy (each part a multiple of 8 bytes)
template <class M> __host__ __device__ constexpr size_t orsa_lds_head(int G) {
  return sizeof(unsigned long long) * G + sizeof(int) * (G + (G & 1)) + (M::LDS_MODELS ? sizeof(float) * (9 * G + (G & 1)) : 0);
}

// models: n_models x 9 floats.  ModelF reads them.  ModelH with samples != nullptr (n_models x 4 point indices below n) solves
// its G systems first, one thread per system - a solve is some 400 fp64 operations next to the n error keys and the sort of the
// same model, so the simpler layout was taken - keeps the 9 floats in LDS and writes them to models for the host; with
// samples == nullptr it copies the given models into LDS (the "models given" entry the refit model takes).
template <class M, bool LDS>
__global__ __launch_bounds__(1024) void orsa_score_kernel(OrsaConst k, float *__restrict__ models, const int *__restrict__ samples,
                                                          unsigned *__restrict__ gkeys, OrsaOut *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char orsa_smem[];
  const int G = k.G, P = k.P, n = k.n;
  unsigned long long *s_min = (unsigned long long *)orsa_smem;   // G entries
  int *s_nan = (int *)(s_min + G);                                // G entries
  float *s_model = (float *)(s_nan + G + (G & 1));                // 9 G entries (LDS_MODELS)
  unsigned *keys = LDS ? (unsigned *)(orsa_smem + orsa_lds_head<M>(G)) : gkeys + (size_t)blockIdx.x * P;
  const int N = G * P;
  for (int m0 = blockIdx.x * G; m0 < k.n_models; m0 += gridDim.x * G) {
    for (int g = threadIdx.x; g < G; g += blockDim.x) { s_min[g] = ~0ull; s_nan[g] = 0; }
    if constexpr (M::LDS_MODELS) {
      for (int g = threadIdx.x; g < G; g += blockDim.x) {   // (thread g cleared flag g itself)
        const int m = m0 + g;
        if (m >= k.n_models) continue;
        float h[9];
        if (samples) {
          float c[16];
          for (int i = 0; i < 4; i++) {
            const float4 p = k.pts[samples[(size_t)m * 4 + i]];
            c[4 * i] = p.x; c[4 * i + 1] = p.y; c[4 * i + 2] = p.z; c[4 * i + 3] = p.w;
          }
          if (!orsa_h::solve_h4(c, h)) s_nan[g] = 1;
          for (int q = 0; q < 9; q++) models[(size_t)m * 9 + q] = h[q];
        } else {
          for (int q = 0; q < 9; q++) h[q] = models[(size_t)m * 9 + q];
        }
        for (int q = 0; q < 9; q++) s_model[g * 9 + q] = h[q];
      }
    }
    __syncthreads();   // the flags are cleared before any thread of the key loop may raise one
    for (int s = threadIdx.x; s < N; s += blockDim.x) {
      const int g = s / P, i = s - g * P, m = m0 + g;
      unsigned key = 0xffffffffu;
      if (m < k.n_models && i < n) {
        key = M::key(M::LDS_MODELS ? s_model + g * 9 : models + (size_t)m * 9, k.pts[i]);
        if ((key & 0x7fffffffu) > 0x7f800000u) s_nan[g] = 1;
      }
      keys[s] = key;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < N / 2; t += blockDim.x) {
          const int i = 2 * t - (t & (j - 1)), l = i + j;
          const bool asc = kk == P || (i & kk) == 0;
          const unsigned a = keys[i], b = keys[l];
          if ((a > b) == asc) { keys[i] = b; keys[l] = a; }
        }
        __syncthreads();
      }
    }
    for (int s = threadIdx.x; s < N; s += blockDim.x) {
      const int g = s / P, i = s - g * P;
      if (m0 + g >= k.n_models || i < M::S || i >= n) continue;
      float la;
      const float nfa = nfa_term_dev<M>(k, __uint_as_float(keys[s]), i, &la);
      if (nfa < 10000.f) atomicMin(&s_min[g], nfa_order(nfa, i));
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
      const int m = m0 + g;
      if (m >= k.n_models) continue;
      OrsaOut o = {10000.f, 0, 10000.f, s_nan[g]};
      if (s_min[g] != ~0ull && !(M::LDS_MODELS && s_nan[g])) {
        const int i = (int)(unsigned)(s_min[g] & 0xffffffffu);
        o.imin = i;
        o.nfa = nfa_term_dev<M>(k, __uint_as_float(keys[g * P + i]), i, &o.logalpha);
      }
      out[m] = o;
    }
    __syncthreads();
  }
}

__global__ void orsa_log10_kernel(unsigned begin, unsigned count, float *__restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = log10_ref_dev(__uint_as_float(begin + i));
}

// ---- device workspace (per thread, as the degensac entry points) --------------------------------------------------------------

struct OrsaGpu {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  Buf<float4> pts; Buf<float> tabs;                                    // n points, 2 (n + 1) table entries: reserved together
  Buf<float> models; Buf<OrsaOut> out; PinnedBuf<OrsaOut> out_host;    // 9 floats in, a record out per model: reserved together
  Buf<unsigned> gkeys;
  Buf<int> samples; PinnedBuf<float> models_host;                       // ORSA-H: 4 indices in, 9 floats back per model
  ~OrsaGpu() {                                                         // (the buffers free themselves)
    if (device < 0) return;
    (void)hipSetDevice(device);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

static OrsaGpu *orsa_gpu() {
  static thread_local ThreadWorkspace<OrsaGpu> tl;   // (ransac_gpu.hpp: the main thread's is not released at process exit)
  OrsaGpu &ws = tl.get();
  if (ws.device < 0) {
    RansacGpu *r = ransac_gpu();   // the device the degensac entry points of this thread use (mods_ransac_set_device)
    if (!r) return nullptr;
    // highest priority, as the degensac workspace (ransac.hip): the host waits on every scoring round trip, which must not
    // queue behind the pair pipeline's describe batches
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    if (hipSetDevice(r->device) != hipSuccess || hipStreamCreateWithPriority(&ws.stream, hipStreamNonBlocking, prio_high) != hipSuccess ||
        hipEventCreate(&ws.ev0) != hipSuccess || hipEventCreate(&ws.ev1) != hipSuccess) {
      set_error("orsa: stream / event creation failed");
      return nullptr;
    }
    ws.device = r->device;
  }
  if (hipSetDevice(ws.device) != hipSuccess) { set_error("orsa: hipSetDevice failed"); return nullptr; }
  return &ws;
}

static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e && *e ? atoi(e) : dflt; }

// ---- scoring back ends -----------------------------------------------------------------------------------------------------

struct OrsaProf { double solve_ms = 0, score_ms = 0, kernel_ms = 0, replay_ms = 0, total_ms = 0; long launches = 0; };

using ScoreFn = std::function<bool(const std::vector<float> &F, int m, std::vector<orsa::Score> &out)>;

static inline int next_pow2(int n) { int p = 8; while (p < n) p <<= 1; return p; }

struct DeviceScorer {
  OrsaGpu *ws = nullptr;
  int n = 0, seg = 0, G = 1, block = 256;
  float logalpha0 = 0, loge0 = 0;
  bool lds = true;
  OrsaProf *prof = nullptr;

  // p1, p2: n normalised points each; logcn, logck: the two tables of n + 1 entries
  bool init(int n_, const float *p1, const float *p2, const float *logcn, const float *logck, float la0, float le0, int wg_keys) {
    n = n_; logalpha0 = la0; loge0 = le0;
    ws = orsa_gpu();
    if (!ws) return false;
    RS_CHECK(reserve_group(ws->pts, (size_t)n, ws->tabs, 2 * ((size_t)n + 1)));
    std::vector<float4> pts(n);
    for (int i = 0; i < n; i++) pts[i] = make_float4(p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
    std::vector<float> tabs(2 * (n + 1));
    memcpy(tabs.data(), logcn, sizeof(float) * (n + 1));
    memcpy(tabs.data() + n + 1, logck, sizeof(float) * (n + 1));
    RS_CHECK(hipMemcpyAsync(ws->pts, pts.data(), sizeof(float4) * n, hipMemcpyHostToDevice, ws->stream));
    RS_CHECK(hipMemcpyAsync(ws->tabs, tabs.data(), sizeof(float) * 2 * (n + 1), hipMemcpyHostToDevice, ws->stream));
    RS_CHECK(hipStreamSynchronize(ws->stream));
    seg = next_pow2(n);
    lds = seg <= ORSA_LDS_KEYS;
    if (wg_keys < seg) wg_keys = seg;
    if (wg_keys > ORSA_LDS_KEYS) wg_keys = ORSA_LDS_KEYS;
    G = lds ? std::min(wg_keys / seg, ORSA_MAX_PACK) : 1;
    const int pairs = G * seg / 2;
    block = std::min(1024, std::max(256, (pairs + 63) & ~63));
    return true;
  }
  bool init(const orsa::Problem &Pr, int wg_keys) {
    return init(Pr.n, Pr.p1.data(), Pr.p2.data(), Pr.logcn.data(), Pr.logc7.data(), Pr.logalpha0, Pr.loge0, wg_keys);
  }
  bool init(const orsa_h::Problem &Pr, int wg_keys) {
    return init(Pr.n, Pr.p1.data(), Pr.p2.data(), Pr.logcn.data(), Pr.logc4.data(), Pr.logalpha0, Pr.loge0, wg_keys);
  }

  // m models: given as F (m x 9 floats), or - ModelH only - as samples (m x 4 point indices, F == nullptr), solved on the
  // device and returned in *solved (m x 9 floats)
  template <class M>
  bool score(const float *F, const int *samples, int m, std::vector<orsa::Score> &res, std::vector<float> *solved = nullptr) {
    res.resize(m);
    if (solved) solved->resize((size_t)9 * m);
    if (m == 0) return true;
    if ((size_t)m > ws->out.capacity()) {
      size_t cap = ws->out.capacity() ? ws->out.capacity() : 1024;
      while (cap < (size_t)m) cap *= 2;
      RS_CHECK(reserve_group(ws->models, 9 * cap, ws->out, cap, ws->out_host, cap));
    }
    if (samples && (size_t)m > ws->models_host.capacity() / 9)
      RS_CHECK(reserve_group(ws->samples, 4 * ws->out.capacity(), ws->models_host, 9 * ws->out.capacity()));
    const int wgs_needed = (m + G - 1) / G;
    int grid = wgs_needed;
    if (!lds) {
      grid = wgs_needed < 256 ? wgs_needed : 256;
      const size_t need = (size_t)grid * seg;
      RS_CHECK(ws->gkeys.reserve(need));
    }
    if (samples) RS_CHECK(hipMemcpyAsync(ws->samples, samples, sizeof(int) * 4 * m, hipMemcpyHostToDevice, ws->stream));
    else RS_CHECK(hipMemcpyAsync(ws->models, F, sizeof(float) * 9 * m, hipMemcpyHostToDevice, ws->stream));
    OrsaConst k;
    k.pts = ws->pts; k.logcn = ws->tabs; k.logck = ws->tabs + n + 1;
    k.n = n; k.P = seg; k.G = G; k.n_models = m; k.logalpha0 = logalpha0; k.loge0 = loge0;
    const size_t shm = orsa_lds_head<M>(G) + (lds ? sizeof(unsigned) * (size_t)G * seg : 0);
    const int *dsamples = samples ? ws->samples.get() : nullptr;
    RS_CHECK(hipEventRecord(ws->ev0, ws->stream));
    if (lds) {
      static thread_local bool attr = false;   // (one per instantiation of this function, that is per model policy)
      if (!attr) {
        RS_CHECK(hipFuncSetAttribute((const void *)orsa_score_kernel<M, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(sizeof(unsigned) * ORSA_LDS_KEYS + orsa_lds_head<M>(ORSA_MAX_PACK))));
        attr = true;
      }
      hipLaunchKernelGGL((orsa_score_kernel<M, true>), dim3(grid), dim3(block), shm, ws->stream, k, ws->models.get(), dsamples, nullptr,
                         ws->out.get());
    } else {
      hipLaunchKernelGGL((orsa_score_kernel<M, false>), dim3(grid), dim3(1024), shm, ws->stream, k, ws->models.get(), dsamples,
                         ws->gkeys.get(), ws->out.get());
    }
    RS_CHECK(hipGetLastError());
    RS_CHECK(hipEventRecord(ws->ev1, ws->stream));
    RS_CHECK(hipMemcpyAsync(ws->out_host, ws->out, sizeof(OrsaOut) * m, hipMemcpyDeviceToHost, ws->stream));
    if (samples) RS_CHECK(hipMemcpyAsync(ws->models_host, ws->models, sizeof(float) * 9 * m, hipMemcpyDeviceToHost, ws->stream));
    RS_CHECK(hipStreamSynchronize(ws->stream));
    float kms = 0;
    if (hipEventElapsedTime(&kms, ws->ev0, ws->ev1) == hipSuccess && prof) prof->kernel_ms += kms;
    if (prof) prof->launches++;
    for (int i = 0; i < m; i++) {
      const OrsaOut &o = ws->out_host[i];
      res[i] = {o.nfa, o.imin, o.logalpha, o.nan};
    }
    if (samples && solved) memcpy(solved->data(), ws->models_host.get(), sizeof(float) * 9 * m);
    return true;
  }
  bool score(const std::vector<float> &F, int m, std::vector<orsa::Score> &res) { return score<ModelF>(F.data(), nullptr, m, res); }
};

// ---- the control loop ------------------------------------------------------------------------------------------------------

struct OrsaResult {
  float nfa = 10000.f;
  int miniall = 0, niter = 0, models = 0, rewinds = 0;
  double Fout[9];                 // orsa()'s Fout: T^T f T, row-major
  std::vector<float> index;       // the first miniall + 1 entries of orsa()'s index (the last one stale)
};

// orsa() with mode 2, t = 10000, stop = 0 (matching.cpp:870-879), after srand(seed); score = the back end of a block of models
static bool orsa_run(orsa::Problem &P, unsigned seed, int batch, const ScoreFn &score, OrsaResult &R, OrsaProf &prof) {
  const int n = P.n, t = 10000;
  rs::GlibcRand rng;
  rng.seed(seed);
  std::vector<int32_t> raw;
  std::vector<int> id(n);
  for (int i = 0; i < n; i++) id[i] = i;
  int nid = n, maxniter = t - t / 10, optimization = 0, niter = 0, miniall = 0;
  float minepsall = 10000.f;
  float f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<float> index(n, 0.0f), e((size_t)2 * n);
  std::vector<float> Fs;
  std::vector<orsa::Score> sc;
  if (batch < 1) batch = 1;
  while (niter < maxniter) {
    const double t0 = now_ms();
    const int B = std::min(batch, maxniter - niter);
    while ((int)raw.size() < 7 * (niter + B)) raw.push_back(rng.next());
    // solve the block's samples with the current (nid, id); 3 slots per iteration, compacted in order afterwards
    std::vector<float> sol((size_t)B * 27);
    std::vector<int> nroot(B);
    auto solve = [&](int b) {
      int k[8], idk[7];
      orsa::map_p7(&raw[(size_t)7 * (niter + b)], nid, k);
      for (int i = 0; i < 7; i++) idk[i] = id[k[i]];
      float z[3], F1[9], F2[9];
      const int m = orsa::epipolar(P.p1.data(), P.p2.data(), idk, z, F1, F2);
      nroot[b] = m;
      for (int r = 0, mm = m; mm--; r++)   // roots in reverse order, F = F1 + z F2
        for (int q = 0; q < 9; q++) sol[(size_t)b * 27 + r * 9 + q] = F1[q] + z[mm] * F2[q];
    };
    rs::TaskPool::get().run(B, solve);
    Fs.clear();
    std::vector<int> first(B + 1, 0);
    for (int b = 0; b < B; b++) {
      first[b + 1] = first[b] + nroot[b];
      Fs.insert(Fs.end(), &sol[(size_t)b * 27], &sol[(size_t)b * 27 + 9 * nroot[b]]);
    }
    const int M = first[B];
    const double t1 = now_ms();
    if (!score(Fs, M, sc)) return false;
    const double t2 = now_ms();
    prof.solve_ms += t1 - t0;
    prof.score_ms += t2 - t1;
    // replay orsa.cpp:547-628 in order
    bool rewind = false;
    int b = 0;
    for (; b < B && !rewind; b++) {
      niter++;
      for (int mi = first[b]; mi < first[b + 1]; mi++) {   // the rest of the iteration's roots stand after a trigger
        orsa::Score s = sc[mi];
        R.models++;
        if (s.nan) s = orsa::score_host(&Fs[(size_t)mi * 9], P, e.data());
        bool better = false;
        if (s.nfa < minepsall) {
          better = true;
          minepsall = s.nfa;
          miniall = s.imin;
          for (int q = 0; q < 9; q++) f[q] = Fs[(size_t)mi * 9 + q];
          orsa::errors_sorted(&Fs[(size_t)mi * 9], P, e.data());
          for (int i = 0; i < s.imin; i++) index[i] = e[i * 2 + 1];
        }
        if ((better && minepsall < 0.) || (niter == maxniter && !optimization)) {
          if (!optimization) maxniter = niter + t / 10;
          optimization = 1;
          nid = miniall + 1;
          for (int j = 0; j < miniall; j++) id[j] = (int)index[j];
          rewind = true;
        }
      }
    }
    if (rewind && b < B) R.rewinds++;   // the block's later samples were mapped with the old (nid, id): drawn again from raw
    prof.replay_ms += now_ms() - t2;
  }
  R.nfa = minepsall;
  R.miniall = miniall;
  R.niter = niter;
  R.index.assign(index.begin(), index.begin() + miniall + 1);
  // Fout = T^T f T (orsa.cpp:640-662)
  double Fo[9], T[9], Tt[9], tmp[9];
  for (int q = 0; q < 9; q++) Fo[q] = f[q];
  T[0] = P.norm; T[1] = 0; T[2] = -0.5 * P.nx * P.norm;
  T[3] = 0; T[4] = P.norm; T[5] = -0.5 * P.ny * P.norm;
  T[6] = 0; T[7] = 0; T[8] = 1.0;
  Tt[0] = T[0]; Tt[1] = T[3]; Tt[2] = T[6];
  Tt[3] = T[1]; Tt[4] = T[4]; Tt[5] = T[7];
  Tt[6] = T[2]; Tt[7] = T[5]; Tt[8] = T[8];
  auto mul = [](const double *L, const double *Rm, double *res) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) res[3 * r + c] = L[3 * r] * Rm[c] + L[3 * r + 1] * Rm[3 + c] + L[3 * r + 2] * Rm[6 + c];
  };
  mul(Tt, Fo, tmp);
  mul(tmp, T, R.Fout);
  return true;
}

static bool host_score_block(const orsa::Problem &P, const std::vector<float> &F, int m, std::vector<orsa::Score> &out) {
  out.resize(m);
  const int chunks = std::min(m, 64);
  rs::TaskPool::get().run(chunks, [&](int c) {
    std::vector<float> e((size_t)2 * P.n);
    for (int i = c; i < m; i += chunks) out[i] = orsa::score_host(&F[(size_t)i * 9], P, e.data());
  });
  return true;
}

static thread_local OrsaProf g_orsa_prof;

// ORSAFiltering (matching.cpp:825-914) around orsa_run; on_device 0: the host scoring path (the device's oracle)
static int orsa_filter(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                       double *F_out, int *n_inliers, float *log_nfa, int *index_out, int *n_index, int *stats3, bool on_device,
                       long seed_time, int batch, int wg_keys) {
  if (!par || !mask || !F_out || !n_inliers || (n > 0 && !u6)) { set_error("orsa_f: null argument"); return MODS_E_ARG; }
  if (w <= 0 || h <= 0) { set_error("orsa_f: the image size (w, h) must be positive, got %d x %d", w, h); return MODS_E_ARG; }
  *n_inliers = 0;
  for (int i = 0; i < 9; i++) F_out[i] = -1;
  for (int i = 0; i < n; i++) mask[i] = 0;
  if (log_nfa) *log_nfa = 10000.f;
  if (n_index) *n_index = 0;
  if (stats3) { stats3[0] = stats3[1] = stats3[2] = 0; }
  g_orsa_prof = OrsaProf();
  const int MIN_POINTS = 8;
  if (n < MIN_POINTS) return MODS_OK;
  const double t_enter = now_ms();
  orsa::Problem P;
  P.n = n;
  P.p1.resize(2 * n); P.p2.resize(2 * n);
  for (int i = 0; i < n; i++) {   // Match: x1, y1 = the second image's point, x2, y2 = the first's (matching.cpp:861-866)
    P.p1[2 * i] = (float)u6[6 * i + 3]; P.p1[2 * i + 1] = (float)u6[6 * i + 4];
    P.p2[2 * i] = (float)u6[6 * i]; P.p2[2 * i + 1] = (float)u6[6 * i + 1];
  }
  orsa::setup(P, w, h);
  const unsigned seed = (unsigned)(seed_time >= 0 ? (time_t)seed_time : time(NULL));
  OrsaResult R;
  DeviceScorer dev;
  ScoreFn fn;
  if (on_device) {
    if (!dev.init(P, wg_keys)) return MODS_E_NODEVICE;
    dev.prof = &g_orsa_prof;
    fn = [&](const std::vector<float> &F, int m, std::vector<orsa::Score> &out) { return dev.score(F, m, out); };
  } else {
    fn = [&](const std::vector<float> &F, int m, std::vector<orsa::Score> &out) { return host_score_block(P, F, m, out); };
  }
  if (!orsa_run(P, seed, batch, fn, R, g_orsa_prof)) return MODS_E_HIP;
  g_orsa_prof.total_ms = now_ms() - t_enter;
  if (stats3) { stats3[0] = R.niter; stats3[1] = R.models; stats3[2] = R.rewinds; }
  if (log_nfa) *log_nfa = R.nfa;
  if (index_out) for (int i = 0; i < R.miniall; i++) index_out[i] = (int)R.index[i];
  if (n_index) *n_index = R.miniall;
  if (!(R.nfa < -2.0f)) return MODS_OK;   // nfa_max = -2: not significant
  const double *Ft = R.Fout;
  const double F[9] = {Ft[0], Ft[3], Ft[6], Ft[1], Ft[4], Ft[7], Ft[2], Ft[5], Ft[8]};
  for (int i = 0; i < 9; i++) F_out[i] = F[i];
  // the verified list: the first miniall + 1 tentatives in input order (matching.cpp:888-891), then F_LAF_check (:192-249)
  const int cnt = std::min((int)R.index.size(), n);
  std::vector<int> cur;
  for (int i = 0; i < cnt; i++) cur.push_back(i);
  void (*fds)(const double *, const double *, double *, int) = par->errorType == 0 ? &FDs : &FDsSym;
  f_laf_check(laf, F, par->LAFCoef * par->err_threshold, fds, cur);
  if ((int)cur.size() < MIN_POINTS) cur.clear();
  for (int i : cur) mask[i] = 1;
  *n_inliers = (int)cur.size();
  return MODS_OK;
}

// ---- ORSA-H: the homography model under the same control loop -----------------------------------------------------------------

// a block of models of ORSA-H, scored: from samples (m x 4 point indices; the models come back in H, m x 9) or from given models
// (samples == nullptr, H holds them)
using ScoreHFn = std::function<bool(const int *samples, std::vector<float> &H, int m, std::vector<orsa::Score> &out)>;

static bool host_score_block_h(const orsa_h::Problem &P, const int *samples, std::vector<float> &H, int m, std::vector<orsa::Score> &out) {
  out.resize(m);
  if (samples) H.resize((size_t)9 * m);
  const int chunks = std::min(m, 64);
  rs::TaskPool::get().run(chunks, [&](int c) {
    std::vector<float> e(P.n);
    for (int i = c; i < m; i += chunks) {
      bool valid = true;
      if (samples) {
        float c16[16];
        orsa_h::gather4(P, samples + (size_t)4 * i, c16);
        valid = orsa_h::solve_h4(c16, &H[(size_t)i * 9]);
      }
      out[i] = orsa_h::score_host(&H[(size_t)i * 9], valid, P, e.data());
    }
  });
  return true;
}

struct OrsaHResult {
  float nfa = 10000.f, e_last = 0, nfa_loop = 10000.f, nfa_refit = 10000.f;
  int imin = 0, niter = 0, models = 0, rewinds = 0, refit_taken = 0;
  float h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // the record's model, normalised coordinates
  std::vector<int> subset;                    // the first imin + 1 indices of its errors sorted by (error, index)
};

// orsa_run's loop with one 4-point model per iteration (t = 10000); the record's subset is the sorted prefix, taken on the host
// for record-setting models only.  Where no model was ever valid the last iteration has no subset to narrow the sampling to: the
// loop then ends without an optimisation phase.
static bool orsa_h_run(const orsa_h::Problem &P, unsigned seed, int batch, const ScoreHFn &score, OrsaHResult &R, OrsaProf &prof) {
  const int n = P.n, t = 10000;
  rs::GlibcRand rng;
  rng.seed(seed);
  std::vector<int32_t> raw;
  std::vector<int> id(n);
  for (int i = 0; i < n; i++) id[i] = i;
  int nid = n, maxniter = t - t / 10, optimization = 0, niter = 0;
  std::vector<int> samples;
  std::vector<float> Hs;
  std::vector<orsa::Score> sc;
  if (batch < 1) batch = 1;
  while (niter < maxniter) {
    const double t0 = now_ms();
    const int B = std::min(batch, maxniter - niter);
    while ((int)raw.size() < 4 * (niter + B)) raw.push_back(rng.next());
    samples.resize((size_t)4 * B);
    for (int b = 0; b < B; b++) {
      int k[4];
      orsa_h::map_p4(&raw[(size_t)4 * (niter + b)], nid, k);
      for (int i = 0; i < 4; i++) samples[(size_t)4 * b + i] = id[k[i]];
    }
    const double t1 = now_ms();
    if (!score(samples.data(), Hs, B, sc)) return false;
    const double t2 = now_ms();
    prof.solve_ms += t1 - t0;
    prof.score_ms += t2 - t1;
    bool rewind = false;
    int b = 0;
    for (; b < B && !rewind; b++) {
      niter++;
      R.models++;
      const orsa::Score &s = sc[b];
      bool better = false;
      if (!s.nan && s.nfa < R.nfa) {
        better = true;
        R.nfa = s.nfa;
        R.imin = s.imin;
        for (int q = 0; q < 9; q++) R.h[q] = Hs[(size_t)b * 9 + q];
        orsa_h::sorted_prefix(R.h, P, s.imin + 1, R.subset, &R.e_last);
      }
      if ((better && R.nfa < 0.) || (niter == maxniter && !optimization && !R.subset.empty())) {
        if (!optimization) maxniter = niter + t / 10;
        optimization = 1;
        nid = (int)R.subset.size();
        for (int j = 0; j < nid; j++) id[j] = R.subset[j];
        rewind = true;
      }
    }
    if (rewind && b < B) R.rewinds++;   // the block's later samples were mapped with the old (nid, id): drawn again from raw
    prof.replay_ms += now_ms() - t2;
  }
  R.niter = niter;
  R.nfa_loop = R.nfa;
  if (R.subset.empty()) return true;
  // the final refit: one least-squares model from the record's subset, scored like any other, taken only on a lower NFA
  std::vector<double> u((size_t)6 * n);
  for (int i = 0; i < n; i++) {   // u2h's model maps u[3..5] to u[0..2]
    u[6 * i] = P.p2[2 * i]; u[6 * i + 1] = P.p2[2 * i + 1]; u[6 * i + 2] = 1.0;
    u[6 * i + 3] = P.p1[2 * i]; u[6 * i + 4] = P.p1[2 * i + 1]; u[6 * i + 5] = 1.0;
  }
  double Hd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  rs::u2h(u.data(), R.subset.data(), (int)R.subset.size(), Hd, nullptr);
  std::vector<float> hr = {(float)Hd[0], (float)Hd[3], (float)Hd[6], (float)Hd[1], (float)Hd[4], (float)Hd[7],
                           (float)Hd[2], (float)Hd[5], (float)Hd[8]};
  bool finite = true;
  for (float v : hr) finite = finite && std::fabs(v) <= FLT_MAX;
  if (!finite) return true;
  if (!score(nullptr, hr, 1, sc)) return false;
  R.models++;
  if (sc[0].nan) return true;
  R.nfa_refit = sc[0].nfa;
  if (sc[0].nfa < R.nfa) {
    R.refit_taken = 1;
    R.nfa = sc[0].nfa;
    R.imin = sc[0].imin;
    for (int q = 0; q < 9; q++) R.h[q] = hr[q];
    orsa_h::sorted_prefix(R.h, P, R.imin + 1, R.subset, &R.e_last);
  }
  return true;
}

struct OrsaHRefit { float nfa_loop = 10000.f, nfa_refit = 10000.f, log_nfa = 10000.f; int taken = 0; double thr_px = 0; };
static thread_local OrsaHRefit g_orsa_h_refit;

static int orsa_h_filter(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                         double *H_out, int *n_inliers, float *log_nfa, double *thr_px, int *index_out, int *n_index, int *stats3,
                         bool on_device, long seed_time, int batch, int wg_keys) {
  if (!par || !mask || !H_out || !n_inliers || (n > 0 && !u6)) { set_error("orsa_h: null argument"); return MODS_E_ARG; }
  if (w <= 0 || h <= 0) { set_error("orsa_h: the image size (w, h) must be positive, got %d x %d", w, h); return MODS_E_ARG; }
  *n_inliers = 0;
  for (int i = 0; i < 9; i++) H_out[i] = -1;
  for (int i = 0; i < n; i++) mask[i] = 0;
  if (log_nfa) *log_nfa = 10000.f;
  if (thr_px) *thr_px = 0;
  if (n_index) *n_index = 0;
  if (stats3) { stats3[0] = stats3[1] = stats3[2] = 0; }
  g_orsa_prof = OrsaProf();
  g_orsa_h_refit = OrsaHRefit();
  const int MIN_POINTS = 8;
  if (n < MIN_POINTS) return MODS_OK;
  const double t_enter = now_ms();
  orsa_h::Problem P;
  P.n = n;
  P.p1.resize(2 * n); P.p2.resize(2 * n);
  for (int i = 0; i < n; i++) {
    P.p1[2 * i] = (float)u6[6 * i]; P.p1[2 * i + 1] = (float)u6[6 * i + 1];
    P.p2[2 * i] = (float)u6[6 * i + 3]; P.p2[2 * i + 1] = (float)u6[6 * i + 4];
  }
  orsa_h::setup(P, w, h);
  const unsigned seed = (unsigned)(seed_time >= 0 ? (time_t)seed_time : time(NULL));
  OrsaHResult R;
  DeviceScorer dev;
  ScoreHFn fn;
  if (on_device) {
    if (!dev.init(P, wg_keys)) return MODS_E_NODEVICE;
    dev.prof = &g_orsa_prof;
    fn = [&](const int *samples, std::vector<float> &H, int m, std::vector<orsa::Score> &out) {
      return dev.score<ModelH>(samples ? nullptr : H.data(), samples, m, out, &H);
    };
  } else {
    fn = [&](const int *samples, std::vector<float> &H, int m, std::vector<orsa::Score> &out) {
      return host_score_block_h(P, samples, H, m, out);
    };
  }
  if (!orsa_h_run(P, seed, batch, fn, R, g_orsa_prof)) return MODS_E_HIP;
  g_orsa_prof.total_ms = now_ms() - t_enter;
  g_orsa_h_refit.nfa_loop = R.nfa_loop; g_orsa_h_refit.nfa_refit = R.nfa_refit; g_orsa_h_refit.taken = R.refit_taken;
  if (stats3) { stats3[0] = R.niter; stats3[1] = R.models; stats3[2] = R.rewinds; }
  if (log_nfa) *log_nfa = R.nfa;
  g_orsa_h_refit.log_nfa = R.nfa;
  if (!(R.nfa < -2.0f)) return MODS_OK;   // not significant
  // H in pixels: T^-1 h T, T = the normalisation of both images
  const double nm = P.norm, cx = 0.5 * P.nx, cy = 0.5 * P.ny;
  const double T[9] = {nm, 0, -cx * nm, 0, nm, -cy * nm, 0, 0, 1.0};
  const double Ti[9] = {1.0 / nm, 0, cx, 0, 1.0 / nm, cy, 0, 0, 1.0};
  double hd[9], tmp[9], Hpx[9];
  for (int q = 0; q < 9; q++) hd[q] = R.h[q];
  auto mul = [](const double *L, const double *Rm, double *res) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) res[3 * r + c] = L[3 * r] * Rm[c] + L[3 * r + 1] * Rm[3 + c] + L[3 * r + 2] * Rm[6 + c];
  };
  mul(Ti, hd, tmp);
  mul(tmp, T, Hpx);
  for (int i = 0; i < 9; i++) H_out[i] = Hpx[i];
  const double thr = std::sqrt((double)R.e_last) / nm;
  if (thr_px) *thr_px = thr;
  g_orsa_h_refit.thr_px = thr;
  if (index_out) for (size_t i = 0; i < R.subset.size(); i++) index_out[i] = R.subset[i];
  if (n_index) *n_index = (int)R.subset.size();
  std::vector<int> cur(R.subset);
  std::sort(cur.begin(), cur.end());
  if (laf && par->HLAFCoef > 0) {
    double H21[9];
    if (invert3x3(Hpx, H21)) h_laf_check(laf, H21, par->HLAFCoef * thr, rs::simd_ops(), cur);
  }
  if ((int)cur.size() < MIN_POINTS) cur.clear();
  for (int i : cur) mask[i] = 1;
  *n_inliers = (int)cur.size();
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_orsa_f(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                double *F_out, int *n_inliers, float *log_nfa, int *index_out, int *n_index, int *stats3) {
  return orsa_filter(u6, laf, n, w, h, par, mask, F_out, n_inliers, log_nfa, index_out, n_index, stats3, true, ransac_pinned_seed(),
                     env_int("MODS_ORSA_BATCH", 512), env_int("MODS_ORSA_WG_KEYS", ORSA_WG_KEYS));
}

int mods_orsa_f_ex(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                   double *F_out, int *n_inliers, float *log_nfa, int *index_out, int *n_index, int *stats3, int on_device, int batch,
                   int wg_keys) {
  return orsa_filter(u6, laf, n, w, h, par, mask, F_out, n_inliers, log_nfa, index_out, n_index, stats3, on_device != 0,
                     ransac_pinned_seed(), batch > 0 ? batch : env_int("MODS_ORSA_BATCH", 512),
                     wg_keys > 0 ? wg_keys : env_int("MODS_ORSA_WG_KEYS", ORSA_WG_KEYS));
}

int mods_orsa_last_profile(double *ms5, long *launches) {
  if (!ms5) return MODS_E_ARG;
  ms5[0] = g_orsa_prof.solve_ms; ms5[1] = g_orsa_prof.score_ms; ms5[2] = g_orsa_prof.kernel_ms; ms5[3] = g_orsa_prof.replay_ms;
  ms5[4] = g_orsa_prof.total_ms;
  if (launches) *launches = g_orsa_prof.launches;
  return MODS_OK;
}

int mods_test_orsa_epipolar(const float *p1, const float *p2, const int *k7, float *F1, float *F2, float *z) {
  if (!p1 || !p2 || !k7 || !F1 || !F2 || !z) return MODS_E_ARG;
  z[0] = z[1] = z[2] = 0;
  return orsa::epipolar(p1, p2, k7, z, F1, F2);
}

int mods_test_orsa_tables(int n, float *logcn, float *logc7) {
  if (n < 0 || !logcn || !logc7) return MODS_E_ARG;
  for (int k = 0; k <= n; k++) logcn[k] = orsa::logcombi(k, n);
  for (int m = 0; m <= n; m++) logc7[m] = orsa::logcombi(7, m);
  return MODS_OK;
}

int mods_test_orsa_log10(const float *x, int n, float *out) {
  if (n < 0 || (n && (!x || !out))) return MODS_E_ARG;
  for (int i = 0; i < n; i++) out[i] = orsa::log10_ref(x[i]);
  return MODS_OK;
}

// the scoring of given models: on_device 1 through orsa_score_kernel, 0 through the host scalar path; p = n x 2 + n x 2 normalised
// (p1 then p2), F = m x 9 row-major; out4 per model = nfa (float bits), imin, logalpha (float bits), nan flag
int mods_test_orsa_score(const float *p1, const float *p2, int n, int w, int h, const float *F, int m, int on_device, int wg_keys,
                         int *out4) {
  if (!p1 || !p2 || !F || !out4 || n < 8 || m < 0 || w <= 0 || h <= 0) { set_error("orsa_score: bad argument"); return MODS_E_ARG; }
  orsa::Problem P;
  P.n = n;
  P.p1.assign(p1, p1 + 2 * n); P.p2.assign(p2, p2 + 2 * n);
  orsa::setup(P, w, h);
  P.p1.assign(p1, p1 + 2 * n); P.p2.assign(p2, p2 + 2 * n);   // the points as given (already normalised)
  std::vector<float> Fv(F, F + (size_t)9 * m);
  std::vector<orsa::Score> res;
  if (on_device) {
    DeviceScorer dev;
    if (!dev.init(P, wg_keys > 0 ? wg_keys : ORSA_WG_KEYS)) return MODS_E_NODEVICE;
    if (!dev.score(Fv, m, res)) return MODS_E_HIP;
  } else {
    host_score_block(P, Fv, m, res);
  }
  for (int i = 0; i < m; i++) {
    memcpy(&out4[4 * i], &res[i].nfa, 4);
    out4[4 * i + 1] = res[i].imin;
    memcpy(&out4[4 * i + 2], &res[i].logalpha, 4);
    out4[4 * i + 3] = res[i].nan;
  }
  return MODS_OK;
}

int mods_orsa_h(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                double *H_out, int *n_inliers, float *log_nfa, double *thr_px, int *index_out, int *n_index, int *stats3) {
  return orsa_h_filter(u6, laf, n, w, h, par, mask, H_out, n_inliers, log_nfa, thr_px, index_out, n_index, stats3, true,
                       ransac_pinned_seed(), env_int("MODS_ORSA_BATCH", 512), env_int("MODS_ORSA_WG_KEYS", ORSA_WG_KEYS));
}

int mods_orsa_h_ex(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                   double *H_out, int *n_inliers, float *log_nfa, double *thr_px, int *index_out, int *n_index, int *stats3,
                   int on_device, int batch, int wg_keys) {
  return orsa_h_filter(u6, laf, n, w, h, par, mask, H_out, n_inliers, log_nfa, thr_px, index_out, n_index, stats3, on_device != 0,
                       ransac_pinned_seed(), batch > 0 ? batch : env_int("MODS_ORSA_BATCH", 512),
                       wg_keys > 0 ? wg_keys : env_int("MODS_ORSA_WG_KEYS", ORSA_WG_KEYS));
}

int mods_orsa_h_last_refit(float *nfa_loop, float *nfa_refit, int *taken) {
  if (!nfa_loop || !nfa_refit || !taken) return MODS_E_ARG;
  *nfa_loop = g_orsa_h_refit.nfa_loop; *nfa_refit = g_orsa_h_refit.nfa_refit; *taken = g_orsa_h_refit.taken;
  return MODS_OK;
}

int mods_orsa_h_last_threshold(double *thr_px, float *log_nfa) {
  if (!thr_px || !log_nfa) return MODS_E_ARG;
  *thr_px = g_orsa_h_refit.thr_px; *log_nfa = g_orsa_h_refit.log_nfa;
  return MODS_OK;
}

int mods_model_kind(int useF) {
  if (useF == 0 || useF == 3) return 0;
  if (useF == 1 || useF == 2) return 1;
  set_error("model_kind: useF = %d is none of 0 (LO-RANSAC H), 1 (DEGENSAC F), 2 (ORSA F), 3 (ORSA H)", useF);
  return MODS_E_ARG;
}

int mods_test_orsa_h_tables(int n, float *logcn, float *logc4) {
  if (n < 0 || !logcn || !logc4) return MODS_E_ARG;
  std::vector<float> cn, c4;
  orsa_h::tables(n, cn, c4);   // the one-pass form mods_orsa_h uses; the tests hold it against logcombi term by term
  memcpy(logcn, cn.data(), sizeof(float) * (n + 1));
  memcpy(logc4, c4.data(), sizeof(float) * (n + 1));
  return MODS_OK;
}

// the solve and the scoring of m samples: on_device 1 through orsa_score_kernel<ModelH>, 0 through the host scalar path; p1 / p2 =
// n x 2 normalised points of image 1 / 2, samples4 = m x 4 distinct indices below n; out4 per model = nfa (float bits), imin,
// logalpha (float bits), invalid flag; H_out9 = m x 9 floats
int mods_test_orsa_h_score(const float *p1, const float *p2, int n, int w, int h, const int *samples4, int m, int on_device,
                           int wg_keys, int *out4, float *H_out9) {
  if (!p1 || !p2 || !samples4 || !out4 || !H_out9 || n < 5 || m < 0 || w <= 0 || h <= 0) {
    set_error("orsa_h_score: bad argument");
    return MODS_E_ARG;
  }
  for (int i = 0; i < 4 * m; i++)
    if (samples4[i] < 0 || samples4[i] >= n) { set_error("orsa_h_score: sample index %d outside [0, %d)", samples4[i], n); return MODS_E_ARG; }
  orsa_h::Problem P;
  P.n = n;
  P.p1.assign(p1, p1 + 2 * n); P.p2.assign(p2, p2 + 2 * n);
  orsa_h::setup(P, w, h, false);   // the points as given (already normalised)
  std::vector<float> Hv;
  std::vector<orsa::Score> res;
  if (on_device) {
    DeviceScorer dev;
    if (!dev.init(P, wg_keys > 0 ? wg_keys : ORSA_WG_KEYS)) return MODS_E_NODEVICE;
    if (!dev.score<ModelH>(nullptr, samples4, m, res, &Hv)) return MODS_E_HIP;
  } else {
    host_score_block_h(P, samples4, Hv, m, res);
  }
  for (int i = 0; i < m; i++) {
    memcpy(&out4[4 * i], &res[i].nfa, 4);
    out4[4 * i + 1] = res[i].imin;
    memcpy(&out4[4 * i + 2], &res[i].logalpha, 4);
    out4[4 * i + 3] = res[i].nan;
  }
  memcpy(H_out9, Hv.data(), sizeof(float) * 9 * m);
  return MODS_OK;
}

// (float)log10((double)x) on the device for the float bit patterns [begin, begin + count) against glibc on the host; returns the
// number of mismatches, the first max_list of their bit patterns in list
long long mods_test_orsa_log10_sweep(unsigned begin, unsigned count, unsigned *list, int max_list) {
  OrsaGpu *ws = orsa_gpu();
  if (!ws) return MODS_E_NODEVICE;
  const unsigned chunk = 1u << 26;
  Buf<float> d; PinnedBuf<float> hbuf;
  if (reserve_group(d, chunk, hbuf, chunk) != hipSuccess) {
    set_error("log10_sweep: allocation failed");
    return MODS_E_HIP;
  }
  long long bad = 0;
  int listed = 0;
  std::mutex mu;
  for (unsigned long long off = 0; off < count; off += chunk) {
    const unsigned c = (unsigned)std::min<unsigned long long>(chunk, count - off);
    const unsigned b0 = begin + (unsigned)off;
    hipLaunchKernelGGL(orsa_log10_kernel, dim3((c + 255) / 256), dim3(256), 0, ws->stream, b0, c, d.get());
    if (hipMemcpyAsync(hbuf, d, sizeof(float) * c, hipMemcpyDeviceToHost, ws->stream) != hipSuccess ||
        hipStreamSynchronize(ws->stream) != hipSuccess) { bad = MODS_E_HIP; break; }
    const int parts = 64;
    rs::TaskPool::get().run(parts, [&](int p) {
      const unsigned lo = (unsigned)((unsigned long long)c * p / parts), hi = (unsigned)((unsigned long long)c * (p + 1) / parts);
      for (unsigned i = lo; i < hi; i++) {
        float x;
        const unsigned bits = b0 + i;
        memcpy(&x, &bits, 4);
        const float want = orsa::log10_ref(x);
        if (memcmp(&want, &hbuf[i], 4) != 0 && !(want != want && hbuf[i] != hbuf[i])) {
          std::lock_guard<std::mutex> lk(mu);
          bad++;
          if (list && listed < max_list) list[listed++] = bits;
        }
      }
    });
  }
  return bad;
}

}  // extern "C"
