// Internal declarations of libmodsgpu (context, device buffers, launch helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mods_hip.h"
#include "buffer.hpp"
#include "pixel_sources.hpp"
#include "detection_mask.hpp"

namespace mods {

void set_error(const char *fmt, ...);

#define MODS_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      mods::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return MODS_E_HIP;                                                                  \
    }                                                                                     \
  } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel AND device: a function's attributes live with the device's
// code object, and a process may hold contexts on several GPUs (mods_multi, MODS_DEVICES).  `site` = a static per call site.
struct DynLdsOnce { std::atomic<unsigned> done{0}; };
inline hipError_t dyn_lds_once(DynLdsOnce &site, const void *fn, int bytes, int device) {
  const unsigned bit = 1u << (device & 31);
  if (site.done.load(std::memory_order_acquire) & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) site.done.fetch_or(bit, std::memory_order_release);
  return e;
}

// How the calling thread waits for a stream.  The runtime's hipStreamSynchronize spins on the completion signal: a pipeline
// worker that waits 40 ms for its batch of pairs then burns a whole core, and eight ranks of a node need the cores for the
// verification.  A thread that sets tl_wait_sleep_ns > 0 (the pipeline's workers do) polls hipStreamQuery instead: a short
// run of back-to-back queries for work that is about to finish, then a nanosleep between queries.  No interrupt path of the
// runtime is involved (hipDeviceScheduleBlockingSync hung on the test boxes).  Everything else keeps the runtime's wait.
inline thread_local long tl_wait_sleep_ns = 0;
inline thread_local long tl_wait_sleep_max_ns = 0;   // the sleep between two polls grows by half per poll up to this (a long wait costs few polls, a short one stays sharp)
inline thread_local int tl_wait_spin_polls = 8;
hipError_t stream_wait(hipStream_t s);
// hipMemcpy / hipMemset that wait, on a stream of the library instead of the legacy stream: an operation on the legacy stream waits
// for every blocking stream of the process and is REFUSED (hipErrorStreamCaptureImplicit) while another thread records a stream
// (mods_ctx_graphs: a pipeline worker recording its launch chain) - seen once as a failed workspace growth of a verify thread
hipError_t copy_wait(hipStream_t s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
hipError_t fill_wait(hipStream_t s, void *dst, int value, size_t bytes);
hipStream_t thread_stream(int dev = -1);   // a non-blocking stream of the calling thread on device `dev` (-1: the current one; entry points without a context)
int device_of_pointer(const void *p);      // the device a device pointer lives on, -1 when the runtime does not know it as one
void wait_mode_for_worker(long default_sleep_ns);   // MODS_SYNC=spin|sleep[:us] decides for the pipeline's threads

constexpr int kMaxOctaves = 16;
constexpr int kMaxLevels = 8;        // numberOfScales + 2 <= 8
constexpr int kMaxBlurRadius = 16;   // fused separable blur: ksize <= 33
constexpr int kAltTapStride = 512;   // widest kernel of the DoG / Harris response blurs (ksize <= 511)

// One octave of the scale space for a batch of images: plane(b) = base + b * w * h.
struct OctaveDev {
  int w, h;
  float pixelDistance;
  float sigma[kMaxLevels];
  float *blur[kMaxLevels];
  float *resp[kMaxLevels];
  unsigned int *omap;                // dedup map (pyramid.cpp octaveMap), one u32 per pixel
};

struct PyramidDev {
  int n_oct;
  int n_levels;                      // numberOfScales + 2
  OctaveDev oct[kMaxOctaves];
};

// raw NMS hit / localisation record, device side (AoS, 64 B)
struct CandDev {
  int octave, level, r0, c0;
  int r, c;
  float x, y, s, pixelDistance, response;
  int type;
  int state;                         // 0 rejected, 1 passed tests (pending dedup), 2 accepted
  float a11, a12, a21, a22;          // Baumberg result
};

struct StageTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<hipEvent_t> pool;
  double total_ms = 0;
  int launches = 0;
  double bytes = 0;
};

}  // namespace mods

__host__ __device__ inline size_t tent_u6_off(size_t n) { return (n * sizeof(mods_tentative) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t tent_laf_off(size_t n) { return tent_u6_off(n) + n * 6 * sizeof(double); }
__host__ __device__ inline size_t tent_bytes(size_t n) { return tent_laf_off(n) + n * 14 * sizeof(double); }

namespace mods {

// The inverse of a row-major 3 x 3 matrix as the guided gate and the overlap search's common-area test take it: the closed form of
// invert3_cv (describe.hip), adjugate times the reciprocal of the determinant, one rounding per operation.  false (and *det) when the
// determinant is 0 or not finite
inline bool invert3_adjugate(const double *S, double *t, double *det) {
  double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
  *det = d;
  if (d == 0. || !std::isfinite(d)) return false;
  d = 1. / d;
  t[0] = (S[4] * S[8] - S[5] * S[7]) * d; t[1] = (S[2] * S[7] - S[1] * S[8]) * d; t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
  t[3] = (S[5] * S[6] - S[3] * S[8]) * d; t[4] = (S[0] * S[8] - S[2] * S[6]) * d; t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
  t[6] = (S[3] * S[7] - S[4] * S[6]) * d; t[7] = (S[1] * S[6] - S[0] * S[7]) * d; t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
  return true;
}

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The packed form of n tentatives (mods_ctx::m_tent) split into / joined from three arrays.  These two and the device code that
// writes and reads the packed form (match.hip: the emit kernel, dedup.hip) are all that knows the layout.  unpack: any of the
// three destinations may be null
inline void tent_unpack(const char *packed, size_t n, mods_tentative *tent, double *u6, double *laf) {
  if (tent) memcpy(tent, packed, sizeof(mods_tentative) * n);
  if (u6) memcpy(u6, packed + tent_u6_off(n), sizeof(double) * 6 * n);
  if (laf) memcpy(laf, packed + tent_laf_off(n), sizeof(double) * 14 * n);
}
inline void tent_pack(char *packed, size_t n, const mods_tentative *tent, const double *u6, const double *laf) {
  memcpy(packed, tent, sizeof(mods_tentative) * n);
  memcpy(packed + tent_u6_off(n), u6, sizeof(double) * 6 * n);
  memcpy(packed + tent_laf_off(n), laf, sizeof(double) * 14 * n);
}

// A tentative list on the host: tent[n], the correspondences u6[n][6] and the frames laf[n][14], always of one length
struct TentList {
  std::vector<mods_tentative> tent;
  std::vector<double> u6, laf;
  size_t size() const { return tent.size(); }
  bool empty() const { return tent.empty(); }
  void clear() { tent.clear(); u6.clear(); laf.clear(); }
  void resize(size_t n) { tent.resize(n); u6.resize(n * 6); laf.resize(n * 14); }
  void truncate(size_t n) { if (n < size()) resize(n); }
  void append(const TentList &o) {
    tent.insert(tent.end(), o.tent.begin(), o.tent.end());
    u6.insert(u6.end(), o.u6.begin(), o.u6.end());
    laf.insert(laf.end(), o.laf.begin(), o.laf.end());
  }
  void unpack_from(const char *packed, size_t n) { resize(n); tent_unpack(packed, n, tent.data(), u6.data(), laf.data()); }
  void pack_into(char *packed) const { tent_pack(packed, size(), tent.data(), u6.data(), laf.data()); }
  // the verified correspondences a verification left in the first rows, as (x1 y1 x2 y2) per match
  void copy_matches(int n, double *matches_out, int max_matches) const {
    if (!matches_out) return;
    for (int m = 0; m < n && m < max_matches && (size_t)m < size(); m++) {
      const double *p = &u6[(size_t)m * 6];
      matches_out[4 * m] = p[0]; matches_out[4 * m + 1] = p[1]; matches_out[4 * m + 2] = p[3]; matches_out[4 * m + 3] = p[4];
    }
  }
};

// mods_ctx::m_count, the pinned counter block: three runs of kCountSlots ints - list lengths the emit kernel writes, lengths the
// device duplicate filter kept, and that filter's status (0 = filtered).  Entry 0 of a run belongs to the last single search
// (kLastSearch), entry 1 + i to pair i of a batch: a batch holds at most kCountSlots - 1 pairs
constexpr int kCountSlots = 64;
constexpr int kCountInts = 3 * kCountSlots;
constexpr int kLastSearch = -1;
constexpr int count_slot(int pair = kLastSearch) { return 1 + pair; }
constexpr int kept_slot(int pair = kLastSearch) { return kCountSlots + 1 + pair; }
constexpr int status_slot(int pair = kLastSearch) { return 2 * kCountSlots + 1 + pair; }
inline int read_slot(const int *counts, int slot) { return ((const volatile int *)counts)[slot]; }   // a device wrote it: after a stream wait

struct MserState;   // mser.hip

}  // namespace mods

struct mods_ctx {
  mods_ctx() = default;
  ~mods_ctx();                       // capi.hip: what is not memory (events, graph execs, helpers, streams); every buffer below frees itself
  int device = 0;
  int n_cu = 256;                    // compute units of the device (sizes the persistent grids)
  int max_w = 0, max_h = 0, batch = 1;
  hipStream_t stream = nullptr;
  hipEvent_t pyr_scope_begin = nullptr;   // MODS_STAGE_PYRAMID: opened by pyramid_build, closed by detect_run after the compaction
  // the octaves from the third on are built on a side stream next to the large octaves' last level and their NMS (pyramid_build
  // forks, detect_run joins before the compaction)
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool pyr_side = false;
  int pyr_side_first = 0;                 // the first octave built on the side stream
  int pyr_streams = 2;                    // mods_ctx_pyramid_streams: 1 keeps the whole scale space on ctx->stream
  // scale space
  mods::PyramidDev pyr;              // host copy of the descriptor table
  mods::Buf<mods::PyramidDev> pyr_dev;
  mods::PyramidDev pyr_dev_image;    // what pyr_dev holds (pyramid_configure uploads the table only when it changed)
  bool pyr_dev_valid = false;
  mods::Buf<float> plane_pool;       // all blur/response planes
  mods::Buf<unsigned int> omap_pool;
  bool omap_dirty = true;            // the pool holds cells that are not 0xFFFFFFFF (detect_run fills it before use)
  mods::Buf<float> input_dev;        // staging for host-pointer entry points
  mods::Buf<float> tmp_dev;
  // DoG / Harris responses (pyramid.cpp:165-194, 256-278): per-level tap tables of the response's own blur and scratch planes
  mods::Buf<float> alt_taps_dev;           // [kMaxLevels][kAltTapStride]
  int alt_ntap[mods::kMaxLevels] = {0};
  float alt_sigma[mods::kMaxLevels] = {0};  // sigma the tables were built for
  mods::Buf<float> alt_planes;       // 4 planes of the first octave's size
  mods::Buf<float> view_dev;         // pixels of the current synthesised view (allocated on first use)
  mods::Buf<float> gauss_taps_dev;   // [16 slots][64] Gaussian taps
  float taps_sigma[16] = {0};        // sigma currently held by each slot (0 = empty)
  float taps_host[16][2 * mods::kMaxBlurRadius + 1] = {{0}};
  int taps_host_n[16] = {0};
  mods::Buf<float> smm_mask_dev;     // computeGaussMask(smmWindowSize)
  mods::Buf<unsigned long long> baum_stats_dev;   // per image slot: {keypoints that entered the Baumberg iteration, iterations run} (mods_baumberg_stats)
  int smm_mask_size = 0;
  // candidates
  int max_cand = 0;                  // per image
  mods::Buf<mods::CandDev> cand;     // [batch][max_cand]
  mods::Buf<int> cand_count;         // [3][batch] raw NMS hits, accepted, keys
  mods::Buf<mods_affkey> keys_dev;   // [batch][max_cand] sorted output
  mods::Buf<unsigned long long> sort_keys;
  mods::Buf<int> sort_idx;
  mods::Buf<int> rank_dev;           // [batch][max_cand]
  mods::Buf<unsigned long long> nms_mask;   // ballot words of one octave's NMS
  mods::PinnedBuf<int> host_counts;
  mods::Buf<unsigned char> u8_stage_dev;   // [batch][max_h][max_w] staging of 8-bit host images (pair pipeline), lazily allocated
  // the images of an 8-bit call once more in 16-byte column strips (u8_strips.hpp), made by the conversion launch of such a call
  // when a kernel of the mask samples from strips: [n_img][strip_count(w)][h rounded up to 8][16].  The library makes it, reads it
  // and forgets it with the call (u8_sources_launch hands it to the call as PixelSources::strips)
  mods::Buf<unsigned char> u8_strip_dev;
  long u8_strip_calls = 0;               // calls that had one (mods_ctx_u8_strip_calls)
  int u8_kernels = -1;                   // which kernels sample from the 8-bit copies: -1 = the default (pixel_sources.hpp), else a mask
  long u8_source_calls = 0;              // calls whose 8-bit images were a sampling source (mods_ctx_u8_source_calls)
  // CLAHE (clahe.hip): LUT scratch [n_img][tiles_y * tiles_x][256] (clahe_reserve); clahe_on: the pair pipeline's 8-bit batches are
  // equalised with clahe_par on their way to fp32 (mods_pipeline_create_clahe)
  mods::Buf<unsigned char> clahe_lut;
  bool clahe_on = false;
  mods_clahe_params clahe_par = {0.0, 0, 0};
  mods::PinnedBuf<char> pin_arena;   // pinned host staging of a batch's tentative lists (pair pipeline), lazily allocated
  mods_hessaff_params par;
  int reg_number_eff = -1;           // par.regionsNumber after the tilt / zoom scaling of DetectAffineKeypoints (scale-space-detector.cpp:20-21)
  // spatial selection of the count modes' cut (mods_ctx_spatial_selection; spatial_select.hip): 0 off, 1 ANMS, 2 ANMS where the
  // call's mode and detector allow it; its scratch is sort_keys and rank_dev, dead after the export
  int spatial_mode = 0;
  double spatial_c = 0.9;
  // a doubled first octave for the scale-space detectors (mods_ctx_upscale_input; pyramid.hip): 0 off, 1 on, 2 on with the first
  // level unfused (the doubled batch goes through up_tmp: reserved by the first call that needs it, also mods_upscale2x's output)
  int upscale_mode = 0;
  mods::Buf<float> up_tmp;
  int last_w = 0, last_h = 0, last_n_img = 0;
  const float *last_img_dev = nullptr; int last_stride = 0;   // the batch the pyramid was built from (sampleFromImage)
  // orientation + description
  mods::Buf<float> desc_tables_dev;  // [orimask 64x64][desc mask 64x64][orientation vote mask 64x64][SiftTab], offsets kTab*
  mods::Buf<int> desc_err_dev;
  int desc_ori_ps = 0, desc_ps = 0;
  mods::Buf<char> ori_dev;           // [batch][max_cand] OriOut (describe.hip), in bytes
  mods::Buf<char> ori_multi_dev;     // [batch][max_cand][ori_cap] OriOut (maxAngles > 1), allocated on first use
  mods::Buf<mods_region> regions_dev;  // [batch][max_cand]
  mods::Buf<mods_region> regions_half_dev;   // HalfRootSIFT twins (allocated on first use)
  bool have_half = false;
  mods::Buf<int> region_count;       // [batch]
  mods::Buf<int> inside_count;       // [batch] keypoints that pass the centre test (the reference's unoriented list)
  std::vector<int> last_inside_counts;
  mods::Buf<float> desc_scratch;
  // domain-size pooling of the SIFT descriptor (mods_ctx_domain_pooling; sift.hip): dsp_scales = 0 is off; the accumulators
  // [batch][reg_cap][128] are reserved by the first describe call with pooling on
  int dsp_scales = 0;
  double dsp_start = 0, dsp_end = 0;
  mods::Buf<double> dsp_acc;
  int blur_table_ps = 0;
  mods::Buf<float> blur_table_dev;   // per-P2 taps / resampling sequence / source indices of the LDS extraction tier (sift.hip: blur_table_kernel)
  // external descriptor (e.g. a ZMQ daemon): when set, patches go to this function instead of the SIFT kernel
  mods_descriptor_fn ext_fn = nullptr;
  void *ext_user = nullptr;
  double ext_mr = 0;
  int ext_ps = 0;
  // AffNet / OriNet in the place of Baumberg / the dominant gradient orientation (imagerepresentation.cpp:786-856, 874-900)
  mods_descriptor_fn shape_fn = nullptr, ori_fn = nullptr;
  void *shape_user = nullptr, *ori_user = nullptr;
  double shape_mr = 0, ori_mr = 0;
  int shape_ps = 0, ori_ps = 0;
  // the same three slots served in-process (nets.hip): a network reads the patch store in HBM, only its 3 / 2 / 128 values per
  // patch go to the host.  A slot holds a callback or a network, never both; the networks are shared, not owned
  mods_net *shape_net = nullptr, *ori_net = nullptr, *ext_net = nullptr;
  int shape_q8 = 0, ori_q8 = 0, ext_q8 = 0;          // round the patches to 8 bits first, as the wire to a daemon does
  mods::Buf<float> net_out_dev;      // the networks' outputs of one image slot (floats), grown on demand
  std::vector<int> last_region_counts;
  // matching
  mods::Buf<int8_t> m_desc;          // [2][pad][128] int8 descriptors (query list, train list)
  mods::Buf<int> m_c;                // [2][pad] precombined norms
  mods::Buf<double2> m_xy;           // [2][pad] centres
  mods::Buf<unsigned long long> m_u64;
  mods::Buf<int> m_int;
  mods::Buf<char> m_mid;             // QueryMid records (match.hip), in bytes
  mods::Buf<char> m_p2;              // pass-1 top-2 keys per train split, pass-2 query subset (see match.hip)
  size_t m_best2_cap = 0;            // entries (pairs of keys) in the top-2 table
  int m_sets = 0;                    // searches the matcher's scratch buffers hold side by side (match_ensure_buffers)
  mods::Buf<char> m_tent;
  // m_tent holds the n tentatives of the last search PACKED: mods_tentative[n] | (16-byte aligned) u6[n][6] = the correspondences
  // (x1 y1 1 x2 y2 1) | laf[n][14] = the frames (x y a11 a12 a21 a22 s) of both regions - one device-to-host copy of
  // tent_bytes(n) bytes brings all three (tent_u6_off / tent_laf_off give the parts)
  mods::PinnedBuf<int> m_count;      // PINNED HOST memory (kCountInts ints), indexed by count_slot / kept_slot / status_slot
  mods_tentative *m_tent_out = nullptr; int *m_count_out = nullptr;   // set by a batch of pairs: where match_run leaves the packed list / its length
  mods::Buf<char> m_tent_batch;      // the packed lists of a batch, one segment per pair
  mods::Buf<mods_region> m_regs;     // [2][max_cand] staging for host-side lists
  mods::Buf<char> dd_buf; int dd_jobs = 0;   // duplicate filter on the device (dedup.hip): per list of a batch sorted coordinates, ranks, near lists
  mods::Buf<char> m_tent2;           // the filtered packed list of the last search (single-pair path)
  mods::TentList h_list;             // host copy for the sequential stages
  int h_verified = 0;                // rows at the head of h_list that the last pair / ladder / verify call verified (mods_ctx_verified_lafs)
  std::vector<unsigned char> h_mask;
  // the searches of two region lists (list_search.hpp): the staging of host lists, which they share
  mods::Buf<mods_region> ls_regs;
  // guided matching (guided.hip), its own buffers: gate records and dense descriptor rows of both lists (queries first), the
  // per-query (nearest, inconsistent second) and per-train keys, accept flags + block counts, the packed result and its length
  mods::Buf<double4> g_rec;
  mods::Buf<unsigned char> g_desc;
  mods::Buf<unsigned long long> g_key;
  mods::Buf<int> g_int;
  mods::Buf<char> g_tent;
  mods::PinnedBuf<int> g_count;
  // overlap matching (overlap.hip), its own buffers: 48-byte fp64 records of both lists (queries first, 6 doubles each), the error
  // keys (per train, per query, per split and query), the integer twins (common counts, per-train owner, per-query train, block
  // counts, per split and query), the matches and (matches, common queries, common trains); o_splits: mods_ctx_overlap_splits
  mods::Buf<double> o_rec;
  mods::Buf<unsigned long long> o_key;
  mods::Buf<int> o_int;
  mods::Buf<mods_overlap_match> o_out;
  mods::PinnedBuf<int> o_count;
  int o_splits = 0;
  // area-overlap matching (overlap_area.hip), its own buffers: the 48-byte records of both lists (queries first), the error keys
  // (per train, per query, per listed pair), the integers (common counts, per-train owner, per-query pair and train, the sweep's
  // block counts, per split and query the pair count and the list offset; oa_pair: the list's (q, t), its three pixel counts and
  // the compaction's block counts), the matches and (items, common queries, common trains, listed pairs as two halves of 64
  // bits); oa_host: the accepted pairs of mode 2
  mods::Buf<double> oa_rec;
  mods::Buf<unsigned long long> oa_key;
  mods::Buf<int> oa_int;
  mods::Buf<int> oa_pair;            // what is sized by the pair list (its length is known between the two gate sweeps)
  mods::Buf<mods_overlap_area_match> oa_out;
  mods::PinnedBuf<int> oa_count;
  std::vector<mods_overlap_area_match> oa_host;
  // mutual check of the FGINN searches (mutual.hip; mods_ctx_match_mutual), reserved on the first search with a mode set: 16 counters
  // and the candidate lists (q, t, d1, D*) of the matcher's sets; the candidate counts again, pinned
  int mutual_mode = 0;
  bool mu_last_checked = false;      // the last single search of the context went through the check
  mods::Buf<int4> mu_cand;
  mods::PinnedBuf<int> mu_count;
  // k-nearest-neighbour search (knn.hip), its own buffers, reserved on first use: the packed lists (queries first: descriptors;
  // norms, seeds, parity words and the pack kernel's two counters; centres), the sorted keys every (train split, query) leaves, the
  // result rows on the device (d2 | idx) and their pinned twin; kn_splits: mods_ctx_knn_splits
  mods::Buf<int8_t> kn_desc;
  mods::Buf<int> kn_c;
  mods::Buf<double2> kn_xy;
  mods::Buf<unsigned long long> kn_part;
  mods::Buf<int> kn_out;
  mods::PinnedBuf<int> kn_host;
  int kn_splits = 0;
  // distractor databases of the FGINN searches (distractor.hip; mods_ctx_distractor_db): the attached databases (a reference each),
  // which of them the next search takes (dr_half_search: set around a HalfRootSIFT search by its caller), the scratch of the veto
  // per set of the matcher - compact packed queries, norms, their query indices, dDB per query, dDB per survivor, 16 counters - and
  // the forward counts, pinned; the staging of the host entry points; dr_splits: mods_ctx_descdb_splits
  const mods_descdb *dr_db[2] = {nullptr, nullptr};
  bool dr_half_search = false;
  bool dr_last_vetoed = false;       // the last single search of the context went through the veto
  mods::Buf<int8_t> dr_desc;
  mods::Buf<int> dr_int;
  mods::PinnedBuf<int> dr_count;
  mods::Buf<unsigned char> dr_stage;
  mods::Buf<int> dr_out;
  mods::PinnedBuf<int> dr_host;
  int dr_splits = 0;
  // local affine consistency filter (local_affine.hip; mods_ctx_local_affine): off by default.  la_buf: the SoA scratch, counters and
  // places of the lists of one set of launches; la_io: source and kept list of the host-list entry point; la_count: list lengths in and
  // out, pinned; the counts of the last filtered list
  bool la_on = false;
  mods_local_affine_params la_par = {160., 3., 4., 0.2, 2., 3, 1, 1};
  mods::Buf<char> la_buf, la_io;
  mods::PinnedBuf<int> la_count;
  int la_n_in = 0, la_n_kept = 0;
  // least-squares refinement of correspondences (refine.hip; mods_refine_matches[_dev]).  lsm_buf: the rows in and out, their
  // statuses, iteration counts and zncc values (and the seam's 49 doubles); lsm_img: the two images of the host entry points
  mods::Buf<char> lsm_buf;
  mods::Buf<float> lsm_img;
  // match propagation (propagate.hip; mods_propagate_matches[_dev]).  prop_grid: per cell the state, the proposal key and the tried
  // maps, then the scan's block sums, the counters and the statistics; prop_seed: the seed rows in and out; prop_cand: the candidate
  // rows of a round in and out; prop_out: the output list (the front of the next round is its tail); prop_img: the two images of the
  // host entry point; prop_ctr: the counters the host reads, pinned
  mods::Buf<char> prop_grid, prop_seed, prop_cand, prop_out;
  mods::Buf<float> prop_img;
  mods::PinnedBuf<int> prop_ctr;
  // detection masks (mods_ctx_detection_mask*; detection_mask.hpp, detect.hip): det_masks = what the caller set per image of a call
  // (det_mask_own: the context's copies of host masks), gate_tab_host / gate_tab_dev = the table the gate kernel reads, per image
  // slot, as the last call bound it (a view worker of the ladder binds its owner's masks: gate_owner, gate_image), gate_counts_dev =
  // [batch][2] entries that reached the gate and entries kept, gate_had_mask = which slots of the last call were gated
  std::vector<mods::DetMaskDev> det_masks;
  std::vector<mods::Buf<unsigned char>> det_mask_own;
  mods::Buf<unsigned char> det_mask_stage;   // [batch][h][w]: the masks of a batch of host pairs (pair pipeline), uploaded with their images
  bool det_mask_staged = false;              // det_masks hold what the last batch of pairs staged, not what the caller set
  std::vector<mods::DetMaskDev> gate_tab_host;
  mods::Buf<mods::DetMaskDev> gate_tab_dev;
  mods::Buf<int> gate_counts_dev;
  std::vector<char> gate_had_mask;
  bool gate_active = false;          // the call in flight has a mask on at least one of its images
  mods::DetGateFrame gate_frame;     // ... and this is the frame they live in
  const mods_ctx *gate_owner = nullptr;
  int gate_image[2] = {0, 1};
  // a ladder call's counts: summed over its views by whichever context ran them, per image of the call {reached the gate, kept};
  // gate_ladder_last: the context's last call was a ladder (mods_ctx_detection_mask_counts then reports these)
  std::atomic<long long> gate_ladder[4] = {{0}, {0}, {0}, {0}};
  bool gate_ladder_last = false;
  mods::MserState *mser = nullptr;   // MserState (mser.hip): buffers of the MSER detector, allocated on first use
  // the step loop spreads the views of a step over a few more contexts of the same GPU (imgrep.hip: run_view_jobs)
  std::vector<mods_ctx *> helpers;
  std::atomic<bool> helpers_failed{false};   // a helper context could not be made (memory): reported once, not retried
  std::vector<mods::Buf<mods_region>> helper_stage;   // view staging, one arena per helper (imgrep.hip)
  // timing
  int timing_mask = 0;
  // mods_ctx_graphs: the launches of a detect + describe call replayed as one hipGraph (capi.hip: mods_detect_describe_dev)
  bool dd_graphs = false;
  // `epoch` = dev_state_epoch when the call was made: every host-side change of device tables or pools bumps that counter
  // (mods::dev_state_changed / dev_pool_reallocated), so a call behind such a change is never taken for a repeat of the one before it
  struct DdKey { mods::PixelSources img;      // the call's images: fp32, and its 8-bit sampling sources (the strip twin's layout follows from w, h)
                 int n_img = 0, w = 0, h = 0, stride = 0; unsigned long long par_hash = 0, epoch = ~0ull;
                 bool operator==(const DdKey &o) const { return img == o.img && n_img == o.n_img && w == o.w && h == o.h && stride == o.stride && par_hash == o.par_hash && epoch == o.epoch; } };
  unsigned long long dev_state_epoch = 0;
  std::vector<std::pair<DdKey, hipGraphExec_t>> dd_cache;   // recorded calls (a worker sees a few batch sizes), oldest first
  bool dd_stale = false;                                    // a pool the recordings point into was reallocated: they are dropped
  DdKey dd_prev;                                            // arguments of the context's previous detect + describe call
  std::vector<DdKey> dd_linear;                             // arguments whose recording had no second branch: never replayed (see dd_run)
  bool pyr_forked = false;                                  // the last pyramid_build put octaves on the side stream
  long dd_replays = 0;
  mods::StageTimer timers[MODS_STAGE_COUNT];
};

namespace mods {

// float offsets of the tables in mods_ctx::desc_tables_dev
constexpr int kTabOriMask = 0, kTabDescMask = 4096, kTabVoteMask = 8192, kTabSift = 12288;

// A hipGraph replay of a detect + describe call is valid only while the device tables and pools it was recorded against are
// untouched: every upload, setter and (re)allocation that changes them from the host goes through one of these two
inline void dev_state_changed(mods_ctx *c) { c->dev_state_epoch++; }                          // tables / parameters refreshed from the host
inline void dev_pool_reallocated(mods_ctx *c) { c->dev_state_epoch++; c->dd_stale = true; }   // a pool moved: recordings are dropped

// How a buffer of a context grows (buffer.hpp knows no streams): launches on ctx->stream may still use the allocation that a growth
// frees, so the stream is waited for first - only when something is freed, never in steady state.  `alloc_elems` is the caller's
// growth policy.  The capacity is set by the buffer, never by the caller
template <class B> inline hipError_t reserve_scratch(mods_ctx *c, B &b, size_t need, size_t alloc_elems, bool *moved = nullptr) {
  if (need <= b.capacity()) return hipSuccess;
  if (b.get()) { const hipError_t e = stream_wait(c->stream); if (e != hipSuccess) return e; }
  return b.reserve(need, alloc_elems, moved);
}
// ... and one that recorded graphs point into: they are dropped when it moved
template <class B> inline hipError_t reserve_pool(mods_ctx *c, B &b, size_t need, size_t alloc_elems) {
  bool moved = false;
  const hipError_t e = reserve_scratch(c, b, need, alloc_elems, &moved);
  if (moved) dev_pool_reallocated(c);
  return e;
}
struct StageScope {                  // brackets launches of one stage with events when enabled
  mods_ctx *ctx; int stage; hipEvent_t e0 = nullptr, e1 = nullptr; bool on;
  StageScope(mods_ctx *c, int s, double bytes = 0);
  ~StageScope();
};

// pyramid.hip
int pyramid_configure(mods_ctx *ctx, int w, int h, int n_img, const mods_hessaff_params *par);
int pyramid_build(mods_ctx *ctx, const float *img_dev, int stride);
int pyramid_join_side(mods_ctx *ctx);   // joins a forked pyramid's side stream into ctx->stream (no-op without a pending fork)
int launch_gauss_blur(mods_ctx *ctx, const float *src, float *dst, int w, int h, int n_img, float sigma);
int launch_hessian_response(mods_ctx *ctx, const float *src, float *dst, int w, int h, int n_img, float norm);
int launch_resize_half(mods_ctx *ctx, const float *src, float *dst, int w, int h, int dw, int dh, int n_img);
int launch_upscale2x(mods_ctx *ctx, const float *src, float *dst, int w, int h, int n_img);   // double_image: [n_img][h][w] -> [n_img][2h][2w]
void resize_half_dims(int w, int h, int *dw, int *dh);
int gauss_ksize(float sigma);
void gauss_kernel_host(int n, double sigma, float *out);
void gauss_mask_host(int size, float *out);
void circular_gauss_mask_host(int size, float sigma, float *out);

// clahe.hip
int clahe_reserve(mods_ctx *ctx, int n_img, const mods_clahe_params *par);   // LUT scratch of n_img images (hipMalloc when it grows)
int clahe_launch(mods_ctx *ctx, const unsigned char *src, int n_img, int w, int h, int src_stride, const mods_clahe_params *par,
                 void *dst, int dst_stride, int dst_f32);                    // LUT + apply launches on ctx->stream, no wait

// detect.hip
int detect_run(mods_ctx *ctx);       // NMS -> localise -> dedup -> Baumberg -> sort, for the configured batch
size_t nms_octave_mask_words(int w, int h, int border, int n_scales);   // ballot words of one image's NMS over one octave
// ranks of the unique 64-bit keys ctx->sort_keys[n_img][max_cand] (key_count[b] of them per image) into ctx->rank_dev: by one
// workgroup's sort or by counting, chosen by n_img
int rank_keys_launch(mods_ctx *ctx, int n_img, const int *key_count);

// The count a count mode's cut keeps of n keys (AffineDetector::prepareKeysForExport, scale-space-detector.hpp:150-166), before the
// clamp to [0, n]
__host__ __device__ inline int count_mode_keep(int mode, int n, int reg_number, float rel_reg_number) {
  if (mode == MODS_DET_FIXED_REG_NUMBER) return n < reg_number ? n : reg_number;
  if (mode == MODS_DET_RELATIVE_REG_NUMBER) return (int)floor((double)rel_reg_number * (double)n);
  return n;
}

// spatial_select.hip: the cut of a count mode taken by suppression radius instead of by response (mods_ctx_spatial_selection), over
// the exported lists in ctx->keys_dev; keep_list (device, per image) stands in for the mode's count when set (the test hook)
int spatial_select_launch(mods_ctx *ctx, int n_img, int *key_count, int mode, int reg_number, float rel_reg_number, float robustness,
                          const int *keep_list);

int detection_mask_bind(mods_ctx *ctx, int n_img, int w, int h, const DetGateFrame *frame);   // the call's masks -> the gate's table; sets gate_active
int launch_detection_mask_keys(mods_ctx *ctx, int n_img);   // the gate over the exported key lists (MSER)

// mser.hip
// frame: the original image and the way to it when the images are synthesised views (detection masks live there); null: the images themselves
int detect_any(mods_ctx *ctx, const float *img_dev, int n_img, int w, int h, int stride, const mods_hessaff_params *par, double tilt,
               double zoom, const DetGateFrame *frame = nullptr);   // the detector the parameter set names: scale space (pyramid + detect_run) or MSER
void mser_release(mods_ctx *ctx);

// match.hip
int match_run(mods_ctx *ctx, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, double ratio,
              double contradDist, int nn);
int match_run_distance(mods_ctx *ctx, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, double threshold);   // MatchFLANNDistance, Hamming
int match_ensure_buffers(mods_ctx *ctx, int n_sets = 1);
int match_run_group(mods_ctx *ctx, int n_jobs, const mods_region *const *q_dev, const int *n_q, const mods_region *const *t_dev, const int *n_t,
                    mods_tentative *const *tent_out, int *const *count_out, double ratio, double contradDist, int nn);   // <= 16 searches in one set of launches

// knn.hip: the K = min(k, n_t) nearest trains of every query of two device lists, in (d, t) order, into host rows [n_q][k] (either
// may be null); checks its arguments, waits for the stream
int knn_search(mods_ctx *ctx, const char *who, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, int k, int *idx_out,
               int *d2_out);
int knn_check(const char *who, int k, const int *idx_out, const int *d2_out);   // the refusals that need no context

// distractor.hip: the database veto of one grouped launch, in two parts around the emit kernels (match.hip: match_run_group; the
// pointers are those of set 0).  distractor_db_of: the database the context's next search takes, null for none
struct MatchJobs; struct MatchConst;
const mods_descdb *distractor_db_of(const mods_ctx *ctx);
int distractor_stage(mods_ctx *ctx, const mods_descdb *db, const MatchJobs &J, const MatchConst &k, int max_q, size_t pad, const void *mid,
                     const unsigned long long *key_ge, const unsigned long long *key_lt, const int *n_lt, int *bad, const int8_t *qd,
                     const int *qc);
int distractor_finish(mods_ctx *ctx, const MatchJobs &J, int max_q, size_t pad);
void distractor_release(mods_ctx *ctx);    // the context's references (its destructor)
// imgrep.hip: what a bank holds, for the files that do not see the struct
void imgrep_view(const mods_imgrep *r, const mods_region **reg, int *n, int *device, hipStream_t *stream);

// dedup.hip
constexpr int DUP_MAX_JOBS = 64;
struct DupJob { const char *src; char *dst; const int *n_src; int *n_dst; int *status; };
int dup_filter_dev(mods_ctx *c, const DupJob *jobs, int n_jobs, int grid_n, double r, int mode);
int dup_filter_reserve(mods_ctx *c, int n_jobs);
static_assert(DUP_MAX_JOBS <= kCountSlots, "every job of the duplicate filter has its slots in m_count");
// local_affine.hip
constexpr int LA_MAX_JOBS = 64, LA_ROWS = 256, LA_TILE = 256;   // lists per set of launches; rows of a block = columns of an LDS tile
struct LaConst { double R2, D2, A2, L2, areaTol; int minSupport, rescue, keepSparse; };
struct LaJob { const char *src; char *dst; const int *n_src; int *n_dst; };
struct LaBatch {
  int n_jobs, max_n;                   // max_n: positions of a list's scratch, a multiple of LA_TILE
  double *soa; size_t soa_stride;      // per list: x1 y1 x2 y2 t00 t01 t10 t11 dT valid, max_n doubles each
  int *counters;                       // per list: neighbours[max_n] | support[max_n] | backed[max_n], contiguous over the lists (one fill)
  int *slots, *res;                    // per list: places[max_n]; {kept, -}
  LaConst k;
  LaJob job[LA_MAX_JOBS];
};
__host__ __device__ inline int la_len(int n, int max_n) { return n < 0 || n > max_n ? 0 : n; }   // a list the launch was not sized for is left alone
int la_check(const mods_local_affine_params *p, LaConst *k);
int la_reserve(mods_ctx *c, int n_jobs, int grid_n);
int la_filter_dev(mods_ctx *c, const LaJob *jobs, int n_jobs, int grid_n, const LaConst &k, const int **diag_counters = nullptr,
                  const int **diag_slots = nullptr, int *diag_stride = nullptr);
struct TentList;
int local_affine_prefilter(mods_ctx *c, const mods_pair_params *par, TentList *list, bool deduped);
static_assert(LA_MAX_JOBS >= kCountSlots - 1, "every pair of a batch has its slots in la_count");
int launch_fast_sqrt_selftest(mods_ctx *ctx, unsigned long long *out5_host);   // describe.hip
int launch_blur_table(mods_ctx *ctx, int ps);   // sift.hip
bool ransac_profile_on();     // MODS_RANSAC_PROF: per-call breakdown of the verification on stderr (ransac.hip)
int ransac_profile_mode();    // 0 off, 1 wall time, 2 the calling thread's CPU time (MODS_RANSAC_PROF=cpu)

// describe.hip
// img: the call's copies of the images (pixel_sources.hpp); a view (H given) and a context with hooks or networks sample from fp32 only
int describe_run(mods_ctx *ctx, const PixelSources &img, int n_img, int w, int h, const mods_describe_params *par);
// pair.hip.  strips: the same launch lays the images out in c->u8_strip_dev as well (packed rows only: u8_strips_wanted)
int u8_to_f32_launch(mods_ctx *c, const unsigned char *src, int n_img, int w, int h, int stride, float *dst, bool strips = false);
// ... into c->input_dev, for a call that came in as 8-bit: *img = what the call samples from.  The 8-bit images themselves are a
// source when `twin` allows it and their rows are packed, the strip twin is made and is one when u8_strips_wanted on top of that;
// counts both (u8_source_calls, u8_strip_calls)
int u8_sources_launch(mods_ctx *c, const unsigned char *src, int n_img, int w, int h, int stride, bool twin, PixelSources *img);
int u8_stage_ensure(mods_ctx *c);          // pair.hip: c->u8_stage_dev and c->u8_strip_dev allocated (a full batch of the context's largest images)
int describe_run_view(mods_ctx *ctx, const PixelSources &img, int n_img, int w, int h, const mods_describe_params *par, const double *H,
                      int orig_w, int orig_h, mods_region *det_copy_dev);
// the frame of a view's regions as describe_run_view takes it from H (w x h: the view, orig_w x orig_h: the original): false for the
// identity view of the same canvas, where nothing is reprojected (frame->Hinv is the identity then)
bool view_region_frame(const double *H, int w, int h, int orig_w, int orig_h, DetGateFrame *frame);
int describe_configure(mods_ctx *ctx, const mods_describe_params *par);
int launch_dominant_angle_test(mods_ctx *ctx, const float *patch_dev, int ps, double th, float *out_dev);
int launch_sift_patch_test(mods_ctx *ctx, const float *patch_dev, int ps, int root, double max_bin, uint8_t *out_dev);
// its pooled twin (mods_test_sift_pooled), and what a describe call with domain-size pooling on cannot be combined with
// (MODS_E_ARG, before anything is launched)
int launch_sift_pooled_test(mods_ctx *ctx, const float *patches_dev, int K, int ps, int root, int half, int photo, double max_bin,
                            uint8_t *out_dev);
int dsp_check(mods_ctx *ctx, const mods_describe_params *par);

// nets.hip
inline bool has_hooks(const mods_ctx *c) { return c->ext_fn || c->shape_fn || c->ori_fn; }          // host callbacks (one context)
inline bool has_nets(const mods_ctx *c) { return c->ext_net || c->shape_net || c->ori_net; }        // built-in networks
// n patches [n][32][32] of the patch store through `net` on ctx->stream; the net's dim values per patch arrive in out_host (waits)
int net_run_to_host(mods_ctx *ctx, mods_net *net, const float *patches_dev, int n, int quantise_u8, float *out_host);

// pair.hip: the two halves of a pair.  The GPU half detects, describes and matches (a batch: the images of all pairs as one batch)
// and leaves every pair's tentatives in its list; the host-driven half filters duplicates and verifies the list in place
int pair_gpu_stage(mods_ctx *c, const float *img_dev, int w, int h, int stride, const mods_pair_params *par, mods_pair_result *res,
                   TentList *list);
int pairs_gpu_stage(mods_ctx *c, const void *const *img, const int *kinds, int n_pairs, int w, int h, const mods_pair_params *par,
                    mods_pair_result *const *res, TentList *const *lists, const unsigned char *const *masks = nullptr);
int pair_verify_stage(int device, const mods_pair_params *par, mods_pair_result *res, TentList *list, double *matches_out,
                      int max_matches, int w, int h);

}  // namespace mods

// entry points of the library that include/mods_hip.h does not list
extern "C" {
// capi.hip: the packed output of the last search in one device-to-host copy, split into the caller's arrays (synchronises the stream)
int mods_match_copy_out(mods_ctx *c, int n, mods_tentative *tent, double *u6, double *laf);
int mods_match_fetch_internal(mods_ctx *c, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out);   // capi.hip
int mods_ransac_warmup(int device, int len);                                                  // ransac.hip
int mods_ctx_warmup(mods_ctx *c, int n_img, int w, int h, const mods_pair_params *par);       // pair.hip
}
