// One pair end to end (include/mods_hip.h: mods_match_pair_dev, mods_verify_tentatives*, mods_duplicate_filter_gpu,
// mods_hmatrix_filter, mods_ctx_warmup) and the two halves the pair pipeline overlaps across pairs (pipeline.hip): the GPU half -
// detect, describe, match, DuplicateFiltering on the device - and the host-driven half - verification of the tentative list.
#include "common.hpp"
#include "u8_strips.hpp"
#include "../../include/mods_degensac.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace mods;

// DuplicateFiltering ahead of RANSAC runs on the device, behind the search (dedup.hip)
static bool dedup_on_device(const mods_pair_params *par) {
  return par->dup_before_ransac && par->dup_dist > 0 && par->dup_mode >= 0 && par->dup_mode <= 3;
}

// the filtered packed list of the single-pair path (mods_ctx::m_tent2), allocated on first use
static int ensure_tent2(mods_ctx *c) {
  MODS_HIP_CHECK(c->m_tent2.reserve(tent_bytes(((size_t)c->max_cand + 127) & ~(size_t)63) + 64));
  return MODS_OK;
}

// the duplicate filter's job for the last single search: m_tent -> m_tent2, the counters of kLastSearch
static DupJob single_pair_dup_job(mods_ctx *c) {
  return {c->m_tent, c->m_tent2, c->m_count + count_slot(), c->m_count + kept_slot(), c->m_count + status_slot()};
}

constexpr size_t kPinArena = (size_t)24 << 20;   // pinned staging of a batch's tentative lists

// The strip twin (u8_strips.hpp) of n_img packed w x h images: a lane makes one 16-byte row of a strip - the pixels 15 s ... 15 s + 15
// of image row y by one 16-byte load at any alignment, or byte by byte where the row ends inside them - and writes zeros where the
// layout pads (rows h ... h8 - 1, columns w ... of the last strip), so every byte of the twin is written.  A wave takes 8 rows of 8
// neighbouring strips: it reads 8 runs of 121 bytes and writes 8 whole 128-byte lines.
struct __attribute__((packed, aligned(1))) StripRowBytes { unsigned v[4]; };
__device__ __forceinline__ void u8_strip_rows(const unsigned char *__restrict__ src, unsigned char *__restrict__ strips, int n_img, int w, int h) {
  const unsigned ns = mods::strip_count(w), bands = ((unsigned)h + 7u) >> 3, pitch = mods::strip_pitch(h), groups = (ns + 7u) >> 3;
  const size_t items = (size_t)n_img * groups * bands;
  const unsigned lane = threadIdx.x & 63, yl = lane & 7, sl = lane >> 3;
  for (size_t it = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (size_t)gridDim.x * 4) {
    const unsigned band = (unsigned)(it % bands), g = (unsigned)((it / bands) % groups), b = (unsigned)(it / ((size_t)bands * groups));
    const unsigned s = 8 * g + sl, y = 8 * band + yl, x0 = mods::kStripCols * s;
    if (s >= ns) continue;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (y < (unsigned)h) {
      const unsigned char *p = src + ((size_t)b * h + y) * w + x0;
      if (x0 + 16 <= (unsigned)w) { const StripRowBytes r = *(const StripRowBytes *)p; v = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]); }
      else {
        unsigned q[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; j++)
          if (x0 + j < (unsigned)w) q[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
        v = make_uint4(q[0], q[1], q[2], q[3]);
      }
    }
    *(uint4 *)(strips + (size_t)b * ns * pitch + (size_t)s * pitch + mods::kStripRowBytes * y) = v;
  }
}
// 8-bit grey -> float (the ImageRepresentation constructor's convertTo(CV_32F), imagerepresentation.cpp:293-302): exact
// n4 groups of four pixels (src 4-byte, dst 16-byte aligned), then the pixels 4 n4 .. n - 1 one by one.  strips != nullptr: the
// n = n_img * w * h pixels are packed images, and the launch lays them out in strips as well while it has them in the caches
extern "C" __global__ __launch_bounds__(256) void u8_to_f32_kernel(const unsigned char *__restrict__ src, float *__restrict__ dst, size_t n4,
                                                                   size_t n, unsigned char *__restrict__ strips, int n_img, int w, int h) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const uchar4 v = ((const uchar4 *)src)[i];
    ((float4 *)dst)[i] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
  }
  for (size_t i = 4 * n4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = (float)src[i];
  if (strips) u8_strip_rows(src, strips, n_img, w, h);
}
// the same for rows of w pixels `stride` bytes apart, packed on the way
extern "C" __global__ __launch_bounds__(256) void u8_rows_to_f32_kernel(const unsigned char *__restrict__ src, size_t stride, size_t w, size_t rows,
                                                                        float *__restrict__ dst) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < rows * w; i += (size_t)gridDim.x * 256) dst[i] = (float)src[(i / w) * stride + i % w];
}
// the context's staging area for 8-bit host images, allocated at its first use
int mods::u8_stage_ensure(mods_ctx *c) {
  MODS_HIP_CHECK(c->u8_stage_dev.reserve((size_t)c->max_w * c->max_h * c->batch + 16));
  if (mods::u8_strips_wanted(c->u8_kernels, c->max_w, c->max_h, c->max_w))     // (a mask that is given later reserves at its first call)
    MODS_HIP_CHECK(c->u8_strip_dev.reserve(mods::strip_image_bytes(c->max_w, c->max_h) * c->batch));
  return MODS_OK;
}
// images [n_img][h][stride] of 8-bit grey in HBM -> fp32 [n_img][h][w]; any size, any alignment of src
int mods::u8_to_f32_launch(mods_ctx *c, const unsigned char *src, int n_img, int w, int h, int stride, float *dst, bool strips) {
  const size_t n = (size_t)n_img * w * h;
  if (strips) {
    if (stride != w || !mods::strip_layout_ok(w, h)) { set_error("u8_to_f32: no strip twin for %d x %d images, stride %d", w, h, stride); return MODS_E_ARG; }
    // (reserved with the staging area for the context's largest images: only a call ahead of that, or an image of the context's
    // area with more columns or rows than max_w x max_h, allocates here)
    bool moved = false;
    MODS_HIP_CHECK(c->u8_strip_dev.reserve(mods::strip_image_bytes(w, h) * n_img, std::max(mods::strip_image_bytes(w, h) * n_img, mods::strip_image_bytes(c->max_w, c->max_h) * c->batch), &moved));
    if (moved) mods::dev_pool_reallocated(c);
  }
  if (stride != w)
    hipLaunchKernelGGL(u8_rows_to_f32_kernel, dim3(1024), dim3(256), 0, c->stream, src, (size_t)stride, (size_t)w, (size_t)n_img * h, dst);
  else {
    const bool vec = (((uintptr_t)src & 3) | ((uintptr_t)dst & 15)) == 0;
    hipLaunchKernelGGL(u8_to_f32_kernel, dim3(1024), dim3(256), 0, c->stream, src, dst, vec ? n / 4 : (size_t)0, n,
                       strips ? c->u8_strip_dev.get() : (unsigned char *)nullptr, n_img, w, h);
  }
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}
int mods::u8_sources_launch(mods_ctx *c, const unsigned char *src, int n_img, int w, int h, int stride, bool twin, PixelSources *img) {
  twin = twin && stride == w;
  const bool strips = twin && mods::u8_strips_wanted(c->u8_kernels, w, h, stride);
  const int rc = mods::u8_to_f32_launch(c, src, n_img, w, h, stride, c->input_dev, strips);
  if (rc) return rc;
  *img = {c->input_dev, twin ? src : nullptr, strips ? c->u8_strip_dev.get() : nullptr};
  if (img->u8) c->u8_source_calls++;
  if (img->strips) c->u8_strip_calls++;
  return MODS_OK;
}

// ---- the GPU half ------------------------------------------------------------------------------------------

// GPU half of a pair: detect + describe both images, match, bring the tentatives to the host.
int mods::pair_gpu_stage(mods_ctx *c, const float *img_dev, int w, int h, int stride, const mods_pair_params *par, mods_pair_result *res,
                         TentList *list) {
  if (!c || !img_dev || !par || !res || !list) { set_error("match_pair: null argument"); return MODS_E_ARG; }
  if (c->batch < 2) { set_error("match_pair needs a context created with batch >= 2"); return MODS_E_ARG; }
  memset(res, 0, sizeof(*res));
  for (int i = 0; i < 9; i++) res->H[i] = -1;
  int rc;
  const double t0 = now_ms();
  if ((rc = mods_detect_describe_dev(c, img_dev, 2, w, h, stride, &par->det, &par->desc, res->n_detected, res->n_described))) return rc;
  const double t1 = now_ms();
  res->ms_detect_describe = t1 - t0;
  if ((rc = match_run(c, c->regions_dev, res->n_described[0], c->regions_dev + c->max_cand, res->n_described[1],
                      par->fginn_ratio, par->contradDist, par->nn))) return rc;
  const bool dedup = dedup_on_device(par);
  if (dedup) {
    if ((rc = ensure_tent2(c))) return rc;
    const DupJob job = single_pair_dup_job(c);
    if ((rc = dup_filter_dev(c, &job, 1, res->n_described[0], par->dup_dist, par->dup_mode))) return rc;
  }
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int n = read_slot(c->m_count, count_slot());
  res->n_tentatives = n;
  if (n > c->max_cand) { set_error("tentative list overflow"); return MODS_E_CAPACITY; }
  const bool filtered = dedup && read_slot(c->m_count, status_slot()) == 0;
  if (filtered) n = read_slot(c->m_count, kept_slot());
  list->resize(n);
  if (filtered) {          // the kept correspondences in their sorted order; the verify stage sees n_unique == list length and does not filter again
    res->n_unique = n;
    if (n > 0) {
      std::vector<char> stage(tent_bytes((size_t)n));
      MODS_HIP_CHECK(hipMemcpyAsync(stage.data(), c->m_tent2, stage.size(), hipMemcpyDeviceToHost, c->stream));
      MODS_HIP_CHECK(mods::stream_wait(c->stream));
      list->unpack_from(stage.data(), (size_t)n);
    }
  } else if ((rc = mods_match_copy_out(c, n, list->tent.data(), list->u6.data(), list->laf.data()))) return rc;
  if (c->la_on) {          // the local affine filter on the list that goes to the verification (behind DuplicateFiltering when that runs first)
    if ((rc = local_affine_prefilter(c, par, list, filtered))) return rc;
    if (par->dup_before_ransac) res->n_unique = (int)list->size();
  }
  res->ms_match = now_ms() - t1;
  return MODS_OK;
}

// GPU half of up to batch/2 pairs in one pass: the images of all pairs go through the pyramid / detector /
// describe kernels as ONE batch (launches n times larger, the many tiny launches of the small octaves amortised
// over n pairs), then every pair is matched on its own.  img[i]: [2][h][w] of pair i; kinds[i] (NULL = all 0):
// 0 fp32 in HBM, 1 fp32 in (pinned) host memory, 2 8-bit grey in (pinned) host memory - host images are uploaded on
// the context's stream, so the transfer of one worker overlaps the kernels of the others.
int mods::pairs_gpu_stage(mods_ctx *c, const void *const *img, const int *kinds, int n_pairs, int w, int h, const mods_pair_params *par,
                          mods_pair_result *const *res, TentList *const *lists, const unsigned char *const *masks) {
  if (!c || !img || !par || !res || !lists || n_pairs < 1) { set_error("match_pairs: null argument"); return MODS_E_ARG; }
  bool any_mask = false;
  for (int i = 0; masks && i < n_pairs; i++) any_mask = any_mask || masks[i] != nullptr;
  if (n_pairs == 1 && (!kinds || kinds[0] == 0) && !c->clahe_on && !any_mask && !c->det_mask_staged) return pair_gpu_stage(c, (const float *)img[0], w, h, w, par, res[0], lists[0]);
  if (c->batch < 2 * n_pairs) { set_error("match_pairs: context batch %d < %d images", c->batch, 2 * n_pairs); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("match_pairs: image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const size_t plane2 = (size_t)2 * w * h;
  const int n_img = 2 * n_pairs;
  // CLAHE pipeline (mods_pipeline_create_clahe): the 8-bit pairs are staged side by side and equalised in one LUT + one apply launch
  // over the batch's 2 n_pairs images, the apply launch writing fp32 into input_dev in the place of u8_to_f32_kernel
  const bool clahe = c->clahe_on;
  // a batch of 8-bit pairs only (and no CLAHE, whose fp32 output is no 8-bit image): the staged 8-bit batch [n_img][h][w] is converted
  // in one launch and stays the sampling source of orientation and description (mods_detect_describe_dev_u8)
  bool all_u8 = !clahe && kinds != nullptr;
  for (int i = 0; all_u8 && i < n_pairs; i++) all_u8 = kinds[i] == 2;
  for (int i = 0; i < n_pairs; i++) {
    memset(res[i], 0, sizeof(*res[i]));
    for (int q = 0; q < 9; q++) res[i]->H[q] = -1;
    const int kind = kinds ? kinds[i] : 0;
    if (clahe && kind != 2) { set_error("match_pairs: a CLAHE pipeline takes 8-bit images only"); return MODS_E_ARG; }
    if (kind == 2) {
      if (int rc_stage = mods::u8_stage_ensure(c)) return rc_stage;
      unsigned char *st = c->u8_stage_dev + plane2 * i;
      if (!clahe && !all_u8 && ((plane2 & 3) || ((uintptr_t)st & 3))) { set_error("match_pairs: 8-bit input needs w*h*2 divisible by 4"); return MODS_E_ARG; }
      // (reading page-locked host images from the conversion kernel itself - no staging copy - was measured: 610 against 636
      // pairs/s, the kernel's waves sit on PCIe reads; the copy engine path stays)
      MODS_HIP_CHECK(hipMemcpyAsync(st, img[i], plane2, hipMemcpyHostToDevice, c->stream));
      const unsigned char *src = st;
      if (!clahe && !all_u8) hipLaunchKernelGGL(u8_to_f32_kernel, dim3(1024), dim3(256), 0, c->stream, src, c->input_dev + plane2 * i, plane2 / 4, plane2, (unsigned char *)nullptr, 0, 0, 0);
    } else {
      MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev + plane2 * i, img[i], sizeof(float) * plane2,
                                    kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    }
  }
  MODS_HIP_CHECK(hipGetLastError());
  // detection masks of the batch's pairs ([2][h][w] bytes on the host, null: an unmasked pair): staged next to the images, on the same
  // stream, and set as the masks of the batch's images 2 i, 2 i + 1.  The set of masked slots is device state a recorded call
  // depends on: a batch whose set differs from the one before it is not taken for its repeat
  if (any_mask || c->det_mask_staged) {
    std::vector<DetMaskDev> want((size_t)c->batch, DetMaskDev{nullptr, 0, 0, 0, 0});
    if (any_mask) MODS_HIP_CHECK(mods::reserve_pool(c, c->det_mask_stage, (size_t)c->batch * c->max_w * c->max_h, (size_t)c->batch * c->max_w * c->max_h));
    for (int i = 0; i < n_pairs; i++) {
      if (!masks || !masks[i]) continue;
      unsigned char *st = c->det_mask_stage + plane2 * i;
      MODS_HIP_CHECK(hipMemcpyAsync(st, masks[i], plane2, hipMemcpyHostToDevice, c->stream));
      want[2 * i] = DetMaskDev{st, w, h, w, 0};
      want[2 * i + 1] = DetMaskDev{st + plane2 / 2, w, h, w, 0};
    }
    if (!(want == c->det_masks)) { c->det_masks = want; mods::dev_state_changed(c); }
    c->det_mask_staged = any_mask;
  }
  std::vector<int> nd(n_img), nr(n_img);
  int rc;
  // (queued ahead of the detect stage's scope: no MODS_STAGE_* bracket includes these two launches, rocprofv3 shows their time)
  if (clahe && (rc = clahe_launch(c, c->u8_stage_dev, n_img, w, h, w, &c->clahe_par, c->input_dev, w, 1))) return rc;
  const double t0 = now_ms();
  if (all_u8) rc = mods_detect_describe_dev_u8(c, c->u8_stage_dev, n_img, w, h, w, &par->det, &par->desc, nd.data(), nr.data());
  else rc = mods_detect_describe_dev(c, c->input_dev, n_img, w, h, w, &par->det, &par->desc, nd.data(), nr.data());
  if (rc) return rc;
  const double t1 = now_ms();
  // The tentative lists of the batch go to the host through a pinned arena: the packed list of a pair (tentatives |
  // correspondences | frames) is ONE transfer queued behind its match kernels, the stream is synchronised once per pair for the COUNT only (4 bytes) and once
  // per batch for the lists; a pair that does not fit the arena takes the direct (pageable, synchronous) path.
  MODS_HIP_CHECK(c->pin_arena.reserve(kPinArena));
  // every pair's search is queued without waiting: the packed list of pair i goes to its own segment of a device arena (a
  // list is at most as long as the query list), its length to slot i of the pinned counter array.  Then ONE synchronisation
  // for the lengths, the transfers of exactly those bytes, and one more for the lists (before: a synchronisation per pair).
  if (n_pairs > kCountSlots - 1) { set_error("match_pairs: at most %d pairs per batch", kCountSlots - 1); return MODS_E_ARG; }
  std::vector<size_t> seg(n_pairs + 1, 0);
  for (int i = 0; i < n_pairs; i++) seg[i + 1] = seg[i] + ((tent_bytes((size_t)std::max(nr[2 * i], 1)) + 255) & ~(size_t)255);
  if ((rc = match_ensure_buffers(c))) return rc;
  const bool dedup = dedup_on_device(par);
  // the local affine filter (mods_ctx_local_affine) takes the batch's lists on the device where they are final there: behind the device
  // duplicate filter, or behind the search when DuplicateFiltering follows RANSAC.  Its compaction then is the one that writes into the
  // pinned arena (la_direct), or into a third run of segments when the arena is too small
  const bool la_dev = c->la_on && (dedup || !par->dup_before_ransac);
  const bool fits_arena = seg[n_pairs] <= c->pin_arena.capacity();
  const bool direct = dedup && !la_dev && fits_arena, la_direct = la_dev && fits_arena;
  // (the second half of the arena takes the filtered lists of the device duplicate filter)
  const size_t seg_runs = la_dev && !la_direct ? 3 : 2;
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->m_tent_batch, seg_runs * seg[n_pairs], seg_runs * seg[n_pairs] + seg[n_pairs] / 2));
  const double tm0 = now_ms();
  // the searches of the batch's pairs in grouped launches (csrc/match.hip: match_run_group), up to 16 pairs per set of launches
  for (int i0 = 0; i0 < n_pairs; i0 += 16) {
    const int g = std::min(16, n_pairs - i0);
    const mods_region *qv[16], *tv[16];
    int nq[16], nt[16];
    mods_tentative *to[16];
    int *co[16];
    for (int e = 0; e < g; e++) {
      const int i = i0 + e;
      mods_pair_result *r = res[i];
      r->n_detected[0] = nd[2 * i]; r->n_detected[1] = nd[2 * i + 1];
      r->n_described[0] = nr[2 * i]; r->n_described[1] = nr[2 * i + 1];
      r->ms_detect_describe = (t1 - t0) / n_pairs;
      qv[e] = c->regions_dev + (size_t)(2 * i) * c->max_cand; nq[e] = nr[2 * i];
      tv[e] = c->regions_dev + (size_t)(2 * i + 1) * c->max_cand; nt[e] = nr[2 * i + 1];
      to[e] = (mods_tentative *)(c->m_tent_batch + seg[i]);
      co[e] = c->m_count + count_slot(i);
    }
    if ((rc = match_run_group(c, g, qv, nq, tv, nt, to, co, par->fginn_ratio, par->contradDist, par->nn))) return rc;
  }
  if (dedup) {     // the lists of the whole batch through the device duplicate filter in one set of launches
    // when the batch's lists fit the pinned arena (they do unless the images are very large) the filter's compaction writes the
    // kept lists straight into it - host memory the device can address - at the segments' offsets: no copy launch per pair and one
    // synchronisation per batch
    std::vector<DupJob> jobs(n_pairs);
    int grid_n = 1;
    for (int i = 0; i < n_pairs; i++) {
      char *dst = direct ? c->pin_arena + seg[i] : c->m_tent_batch + seg[n_pairs] + seg[i];
      jobs[i] = {c->m_tent_batch + seg[i], dst, c->m_count + count_slot(i), c->m_count + kept_slot(i), c->m_count + status_slot(i)};
      grid_n = std::max(grid_n, nr[2 * i]);
    }
    if ((rc = dup_filter_dev(c, jobs.data(), n_pairs, grid_n, par->dup_dist, par->dup_mode))) return rc;
  }
  if (la_dev) {    // the lists of the whole batch in one grouped set of launches (a list the duplicate filter left to the host arrives with length 0)
    LaConst lk;
    if ((rc = la_check(&c->la_par, &lk))) return rc;
    std::vector<LaJob> jobs(n_pairs);
    int grid_n = 1;
    if ((rc = la_reserve(c, n_pairs, 1))) return rc;     // (the pinned counters exist before the jobs point at them)
    for (int i = 0; i < n_pairs; i++) {
      const char *src = dedup ? c->m_tent_batch + seg[n_pairs] + seg[i] : c->m_tent_batch + seg[i];
      jobs[i] = {src, la_direct ? c->pin_arena + seg[i] : c->m_tent_batch + 2 * seg[n_pairs] + seg[i], c->m_count + (dedup ? kept_slot(i) : count_slot(i)), c->la_count + LA_MAX_JOBS + i};
      grid_n = std::max(grid_n, nr[2 * i]);
    }
    if ((rc = la_filter_dev(c, jobs.data(), n_pairs, grid_n, lk))) return rc;
  }
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  std::vector<char> la_pending(n_pairs, c->la_on ? 1 : 0);     // lists the local affine filter has yet to see, on the host
  std::vector<char> host_deduped(n_pairs, 0);
  std::vector<size_t> off(n_pairs, (size_t)-1);
  size_t used = direct || la_direct ? seg[n_pairs] : 0;       // (lists that were not filtered on the device go behind the segments)
  bool copies = false;
  for (int i = 0; i < n_pairs; i++) {
    int n = read_slot(c->m_count, count_slot(i));
    res[i]->n_tentatives = n;
    if (n > c->max_cand || n > nr[2 * i]) { set_error("tentative list overflow"); return MODS_E_CAPACITY; }
    // filtered on the device: the kept correspondences come over, the verify stage sees n_unique == list length and does not filter again
    const bool filtered = dedup && read_slot(c->m_count, status_slot(i)) == 0;
    bool in_arena = filtered && direct;
    const char *list = c->m_tent_batch + seg[i];
    if (filtered) { n = read_slot(c->m_count, kept_slot(i)); res[i]->n_unique = n; list = c->m_tent_batch + seg[n_pairs] + seg[i]; host_deduped[i] = 1; }
    if (la_dev && (filtered || !dedup)) {
      const int m = read_slot(c->la_count, LA_MAX_JOBS + i);
      if (m < 0 || m > n) { set_error("local_affine: the device returned %d of %d", m, n); return MODS_E_CAPACITY; }
      c->la_n_in = n; c->la_n_kept = m;
      n = m; list = c->m_tent_batch + 2 * seg[n_pairs] + seg[i];
      if (par->dup_before_ransac) res[i]->n_unique = n;
      la_pending[i] = 0;
      in_arena = la_direct;
    }
    lists[i]->resize(n);
    if (n > 0) {
      const size_t bytes = tent_bytes((size_t)n);
      if (in_arena) off[i] = seg[i];                    // already in the arena
      else if (used + bytes <= c->pin_arena.capacity()) {
        MODS_HIP_CHECK(hipMemcpyAsync(c->pin_arena + used, list, bytes, hipMemcpyDeviceToHost, c->stream));
        off[i] = used; used += (bytes + 15) & ~(size_t)15;
        copies = true;
      } else {      // a list that does not fit the arena: the direct (pageable, synchronous) path
        std::vector<char> stage(bytes);
        MODS_HIP_CHECK(mods::copy_wait(c->stream, stage.data(), list, bytes, hipMemcpyDeviceToHost));
        lists[i]->unpack_from(stage.data(), (size_t)n);
      }
    }
  }
  if (copies) MODS_HIP_CHECK(mods::stream_wait(c->stream));
  const double tm1 = now_ms();
  for (int i = 0; i < n_pairs; i++) {
    res[i]->ms_match = (tm1 - tm0) / n_pairs;
    if (off[i] != (size_t)-1) lists[i]->unpack_from(c->pin_arena + off[i], lists[i]->size());
  }
  for (int i = 0; i < n_pairs; i++)       // lists that were final only on the host (DuplicateFiltering ran or runs there): the host-list entry point
    if (la_pending[i]) {
      if ((rc = local_affine_prefilter(c, par, lists[i], host_deduped[i] != 0))) return rc;
      if (par->dup_before_ransac) res[i]->n_unique = (int)lists[i]->size();
    }
  return MODS_OK;
}

// ---- the host-driven half ----------------------------------------------------------------------------------

int mods::pair_verify_stage(int device, const mods_pair_params *par, mods_pair_result *res, TentList *list, double *matches_out,
                            int max_matches, int w, int h) {
  int stats[3] = {0, 0, 0};
  // a list the GPU stage has already filtered (DuplicateFiltering on the device, dedup.hip) arrives with n_unique = its length
  mods_pair_params p2;
  if (!list->empty() && res->n_unique == (int)list->size() && par->dup_before_ransac) { p2 = *par; p2.dup_dist = 0; par = &p2; }
  const int rc = mods_verify_tentatives_wh(device, par, list->tent.data(), list->u6.data(), list->laf.data(), (int)list->size(), w, h,
                                           &res->n_unique, &res->n_inliers, res->H, stats, nullptr, &res->ms_duplicates, &res->ms_ransac);
  if (rc) return rc;
  res->ransac_samples = stats[0]; res->ransac_lo = stats[1]; res->ransac_rejects = stats[2];
  list->copy_matches(res->n_inliers, matches_out, max_matches);
  return MODS_OK;
}

// ---- entry points ------------------------------------------------------------------------------------------

extern "C" {

int mods_duplicate_filter_gpu(mods_ctx *c, mods_tentative *tent, double *u6, double *laf, int n, double r, int mode, int *n_out, int *on_device) {
  if (!c || !n_out || (n > 0 && (!tent || !u6 || !laf))) { set_error("duplicate_filter_gpu: null argument"); return MODS_E_ARG; }
  *n_out = n;
  if (on_device) *on_device = 0;
  if (r <= 0 || n <= 0) return MODS_OK;
  if (n > c->max_cand || mode < 0 || mode > 3) return mods_duplicate_filter(tent, u6, laf, n, r, mode, n_out);
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int rc;
  if ((rc = match_ensure_buffers(c)) || (rc = ensure_tent2(c))) return rc;
  std::vector<char> stage(tent_bytes((size_t)n));
  tent_pack(stage.data(), (size_t)n, tent, u6, laf);
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  MODS_HIP_CHECK(mods::copy_wait(c->stream, c->m_tent, stage.data(), stage.size(), hipMemcpyHostToDevice));
  c->m_count[count_slot()] = n;
  const DupJob job = single_pair_dup_job(c);
  if ((rc = dup_filter_dev(c, &job, 1, n, r, mode))) return rc;
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  if (read_slot(c->m_count, status_slot()) != 0) return mods_duplicate_filter(tent, u6, laf, n, r, mode, n_out);
  const int m = read_slot(c->m_count, kept_slot());
  if (m > 0) {
    MODS_HIP_CHECK(mods::copy_wait(c->stream, stage.data(), c->m_tent2, tent_bytes((size_t)m), hipMemcpyDeviceToHost));
    tent_unpack(stage.data(), (size_t)m, tent, u6, laf);
  }
  *n_out = m;
  if (on_device) *on_device = 1;
  return MODS_OK;
}

// One batch of a synthetic blob lattice through detect / describe and one match: allocates every pool a batch of n_img
// images of w x h needs (they are sized by the geometry and the context's capacities) and loads every kernel of the path.
int mods_ctx_warmup(mods_ctx *c, int n_img, int w, int h, const mods_pair_params *par) {
  if (!c || !par || n_img < 1 || n_img > c->batch) { set_error("warmup: bad argument"); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("warmup: image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if (int rc_stage = mods::u8_stage_ensure(c)) return rc_stage;
  MODS_HIP_CHECK(c->pin_arena.reserve(kPinArena));
  std::vector<float> img((size_t)w * h);
  // blobs every 14 px on top of blobs every 90 px: some ten thousand regions of both patch tiers on a 2-megapixel image; on larger
  // images the lattice is stretched so that the count stays there (a 4096 x 4096 image at the 14-px period overflows the lists)
  const float f = sqrtf(std::min(1.0f, 1920.f * 1080.f / ((float)w * (float)h)));
  const float f1 = 0.22f * f, f2 = 0.035f * f;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++)
      img[(size_t)y * w + x] = 128.f + 70.f * sinf(f1 * x) * sinf(f1 * y) + 50.f * sinf(f2 * x + 1.f) * sinf(f2 * y);
  const size_t plane = (size_t)w * h;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, c->input_dev, img.data(), sizeof(float) * plane, hipMemcpyHostToDevice));
  for (int i = 1; i < n_img; i++)
    MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev + plane * i, c->input_dev, sizeof(float) * plane, hipMemcpyDeviceToDevice, c->stream));
  std::vector<int> nd(n_img), nr(n_img);
  int rc = mods_detect_describe_dev(c, c->input_dev, n_img, w, h, w, &par->det, &par->desc, nd.data(), nr.data());
  if (rc) return rc;
  // the same batch as 8-bit grey through the 8-bit entry point: a pipeline's 8-bit batches sample from the staged images, and the
  // first use of those kernels must not load their code objects inside the running pipeline.  (Its regions differ from the fp32
  // lattice's - the lattice is rounded - which does not matter to what follows.)  A CLAHE context never takes that path.
  if (!c->clahe_on) {
    std::vector<unsigned char> img8(plane);
    for (size_t i = 0; i < plane; i++) img8[i] = (unsigned char)std::min(255.f, std::max(0.f, img[i] + 0.5f));
    MODS_HIP_CHECK(mods::copy_wait(c->stream, c->u8_stage_dev, img8.data(), plane, hipMemcpyHostToDevice));
    for (int i = 1; i < n_img; i++)
      MODS_HIP_CHECK(hipMemcpyAsync(c->u8_stage_dev + plane * i, c->u8_stage_dev, plane, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = mods_detect_describe_dev_u8(c, c->u8_stage_dev, n_img, w, h, w, &par->det, &par->desc, nd.data(), nr.data()))) return rc;
  }
  const int last = n_img - 1;
  if ((rc = match_ensure_buffers(c, std::min(16, std::max(1, n_img / 2))))) return rc;     // the searches of a batch's pairs run as one group
  if ((rc = match_run(c, c->regions_dev, nr[0], c->regions_dev + (size_t)last * c->max_cand, nr[last], par->fginn_ratio, par->contradDist, par->nn))) return rc;
  if (dedup_on_device(par)) {
    // the duplicate filter's scratch for the lists of a whole batch and its kernels (a first hipMalloc inside the running pipeline
    // would synchronise the device): the filter runs once over the warm-up search's list, repeated as every job of a batch
    if ((rc = ensure_tent2(c))) return rc;
    const int n_jobs = std::min(DUP_MAX_JOBS, std::max(1, n_img / 2));
    std::vector<DupJob> jobs(n_jobs, single_pair_dup_job(c));
    if ((rc = dup_filter_dev(c, jobs.data(), 1, nr[0], par->dup_dist, par->dup_mode))) return rc;     // kernels + the single-pair path
    if (n_jobs > 1) {   // the allocation for a batch's jobs (every job of this call would write the same output: run none of them twice)
      MODS_HIP_CHECK(mods::stream_wait(c->stream));
      if ((rc = dup_filter_reserve(c, n_jobs))) return rc;
    }
  }
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

// HMatrixFiltering, matching.cpp:917-1012: the reference stacks (second image point, first image point) and hands the
// column-major H to the error function; th = (float)(err_threshold^2) compared in double
int mods_hmatrix_filter(const double *u6, int n, const double *H_rowmajor, const mods_ransac_params *par, unsigned char *mask, int *n_true) {
  if (!par || !H_rowmajor || !n_true || (n > 0 && (!u6 || !mask))) { set_error("hmatrix_filter: null argument"); return MODS_E_ARG; }
  *n_true = 0;
  if (n <= 0) return MODS_OK;
  std::vector<double> u2((size_t)n * 6), d(n);
  for (int i = 0; i < n; i++) {
    const double *s = u6 + (size_t)i * 6;
    double *q = &u2[(size_t)i * 6];
    q[0] = s[3]; q[1] = s[4]; q[2] = 1.; q[3] = s[0]; q[4] = s[1]; q[5] = 1.;
  }
  const double *M = H_rowmajor;
  const double Hc[9] = {M[0], M[3], M[6], M[1], M[4], M[7], M[2], M[5], M[8]};   // Hready[0], [3], [6] <- first row of the file
  if (par->errorType == 0) HDs(nullptr, u2.data(), Hc, d.data(), n);
  else if (par->errorType == 1) HDsSymMax(nullptr, u2.data(), Hc, d.data(), n);
  else HDsSym(nullptr, u2.data(), Hc, d.data(), n);
  const float th = (float)(par->err_threshold * par->err_threshold);
  int c = 0;
  for (int i = 0; i < n; i++) { mask[i] = d[i] <= th ? 1 : 0; c += mask[i]; }
  *n_true = c;
  return MODS_OK;
}

// Host-driven half: duplicate filtering + LO-RANSAC (hypotheses scored on `device`) + checks.
// The verification half of one step of the reference's loop (mods.cpp:278-368), in place on (tent, u6, laf):
//   [DuplicateFiltering] doBeforeRANSAC = 1: DuplicateFiltering on the tentatives, then LORANSACFiltering;
//   doBeforeRANSAC = 0: LORANSACFiltering on every tentative, then DuplicateFiltering on the VERIFIED list (mods.cpp:357-368;
//   TrueMatch1st, which also drives the minMatches stop, is the size of the de-duplicated list).
// On return the first *n_verified entries of the three arrays are the verified correspondences in output order;
// *n_unique = the size of the list RANSAC ran on.
int mods_verify_tentatives_wh(int device, const mods_pair_params *par, mods_tentative *tent, double *u6, double *laf, int n, int w,
                              int h, int *n_unique, int *n_verified, double *H_out, int *stats3, int *gt3, double *ms_dup,
                              double *ms_ransac) {
  if (gt3) gt3[0] = gt3[1] = gt3[2] = 0;
  if (!par || !n_unique || !n_verified || (n > 0 && (!tent || !u6 || !laf))) { set_error("verify_tentatives: null argument"); return MODS_E_ARG; }
  if ((par->ransac.useF == 2 || par->ransac.useF == 3) && !par->ransac.groundTruth && (w <= 0 || h <= 0)) {
    set_error("verify_tentatives: useF = %d (ORSA) needs the image size: call mods_verify_tentatives_wh", par->ransac.useF);
    return MODS_E_ARG;
  }
  int rc;
  const double t0 = now_ms();
  int nu = n;
  if (par->dup_before_ransac && n > 0)
    if ((rc = mods_duplicate_filter(tent, u6, laf, n, par->dup_dist, par->dup_mode, &nu))) return rc;
  *n_unique = nu;
  const double t1 = now_ms();
  int stats[3] = {0, 0, 0}, ninl = 0;
  mods_ransac_set_device(device);
  std::vector<unsigned char> mask(nu > 0 ? nu : 1);
  double H[9];
  if (par->ransac.groundTruth) {
    // GR_TRUTH, mods.cpp:292-320: HMatrixFiltering of all unique tentatives (TrueMatch1st); with doBothRANSACgroundTruth the
    // verified list is instead the LORANSAC inliers that the ground truth confirms
    int n_true = 0;
    if ((rc = mods_hmatrix_filter(u6, nu, par->ransac.gtH, &par->ransac, mask.data(), &n_true))) return rc;
    if (gt3) gt3[0] = n_true;
    ninl = n_true;
    if (par->ransac.groundTruth >= 2) {
      std::vector<unsigned char> mr(nu > 0 ? nu : 1);
      double Hr[9];
      if ((rc = mods_loransac_h(u6, laf, nu, &par->ransac, mr.data(), Hr, &ninl, stats))) return rc;
      std::vector<double> ur((size_t)(ninl > 0 ? ninl : 1) * 6);
      std::vector<unsigned char> mt(ninl > 0 ? ninl : 1);
      int q = 0;
      for (int i = 0; i < nu; i++)
        if (mr[i]) { memcpy(&ur[(size_t)q * 6], &u6[(size_t)i * 6], 6 * sizeof(double)); q++; }
      int n_tr = 0;
      if ((rc = mods_hmatrix_filter(ur.data(), ninl, par->ransac.gtH, &par->ransac, mt.data(), &n_tr))) return rc;
      if (gt3) { gt3[1] = ninl; gt3[2] = n_tr; }
      q = 0;
      for (int i = 0; i < nu; i++) { mask[i] = mr[i] ? mt[q++] : 0; }
      ninl = n_tr;
    }
    memcpy(H, par->ransac.gtH, sizeof(H));     // true_corresp.H = the ground truth, row-major again (matching.cpp:1002-1010)
  } else {
    if (par->ransac.useF == 2)
      rc = mods_orsa_f(u6, laf, nu, w, h, &par->ransac, mask.data(), H, &ninl, nullptr, nullptr, nullptr, stats);
    else if (par->ransac.useF == 3)
      rc = mods_orsa_h(u6, laf, nu, w, h, &par->ransac, mask.data(), H, &ninl, nullptr, nullptr, nullptr, nullptr, stats);
    else if (mods_model_kind(par->ransac.useF) != 0) rc = mods_loransac_f(u6, laf, nu, &par->ransac, mask.data(), H, &ninl, stats);
    else rc = mods_loransac_h(u6, laf, nu, &par->ransac, mask.data(), H, &ninl, stats);
    if (rc) return rc;
  }
  const double t2 = now_ms();
  int m = 0;
  for (int i = 0; i < nu; i++)
    if (mask[i]) {
      if (m != i) {
        tent[m] = tent[i];
        memcpy(&u6[(size_t)m * 6], &u6[(size_t)i * 6], 6 * sizeof(double));
        memcpy(&laf[(size_t)m * 14], &laf[(size_t)i * 14], 14 * sizeof(double));
      }
      m++;
    }
  if (!par->dup_before_ransac && m > 0)
    if ((rc = mods_duplicate_filter(tent, u6, laf, m, par->dup_dist, par->dup_mode, &m))) return rc;
  *n_verified = m;
  if (H_out) memcpy(H_out, H, sizeof(H));
  if (stats3) memcpy(stats3, stats, sizeof(stats));
  const double t3 = now_ms();
  if (ms_dup) *ms_dup = (t1 - t0) + (t3 - t2);
  if (ms_ransac) *ms_ransac = t2 - t1;
  return MODS_OK;
}

// ABI aliases of mods_verify_tentatives_wh: _ex without the image size (no ORSA), the plain name also without the ground-truth counters
int mods_verify_tentatives(int device, const mods_pair_params *par, mods_tentative *tent, double *u6, double *laf, int n,
                           int *n_unique, int *n_verified, double *H_out, int *stats3, double *ms_dup, double *ms_ransac) {
  return mods_verify_tentatives_ex(device, par, tent, u6, laf, n, n_unique, n_verified, H_out, stats3, nullptr, ms_dup, ms_ransac);
}

int mods_verify_tentatives_ex(int device, const mods_pair_params *par, mods_tentative *tent, double *u6, double *laf, int n,
                              int *n_unique, int *n_verified, double *H_out, int *stats3, int *gt3, double *ms_dup, double *ms_ransac) {
  return mods_verify_tentatives_wh(device, par, tent, u6, laf, n, 0, 0, n_unique, n_verified, H_out, stats3, gt3, ms_dup, ms_ransac);
}

int mods_match_pair_dev(mods_ctx *c, const float *img_dev, int w, int h, int stride, const mods_pair_params *par,
                        mods_pair_result *res, double *matches_out, int max_matches) {
  if (!c) { set_error("match_pair: null context"); return MODS_E_ARG; }
  c->h_verified = 0;
  int rc = pair_gpu_stage(c, img_dev, w, h, stride, par, res, &c->h_list);
  if (rc) return rc;
  rc = pair_verify_stage(c->device, par, res, &c->h_list, matches_out, max_matches, w, h);
  if (!rc) c->h_verified = res->n_inliers;
  return rc;
}

}  // extern "C"
