// Homography views: a view of a grey float image through an arbitrary 3 x 3 homography, the regions detected on it carried back
// into the original frame, and the rematch step that uses both under a verified H.
//
// Reference: GenerateSynthImageByH, ReprojectByHReal, ReprojectRegionsBackReal (synth-detection.cpp:519-629) and linH (:1498-1518),
// which the reference began and never wired in.  Its pixel work is one cv::GaussianBlur and one cv::warpPerspective(INTER_LINEAR,
// BORDER_CONSTANT 128).  The warp's contract is this project's own (mods_hip.h: "homography views"), shaped after OpenCV's - the
// inverse map rounded to 1/32 px, the 32 x 32 table of bilinear weights - with parity unpinned, and with ONE deliberate difference:
// a destination pixel on or behind the horizon of the inverse map reads cval, where OpenCV mirrors the far side into the image.
//
// The affine views (synth_view.hip, describe.hip) keep their affine Hinv[6] and their gate: a homography view is detected, oriented
// and described as a plain image in its own frame, and one pass over the finished region list carries it back.
#include "common.hpp"
#include "describe_common.hpp"
#include "detection_mask.hpp"
#include "device_util.hpp"
#include <climits>
#include <cmath>

namespace mods {

struct WarpH { double g[9]; double d0; };   // inverse map dst -> src (adjugate form), and the denominator of H at the source's centre

// grid = (ceil(dw/64), ceil(dh/4)), block = (64, 4): the tile shape of warp_affine_kernel (a wave stores one row segment; the four
// taps are gathered through L2).  Every coordinate comes from (x, y) directly, in fp64, one rounding per operation: nothing is
// stepped along a row, so the result does not depend on the tile geometry.
__global__ void __launch_bounds__(256) warp_perspective_kernel(const float *__restrict__ src, int sw, int sh, int sstride, WarpH M,
                                                               float *__restrict__ dst, int dw, int dh, int dstride, float cval) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= dw || y >= dh) return;
  const int INTER_BITS = 5, TAB = 1 << INTER_BITS;
  const double dx = (double)x, dy = (double)y;
  const double W = (M.g[6] * dx + M.g[7] * dy) + M.g[8];
  float out = cval;
  if (W * M.d0 > 0) {                                    // (false for NaN too) else: on or behind the horizon
    const double t = 32.0 / W;
    double fX = ((M.g[0] * dx + M.g[1] * dy) + M.g[2]) * t;
    double fY = ((M.g[3] * dx + M.g[4] * dy) + M.g[5]) * t;
    if (fX == fX && fY == fY) {
      fX = fX < (double)INT_MIN ? (double)INT_MIN : (fX > (double)INT_MAX ? (double)INT_MAX : fX);
      fY = fY < (double)INT_MIN ? (double)INT_MIN : (fY > (double)INT_MAX ? (double)INT_MAX : fY);
      const int X = (int)rint(fX), Y = (int)rint(fY);
      const int sx = X >> INTER_BITS, sy = Y >> INTER_BITS;
      const float fx = (float)(X & (TAB - 1)) * (1.f / TAB), fy = (float)(Y & (TAB - 1)) * (1.f / TAB);
      const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
      if ((unsigned)sx < (unsigned)max(sw - 1, 0) && (unsigned)sy < (unsigned)max(sh - 1, 0)) {
        const float *S = src + (size_t)sy * sstride + sx;
        out = S[0] * w0 + S[1] * w1 + S[sstride] * w2 + S[sstride + 1] * w3;
      } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
        out = cval;
      } else {
        const bool x0 = sx >= 0 && sx < sw, x1 = sx + 1 >= 0 && sx + 1 < sw;
        const bool y0 = sy >= 0 && sy < sh, y1 = sy + 1 >= 0 && sy + 1 < sh;
        const float v0 = x0 && y0 ? src[(size_t)sy * sstride + sx] : cval;
        const float v1 = x1 && y0 ? src[(size_t)sy * sstride + sx + 1] : cval;
        const float v2 = x0 && y1 ? src[(size_t)(sy + 1) * sstride + sx] : cval;
        const float v3 = x1 && y1 ? src[(size_t)(sy + 1) * sstride + sx + 1] : cval;
        out = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3;
      }
    }
  }
  dst[(size_t)y * dstride + x] = out;
}

struct ViewHConst {
  double G[9];       // view -> original: adj(H) / det(H)
  double d0;         // denominator of H at the original's centre: the side of the horizon the image lies on
  double ks;         // k_sigma = 2*3*sqrt(3): the measurement box of the border test (describe.hip)
  int ow, oh;        // the original image
  int max_reg, pad;
  DetMaskDev mask;   // the slot's detection mask (original frame); mask == nullptr: none
};

// linH (synth-detection.cpp:1498-1516) at (x, y) under G, operation by operation
__host__ __device__ inline void lin_h(const double *G, double x, double y, double *L) {
  const double den = (G[6] * x + G[7] * y) + G[8];
  const double den_sq = den * den;
  const double num1_densq = ((G[0] * x + G[1] * y) + G[2]) / den_sq;
  const double num2_densq = ((G[3] * x + G[4] * y) + G[5]) / den_sq;
  L[0] = G[0] / den - num1_densq * G[6];
  L[1] = G[1] / den - num1_densq * G[7];
  L[2] = G[3] / den - num2_densq * G[6];
  L[3] = G[4] / den - num2_densq * G[7];
}

// det_kp -> reproj_kp of the finished regions of a homography view, and ReprojectRegionsBackReal's tests in the original frame
// (synth-detection.cpp:588-629): centre through G, frame through the linearisation of G at the centre; s, response and the
// descriptor stay.  A region is dropped when it lies on or behind the horizon (den * d0 <= 0), when its centre is not strictly
// inside the original, when its measurement box touches the border, or - with a detection mask on the slot - when its centre is
// off the mask.  The survivors are compacted in place in list order (id = the new position), the HalfRootSIFT twin list by the
// same keep flags.  One workgroup walks the list in chunks of 256: a chunk is in registers before anything of it is overwritten,
// and the slots it writes lie below the next chunk, so no atomics and no second buffer.  grid = 1, block = 256.
__global__ __launch_bounds__(256) void reproject_regions_h_kernel(ViewHConst k, mods_region *reg, mods_region *half, int *reg_count) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int n = *reg_count;
  if (n > k.max_reg) n = k.max_reg;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    bool keep = false;
    mods_region r, rh;
    if (i < n) {
      r = reg[i];
      if (half) rh = half[i];
      const double x = r.x, y = r.y;
      const double den = (k.G[6] * x + k.G[7] * y) + k.G[8];
      if (den * k.d0 > 0) {
        const double rx = ((k.G[0] * x + k.G[1] * y) + k.G[2]) / den;
        const double ry = ((k.G[3] * x + k.G[4] * y) + k.G[5]) / den;
        double L[4];
        lin_h(k.G, x, y, L);
        const double a11 = (L[0] * r.a11 + L[1] * r.a21), a12 = (L[0] * r.a12 + L[1] * r.a22);
        const double a21 = (L[2] * r.a11 + L[3] * r.a21), a22 = (L[2] * r.a12 + L[3] * r.a22);
        const int box = (int)(k.ks * r.s);
        keep = (rx > 0) && (rx < k.ow) && (ry > 0) && (ry < k.oh) &&
               !check_borders(k.ow, k.oh, (float)rx, (float)ry, (float)a11, (float)a12, (float)a21, (float)a22, box, box);
        if (keep && k.mask.mask) keep = detection_mask_on(k.mask.mask, k.mask.w, k.mask.h, k.mask.stride, rx, ry);
        r.x = rx; r.y = ry; r.a11 = a11; r.a12 = a12; r.a21 = a21; r.a22 = a22;
      }
    }
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(kept);
    __syncthreads();                       // every read of the chunk is done
    int slot = s_base + __popcll(kept & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; q++) slot += s_wave[q];
    if (keep) {
      r.id = slot;
      reg[slot] = r;
      if (half) {
        rh.x = r.x; rh.y = r.y; rh.a11 = r.a11; rh.a12 = r.a12; rh.a21 = r.a21; rh.a22 = r.a22; rh.id = slot;
        half[slot] = rh;
      }
    }
    __syncthreads();
    if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (tid == 0) *reg_count = s_base;
}

// G = adj(H) / det(H) and d0 for a w x h source; MODS_E_ARG for an H that has no view
static int view_h_inverse(const char *who, const double *H, int w, int h, double *G, double *d0) {
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(H[i])) { set_error("%s: H[%d] is not finite", who, i); return MODS_E_ARG; }
  double det;
  if (!invert3_adjugate(H, G, &det)) { set_error("%s: singular homography (determinant %g)", who, det); return MODS_E_ARG; }
  const double cx = (double)(w - 1) / 2.0, cy = (double)(h - 1) / 2.0;
  *d0 = (H[6] * cx + H[7] * cy) + H[8];
  if (*d0 == 0 || !std::isfinite(*d0)) { set_error("%s: the horizon of H passes through the image centre", who); return MODS_E_ARG; }
  return MODS_OK;
}

static int launch_warp_perspective(mods_ctx *c, const float *src, int sw, int sh, int sstride, const double *H, float *dst, int dw, int dh,
                                   int dstride, float cval) {
  WarpH M;
  const int rc = view_h_inverse("warp_perspective", H, sw, sh, M.g, &M.d0);
  if (rc) return rc;
  if (dw <= 0 || dh <= 0) return MODS_OK;
  hipLaunchKernelGGL(warp_perspective_kernel, dim3((dw + 63) / 64, (dh + 3) / 4), dim3(64, 4), 0, c->stream, src, sw, sh, sstride, M, dst, dw,
                     dh, dstride, cval);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

int launch_blur_xy_reflect(mods_ctx *c, const float *src, float *tmp, float *dst, int w, int h, int kx, int ky, double sx, double sy);   // synth_view.hip

// the post-pass over slot `slot` of the context's region lists (and its HalfRootSIFT twins when with_half); ow x oh: the original
// mask_slot: the image of the call whose detection mask applies (the pair entry points' numbering: 0 / 1 = image 1 / 2)
static int launch_reproject_regions_h(mods_ctx *c, int slot, int mask_slot, const double *H, int ow, int oh, bool with_half) {
  ViewHConst k;
  const int rc = view_h_inverse("reproject_regions_h", H, ow, oh, k.G, &k.d0);
  if (rc) return rc;
  k.ks = 2 * 3.0 * sqrt(3.0);
  k.ow = ow; k.oh = oh; k.max_reg = c->max_cand; k.pad = 0;
  k.mask = DetMaskDev{nullptr, 0, 0, 0, 0};
  if (mask_slot >= 0 && mask_slot < (int)c->det_masks.size() && c->det_masks[mask_slot].mask) {
    k.mask = c->det_masks[mask_slot];
    if (k.mask.w != ow || k.mask.h != oh) {
      set_error("detection mask of image %d is %d x %d, the image of the call %d x %d", mask_slot, k.mask.w, k.mask.h, ow, oh);
      return MODS_E_ARG;
    }
  }
  StageScope ts(c, MODS_STAGE_REPROJECT_H);
  hipLaunchKernelGGL(reproject_regions_h_kernel, dim3(1), dim3(256), 0, c->stream, k, c->regions_dev + (size_t)slot * c->max_cand,
                     with_half ? c->regions_half_dev + (size_t)slot * c->max_cand : (mods_region *)nullptr, c->region_count + slot);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

// What GenerateSynthImageByH derives before it touches pixels (synth-detection.cpp:523-572).  Host arithmetic only.
int mods_view_geometry_h(int w, int h, const double *H, int clip_w, int clip_h, double initSigma, mods_view_geom *g) {
  if (!g || !H || w <= 0 || h <= 0 || clip_w <= 0 || clip_h <= 0) { set_error("view_geometry_h: bad arguments"); return MODS_E_ARG; }
  double G[9], d0;
  const int rc = view_h_inverse("view_geometry_h", H, w, h, G, &d0);
  if (rc) return rc;
  memset(g, 0, sizeof(*g));
  for (int i = 0; i < 9; i++) g->H[i] = H[i];
  g->identity = 0; g->rotation = 0.0; g->tilt = 1.0; g->zoom = 1.0;
  g->w_rot = w; g->h_rot = h;             // the blurred intermediate has the source's size
  // the four corners (0, 0), (0, h), (w, 0), (w, h); a cv::Point holds ints, so each coordinate is truncated before the maximum
  const double bx[4] = {0, 0, (double)w, (double)w}, by[4] = {0, (double)h, 0, (double)h};
  double xmax = 0, ymax = 0;
  for (int i = 0; i < 4; i++) {
    const double den = H[6] * bx[i] + H[7] * by[i] + H[8];
    if (!(den * d0 > 0)) { set_error("view_geometry_h: corner (%g, %g) lies on or behind the horizon of H", bx[i], by[i]); return MODS_E_ARG; }
    double px = (H[0] * bx[i] + H[1] * by[i] + H[2]) / den, py = (H[3] * bx[i] + H[4] * by[i] + H[5]) / den;
    if (!std::isfinite(px) || !std::isfinite(py)) { set_error("view_geometry_h: corner (%g, %g) has no finite image", bx[i], by[i]); return MODS_E_ARG; }
    px = std::trunc(std::fmin(std::fmax(px, -1e9), 1e9)); py = std::trunc(std::fmin(std::fmax(py, -1e9), 1e9));
    if (i == 0 || px > xmax) xmax = px;
    if (i == 0 || py > ymax) ymax = py;
  }
  int dx = (int)floor(xmax), dy = (int)floor(ymax);
  if (dx > clip_w) dx = clip_w;
  if (dy > clip_h) dy = clip_h;
  if (dx < 0) dx = 0;
  if (dy < 0) dy = 0;
  g->w_new = dx; g->h_new = dy;
  const double sigma = initSigma / (4.0);
  int ks = (int)floor(2.0 * 4.0 * sigma + 1.0);
  if (ks % 2 == 0) ks++;
  if (ks < 3) ks = 3;
  g->sigma_x = g->sigma_y = sigma;
  g->ksize_x = g->ksize_y = ks;
  return MODS_OK;
}

// host-buffer primitive (the test seam of the warp): src w x h with a row stride of `stride` floats
int mods_test_warp_perspective_strided(mods_ctx *c, const float *src, int w, int h, int stride, const double *H, int dw, int dh, float cval,
                                       float *dst) {
  if (!c || !src || !H || !dst || w <= 0 || h <= 0 || stride < w || dw < 0 || dh < 0) { set_error("warp_perspective: bad arguments"); return MODS_E_ARG; }
  const size_t cap = (size_t)c->max_w * c->max_h * c->batch;
  if ((size_t)stride * h > cap || (size_t)dw * dh > cap) { set_error("image larger than the context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(hipMemcpyAsync(c->input_dev, src, sizeof(float) * (size_t)stride * h, hipMemcpyHostToDevice, c->stream));
  const int rc = launch_warp_perspective(c, c->input_dev, w, h, stride, H, c->tmp_dev, dw, dh, dw, cval);
  if (rc) return rc;
  if (dw > 0 && dh > 0) MODS_HIP_CHECK(hipMemcpyAsync(dst, c->tmp_dev, sizeof(float) * (size_t)dw * dh, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

int mods_warp_perspective(mods_ctx *c, const float *src, int w, int h, const double *H, int dw, int dh, float cval, float *dst) {
  return mods_test_warp_perspective_strided(c, src, w, h, w, H, dw, dh, cval, dst);
}

// Pixels of a homography view: the isotropic blur (when asked for), then the warp with cval = 128.  dst_dev: g->w_new x g->h_new,
// dense.  The blur runs on a dense copy in the context's scratch images, so w * h <= max_w * max_h * batch.
int mods_synth_view_h_dev(mods_ctx *c, const float *src_dev, int w, int h, int stride, const mods_view_geom *g, int doBlur, float *dst_dev) {
  if (!c || !src_dev || !g || !dst_dev || w <= 0 || h <= 0 || stride < w) { set_error("synth_view_h: bad argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  StageScope ts(c, MODS_STAGE_SYNTH, 4.0 * ((doBlur ? 5.0 : 1.0) * w * h + (double)g->w_new * g->h_new));
  if (!doBlur) return launch_warp_perspective(c, src_dev, w, h, stride, g->H, dst_dev, g->w_new, g->h_new, g->w_new, 128.f);
  const size_t cap = (size_t)c->max_w * c->max_h * c->batch;
  if ((size_t)w * h > cap) { set_error("image %dx%d larger than the context", w, h); return MODS_E_ARG; }
  float *dense = c->tmp_dev, *scratch = c->input_dev;
  MODS_HIP_CHECK(hipMemcpy2DAsync(dense, sizeof(float) * w, src_dev, sizeof(float) * stride, sizeof(float) * w, h, hipMemcpyDeviceToDevice, c->stream));
  int rc;
  if ((rc = launch_blur_xy_reflect(c, dense, scratch, dense, w, h, g->ksize_x, g->ksize_y, g->sigma_x, g->sigma_y))) return rc;
  return launch_warp_perspective(c, dense, w, h, w, g->H, dst_dev, g->w_new, g->h_new, g->w_new, 128.f);
}

// One homography view: synthesise -> detect -> orient and describe in the view frame (the plain-image path) -> the post-pass.
// The regions of slot 0 are left in the ORIGINAL frame.  Detection masks live in the original frame, which no affine gate reaches
// from here: the detector runs unmasked and the post-pass applies the mask, so off-mask regions still used detector budget.
static int view_h_detect_describe(mods_ctx *c, int mask_slot, const float *src_dev, int w, int h, int stride, const double *H, int clip_w, int clip_h,
                                  double initSigma, int doBlur, const mods_hessaff_params *det, const mods_describe_params *desc,
                                  mods_view_geom *geom_out, int *n_detected, int *n_regions) {
  if (!c || !src_dev || !H || !det || !desc) { set_error("detect_describe_view_h: null argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  mods_view_geom g;
  int rc = mods_view_geometry_h(w, h, H, clip_w, clip_h, initSigma, &g);
  if (rc) return rc;
  if (geom_out) *geom_out = g;
  if ((size_t)g.w_new * g.h_new > (size_t)c->max_w * c->max_h) { set_error("view %dx%d larger than the context", g.w_new, g.h_new); return MODS_E_ARG; }
  if (g.w_new < 16 || g.h_new < 16) {   // nothing to detect on a sliver
    if (n_detected) *n_detected = 0;
    if (n_regions) *n_regions = 0;
    MODS_HIP_CHECK(hipMemsetAsync(c->region_count, 0, sizeof(int), c->stream));
    c->last_region_counts.assign(1, 0);
    c->last_inside_counts.assign(1, 0);
    return MODS_OK;
  }
  MODS_HIP_CHECK(c->view_dev.reserve((size_t)c->max_w * c->max_h * c->batch));
  if ((rc = mods_synth_view_h_dev(c, src_dev, w, h, stride, &g, doBlur, c->view_dev))) return rc;
  {
    // the view is a plain image to the detector; the masks (original frame) wait for the post-pass
    std::vector<DetMaskDev> masks;
    masks.swap(c->det_masks);
    rc = detect_any(c, c->view_dev, 1, g.w_new, g.h_new, g.w_new, det, 1.0, 1.0, nullptr);
    masks.swap(c->det_masks);
    if (rc) return rc;
  }
  if ((rc = describe_run(c, {c->view_dev}, 1, g.w_new, g.h_new, desc))) return rc;
  if ((rc = launch_reproject_regions_h(c, 0, mask_slot, g.H, w, h, c->have_half))) return rc;
  int *hc = c->host_counts;
  MODS_HIP_CHECK(hipMemcpyAsync(hc, c->cand_count, sizeof(int) * 3 * c->batch, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(hc + 3 * c->batch, c->region_count, sizeof(int) * c->batch, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(hc + 4 * c->batch, c->inside_count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(hc + 5 * c->batch, c->desc_err_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  c->last_region_counts.assign(1, 0);
  c->last_inside_counts.assign(1, 0);
  if (hc[0] > c->max_cand) { set_error("NMS hit list overflow: %d > %d", hc[0], c->max_cand); return MODS_E_CAPACITY; }
  if (hc[5 * c->batch]) {
    MODS_HIP_CHECK(hipMemsetAsync(c->desc_err_dev, 0, sizeof(int), c->stream));
    set_error("measurement region larger than the descriptor scratch");
    return MODS_E_CAPACITY;
  }
  const int nr = hc[3 * c->batch];
  if (nr > (c->max_cand < (1 << 17) ? c->max_cand : (1 << 17))) { set_error("region list overflow: %d", nr); return MODS_E_CAPACITY; }
  if (n_detected) *n_detected = hc[2 * c->batch];
  if (n_regions) *n_regions = nr;
  c->last_region_counts[0] = nr;
  c->last_inside_counts[0] = hc[4 * c->batch];
  return MODS_OK;
}

int mods_detect_describe_view_h_dev(mods_ctx *c, const float *src_dev, int w, int h, int stride, const double *H, int clip_w, int clip_h,
                                    double initSigma, int doBlur, const mods_hessaff_params *det, const mods_describe_params *desc,
                                    mods_view_geom *geom_out, int *n_detected, int *n_regions) {
  return view_h_detect_describe(c, 0, src_dev, w, h, stride, H, clip_w, clip_h, initSigma, doBlur, det, desc, geom_out, n_detected, n_regions);
}

// the test seam of the post-pass: n host regions (and their twins, or null) through slot 0 and back, *n_out survivors
int mods_test_reproject_regions_h(mods_ctx *c, const double *H, int ow, int oh, mods_region *regions, mods_region *half, int n, int *n_out) {
  if (!c || !H || !n_out || n < 0 || (n > 0 && !regions) || ow <= 0 || oh <= 0) { set_error("reproject_regions_h: bad arguments"); return MODS_E_ARG; }
  if (n > c->max_cand) { set_error("reproject_regions_h: %d regions, the context holds %d", n, c->max_cand); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if (half) MODS_HIP_CHECK(c->regions_half_dev.reserve((size_t)c->max_cand * c->batch));
  if (n) {
    MODS_HIP_CHECK(hipMemcpyAsync(c->regions_dev, regions, sizeof(mods_region) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (half) MODS_HIP_CHECK(hipMemcpyAsync(c->regions_half_dev, half, sizeof(mods_region) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  }
  MODS_HIP_CHECK(hipMemcpyAsync(c->region_count, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  const int rc = launch_reproject_regions_h(c, 0, 0, H, ow, oh, half != nullptr);
  if (rc) return rc;
  int kept = 0;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, &kept, c->region_count, sizeof(int), hipMemcpyDeviceToHost));
  if (kept < 0 || kept > n) { set_error("reproject_regions_h: %d survivors of %d", kept, n); return MODS_E_HIP; }
  if (kept) {
    MODS_HIP_CHECK(mods::copy_wait(c->stream, regions, c->regions_dev, sizeof(mods_region) * (size_t)kept, hipMemcpyDeviceToHost));
    if (half) MODS_HIP_CHECK(mods::copy_wait(c->stream, half, c->regions_half_dev, sizeof(mods_region) * (size_t)kept, hipMemcpyDeviceToHost));
  }
  c->last_region_counts.assign(1, kept);
  c->have_half = half != nullptr;
  *n_out = kept;
  return MODS_OK;
}

// The rematch step under a verified H (img1 -> img2): image 1 seen through H nearly coincides with image 2, so a detector run on
// that view finds regions that repeat where those of the originals did not.  Their regions join bank 1 in image 1's frame (with
// `both`: image 2 through inv(H) joins bank 2), then the banks go through what mods_match_verify_reps runs.
int mods_rematch_under_h_dev(mods_ctx *c, const float *img1_dev, int w1, int h1, const float *img2_dev, int w2, int h2, const double *H, int both,
                             double initSigma, int doBlur, const mods_pair_params *par, mods_imgrep *rep1, mods_imgrep *rep2, double fginn_ratio,
                             mods_ladder_result *res, double *matches_out, int max_matches) {
  if (!c || !img1_dev || !img2_dev || !H || !par || !rep1 || !rep2 || !res) { set_error("rematch_under_h: null argument"); return MODS_E_ARG; }
  if (par->ransac.useF != 0 && par->ransac.useF != 3) {
    set_error("rematch_under_h: useF = %d verifies no homography (0: LO-RANSAC H, 3: ORSA-H)", par->ransac.useF);
    return MODS_E_ARG;
  }
  int rc;
  if ((rc = view_h_detect_describe(c, 0, img1_dev, w1, h1, w1, H, w2, h2, initSigma, doBlur, &par->det, &par->desc, nullptr, nullptr, nullptr))) return rc;
  if ((rc = mods_imgrep_append_ctx(rep1, c, 0))) return rc;
  if (both) {
    double Hi[9], det;
    if (!invert3_adjugate(H, Hi, &det)) { set_error("rematch_under_h: singular homography (determinant %g)", det); return MODS_E_ARG; }
    if ((rc = view_h_detect_describe(c, 1, img2_dev, w2, h2, w2, Hi, w1, h1, initSigma, doBlur, &par->det, &par->desc, nullptr, nullptr, nullptr))) return rc;
    if ((rc = mods_imgrep_append_ctx(rep2, c, 0))) return rc;
  }
  return mods_match_verify_reps(c, rep1, rep2, fginn_ratio, par, res, matches_out, max_matches);
}

}  // extern "C"
