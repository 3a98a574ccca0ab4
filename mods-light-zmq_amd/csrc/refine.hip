// Refinement of correspondences by affine least-squares matching (include/mods_hip.h: mods_refine_matches[_dev]; no counterpart in
// the reference).  The (2R+1)^2 window of the image where the region is smaller is registered onto the other image by an iterated
// Gauss-Newton fit of a translation and a 2 x 2 affinity with gain and offset; all of it fp64 on fp32 pixels.
//   lsm_kernel<K>   one wave per correspondence, four waves per workgroup, every iteration inside the kernel.  A lane holds the samples
//                   k = lane, lane + 64, ... of the window (K = the most a lane can hold, 1 .. 16): the centred template, and per
//                   iteration the search window's value and gradient, all in registers.  A sum over the window is the lane's
//                   partial sum in ascending k, then a butterfly over lane xor 32, 16, 8, 4, 2, 1 (lsm_wave_sum): every lane ends
//                   with the same bits, so the 6 x 6 Cholesky and every decision run redundantly in all lanes and nothing is
//                   broadcast.  Three rounds per iteration: 7 sums (means), 2 (gain, zncc), 27 (normal equations).
//                   No LDS, no atomics, no barrier: the waves of a workgroup share nothing and each leaves when its row is done.
// The order of a sum does not depend on K, on n or on the row's place: a row's bits are a function of the row and the two images.
#include "common.hpp"
#include "lsm_row.hpp"
#include "ransac_f_host.hpp"
#include <algorithm>

namespace mods {

// grid = ceil(n / LSM_WAVES), block = 64 * LSM_WAVES: one wave per row (lsm_row.hpp)
template <int K>
__global__ __launch_bounds__(64 * LSM_WAVES) void lsm_kernel(LsmArgs A) {
  const int row = blockIdx.x * LSM_WAVES + (threadIdx.x >> 6);
  if (row >= A.n) return;
  lsm_row<K>(A, row, threadIdx.x & 63);
}

// `who`: the entry point the refusal names ("refine_matches", "propagate_matches")
int lsm_check(const mods_lsm_params *p, const char *who) {
  if (p->radius < 1 || p->radius > 15) { set_error("%s: radius %d (1 .. 15)", who, p->radius); return MODS_E_ARG; }
  if (p->max_iter < 1 || p->max_iter > 1000) { set_error("%s: max_iter %d (1 .. 1000)", who, p->max_iter); return MODS_E_ARG; }
  if (!std::isfinite(p->eps_shift) || !(p->eps_shift > 0)) { set_error("%s: eps_shift %g (finite and > 0)", who, p->eps_shift); return MODS_E_ARG; }
  if (!std::isfinite(p->max_shift) || !(p->max_shift > 0)) { set_error("%s: max_shift %g (finite and > 0)", who, p->max_shift); return MODS_E_ARG; }
  if (!std::isfinite(p->lambda) || !(p->lambda > 0)) { set_error("%s: lambda %g (finite and > 0)", who, p->lambda); return MODS_E_ARG; }
  if (!std::isfinite(p->max_scale_change) || !(p->max_scale_change >= 1)) { set_error("%s: max_scale_change %g (finite and >= 1)", who, p->max_scale_change); return MODS_E_ARG; }
  if (!std::isfinite(p->max_magnification) || !(p->max_magnification >= 1)) { set_error("%s: max_magnification %g (finite and >= 1)", who, p->max_magnification); return MODS_E_ARG; }
  if (!(p->min_zncc >= -1 && p->min_zncc <= 1)) { set_error("%s: min_zncc %g (-1 .. 1)", who, p->min_zncc); return MODS_E_ARG; }
  if (p->affine != 0 && p->affine != 1) { set_error("%s: affine %d (0 or 1)", who, p->affine); return MODS_E_ARG; }
  return MODS_OK;
}

// every refusal of the header's list that needs no device; *p = the parameters the call runs with
static int lsm_check_call(const mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2,
                          const double *laf14, int n, const mods_lsm_params *par, mods_lsm_params *p) {
  if (par) *p = *par; else mods_lsm_defaults(p);
  const int rc = lsm_check(p, "refine_matches");
  if (rc) return rc;
  if (n < 0) { set_error("refine_matches: n = %d", n); return MODS_E_ARG; }
  if (w1 < 2 || h1 < 2 || w2 < 2 || h2 < 2) { set_error("refine_matches: image size %d x %d, %d x %d (at least 2 x 2)", w1, h1, w2, h2); return MODS_E_ARG; }
  if (stride1 < w1 || stride2 < w2) { set_error("refine_matches: stride %d, %d below the width %d, %d", stride1, stride2, w1, w2); return MODS_E_ARG; }
  if (!c || !img1 || !img2 || (n > 0 && !laf14)) { set_error("refine_matches: null argument"); return MODS_E_ARG; }
  return MODS_OK;
}

static int lsm_run(mods_ctx *c, const LsmImg &i1, const LsmImg &i2, const double *laf14, int n, const mods_lsm_params &p, double *laf_out,
                   double *u6_out, int *status_out, int *iters_out, double *zb_out, double *za_out, double *dbg_out) {
  const size_t N = (size_t)n;
  const size_t off_out = N * 14 * sizeof(double), off_zb = 2 * off_out, off_za = off_zb + N * sizeof(double);
  const size_t off_dbg = off_za + N * sizeof(double), off_st = off_dbg + LSM_DBG * sizeof(double), off_it = off_st + N * sizeof(int);
  const size_t bytes = off_it + N * sizeof(int);
  MODS_HIP_CHECK(reserve_scratch(c, c->lsm_buf, bytes, bytes + bytes / 4));
  char *d = c->lsm_buf.get();
  static thread_local std::vector<char> stage;
  stage.resize(bytes);
  MODS_HIP_CHECK(hipMemcpyAsync(d, laf14, off_out, hipMemcpyHostToDevice, c->stream));
  LsmArgs a;
  a.img[0] = i1; a.img[1] = i2;
  a.laf = (const double *)d; a.laf_out = (double *)(d + off_out); a.zb = (double *)(d + off_zb); a.za = (double *)(d + off_za);
  a.dbg = dbg_out ? (double *)(d + off_dbg) : nullptr;
  a.status = (int *)(d + off_st); a.iters = (int *)(d + off_it);
  a.n = n; a.R = p.radius; a.max_iter = p.max_iter; a.affine = p.affine;
  a.eps_shift = p.eps_shift; a.max_shift = p.max_shift; a.max_scale = p.max_scale_change; a.max_mag = p.max_magnification;
  a.min_zncc = p.min_zncc; a.lambda = p.lambda;
  if (dbg_out) MODS_HIP_CHECK(hipMemsetAsync(d + off_dbg, 0, LSM_DBG * sizeof(double), c->stream));
  {
    StageScope ts(c, MODS_STAGE_REFINE);
    const dim3 grid((unsigned)((n + LSM_WAVES - 1) / LSM_WAVES)), block(64 * LSM_WAVES);
    const int S = (2 * p.radius + 1) * (2 * p.radius + 1), per_lane = (S + 63) / 64;
    if (per_lane <= 1) hipLaunchKernelGGL(lsm_kernel<1>, grid, block, 0, c->stream, a);
    else if (per_lane <= 2) hipLaunchKernelGGL(lsm_kernel<2>, grid, block, 0, c->stream, a);
    else if (per_lane <= 4) hipLaunchKernelGGL(lsm_kernel<4>, grid, block, 0, c->stream, a);
    else if (per_lane <= 8) hipLaunchKernelGGL(lsm_kernel<8>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(lsm_kernel<16>, grid, block, 0, c->stream, a);
    MODS_HIP_CHECK(hipGetLastError());
  }
  MODS_HIP_CHECK(copy_wait(c->stream, stage.data() + off_out, d + off_out, bytes - off_out, hipMemcpyDeviceToHost));
  const double *lo = (const double *)(stage.data() + off_out);
  if (laf_out) memcpy(laf_out, lo, off_out);
  if (u6_out) for (size_t i = 0; i < N; i++) {
    double *u = u6_out + 6 * i;
    u[0] = lo[14 * i]; u[1] = lo[14 * i + 1]; u[2] = 1.; u[3] = lo[14 * i + 7]; u[4] = lo[14 * i + 8]; u[5] = 1.;
  }
  if (zb_out) memcpy(zb_out, stage.data() + off_zb, N * sizeof(double));
  if (za_out) memcpy(za_out, stage.data() + off_za, N * sizeof(double));
  if (dbg_out) memcpy(dbg_out, stage.data() + off_dbg, LSM_DBG * sizeof(double));
  if (status_out) memcpy(status_out, stage.data() + off_st, N * sizeof(int));
  if (iters_out) memcpy(iters_out, stage.data() + off_it, N * sizeof(int));
  return MODS_OK;
}

// the two host images, dense, into a buffer of the context's
int lsm_upload(mods_ctx *c, Buf<float> &buf, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2, LsmImg *i1, LsmImg *i2) {
  const size_t n1 = (size_t)w1 * h1, n2 = (size_t)w2 * h2;
  MODS_HIP_CHECK(reserve_scratch(c, buf, n1 + n2, n1 + n2));
  float *d = buf.get();
  MODS_HIP_CHECK(hipMemcpy2DAsync(d, sizeof(float) * w1, img1, sizeof(float) * stride1, sizeof(float) * w1, h1, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpy2DAsync(d + n1, sizeof(float) * w2, img2, sizeof(float) * stride2, sizeof(float) * w2, h2, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(stream_wait(c->stream));        // the host images may go away behind the call
  *i1 = LsmImg{d, w1, h1, w1}; *i2 = LsmImg{d + n1, w2, h2, w2};
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

void mods_lsm_defaults(mods_lsm_params *p) {
  if (!p) return;
  p->radius = 10; p->max_iter = 20; p->eps_shift = 0.01; p->max_shift = 3.0; p->max_scale_change = 1.5; p->max_magnification = 8;
  p->min_zncc = 0.8; p->lambda = 1e-9; p->affine = 1; p->pad = 0;
}

int mods_refine_matches_dev(mods_ctx *c, const float *img1_dev, int w1, int h1, int stride1, const float *img2_dev, int w2, int h2,
                            int stride2, const double *laf14, int n, const mods_lsm_params *par, double *laf_out, double *u6_out,
                            int *status_out, int *iters_out, double *zncc_before_out, double *zncc_after_out) {
  mods_lsm_params p;
  const int rc = lsm_check_call(c, img1_dev, w1, h1, stride1, img2_dev, w2, h2, stride2, laf14, n, par, &p);
  if (rc) return rc;
  if (n == 0) return MODS_OK;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  return lsm_run(c, LsmImg{img1_dev, w1, h1, stride1}, LsmImg{img2_dev, w2, h2, stride2}, laf14, n, p, laf_out, u6_out, status_out,
                 iters_out, zncc_before_out, zncc_after_out, nullptr);
}

int mods_refine_matches(mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2,
                        const double *laf14, int n, const mods_lsm_params *par, double *laf_out, double *u6_out, int *status_out,
                        int *iters_out, double *zncc_before_out, double *zncc_after_out) {
  mods_lsm_params p;
  int rc = lsm_check_call(c, img1, w1, h1, stride1, img2, w2, h2, stride2, laf14, n, par, &p);
  if (rc) return rc;
  if (n == 0) return MODS_OK;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  LsmImg i1, i2;
  if ((rc = lsm_upload(c, c->lsm_img, img1, w1, h1, stride1, img2, w2, h2, stride2, &i1, &i2))) return rc;
  return lsm_run(c, i1, i2, laf14, n, p, laf_out, u6_out, status_out, iters_out, zncc_before_out, zncc_after_out, nullptr);
}

int mods_test_lsm_iteration(mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2,
                            const double *laf14_row, const mods_lsm_params *par, double *N36, double *g6, double *a, double *delta6,
                            int *status_out) {
  mods_lsm_params p;
  int rc = lsm_check_call(c, img1, w1, h1, stride1, img2, w2, h2, stride2, laf14_row, 1, par, &p);
  if (rc) return rc;
  if (!N36 || !g6 || !a || !delta6 || !status_out) { set_error("refine_matches: null argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  LsmImg i1, i2;
  if ((rc = lsm_upload(c, c->lsm_img, img1, w1, h1, stride1, img2, w2, h2, stride2, &i1, &i2))) return rc;
  double dbg[LSM_DBG];
  p.max_iter = 1;
  if ((rc = lsm_run(c, i1, i2, laf14_row, 1, p, nullptr, nullptr, status_out, nullptr, nullptr, nullptr, dbg))) return rc;
  memcpy(N36, dbg, 36 * sizeof(double)); memcpy(g6, dbg + 36, 6 * sizeof(double)); *a = dbg[42]; memcpy(delta6, dbg + 43, 6 * sizeof(double));
  return MODS_OK;
}

int mods_refit_model(const double *u6, int n, int model_type, double *model_out) {
  if (!u6 || !model_out) { set_error("refit_model: null argument"); return MODS_E_ARG; }
  if (model_type != 0 && model_type != 1) { set_error("refit_model: model_type %d (0 = H, 1 = F)", model_type); return MODS_E_ARG; }
  if (n < (model_type == 0 ? 4 : 8)) { set_error("refit_model: %d rows (at least %d)", n, model_type == 0 ? 4 : 8); return MODS_E_ARG; }
  std::vector<int> all((size_t)n);
  for (int i = 0; i < n; i++) all[i] = i;
  std::vector<double> buffer((size_t)18 * n + 96);
  if (model_type == 1) { rs::u2f(u6, all.data(), n, model_out, buffer.data()); return MODS_OK; }
  // as the verification does with the LO step's model (capi.hip: h_post_checks): row-major image 1 -> image 2 = inv(h^T)
  // (four rows: each twice, so that they too go through the normalised fit and not the minimal solver of a RANSAC sample)
  if (n == 4) for (int i = 0; i < 4; i++) all.push_back(i);
  double h[9], d = 0.;
  rs::u2h(u6, all.data(), (int)all.size(), h, buffer.data());
  const double Ht[9] = {h[0], h[3], h[6], h[1], h[4], h[7], h[2], h[5], h[8]};
  if (!invert3_adjugate(Ht, model_out, &d)) { set_error("refit_model: degenerate rows (determinant %g)", d); return MODS_E_ARG; }
  return MODS_OK;
}

}  // extern "C"
