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
#include "ransac_f_host.hpp"
#include <algorithm>

namespace mods {

constexpr int LSM_WAVES = 4;      // waves (= rows) per workgroup
constexpr int LSM_DBG = 49;       // the seam's doubles: N[36] g[6] a delta[6]

struct LsmImg { const float *p; int w, h, stride; };
struct LsmArgs {
  LsmImg img[2];
  const double *laf;
  double *laf_out, *zb, *za, *dbg;
  int *status, *iters;
  int n, R, max_iter, affine;
  double eps_shift, max_shift, max_scale, max_mag, min_zncc, lambda;
};

__device__ __forceinline__ double lsm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

// the bilinear patch at (x, y) and its analytic gradient; false: a tap outside the image (or a position that is not finite)
__device__ __forceinline__ bool lsm_bil(const LsmImg &I, double x, double y, double &v, double &gx, double &gy) {
  const double xf = floor(x), yf = floor(y);
  if (!(xf >= 0. && yf >= 0. && xf <= (double)(I.w - 2) && yf <= (double)(I.h - 2))) return false;
  const double fx = x - xf, fy = y - yf, ex = 1. - fx, ey = 1. - fy;
  const float *r0 = I.p + (size_t)(int)yf * (size_t)I.stride + (size_t)(int)xf, *r1 = r0 + I.stride;
  const double a = r0[0], b = r0[1], c = r1[0], d = r1[1];
  v = (a * ex + b * fx) * ey + (c * ex + d * fx) * fy;
  gx = (b - a) * ey + (d - c) * fy;
  gy = (c - a) * ex + (d - b) * fx;
  return true;
}

// N = L L^T (lower, column by column), then L y = g and L^T x = y, for the leading P x P block; false: a pivot that is not > 0
template <int P> __device__ __forceinline__ bool lsm_solve(const double (&N)[6][6], const double (&g)[6], double (&x)[6]) {
  double L[P][P], y[P];
#pragma unroll
  for (int j = 0; j < P; j++) {
    double s = N[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
    if (!(s > 0.)) return false;
    L[j][j] = sqrt(s);
#pragma unroll
    for (int i = j + 1; i < P; i++) {
      double t = N[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) t = t - L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
#pragma unroll
  for (int i = 0; i < P; i++) {
    double t = g[i];
#pragma unroll
    for (int k = 0; k < i; k++) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = P - 1; i >= 0; i--) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < P; k++) t = t - L[k][i] * x[k];
    x[i] = t / L[i][i];
  }
  return true;
}

__device__ __forceinline__ double lsm_zncc(double Swt, double Sww, double Stt) {
  const double q = Sww * Stt;
  return q > 0. ? Swt / sqrt(q) : 0.;
}

// grid = ceil(n / LSM_WAVES), block = 64 * LSM_WAVES; every branch below is uniform over the wave
template <int K>
__global__ __launch_bounds__(64 * LSM_WAVES) void lsm_kernel(LsmArgs A) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LSM_WAVES + (threadIdx.x >> 6);
  if (row >= A.n) return;
  double f[14];
#pragma unroll
  for (int q = 0; q < 14; q++) f[q] = A.laf[(size_t)row * 14 + q];
  int status = MODS_LSM_BAD_FRAME, iters = 0;
  double zb = 0., za = 0.;
  double cx = 0., cy = 0., B00 = 0., B01 = 0., B10 = 0., B11 = 0.;
  double t00 = 0., t01 = 0., t10 = 0., t11 = 0.;
  bool swapped = false;
  const bool dbg = A.dbg != nullptr && row == 0;
  do {
    bool fin = true;
#pragma unroll
    for (int q = 0; q < 14; q++) fin = fin && isfinite(f[q]);
    const double m00 = f[6] * f[2], m01 = f[6] * f[3], m10 = f[6] * f[4], m11 = f[6] * f[5];
    const double n00 = f[13] * f[9], n01 = f[13] * f[10], n10 = f[13] * f[11], n11 = f[13] * f[12];
    const double d1 = m00 * m11 - m01 * m10, d2 = n00 * n11 - n01 * n10;
    const double i00 = m11 / d1, i01 = (-m01) / d1, i10 = (-m10) / d1, i11 = m00 / d1;
    const double b00 = n00 * i00 + n01 * i10, b01 = n00 * i01 + n01 * i11, b10 = n10 * i00 + n11 * i10, b11 = n10 * i01 + n11 * i11;
    const double dB0 = b00 * b11 - b01 * b10;
    if (!fin || d1 == 0. || d2 == 0. || !isfinite(b00) || !isfinite(b01) || !isfinite(b10) || !isfinite(b11) || !isfinite(dB0) || !(dB0 > 0.)) break;
    swapped = !(dB0 >= 1.);
    if (swapped) { B00 = b11 / dB0; B01 = (-b01) / dB0; B10 = (-b10) / dB0; B11 = b00 / dB0; t00 = n00; t01 = n01; t10 = n10; t11 = n11; }
    else { B00 = b00; B01 = b01; B10 = b10; B11 = b11; t00 = m00; t01 = m01; t10 = m10; t11 = m11; }
    const double detB0 = B00 * B11 - B01 * B10;
    if (!(sqrt(detB0) <= A.max_mag)) break;
    const LsmImg It = A.img[swapped ? 1 : 0], Is = A.img[swapped ? 0 : 1];
    const double ctx = f[swapped ? 7 : 0], cty = f[swapped ? 8 : 1], csx = f[swapped ? 0 : 7], csy = f[swapped ? 1 : 8];
    const int R = A.R, Wd = 2 * R + 1, S = Wd * Wd;
    const double Sd = (double)S;

    // the template: its samples, centred, stay in registers
    double T[K];
    int U[K];      // the offset of sample k: (uy + R) << 8 | (ux + R)
    bool ok = true;
    double acc = 0.;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int idx = lane + 64 * k;
      T[k] = 0.; U[k] = 0;
      if (idx < S) {
        U[k] = (idx / Wd) << 8 | (idx % Wd);
        double v = 0., gx, gy;
        ok = lsm_bil(It, ctx + (double)((U[k] & 255) - R), cty + (double)((U[k] >> 8) - R), v, gx, gy) && ok;
        T[k] = v; acc = acc + v;
      }
    }
    status = MODS_LSM_OUTSIDE;
    if (__any(!ok)) break;
    const double Tm = lsm_wave_sum(acc) / Sd;
    acc = 0.;
#pragma unroll
    for (int k = 0; k < K; k++) if (lane + 64 * k < S) { T[k] = T[k] - Tm; acc = acc + T[k] * T[k]; }
    const double Stt = lsm_wave_sum(acc);
    status = MODS_LSM_FLAT;
    if (Stt <= 1e-6 * Sd) break;

    cx = csx; cy = csy;
    bool final_pass = false, maxiter = false, done = false;
    for (int it = 0;; it++) {
      double W[K], GX[K], GY[K], s[7];
#pragma unroll
      for (int q = 0; q < 7; q++) s[q] = 0.;
      ok = true;
#pragma unroll
      for (int k = 0; k < K; k++) {
        W[k] = 0.; GX[k] = 0.; GY[k] = 0.;
        if (lane + 64 * k < S) {
          const double ux = (double)((U[k] & 255) - R), uy = (double)((U[k] >> 8) - R);
          const double px = cx + (B00 * ux + B01 * uy), py = cy + (B10 * ux + B11 * uy);
          double v = 0., gx = 0., gy = 0.;
          ok = lsm_bil(Is, px, py, v, gx, gy) && ok;
          W[k] = v; GX[k] = gx; GY[k] = gy;
          s[0] = s[0] + v; s[1] = s[1] + gx; s[2] = s[2] + gy;
          s[3] = s[3] + gx * ux; s[4] = s[4] + gx * uy; s[5] = s[5] + gy * ux; s[6] = s[6] + gy * uy;
        }
      }
      status = MODS_LSM_OUTSIDE;
      if (__any(!ok)) break;
#pragma unroll
      for (int q = 0; q < 7; q++) s[q] = lsm_wave_sum(s[q]) / Sd;
      double swt = 0., sww = 0.;
#pragma unroll
      for (int k = 0; k < K; k++) if (lane + 64 * k < S) { W[k] = W[k] - s[0]; swt = swt + W[k] * T[k]; sww = sww + W[k] * W[k]; }
      const double Swt = lsm_wave_sum(swt), Sww = lsm_wave_sum(sww);
      const double z = lsm_zncc(Swt, Sww, Stt);
      if (it == 0) zb = z;
      if (final_pass) { za = z; done = true; break; }
      const double a = Swt / Sww;
      double nn[21], gg[6];
#pragma unroll
      for (int q = 0; q < 21; q++) nn[q] = 0.;
#pragma unroll
      for (int q = 0; q < 6; q++) gg[q] = 0.;
#pragma unroll
      for (int k = 0; k < K; k++) if (lane + 64 * k < S) {
        const double ux = (double)((U[k] & 255) - R), uy = (double)((U[k] >> 8) - R), gx = GX[k], gy = GY[k];
        const double r = T[k] - a * W[k];
        const double J[6] = {a * (gx - s[1]), a * (gy - s[2]), a * (gx * ux - s[3]), a * (gx * uy - s[4]), a * (gy * ux - s[5]), a * (gy * uy - s[6])};
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
          for (int j = 0; j <= i; j++, q++) nn[q] = nn[q] + J[i] * J[j];
          gg[i] = gg[i] + J[i] * r;
        }
      }
      double N[6][6], g[6], delta[6] = {0., 0., 0., 0., 0., 0.};
      {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
          for (int j = 0; j <= i; j++, q++) { const double v = lsm_wave_sum(nn[q]); N[i][j] = v; N[j][i] = v; }
          g[i] = lsm_wave_sum(gg[i]);
        }
      }
      bool solved;
      if (A.affine) {
        const double tr = ((((N[0][0] + N[1][1]) + N[2][2]) + N[3][3]) + N[4][4]) + N[5][5];
#pragma unroll
        for (int i = 0; i < 6; i++) N[i][i] = N[i][i] + A.lambda * tr;
        solved = lsm_solve<6>(N, g, delta);
      } else {
        const double tr = N[0][0] + N[1][1];
        N[0][0] = N[0][0] + A.lambda * tr; N[1][1] = N[1][1] + A.lambda * tr;
        solved = lsm_solve<2>(N, g, delta);
      }
      if (dbg && it == 0 && lane == 0) {
        const int P = A.affine ? 6 : 2;
        for (int i = 0; i < 6; i++) {
          for (int j = 0; j < 6; j++) A.dbg[6 * i + j] = i < P && j < P ? N[i][j] : 0.;
          A.dbg[36 + i] = i < P ? g[i] : 0.;
          A.dbg[43 + i] = solved ? delta[i] : 0.;
        }
        A.dbg[42] = a;
      }
      status = MODS_LSM_FLAT;
      if (!solved) break;
      cx = cx + delta[0]; cy = cy + delta[1];
      B00 = B00 + delta[2]; B01 = B01 + delta[3]; B10 = B10 + delta[4]; B11 = B11 + delta[5];
      iters = it + 1;
      const bool conv = sqrt(delta[0] * delta[0] + delta[1] * delta[1]) < A.eps_shift;
      if (conv || iters >= A.max_iter) { final_pass = true; maxiter = !conv; }
    }
    if (!done) break;
    const double dx = cx - csx, dy = cy - csy;
    const double shift = sqrt(dx * dx + dy * dy), q = sqrt((B00 * B11 - B01 * B10) / detB0), lo = 1. / A.max_scale;
    if (!(shift <= A.max_shift) || !(q >= lo && q <= A.max_scale)) status = MODS_LSM_DIVERGED;
    else if (!(za >= A.min_zncc)) status = MODS_LSM_LOW_ZNCC;
    else status = maxiter ? MODS_LSM_MAXITER : MODS_LSM_OK;
  } while (false);

  if (lane != 0) return;
  if (status == MODS_LSM_OK || status == MODS_LSM_MAXITER) {
    const double p00 = B00 * t00 + B01 * t10, p01 = B00 * t01 + B01 * t11, p10 = B10 * t00 + B11 * t10, p11 = B10 * t01 + B11 * t11;
    const double sc = sqrt(fabs(p00 * p11 - p01 * p10));
    const int o = swapped ? 0 : 7;
    f[o] = cx; f[o + 1] = cy; f[o + 2] = p00 / sc; f[o + 3] = p01 / sc; f[o + 4] = p10 / sc; f[o + 5] = p11 / sc; f[o + 6] = sc;
  }
#pragma unroll
  for (int q = 0; q < 14; q++) A.laf_out[(size_t)row * 14 + q] = f[q];
  A.status[row] = status; A.iters[row] = iters; A.zb[row] = zb; A.za[row] = za;
}

static int lsm_check(const mods_lsm_params *p) {
  if (p->radius < 1 || p->radius > 15) { set_error("refine_matches: radius %d (1 .. 15)", p->radius); return MODS_E_ARG; }
  if (p->max_iter < 1 || p->max_iter > 1000) { set_error("refine_matches: max_iter %d (1 .. 1000)", p->max_iter); return MODS_E_ARG; }
  if (!std::isfinite(p->eps_shift) || !(p->eps_shift > 0)) { set_error("refine_matches: eps_shift %g (finite and > 0)", p->eps_shift); return MODS_E_ARG; }
  if (!std::isfinite(p->max_shift) || !(p->max_shift > 0)) { set_error("refine_matches: max_shift %g (finite and > 0)", p->max_shift); return MODS_E_ARG; }
  if (!std::isfinite(p->lambda) || !(p->lambda > 0)) { set_error("refine_matches: lambda %g (finite and > 0)", p->lambda); return MODS_E_ARG; }
  if (!std::isfinite(p->max_scale_change) || !(p->max_scale_change >= 1)) { set_error("refine_matches: max_scale_change %g (finite and >= 1)", p->max_scale_change); return MODS_E_ARG; }
  if (!std::isfinite(p->max_magnification) || !(p->max_magnification >= 1)) { set_error("refine_matches: max_magnification %g (finite and >= 1)", p->max_magnification); return MODS_E_ARG; }
  if (!(p->min_zncc >= -1 && p->min_zncc <= 1)) { set_error("refine_matches: min_zncc %g (-1 .. 1)", p->min_zncc); return MODS_E_ARG; }
  if (p->affine != 0 && p->affine != 1) { set_error("refine_matches: affine %d (0 or 1)", p->affine); return MODS_E_ARG; }
  return MODS_OK;
}

// every refusal of the header's list that needs no device; *p = the parameters the call runs with
static int lsm_check_call(const mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2,
                          const double *laf14, int n, const mods_lsm_params *par, mods_lsm_params *p) {
  if (par) *p = *par; else mods_lsm_defaults(p);
  const int rc = lsm_check(p);
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

// the two host images, dense, into the context's own buffer
static int lsm_upload(mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2, LsmImg *i1, LsmImg *i2) {
  const size_t n1 = (size_t)w1 * h1, n2 = (size_t)w2 * h2;
  MODS_HIP_CHECK(reserve_scratch(c, c->lsm_img, n1 + n2, n1 + n2));
  float *d = c->lsm_img.get();
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
  if ((rc = lsm_upload(c, img1, w1, h1, stride1, img2, w2, h2, stride2, &i1, &i2))) return rc;
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
  if ((rc = lsm_upload(c, img1, w1, h1, stride1, img2, w2, h2, stride2, &i1, &i2))) return rc;
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
