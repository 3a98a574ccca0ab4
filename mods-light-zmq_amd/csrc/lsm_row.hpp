// The row body of the least-squares refinement (include/mods_hip.h: the contract of mods_refine_matches), shared by its two users:
// refine.hip (lsm_kernel: rows staged from the host) and propagate.hip (prop_lsm_kernel: the candidate rows of a round, made on the
// device).  Both instantiate lsm_row<K>, so a row gives the same bits through either.
#pragma once
#include "common.hpp"

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

// one row by one wave (lane = 0 .. 63 of it); every branch below is uniform over the wave.  K = the most samples a lane holds
template <int K>
__device__ __forceinline__ void lsm_row(const LsmArgs &A, const int row, const int lane) {
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

// the instantiation a radius needs: the samples of a lane, rounded up to 1, 2, 4, 8 or 16
inline int lsm_per_lane(int radius) { const int S = (2 * radius + 1) * (2 * radius + 1); return (S + 63) / 64; }

// refine.hip
int lsm_check(const mods_lsm_params *p, const char *who);
int lsm_upload(mods_ctx *c, Buf<float> &buf, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2, LsmImg *i1, LsmImg *i2);

}  // namespace mods
