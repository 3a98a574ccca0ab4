// Host SIMD forms of the per-correspondence error functions of the LO step (Htools.c:160-240) and of the
// truncated-quadratic gains (rtools.c:228-236).  Included by ransac_simd_x{1,4,8}.cpp with VW (lanes) and NS defined;
// every lane executes the scalar code's operations in the scalar code's order (GCC/clang vector extensions, one IEEE
// operation per source operation, built with -ffp-contract=off), so the results are bit-identical to rs::hds_point /
// rs::hsym_point / rs::trunc_quad for every lane count.  No headers: these translation units are built with wider
// -m flags than the rest of the library and must not emit any shared inline function.
namespace mods { namespace rs { namespace NS {
typedef double V __attribute__((vector_size(8 * VW), aligned(8)));
static inline V ld(const double *p) { V v; __builtin_memcpy(&v, p, sizeof(V)); return v; }
static inline void st(double *p, V v) { __builtin_memcpy(p, &v, sizeof(V)); }
static inline V bc(double x) { V v; for (int i = 0; i < VW; i++) v[i] = x; return v; }

// hds_point over VW correspondences (Htools.c:160-199)
static inline V hds_v(V u0, V u1, V u3, V u4, V u5, const double *H) {
  const V zero = bc(0.0);
  const V z0[9] = {u3, zero, -u0 * u3, u4, zero, -u0 * u4, u5, zero, -u0 * u5};
  const V z1[9] = {zero, u3, -u1 * u3, zero, u4, -u1 * u4, zero, u5, -u1 * u5};
  V r1 = zero, r2 = zero;
  for (int j = 0; j < 9; j++) { r1 += H[j] * z0[j]; r2 += H[j] * z1[j]; }
  const V a = H[0] - H[2] * u0;
  const V b = H[3] - H[5] * u0;
  const V c = -H[8] - H[2] * u3 - H[5] * u4;
  const V d = H[1] - H[2] * u1;
  const V e = H[4] - H[5] * u1;
  V pJ[8];
  {
    const V a2 = a * a, b2 = b * b, c2 = c * c, d2 = d * d, e2 = e * e;
    const V c2pd2 = c2 + d2, ab = a * b, de = d * e;
    const V Q = c * (c2pd2 + e2);
    pJ[0] = -b * de + a * (c2 + e2);
    pJ[1] = b * c2pd2 - a * de;
    pJ[2] = Q;
    pJ[3] = -c * (a * d + b * e);
    pJ[4] = d * (b2 + c2) - ab * e;
    pJ[5] = -ab * d + e * (a2 + c2);
    pJ[6] = pJ[3];
    pJ[7] = c * (a2 + b2 + c2);
    const V N = a * pJ[0] + b * pJ[1] + c * pJ[2];
    for (int i = 0; i < 8; i++) pJ[i] /= N;
  }
  V p = zero;
  for (int j = 0; j < 4; j++) {
    const V t = pJ[j] * r1 + pJ[j + 4] * r2;
    p += t * t;
  }
  return p;
}
// soa: 5 arrays (u0 u1 u3 u4 u5) of n_pad doubles, n_pad a multiple of VW; d has room for n_pad values
void hds_all(const double *const *soa, int n_pad, const double *H, double *d) {
  for (int i = 0; i < n_pad; i += VW) st(d + i, hds_v(ld(soa[0] + i), ld(soa[1] + i), ld(soa[2] + i), ld(soa[3] + i), ld(soa[4] + i), H));
}
// hsym_point (Htools.c:223-240); mode 0: d1 + d2, 1: MAX(d1, d2) as Htools.c:15 writes it, `d1 < d2 ? d2 : d1` (a NaN d2 leaves d1)
void hsym_all(const double *const *soa, int n_pad, const double *H1, const double *Hinv, int mode, double *d) {
  for (int i = 0; i < n_pad; i += VW) {
    const V u0 = ld(soa[0] + i), u1 = ld(soa[1] + i), u3 = ld(soa[2] + i), u4 = ld(soa[3] + i);
    const V a = H1[6] * u0 + H1[7] * u1 + H1[8];
    const V b = Hinv[6] * u3 + Hinv[7] * u4 + Hinv[8];
    V xa = (H1[0] * u0 + H1[1] * u1 + H1[2]) / a;
    V ya = (H1[3] * u0 + H1[4] * u1 + H1[5]) / a;
    V xd = u3 - xa, yd = u4 - ya;
    const V d1 = xd * xd + yd * yd;
    xa = (Hinv[0] * u3 + Hinv[1] * u4 + Hinv[2]) / b;
    ya = (Hinv[3] * u3 + Hinv[4] * u4 + Hinv[5]) / b;
    xd = u0 - xa; yd = u1 - ya;
    const V d2 = xd * xd + yd * yd;
    V r;
    if (mode == 0) r = d1 + d2;
    else r = d1 < d2 ? d2 : d1;
    st(d + i, r);
  }
}
// both parts of the symmetric transfer error (the d1, d2 of hsym_point) side by side: NaiveHCheck (matching.cpp:1014-1043) tests each
// against its bound; soa = {x1, y1, x2, y2}
void hsym_both_all(const double *const *soa, int n_pad, const double *H1, const double *Hinv, double *d1o, double *d2o) {
  for (int i = 0; i < n_pad; i += VW) {
    const V u0 = ld(soa[0] + i), u1 = ld(soa[1] + i), u3 = ld(soa[2] + i), u4 = ld(soa[3] + i);
    const V a = H1[6] * u0 + H1[7] * u1 + H1[8];
    const V b = Hinv[6] * u3 + Hinv[7] * u4 + Hinv[8];
    V xa = (H1[0] * u0 + H1[1] * u1 + H1[2]) / a;
    V ya = (H1[3] * u0 + H1[4] * u1 + H1[5]) / a;
    V xd = u3 - xa, yd = u4 - ya;
    st(d1o + i, xd * xd + yd * yd);
    xa = (Hinv[0] * u3 + Hinv[1] * u4 + Hinv[2]) / b;
    ya = (Hinv[3] * u3 + Hinv[4] * u4 + Hinv[5]) / b;
    xd = u0 - xa; yd = u1 - ya;
    st(d2o + i, xd * xd + yd * yd);
  }
}
// truncQuad gains (rtools.c:228-236) for thr != 0: g = eps >= lim ? 0 : 1 - eps / lim, lim = thr*9/4
void gains_all(const double *err, int n_pad, double lim, double *g) {
  const V zero = bc(0.0), one = bc(1.0), L = bc(lim);
  for (int i = 0; i < n_pad; i += VW) {
    const V e = ld(err + i);
    const V q = one - e / L;
    st(g + i, e >= L ? zero : q);
  }
}
// FDs / FDsSym / exFDs / exFDsSym over all correspondences (Ftools.c:94-135, 163-209).  mode 0: Sampson error; 1: symmetric
// epipolar distance r^2 (a + b) / (a b); 2: Sampson error + weight 1 / sqrt(w); 3: r^2 / q with the weight q = a b / (a + b)
static inline V vsqrt(V x) { V r; for (int i = 0; i < VW; i++) r[i] = __builtin_sqrt(x[i]); return r; }
void fds_all(const double *const *soa, int n_pad, const double *F, int mode, double *p, double *w) {
  const V one = bc(1.0);
  for (int i = 0; i < n_pad; i += VW) {
    const V u0 = ld(soa[0] + i), u1 = ld(soa[1] + i), u3 = ld(soa[2] + i), u4 = ld(soa[3] + i);
    const V rxc = F[0] * u3 + F[3] * u4 + F[6];
    const V ryc = F[1] * u3 + F[4] * u4 + F[7];
    const V rwc = F[2] * u3 + F[5] * u4 + F[8];
    const V r = (u0 * rxc + u1 * ryc + rwc);
    const V rx = F[0] * u0 + F[1] * u1 + F[2];
    const V ry = F[3] * u0 + F[4] * u1 + F[5];
    if (mode == 0 || mode == 2) {
      const V ws = rxc * rxc + ryc * ryc + rx * rx + ry * ry;
      st(p + i, r * r / ws);
      if (mode == 2) st(w + i, one / vsqrt(ws));
    } else {
      const V a = rxc * rxc + ryc * ryc;
      const V b = rx * rx + ry * ry;
      if (mode == 1) st(p + i, r * r * (a + b) / (a * b));
      else { const V q = (a * b) / (a + b); st(w + i, q); st(p + i, r * r / q); }
    }
  }
}
// The 30 ordered sums of the homography's moment matrix (rs::cov_hgN, ransac_host.hpp: lin_hgN + cov_mat, Htools.c:60-98,
// utools.c:172-185): sums30 = bb[6] | cd[6] | bc[9] | bd[9] with b = (b0, b1, 1), c = -a0 b, d = -a1 b per correspondence;
// bb / cd over the pairs (j, k <= j), bc / bd over (j, k).  8 lanes: the running sums sit side by side in four vectors (+ the two
// ninth entries of bc / bd), every lane receives the scalar code's products in the scalar code's order.
#if VW == 8
void cov_hg_all(const double *u, const int *inl, int len, const double *A1, const double *A2, double *sums30) {
  V abb = bc(0.0), acd = bc(0.0), abc = bc(0.0), abd = bc(0.0);
  double bc8 = 0.0, bd8 = 0.0;
  const double s1 = A1[0], t10 = A1[1], t11 = A1[2], s2 = A2[0], t20 = A2[1], t21 = A2[2];
  for (int i = 0; i < len; i++) {
    const double *s = u + 6 * inl[i];
    const double a0 = s[0] * s1 + t10, a1 = s[1] * s1 + t11;
    V t = bc(1.0);
    t[0] = s[3] * s2 + t20;
    t[1] = s[4] * s2 + t21;
    const V B = __builtin_shufflevector(t, t, 0, 1, 2, 0, 1, 2, 0, 1);        // b[l % 3]
    const V Bj = __builtin_shufflevector(t, t, 0, 0, 0, 1, 1, 1, 2, 2);       // b[l / 3]
    const V Cv = bc(-a0) * B, Dv = bc(-a1) * B;                               // c[l % 3], d[l % 3]
    // pairs (j, k): (0,0) (1,0) (1,1) (2,0) (2,1) (2,2); lanes 6, 7 unused
    const V bj = __builtin_shufflevector(B, B, 0, 1, 1, 2, 2, 2, 0, 0), bk = __builtin_shufflevector(B, B, 0, 0, 1, 0, 1, 2, 0, 0);
    const V cj = __builtin_shufflevector(Cv, Cv, 0, 1, 1, 2, 2, 2, 0, 0), ck = __builtin_shufflevector(Cv, Cv, 0, 0, 1, 0, 1, 2, 0, 0);
    const V dj = __builtin_shufflevector(Dv, Dv, 0, 1, 1, 2, 2, 2, 0, 0), dk = __builtin_shufflevector(Dv, Dv, 0, 0, 1, 0, 1, 2, 0, 0);
    abb += bj * bk;
    acd += cj * ck;
    acd += dj * dk;
    abc += Bj * Cv;
    abd += Bj * Dv;
    bc8 += 1.0 * Cv[2];
    bd8 += 1.0 * Dv[2];
  }
  for (int q = 0; q < 6; q++) { sums30[q] = abb[q]; sums30[6 + q] = acd[q]; }
  for (int q = 0; q < 8; q++) { sums30[12 + q] = abc[q]; sums30[21 + q] = abd[q]; }
  sums30[20] = bc8; sums30[29] = bd8;
}
#else
void cov_hg_all(const double *u, const int *inl, int len, const double *A1, const double *A2, double *sums30) {
  double *bb = sums30, *cd = sums30 + 6, *bcs = sums30 + 12, *bd = sums30 + 21;
  for (int q = 0; q < 30; q++) sums30[q] = 0.0;
  for (int i = 0; i < len; i++) {
    const double *s = u + 6 * inl[i];
    const double a0 = s[0] * A1[0] + A1[1], a1 = s[1] * A1[0] + A1[2];
    double b[3], c[3], d[3];
    b[0] = s[3] * A2[0] + A2[1]; b[1] = s[4] * A2[0] + A2[2]; b[2] = 1;
    for (int j = 0; j < 3; j++) { c[j] = -a0 * b[j]; d[j] = -a1 * b[j]; }
    int q = 0;
    for (int j = 0; j < 3; j++)
      for (int k = 0; k <= j; k++, q++) { bb[q] += b[j] * b[k]; cd[q] += c[j] * c[k]; cd[q] += d[j] * d[k]; }
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) { bcs[3 * j + k] += b[j] * c[k]; bd[3 * j + k] += b[j] * d[k]; }
  }
}
#endif
// lin_fmN (+ the row weights of u2fw) + cov_mat (Ftools.c:246-276, 302-405; utools.c:172-185) without the len x 9 matrix, the
// 45 running sums side by side in vector lanes: row r of the lower triangle is z[r] * z[0..r], accumulated as whole vectors of
// z[r] * z[c] (the lanes c > r hold the mirror entries and are not read back).  Every used lane receives the scalar code's
// products in the scalar code's row order, so the sums are bit-identical for every lane count.  acc45: lower triangle, row-major.
#if VW == 8
// 8 lanes: z[0..7] is made in a register as {a0,a1,1,a0,a1,1,a0,a1} * {b0,b0,b0,b1,b1,b1,1,1} (the same nine products a[l] * b[k];
// going through memory would put a failed store-to-load forwarding on every row), z[8] = 1 * 1 stays scalar
void cov_fm_all(const double *u, const int *inl, const double *w, int len, const double *A1, const double *A2, double *acc45) {
  V acc[9];
  for (int r = 0; r < 9; r++) acc[r] = bc(0.0);
  double acc88 = 0.0;
  for (int i = 0; i < len; i++) {
    const double *s = u + 6 * inl[i];
    V t = bc(1.0);
    t[0] = s[0] * A1[0] + A1[1];
    t[1] = s[1] * A1[0] + A1[2];
    t[3] = s[3] * A2[0] + A2[1];
    t[4] = s[4] * A2[0] + A2[2];
    const V va = __builtin_shufflevector(t, t, 0, 1, 2, 0, 1, 2, 0, 1);
    const V vb = __builtin_shufflevector(t, t, 3, 3, 3, 4, 4, 4, 5, 5);
    V z = va * vb;
    double z8 = 1.0 * 1.0;
    if (w) {
      const double m = w[inl[i]];
      z *= bc(m);
      z8 *= m;
    }
    acc[0] += __builtin_shufflevector(z, z, 0, 0, 0, 0, 0, 0, 0, 0) * z;
    acc[1] += __builtin_shufflevector(z, z, 1, 1, 1, 1, 1, 1, 1, 1) * z;
    acc[2] += __builtin_shufflevector(z, z, 2, 2, 2, 2, 2, 2, 2, 2) * z;
    acc[3] += __builtin_shufflevector(z, z, 3, 3, 3, 3, 3, 3, 3, 3) * z;
    acc[4] += __builtin_shufflevector(z, z, 4, 4, 4, 4, 4, 4, 4, 4) * z;
    acc[5] += __builtin_shufflevector(z, z, 5, 5, 5, 5, 5, 5, 5, 5) * z;
    acc[6] += __builtin_shufflevector(z, z, 6, 6, 6, 6, 6, 6, 6, 6) * z;
    acc[7] += __builtin_shufflevector(z, z, 7, 7, 7, 7, 7, 7, 7, 7) * z;
    acc[8] += bc(z8) * z;
    acc88 += z8 * z8;
  }
  int q = 0;
  for (int r = 0; r < 9; r++)
    for (int c = 0; c <= r; c++) acc45[q++] = c < 8 ? acc[r][c] : acc88;
}
#else
void cov_fm_all(const double *u, const int *inl, const double *w, int len, const double *A1, const double *A2, double *acc45) {
  constexpr int NV = (9 + VW - 1) / VW;          // vectors per padded row of z
  V acc[9][NV];
  for (int r = 0; r < 9; r++) for (int v = 0; v < NV; v++) acc[r][v] = bc(0.0);
  double zp[NV * VW];
  for (int q = 9; q < NV * VW; q++) zp[q] = 0.0;
  double a[3], b[3];
  a[2] = 1; b[2] = 1;
  for (int i = 0; i < len; i++) {
    const double *s = u + 6 * inl[i];
    a[0] = s[0] * A1[0] + A1[1];
    a[1] = s[1] * A1[0] + A1[2];
    b[0] = s[3] * A2[0] + A2[1];
    b[1] = s[4] * A2[0] + A2[2];
    for (int k = 0; k < 3; k++)
      for (int l = 0; l < 3; l++) zp[3 * k + l] = a[l] * b[k];
    if (w) {
      const double m = w[inl[i]];
      for (int k = 0; k < 9; k++) zp[k] *= m;
    }
    V zv[NV];
    for (int v = 0; v < NV; v++) zv[v] = ld(zp + v * VW);
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const V zr = bc(zp[r]);
#pragma unroll
      for (int v = 0; v <= r / VW; v++) acc[r][v] += zr * zv[v];
    }
  }
  int q = 0;
  for (int r = 0; r < 9; r++)
    for (int c = 0; c <= r; c++) acc45[q++] = acc[r][c / VW][c % VW];
}
#endif
}}}  // namespace mods::rs::NS
