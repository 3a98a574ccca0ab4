// Host half of ORSA, the a-contrario fundamental-matrix verifier (orsa.cpp:95-678, matching.cpp:824-914): what the device does
// not do, restated so that every bit the reference computes is reproduced.
//
//  - the 7-point solve: epipolar() takes columns 8 and 7 of V of JacobiSVD<MatrixXf>(c, ComputeFullV) of the 7 x 9 design matrix.
//    For 7 x 9 inputs those two columns are never touched by the Jacobi sweeps or the final sort (both only rotate / permute the
//    first 7 columns): they are columns 8 and 7 of householderQ() of the ColPivHouseholderQR of (c / max|c|)^T, 9 x 7, that
//    JacobiSVD runs as its preconditioner.  That QR and Q are restated below with Eigen 3.3's operation order for the reference's
//    build (SSE2 packets of 4 floats, no FMA contraction): the reductions of squaredNorm (two packet accumulators, predux, then the
//    unaligned head and tail) and the row-major GEMV kernel behind essential^T * bottom (packet lanes over the aligned part of the
//    vector, a scalar head and tail) depend on where each column segment starts relative to a 16-byte boundary.  Both matrices
//    are freshly allocated, hence 16-byte aligned, and have 9 rows, so the alignment of every segment follows from its offset.
//  - the cubic det(F1 + z F2) = 0 in float and FindCubicRoots in double (mixed float steps kept where the reference has them);
//  - the logcombi tables, the normalisation, glibc's generator and random_p7's mapping of raw values to indices;
//  - the scalar scoring of one model (matcherrorn + qsort + NFA scan): the oracle of the device kernel, and the path for models
//    whose errors hold a NaN (compf is then not a strict weak order and only glibc's own qsort says what comes out).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "ransac_host.hpp"

namespace mods {
namespace orsa {

// ---- Eigen 3.3 ColPivHouseholderQR + householderQ of a 9 x 7 float matrix, columns 7 and 8 of Q --------------------------------

// first_default_aligned for a float segment starting at element offset `off` of a 16-byte aligned buffer
static inline int first_aligned(int off, int size) {
  const int first = (4 - (off & 3)) & 3;
  return first < size ? first : size;
}
static inline float predux4(const float p[4]) { return (p[0] + p[2]) + (p[1] + p[3]); }

// redux_impl<sum, LinearVectorizedTraversal> over v[i]^2, v = base + off, size elements.  The expression it reduces (the squares)
// has no direct access, so first_default_aligned() is 0 whatever the segment's address: unaligned packets from element 0.
static inline float eig_sqnorm(const float *base, int off, int size) {
  const float *v = base + off;
  const int as = 0;
  const int asz2 = ((size - as) / 8) * 8, asz = ((size - as) / 4) * 4;
  const int ae2 = as + asz2, ae = as + asz;
  float res;
  if (asz) {
    float p0[4], p1[4];
    for (int q = 0; q < 4; q++) p0[q] = v[as + q] * v[as + q];
    if (asz > 4) {
      for (int q = 0; q < 4; q++) p1[q] = v[as + 4 + q] * v[as + 4 + q];
      for (int i = as + 8; i < ae2; i += 8)
        for (int q = 0; q < 4; q++) { p0[q] = p0[q] + v[i + q] * v[i + q]; p1[q] = p1[q] + v[i + 4 + q] * v[i + 4 + q]; }
      for (int q = 0; q < 4; q++) p0[q] = p0[q] + p1[q];
      if (ae > ae2) for (int q = 0; q < 4; q++) p0[q] = p0[q] + v[ae2 + q] * v[ae2 + q];
    }
    res = predux4(p0);
    for (int i = 0; i < as; i++) res = res + v[i] * v[i];
    for (int i = ae; i < size; i++) res = res + v[i] * v[i];
  } else {
    res = v[0] * v[0];
    for (int i = 1; i < size; i++) res = res + v[i] * v[i];
  }
  return res;
}

// general_matrix_vector_product<RowMajor>: out[c] = sum_j L[lofs + 9 c + j] * R[rofs + j], c < rows, j < depth
static inline void eig_gemv_t(const float *L, int lofs, int rows, int depth, const float *R, int rofs, float *out) {
  int as = first_aligned(rofs, depth);
  int asz = as + ((depth - as) & ~3);
  const int lhs_off = first_aligned(lofs, depth), rhs_off = first_aligned(rofs, rows);
  if (lhs_off == depth || rhs_off == rows) { as = 0; asz = 0; }
  for (int c = 0; c < rows; c++) {
    const float *l = L + lofs + 9 * c, *r = R + rofs;
    float t = 0.0f;
    for (int j = 0; j < as; j++) t += l[j] * r[j];
    if (asz > as) {
      float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int j = as; j < asz; j += 4)
        for (int q = 0; q < 4; q++) p[q] = l[j + q] * r[j + q] + p[q];
      t += predux4(p);
    }
    for (int j = asz; j < depth; j++) t += l[j] * r[j];
    out[c] = 0.0f + 1.0f * t;
  }
}

// MatrixBase::applyHouseholderOnTheLeft on the block of M (9 rows, column-major) with top-left (r0, c0), nr x nc, essential
// vector at E + eofs (nr - 1 entries), tau
static inline void eig_house_left(float *M, int r0, int c0, int nr, int nc, const float *E, int eofs, float tau) {
  if (nr == 1) {
    for (int c = 0; c < nc; c++) M[9 * (c0 + c) + r0] *= 1.0f - tau;
    return;
  }
  if (tau == 0.0f) return;
  float tmp[9];
  eig_gemv_t(M, 9 * c0 + r0 + 1, nc, nr - 1, E, eofs, tmp);
  for (int c = 0; c < nc; c++) tmp[c] += M[9 * (c0 + c) + r0];
  for (int c = 0; c < nc; c++) M[9 * (c0 + c) + r0] -= tau * tmp[c];
  float te[9];
  for (int i = 0; i < nr - 1; i++) te[i] = tau * E[eofs + i];
  for (int c = 0; c < nc; c++)
    for (int i = 0; i < nr - 1; i++) M[9 * (c0 + c) + r0 + 1 + i] -= tmp[c] * te[i];
}

static inline int find_cubic_roots(const float coeff[4], float x[3]) {   // orsa.cpp:95-127
  const float a1 = coeff[2] / coeff[3];
  const float a2 = coeff[1] / coeff[3];
  const float a3 = coeff[0] / coeff[3];
  const double Q = (a1 * a1 - 3 * a2) / 9;
  const double R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) / 54;
  const double Qcubed = Q * Q * Q;
  const double d = Qcubed - R * R;
  if (d >= 0) {
    const double theta = acos(R / sqrt(Qcubed));
    const double sqrtQ = sqrt(Q);
    x[0] = -2 * sqrtQ * cos(theta / 3) - a1 / 3;
    x[1] = -2 * sqrtQ * cos((theta + 2 * M_PI) / 3) - a1 / 3;
    x[2] = -2 * sqrtQ * cos((theta + 4 * M_PI) / 3) - a1 / 3;
    return 3;
  }
  double e = pow(sqrt(-d) + fabs(R), 1. / 3.);
  if (R > 0) e = -e;
  x[0] = (e + Q / e) - a1 / 3.;
  return 1;
}

// columns 8 and 7 of V of JacobiSVD<MatrixXf>(c, ComputeFullV), c 7 x 9 given row by row
static inline void null_basis_7x9(const float c[63], float F1v[9], float F2v[9]) {
  float scale = 0.0f;
  for (int i = 0; i < 63; i++) { const float a = std::fabs(c[i]); if (a > scale) scale = a; }
  if (scale == 0.0f) scale = 1.0f;
  float A[63];   // 9 x 7 column-major: A(r, k) = c(k, r) / scale
  for (int k = 0; k < 7; k++)
    for (int r = 0; r < 9; r++) A[9 * k + r] = c[9 * k + r] / scale;
  float tau[7], nUpd[7], nDir[7];
  for (int k = 0; k < 7; k++) { nDir[k] = std::sqrt(eig_sqnorm(A, 9 * k, 9)); nUpd[k] = nDir[k]; }
  const float thr = std::sqrt(1.1920928955078125e-07f);
  for (int k = 0; k < 7; k++) {
    int big = k;
    float bv = nUpd[k];
    for (int j = k + 1; j < 7; j++) if (nUpd[j] > bv) { bv = nUpd[j]; big = j; }
    if (big != k) {
      for (int r = 0; r < 9; r++) { const float t = A[9 * k + r]; A[9 * k + r] = A[9 * big + r]; A[9 * big + r] = t; }
      float t = nUpd[k]; nUpd[k] = nUpd[big]; nUpd[big] = t;
      t = nDir[k]; nDir[k] = nDir[big]; nDir[big] = t;
    }
    // makeHouseholderInPlace on A(k.., k)
    const int off = 9 * k + k, tl = 8 - k;
    const float tailSq = tl == 0 ? 0.0f : eig_sqnorm(A, off + 1, tl);
    const float c0 = A[off];
    float beta;
    if (tailSq <= 1.17549435e-38f) {
      tau[k] = 0.0f; beta = c0;
      for (int i = 0; i < tl; i++) A[off + 1 + i] = 0.0f;
    } else {
      beta = std::sqrt(c0 * c0 + tailSq);
      if (c0 >= 0.0f) beta = -beta;
      const float den = c0 - beta;
      for (int i = 0; i < tl; i++) A[off + 1 + i] = A[off + 1 + i] / den;
      tau[k] = (beta - c0) / beta;
    }
    A[off] = beta;
    eig_house_left(A, k, k + 1, 9 - k, 6 - k, A, off + 1, tau[k]);
    for (int j = k + 1; j < 7; j++) {
      if (nUpd[j] != 0.0f) {
        float t = std::fabs(A[9 * j + k]) / nUpd[j];
        t = (1.0f + t) * (1.0f - t);
        t = t < 0 ? 0.0f : t;
        const float q = nUpd[j] / nDir[j];
        const float t2 = t * (q * q);
        if (t2 <= thr) {
          nDir[j] = std::sqrt(eig_sqnorm(A, 9 * j + k + 1, 8 - k));
          nUpd[j] = nDir[j];
        } else {
          nUpd[j] *= std::sqrt(t);
        }
      }
    }
  }
  float V[81];   // householderQ().evalTo: identity, then H_6 ... H_0 from the left on the bottom-right corners
  for (int i = 0; i < 81; i++) V[i] = 0.0f;
  for (int i = 0; i < 9; i++) V[10 * i] = 1.0f;
  for (int k = 6; k >= 0; k--) eig_house_left(V, k, k, 9 - k, 9 - k, A, 9 * k + k + 1, tau[k]);
  for (int i = 0; i < 9; i++) { F1v[i] = V[72 + i]; F2v[i] = V[63 + i]; }
}

// epipolar() (orsa.cpp:281-348): F1, F2 row-major 3 x 3 (the reference's F[i][j] at (i-1)*3 + j-1); returns the number of real
// roots z[]
static inline int epipolar(const float *m1, const float *m2, const int *k, float z[3], float F1[9], float F2[9]) {
  float c[63];   // row i of the 7 x 9 design matrix at 9 i (= column i of its transpose, the matrix the QR factors)
  for (int i = 0; i < 7; i++) {
    const float x1 = m1[k[i] * 2], y1 = m1[k[i] * 2 + 1], x2 = m2[k[i] * 2], y2 = m2[k[i] * 2 + 1];
    const float row[9] = {x1 * x2, y1 * x2, x2, x1 * y2, y1 * y2, y2, x1, y1, 1.0f};
    for (int j = 0; j < 9; j++) c[9 * i + j] = row[j];
  }
  null_basis_7x9(c, F1, F2);
  float a[4] = {0, 0, 0, 0};
#define F1_(i, j) F1[((i) - 1) * 3 + (j) - 1]
#define F2_(i, j) F2[((i) - 1) * 3 + (j) - 1]
  for (int i = 1; i <= 3; i++) {
    const int i2 = i % 3 + 1, i3 = i2 % 3 + 1;
    a[0] += F1_(i, 1) * F1_(i2, 2) * F1_(i3, 3);
    a[1] += F2_(i, 1) * F1_(i2, 2) * F1_(i3, 3) + F1_(i, 1) * F2_(i2, 2) * F1_(i3, 3) + F1_(i, 1) * F1_(i2, 2) * F2_(i3, 3);
    a[2] += F1_(i, 1) * F2_(i2, 2) * F2_(i3, 3) + F2_(i, 1) * F1_(i2, 2) * F2_(i3, 3) + F2_(i, 1) * F2_(i2, 2) * F1_(i3, 3);
    a[3] += F2_(i, 1) * F2_(i2, 2) * F2_(i3, 3);
  }
  for (int i = 1; i <= 3; i++) {
    const int i2 = (i + 1) % 3 + 1, i3 = (i2 + 1) % 3 + 1;
    a[0] -= F1_(i, 1) * F1_(i2, 2) * F1_(i3, 3);
    a[1] -= F2_(i, 1) * F1_(i2, 2) * F1_(i3, 3) + F1_(i, 1) * F2_(i2, 2) * F1_(i3, 3) + F1_(i, 1) * F1_(i2, 2) * F2_(i3, 3);
    a[2] -= F1_(i, 1) * F2_(i2, 2) * F2_(i3, 3) + F2_(i, 1) * F1_(i2, 2) * F2_(i3, 3) + F2_(i, 1) * F2_(i2, 2) * F1_(i3, 3);
    a[3] -= F2_(i, 1) * F2_(i2, 2) * F2_(i3, 3);
  }
#undef F1_
#undef F2_
  return find_cubic_roots(a, z);
}

// ---- tables, normalisation, sampling ------------------------------------------------------------------------------------

static inline float logcombi(int k, int n) {   // orsa.cpp:131-143
  if (k >= n || k <= 0) return 0.;
  if (n - k < k) k = n - k;
  double r = 0.;
  for (int i = 1; i <= k; i++) r += log10((double)(n - i + 1)) - log10((double)i);
  return (float)r;
}

static inline float log10_ref(float e) { return (float)log10((double)e); }   // the rounding the NFA scan takes

// everything orsa() derives from (w, h, the points) before its main loop; p1 = the second image's points, p2 = the first's
struct Problem {
  int n = 0;
  float nx = 0, ny = 0, norm = 0, logalpha0 = 0, loge0 = 0;
  std::vector<float> p1, p2, logcn, logc7;   // normalised coordinates x, y interleaved; tables of n + 1 entries
};

static inline void setup(Problem &P, int width, int height) {   // orsa.cpp:464-517
  const int n = P.n;
  P.loge0 = (float)log10(3. * (double)(n - 7));
  P.logcn.resize(n + 1);
  P.logc7.resize(n + 1);
  for (int k = 0; k <= n; k++) P.logcn[k] = logcombi(k, n);
  for (int m = 0; m <= n; m++) P.logc7[m] = logcombi(7, m);
  P.nx = (float)width;
  P.ny = (float)height;
  P.norm = 1. / (float)sqrt((double)(P.nx * P.ny));
  P.logalpha0 = (float)(log10(2.) + 0.5 * log10((double)((P.nx * P.nx + P.ny * P.ny) * P.norm * P.norm)));
  for (int i = 0; i < n; i++) {
    P.p1[i * 2] = (P.p1[i * 2] - 0.5 * P.nx) * P.norm;
    P.p1[i * 2 + 1] = (P.p1[i * 2 + 1] - 0.5 * P.ny) * P.norm;
    P.p2[i * 2] = (P.p2[i * 2] - 0.5 * P.nx) * P.norm;
    P.p2[i * 2 + 1] = (P.p2[i * 2 + 1] - 0.5 * P.ny) * P.norm;
  }
}

// random_p7 (orsa.cpp:164-175) with its 7 rand() values given
static inline void map_p7(const int32_t *raw, int n, int *k) {
  for (int i = 0; i < 7; i++) {
    int r = (raw[i] >> 3) % (n - i), j;
    for (j = 0; j < i && r >= k[j]; j++) r++;
    const int j0 = j;
    for (j = i; j > j0; j--) k[j] = k[j - 1];
    k[j0] = r;
  }
}

// ---- scoring of one model on the host -------------------------------------------------------------------------------------

struct Score {
  float nfa;        // minepscur: 10000 when no subset reaches below it
  int imin;         // minicur (valid when nfa < 10000)
  float logalpha;   // minlogalphacur
  int nan;          // 1: an error is NaN (the device hands such models to score_host)
};

static int compf(const void *i, const void *j) {   // orsa.cpp:216-224
  const float a = *((const float *)i), b = *((const float *)j);
  return a < b ? -1 : (a > b ? 1 : 0);
}

// matcherrorn (orsa.cpp:229-274): e[2i] = error, e[2i+1] = (float)i, sorted by glibc's qsort (a stable merge sort for these records)
static inline void errors_sorted(const float F[9], const Problem &P, float *e) {
  const int n = P.n;
  const double F11 = F[0], F12 = F[1], F13 = F[2], F21 = F[3], F22 = F[4], F23 = F[5], F31 = F[6], F32 = F[7], F33 = F[8];
  for (int i = 0; i < n; i++) {
    const double x1 = P.p1[i * 2], y1 = P.p1[i * 2 + 1], x2 = P.p2[i * 2], y2 = P.p2[i * 2 + 1];
    const double rxc = F11 * x2 + F21 * y2 + F31;
    const double ryc = F12 * x2 + F22 * y2 + F32;
    const double rwc = F13 * x2 + F23 * y2 + F33;
    const double r = (rxc * x1 + ryc * y1 + rwc);
    const double rx = F11 * x1 + F12 * y1 + F13;
    const double ry = F21 * x1 + F22 * y1 + F23;
    const double a = rxc * rxc + ryc * ryc;
    const double b = rx * rx + ry * ry;
    e[i * 2] = r * r * (a + b) / (a * b);
    e[i * 2 + 1] = (float)i;
  }
  qsort(e, n, 2 * sizeof(float), compf);
}

// the NFA term of sorted position i (orsa.cpp:588-590)
static inline float nfa_term(const Problem &P, float e_i, int i, float *logalpha) {
  const float la = P.logalpha0 + 0.5 * (float)log10((double)e_i);
  *logalpha = la;
  return P.loge0 + la * (float)(i - 6) + P.logcn[i + 1] + P.logc7[i + 1];
}

static inline Score score_host(const float F[9], const Problem &P, float *e) {
  errors_sorted(F, P, e);
  Score s = {10000.f, 0, 10000.f, 0};
  for (int i = 0; i < P.n; i++) if (e[i * 2] != e[i * 2]) s.nan = 1;
  for (int i = 7; i < P.n; i++) {
    float la;
    const float nfa = nfa_term(P, e[i * 2], i, &la);
    if (nfa < s.nfa) { s.nfa = nfa; s.imin = i; s.logalpha = la; }
  }
  return s;
}

}  // namespace orsa
}  // namespace mods
