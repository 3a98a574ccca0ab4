// ORSA-H, the a-contrario homography verifier (Moisan, Moulon, Monasse, IPOL 2012; the contract is include/mods_hip.h's, parity
// with the IPOL code unpinned): what the host and the device share, and the host scalar path that is the device's oracle.
//
//  - solve_h4: the minimal solve, one __host__ __device__ function so that both paths run the same operations;
//  - h_error: the transfer error of one correspondence, whose float bits are the sort key;
//  - the tables, the normalisation, the mapping of 4 raw rand() values to 4 distinct indices;
//  - score_host: errors, sort, NFA scan of one model, and sorted_prefix: the record's subset.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "orsa_host.hpp"

#if defined(__HIPCC__)
#define ORSA_HD __host__ __device__
#else
#define ORSA_HD
#endif

namespace mods {
namespace orsa_h {

// The homography through 4 correspondences c = 4 x (x1, y1, x2, y2), image 1 to image 2, h33 = 1: the 8 x 8 system in fp64,
// Gaussian elimination with partial pivoting (the first largest magnitude of a column wins), fixed operation order, contraction
// off, the result rounded to 9 floats.  false (H all zero) on a zero or NaN pivot or a non-finite entry.
ORSA_HD inline bool solve_h4(const float c[16], float H[9]) {
#pragma clang fp contract(off)
  double A[8][9];
  for (int i = 0; i < 4; i++) {
    const double x = c[4 * i], y = c[4 * i + 1], u = c[4 * i + 2], v = c[4 * i + 3];
    double *r0 = A[2 * i], *r1 = A[2 * i + 1];
    r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -u * x; r0[7] = -u * y; r0[8] = u;
    r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x; r1[4] = y; r1[5] = 1.0; r1[6] = -v * x; r1[7] = -v * y; r1[8] = v;
  }
  for (int q = 0; q < 9; q++) H[q] = 0.0f;
  for (int k = 0; k < 8; k++) {
    int p = k;
    double best = A[k][k] < 0 ? -A[k][k] : A[k][k];
    for (int r = k + 1; r < 8; r++) {
      const double a = A[r][k] < 0 ? -A[r][k] : A[r][k];
      if (a > best) { best = a; p = r; }
    }
    if (!(best > 0.0)) return false;
    if (p != k)
      for (int j = 0; j < 9; j++) { const double t = A[k][j]; A[k][j] = A[p][j]; A[p][j] = t; }
    for (int r = k + 1; r < 8; r++) {
      const double f = A[r][k] / A[k][k];
      for (int j = k + 1; j < 9; j++) A[r][j] = A[r][j] - f * A[k][j];
    }
  }
  double x[8];
  for (int k = 7; k >= 0; k--) {
    double s = A[k][8];
    for (int j = k + 1; j < 8; j++) s = s - A[k][j] * x[j];
    x[k] = s / A[k][k];
  }
  float h[9];
  for (int q = 0; q < 8; q++) {
    h[q] = (float)x[q];
    if (!((h[q] < 0 ? -h[q] : h[q]) <= FLT_MAX)) return false;
  }
  h[8] = 1.0f;
  for (int q = 0; q < 9; q++) H[q] = h[q];
  return true;
}

// the squared distance in image 2 between H p1 (after the projective division) and p2, in double from the float operands,
// rounded to float
ORSA_HD inline float h_error(const float *H, float x1f, float y1f, float x2f, float y2f) {
#pragma clang fp contract(off)
  const double x1 = x1f, y1 = y1f, x2 = x2f, y2 = y2f;
  const double H11 = H[0], H12 = H[1], H13 = H[2], H21 = H[3], H22 = H[4], H23 = H[5], H31 = H[6], H32 = H[7], H33 = H[8];
  const double w = H31 * x1 + H32 * y1 + H33;
  const double X = (H11 * x1 + H12 * y1 + H13) / w;
  const double Y = (H21 * x1 + H22 * y1 + H23) / w;
  const double dx = X - x2, dy = Y - y2;
  return (float)(dx * dx + dy * dy);
}

struct Problem {
  int n = 0;
  float nx = 0, ny = 0, norm = 0, logalpha0 = 0, loge0 = 0;
  std::vector<float> p1, p2, logcn, logc4;   // normalised x, y interleaved (p1: image 1, p2: image 2); tables of n + 1 entries
};

// logcn[k] = logcombi(k, n), logc4[m] = logcombi(4, m), n + 1 entries each.  logcombi(k, n) sums log10(n - i + 1) - log10(i) over
// i = 1 .. min(k, n - k) in that order, so the whole first table is the running sums of one pass: the same additions in the same
// order, the same bits, n terms instead of n^2 / 4 (17 of the 20 ms of a 3000-tentative call otherwise)
static inline void tables(int n, std::vector<float> &logcn, std::vector<float> &logc4) {
  logcn.assign(n + 1, 0.0f);
  logc4.resize(n + 1);
  std::vector<double> run(n / 2 + 1, 0.0);
  double r = 0.;
  for (int i = 1; i <= n / 2; i++) { r += log10((double)(n - i + 1)) - log10((double)i); run[i] = r; }
  for (int k = 1; k < n; k++) logcn[k] = (float)run[n - k < k ? n - k : k];
  for (int m = 0; m <= n; m++) logc4[m] = orsa::logcombi(4, m);
}

// as orsa::setup: norm = 1 / (float)sqrt(nx ny), points centred by half the size and scaled; the normalised image has area 1, so
// the probability of a point error below sqrt(e) is pi e: logalpha0 = log10(pi) and the log of e enters with multiplier 1
static inline void setup(Problem &P, int width, int height, bool normalise = true) {
  const int n = P.n;
  P.loge0 = (float)log10((double)(n - 4));
  tables(n, P.logcn, P.logc4);
  P.nx = (float)width;
  P.ny = (float)height;
  P.norm = 1. / (float)sqrt((double)(P.nx * P.ny));
  P.logalpha0 = (float)log10(M_PI);
  if (!normalise) return;
  for (int i = 0; i < n; i++) {
    P.p1[i * 2] = (P.p1[i * 2] - 0.5 * P.nx) * P.norm;
    P.p1[i * 2 + 1] = (P.p1[i * 2 + 1] - 0.5 * P.ny) * P.norm;
    P.p2[i * 2] = (P.p2[i * 2] - 0.5 * P.nx) * P.norm;
    P.p2[i * 2 + 1] = (P.p2[i * 2 + 1] - 0.5 * P.ny) * P.norm;
  }
}

// 4 rand() values to 4 distinct indices below n, kept sorted, the way orsa::map_p7 maps 7
static inline void map_p4(const int32_t *raw, int n, int *k) {
  for (int i = 0; i < 4; i++) {
    int r = (raw[i] >> 3) % (n - i), j;
    for (j = 0; j < i && r >= k[j]; j++) r++;
    const int j0 = j;
    for (j = i; j > j0; j--) k[j] = k[j - 1];
    k[j0] = r;
  }
}

static inline void gather4(const Problem &P, const int *idx, float c[16]) {
  for (int i = 0; i < 4; i++) {
    c[4 * i] = P.p1[2 * idx[i]]; c[4 * i + 1] = P.p1[2 * idx[i] + 1];
    c[4 * i + 2] = P.p2[2 * idx[i]]; c[4 * i + 3] = P.p2[2 * idx[i] + 1];
  }
}

// the NFA term of sorted position i >= 4, all in float
static inline float nfa_term(const Problem &P, float e_i, int i, float *logalpha) {
  const float la = P.logalpha0 + orsa::log10_ref(e_i < FLT_MIN ? FLT_MIN : e_i);
  *logalpha = la;
  return P.loge0 + la * (float)(i - 3) + P.logcn[i + 1] + P.logc4[i + 1];
}

// errors of all correspondences under H; false when one is NaN
static inline bool errors(const float H[9], const Problem &P, float *e) {
  bool ok = true;
  for (int i = 0; i < P.n; i++) {
    e[i] = h_error(H, P.p1[2 * i], P.p1[2 * i + 1], P.p2[2 * i], P.p2[2 * i + 1]);
    if (e[i] != e[i]) ok = false;
  }
  return ok;
}

// one model on the host: nan = 1 marks an invalid model (a failed solve or a NaN error), which scores nfa = 10000, imin = 0
static inline orsa::Score score_host(const float H[9], bool valid, const Problem &P, float *e) {
  orsa::Score s = {10000.f, 0, 10000.f, 0};
  if (!valid || !errors(H, P, e)) { s.nan = 1; return s; }
  std::sort(e, e + P.n);
  for (int i = 4; i < P.n; i++) {
    float la;
    const float nfa = nfa_term(P, e[i], i, &la);
    if (nfa < s.nfa) { s.nfa = nfa; s.imin = i; s.logalpha = la; }
  }
  return s;
}

// the first count indices of the errors under H sorted stably by (error, index); *e_last = the error of the last of them
static inline void sorted_prefix(const float H[9], const Problem &P, int count, std::vector<int> &idx, float *e_last) {
  std::vector<float> e(P.n);
  errors(H, P, e.data());
  std::vector<int> order(P.n);
  for (int i = 0; i < P.n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return e[a] < e[b]; });
  idx.assign(order.begin(), order.begin() + count);
  *e_last = e[order[count - 1]];
}

}  // namespace orsa_h
}  // namespace mods
