// What the two overlap searches (overlap.hip: the linearised error, overlap_area.hip: intersection over union) share: the 48-byte
// fp64 record of a region, the query record of their contracts (include/mods_hip.h: mods_match_overlap) and the common-area test.
// One rounding per operation in the order the contract writes them.  Then what they do alike around their sweeps: the pack of a
// list into records, the one-to-one rule, the answer for empty lists, the check of the parameters they both take and the counts
// they both report.  The shape of a search of two lists and its compaction are in list_search.hpp.
#pragma once
#include "list_search.hpp"
#include <cmath>

namespace mods {

// the geometry of a pair of images: the parameters both searches take
struct OvGeom {
  double H[9], Hinv[9];   // row-major; Hinv = adjugate / determinant
  int area;               // the common-area test runs (all four sizes > 0)
  double w1, h1, w2, h2;
};

// query: px py C11 C12 C21 C22     train: x2 y2 and its frame (overlap.hip: the inverse, overlap_area.hip: the frame itself)
struct OvRec { double a, b, m11, m12, m21, m22; };
static_assert(sizeof(OvRec) == 48, "overlap record");

// a record that matches nothing: every comparison with it fails
__device__ __forceinline__ OvRec overlap_nan_rec() {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  OvRec r; r.a = r.b = r.m11 = r.m12 = r.m21 = r.m22 = nan;
  return r;
}

// x, y and B = (3.0 * s) * A of a region
__device__ __forceinline__ OvRec overlap_frame(const mods_region &reg) {
  const double ks = 3.0 * reg.s;
  OvRec r;
  r.a = reg.x; r.b = reg.y;
  r.m11 = ks * reg.a11; r.m12 = ks * reg.a12; r.m21 = ks * reg.a21; r.m22 = ks * reg.a22;
  return r;
}

// the query record of a region of image 1 with the frame f: the projected centre and C = linH(x) * B
__device__ __forceinline__ OvRec overlap_query_rec(const double *H, const OvRec &f) {
  const double x = f.a, y = f.b;
  const double X = (H[0] * x + H[1] * y) + H[2];
  const double Y = (H[3] * x + H[4] * y) + H[5];
  const double den = (H[6] * x + H[7] * y) + H[8];
  const double px = X / den, py = Y / den;
  const double den2 = den * den;
  const double n1 = X / den2, n2 = Y / den2;
  const double L11 = H[0] / den - n1 * H[6], L12 = H[1] / den - n1 * H[7];
  const double L21 = H[3] / den - n2 * H[6], L22 = H[4] / den - n2 * H[7];
  OvRec r;
  r.a = px; r.b = py;
  r.m11 = L11 * f.m11 + L12 * f.m21; r.m12 = L11 * f.m12 + L12 * f.m22;
  r.m21 = L21 * f.m11 + L22 * f.m21; r.m22 = L21 * f.m12 + L22 * f.m22;
  return r;
}

// The common-area test: a query's projected centre strictly inside image 2, a train's centre sent back with G = Hinv strictly
// inside image 1
__device__ __forceinline__ bool overlap_in_image(double px, double py, double w, double h) { return 0. < px && px < w && 0. < py && py < h; }
__device__ __forceinline__ bool overlap_maps_into(const double *G, double x, double y, double w, double h) {
  const double X = (G[0] * x + G[1] * y) + G[2];
  const double Y = (G[3] * x + G[4] * y) + G[5];
  const double W = (G[6] * x + G[7] * y) + G[8];
  return overlap_in_image(X / W, Y / W, w, h);
}

// One list, a thread per region.  cnt[is_train] += the regions of the list that take part (all of them without the area test).
// A region outside the common area gets a record of NaNs.  A train's record holds its frame or (INVERSE_TRAIN) the frame's inverse
template <bool INVERSE_TRAIN>
__global__ __launch_bounds__(LS_THREADS) void overlap_pack_kernel(OvGeom g, const mods_region *__restrict__ reg, int n, int is_train,
                                                                  OvRec *__restrict__ rec, int *__restrict__ cnt) {
  const int i = blockIdx.x * LS_THREADS + threadIdx.x;
  bool part = false;
  if (i < n) {
    OvRec r = overlap_frame(reg[i]);
    if (!is_train) {
      r = overlap_query_rec(g.H, r);
      part = !g.area || overlap_in_image(r.a, r.b, g.w2, g.h2);
    } else {
      part = !g.area || overlap_maps_into(g.Hinv, r.a, r.b, g.w1, g.h1);
      if (INVERSE_TRAIN) {
        const OvRec f = r;
        const double d = 1.0 / (f.m11 * f.m22 - f.m12 * f.m21);
        r.m11 = f.m22 * d; r.m12 = -(f.m12 * d); r.m21 = -(f.m21 * d); r.m22 = f.m11 * d;
      }
    }
    rec[i] = part ? r : overlap_nan_rec();
  }
  const int c = __syncthreads_count(part ? 1 : 0);
  if (threadIdx.x == 0 && c) atomicAdd(&cnt[is_train], c);
}
template <bool INVERSE_TRAIN>
inline void overlap_pack(mods_ctx *c, const OvGeom &g, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, OvRec *rec, int *cnt) {
  if (n_q)
    hipLaunchKernelGGL((overlap_pack_kernel<INVERSE_TRAIN>), dim3((n_q + LS_THREADS - 1) / LS_THREADS), dim3(LS_THREADS), 0, c->stream, g, q_dev,
                       n_q, 0, rec, cnt);
  if (n_t)
    hipLaunchKernelGGL((overlap_pack_kernel<INVERSE_TRAIN>), dim3((n_t + LS_THREADS - 1) / LS_THREADS), dim3(LS_THREADS), 0, c->stream, g, t_dev,
                       n_t, 1, rec + n_q, cnt);
}

// The one-to-one rule.  The accept kernel of a search leaves best_e / best_t[q] = the query's error bits and train (-1: none) and
// takes atomicMin(&train_e[t], e); here, of the queries with that error on the train, the lowest index owns it
static __global__ __launch_bounds__(LS_THREADS) void overlap_owner_kernel(int n_q, const unsigned long long *__restrict__ best_e,
                                                                         const int *__restrict__ best_t,
                                                                         const unsigned long long *__restrict__ train_e,
                                                                         int *__restrict__ train_q) {
  const int q = blockIdx.x * LS_THREADS + threadIdx.x;
  if (q >= n_q) return;
  const int t = best_t[q];
  if (t >= 0 && train_e[t] == best_e[q]) atomicMin(&train_q[t], q);
}
// ... and what the two atomicMin start from: no error on a train, no owner
inline hipError_t overlap_owner_reset(mods_ctx *c, unsigned long long *train_e, int *train_q, size_t n_t) {
  const hipError_t e = hipMemsetAsync(train_e, 0xff, sizeof(unsigned long long) * n_t, c->stream);
  return e != hipSuccess ? e : hipMemsetAsync(train_q, 0x7f, sizeof(int) * n_t, c->stream);
}

// nothing to match (an empty list on either side, or no pair to evaluate): no match, the common counts stand
static __global__ void overlap_empty_kernel(const int *__restrict__ cnt, int *__restrict__ counts_out) {
  counts_out[0] = 0; counts_out[1] = cnt[0]; counts_out[2] = cnt[1];
}

// Every refusal of the parameters that needs no device, in the order of the contracts: a null struct, H not finite, what `own`
// refuses of the search's own parameters (it has set the error and returns the code), the image sizes, a singular H.  `who`
// starts every message.  Fills *g
template <class Par, class Own> inline int overlap_check_geom(const char *who, const Par *par, Own own, OvGeom *g) {
  if (!par) { set_error("%s: null argument", who); return MODS_E_ARG; }
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(par->H[i])) { set_error("%s: H entry %d is not finite", who, i); return MODS_E_ARG; }
  if (const int rc = own()) return rc;
  if (par->w1 < 0 || par->h1 < 0 || par->w2 < 0 || par->h2 < 0) {
    set_error("%s: negative image size (%d x %d, %d x %d)", who, par->w1, par->h1, par->w2, par->h2);
    return MODS_E_ARG;
  }
  double d;
  if (!invert3_adjugate(par->H, g->Hinv, &d)) { set_error("%s: singular homography (determinant %g)", who, d); return MODS_E_ARG; }
  for (int i = 0; i < 9; i++) g->H[i] = par->H[i];
  g->area = par->w1 > 0 && par->h1 > 0 && par->w2 > 0 && par->h2 > 0;
  g->w1 = (double)par->w1; g->h1 = (double)par->h1; g->w2 = (double)par->w2; g->h2 = (double)par->h2;
  return MODS_OK;
}

// the refusals that concern the output, behind those of the parameters
inline int overlap_check_out(const char *who, const void *out, int max_out, const int *n_out, const mods_overlap_counts *counts) {
  if (!n_out || !counts || max_out < 0 || (max_out > 0 && !out)) { set_error("%s: null argument", who); return MODS_E_ARG; }
  return MODS_OK;
}

// the counts of a finished search: n matches next to the common counts of the pinned slots (valid after a stream wait)
inline void overlap_fill_counts(const int *slots, int n, mods_overlap_counts *counts) {
  counts->n_q_common = read_slot(slots, 1);
  counts->n_t_common = read_slot(slots, 2);
  counts->n_matches = n;
  const int lo = std::min(counts->n_q_common, counts->n_t_common);
  counts->repeatability = lo > 0 ? (double)n / (double)lo : 0.;
}

}  // namespace mods
