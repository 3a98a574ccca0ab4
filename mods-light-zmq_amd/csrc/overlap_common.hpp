// What the two overlap searches (overlap.hip: the linearised error, overlap_area.hip: intersection over union) share: the 48-byte
// fp64 record of a region, the query record of their contracts (include/mods_hip.h: mods_match_overlap) and the common-area test.
// One rounding per operation in the order the contract writes them.
#pragma once
#include "common.hpp"

namespace mods {

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

}  // namespace mods
