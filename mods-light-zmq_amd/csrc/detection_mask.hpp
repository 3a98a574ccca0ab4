// Detection masks (mods_ctx_detection_mask*): the on-mask rule, the centre a finished region carries, and what the gate kernel
// (detect.hip: detection_mask_kernel) is handed.  "Mask" alone means other things in this code base (the NMS ballot words, the
// descriptor's circular weight, bit masks): everything here is named detection_mask / gate.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>

namespace mods {

// The rule, once, for the host (mods_detection_mask_test) and the device: ix = (int)floor(x + 0.5), iy likewise, on the mask iff
// 0 <= ix < w, 0 <= iy < h and mask[iy * stride + ix] != 0.  The comparisons are made on the floored doubles, so a coordinate no
// int holds (or a NaN) is off the mask instead of undefined.
__host__ __device__ inline bool detection_mask_on(const unsigned char *mask, int w, int h, int stride, double x, double y) {
  const double fx = floor(x + 0.5), fy = floor(y + 0.5);
  if (!(fx >= 0.0 && fx < (double)w && fy >= 0.0 && fy < (double)h)) return false;
  return mask[(size_t)(int)fy * (size_t)stride + (size_t)(int)fx] != 0;
}

// Centre of a view-frame point in the original image: the affine part of inv(H) (row-major 2 x 3) as ReprojectByH applies it.
// reproject_regions_kernel (describe.hip) and the gate both take the centre from here, so that the gate tests the very doubles
// the finished region will carry.
__device__ __forceinline__ void reproject_centre(const double *Hinv, double x, double y, double *ox, double *oy) {
  *ox = (Hinv[0] * x + Hinv[1] * y + Hinv[2]);
  *oy = (Hinv[3] * x + Hinv[4] * y + Hinv[5]);
}

// One image slot's mask as the gate reads it; mask == nullptr: the slot has none
struct DetMaskDev {
  const unsigned char *mask;
  int w, h, stride, pad;
};
inline bool operator==(const DetMaskDev &a, const DetMaskDev &b) { return a.mask == b.mask && a.w == b.w && a.h == b.h && a.stride == b.stride; }

// The frame a call's masks live in: the image itself, or - for a synthesised view - the original image, reached through Hinv
struct DetGateFrame {
  int ow, oh;
  double Hinv[6];
};

struct DetGateConst {
  const DetMaskDev *tab;   // [n_img]
  int *counts;             // [n_img][2]: entries that reached the gate, entries it kept
  double Hinv[6];
  int max_cand;            // stride of the lists
};

}  // namespace mods
