// Shared declarations of the orientation / description stage (describe.hip, sift.hip).
#pragma once
#include "common.hpp"

namespace mods {

struct DescConst {
  int w, h;
  int max_cand, max_reg;   // strides of the key / region lists
  int reg_cap;             // regions that can be described per image (patch store capacity)
  double ks;               // synth-detection.cpp:21  k_sigma = 2*3*sqrt(3)
  int ori_ps;
  double ori_i2p;          // imageToPatchScale of DetectOrientation = (2*int(mrSize)+1)/patchSize
  int max_angles;
  int ori_cap;             // oriented copies kept per keypoint: 1, or min(maxAngles, 18) (18 = the most peaks a 36-bin histogram has)
  double ori_th;
  int ori_half;            // doHalfSIFT of EstimateDominantAnglesFunctor
  int add_upright;         // [DominantOrientation] addUpRight: unrotated copies, ahead of the oriented ones
  int half_desc;           // sift_kernel: HalfRootSIFT (64 values) instead of the 128-value descriptor
  double desc_mr;
  int desc_ps;
  int photo, root;
  double max_bin;
  int p2_lo, p2_hi;        // size tier handled by a launch: p2_lo < P2 <= p2_hi (P2 = 0: direct branch)
  size_t scratch_stride;   // floats per block
  int tap_cap;
  // synthesised view (H != I): keypoints live in the view frame; the inside / touch-boundary tests of
  // ReprojectRegions* run on their reprojection into the original image (ow x oh) through Hinv
  int patch_rule;          // size of the sampled region: 0 = DescribeRegions (2*ceil(s*mr)+1, synth-detection.hpp:189),
                           // 1 = ExtractPatchesColumn (the same for odd patch sizes, 2*ceil(s*mr) for even ones, synth-detection.cpp:57),
                           // 2 = the fast branch of DescribeRegions (direct interpolation at (2*int(mr*s)+1)/patchSize, :232-253)
  int view;                // 0: identity view (reproj_kp == det_kp)
  int ow, oh;
  double Hinv[6];          // affine part of inv(H), row-major 2x3
};

struct SiftTab {           // precomputeBinsAndWeights, siftdesc.cpp:22-71 (host built, patchSize <= 64)
  int bin0[64], bin1[64];  // already multiplied by orientationBins
  float w0[64], w1[64];    // stored as double in the reference but float valued
};

// The kernels that gather from the input image (orient_kernel, extract_small_kernel, big_fused_kernel, big_sample_kernel) exist for
// fp32 and for 8-bit pixels.  A call that has the batch as 8-bit grey in HBM as well (mods_detect_describe_dev_u8) samples from that
// copy in the kernels whose switch is 1: the same values from a quarter of the bytes.  Each kernel keeps the form that was faster at
// the benchmark's 32-image batch ("Sampling from the 8-bit twin"; profiles/u8_sampling_*); times per batch:
#ifndef ORIENT_FROM_U8
#define ORIENT_FROM_U8 0          // 1.853 against 1.861 ms, run-to-run deviation 0.067: no gain, stays on fp32
#endif
#ifndef EXTRACT_SMALL_FROM_U8
#define EXTRACT_SMALL_FROM_U8 1   // 3 x 0.985 against 3 x 1.036 ms
#endif
#ifndef BIG_FUSED_FROM_U8
#define BIG_FUSED_FROM_U8 1       // 2.67 against 2.88 ms
#endif
#ifndef BIG_SAMPLE_FROM_U8
#define BIG_SAMPLE_FROM_U8 0      // no region of the benchmark's images reaches this kernel (P2 > 1024): not measured, stays on fp32
#endif
// The strip layout of the twin (u8_strips.hpp) is the third form of each: 1 = the kernel samples from the strips when the call has
// them, whatever its switch above says (the strip columns of the same table; profiles/strip_u8_*).  Times per
// batch against the kernel's form above:
#ifndef ORIENT_FROM_STRIPS
#define ORIENT_FROM_STRIPS 1          // 1.759 against 1.867 ms (fp32)
#endif
#ifndef EXTRACT_SMALL_FROM_STRIPS
#define EXTRACT_SMALL_FROM_STRIPS 1   // 3 x 0.942 against 3 x 0.991 ms (row-major 8-bit)
#endif
#ifndef BIG_FUSED_FROM_STRIPS
#define BIG_FUSED_FROM_STRIPS 1       // 2.36 against 2.68 ms (row-major 8-bit)
#endif
#ifndef BIG_SAMPLE_FROM_STRIPS
#define BIG_SAMPLE_FROM_STRIPS 0      // not measured, as above: stays on fp32
#endif
// the same choice as a mask, and the one a context was given for its calls instead (mods_ctx_u8_kernels: the tests run the forms that
// the defaults leave out)
// bits 4-7: the same kernel samples from the strip twin of the 8-bit images (u8_strips.hpp) when the call has one; it goes before bits 0-3
enum { U8K_ORIENT = 1, U8K_EXTRACT_SMALL = 2, U8K_BIG_FUSED = 4, U8K_BIG_SAMPLE = 8, U8K_STRIPS_SHIFT = 4, U8K_ALL = 255 };
constexpr int kU8KernelsDefault = (ORIENT_FROM_U8 ? U8K_ORIENT : 0) | (EXTRACT_SMALL_FROM_U8 ? U8K_EXTRACT_SMALL : 0) |
                                  (BIG_FUSED_FROM_U8 ? U8K_BIG_FUSED : 0) | (BIG_SAMPLE_FROM_U8 ? U8K_BIG_SAMPLE : 0) |
                                  ((ORIENT_FROM_STRIPS ? U8K_ORIENT : 0) | (EXTRACT_SMALL_FROM_STRIPS ? U8K_EXTRACT_SMALL : 0) |
                                   (BIG_FUSED_FROM_STRIPS ? U8K_BIG_FUSED : 0) | (BIG_SAMPLE_FROM_STRIPS ? U8K_BIG_SAMPLE : 0)) << U8K_STRIPS_SHIFT;
inline int u8_kernel_mask(const mods_ctx *ctx) { return ctx->u8_kernels < 0 ? kU8KernelsDefault : ctx->u8_kernels; }
inline bool kernel_from_u8(const mods_ctx *ctx, int kernel) { return (u8_kernel_mask(ctx) & kernel) != 0; }
inline bool kernel_from_strips(const mods_ctx *ctx, int kernel) { return (u8_kernel_mask(ctx) & (kernel << U8K_STRIPS_SHIFT)) != 0; }

// sift.hip.  img_u8: the same images [n_img][h][w] as 8-bit grey, or nullptr; img_strips: those in column strips, or nullptr
int launch_extract_and_sift(mods_ctx *ctx, const float *img_dev, int n_img, DescConst k, const float *dmask, const SiftTab *tab,
                            bool run_sift = true, const unsigned char *img_u8 = nullptr, const unsigned char *img_strips = nullptr);
// HalfRootSIFT twins of the described regions: copies regions_dev to regions_half_dev and overwrites the descriptors from the
// patch store left by launch_extract_and_sift (block-per-region SIFT kernel)
int launch_half_sift(mods_ctx *ctx, int n_img, DescConst k, const float *dmask, const SiftTab *tab);
int launch_sift_patch_test(mods_ctx *ctx, const float *patch_dev, int ps, int root, double max_bin, uint8_t *out_dev);
// domain-size pooling (mods_ctx_domain_pooling): the raw histograms of the patch store added into ctx->dsp_acc (first: stored), and
// the tail on the sums -> regions_dev (and the HalfSIFT twins)
int launch_dsp_accumulate(mods_ctx *ctx, int n_img, DescConst k, const float *dmask, const SiftTab *tab, bool first);
int launch_dsp_finish(mods_ctx *ctx, int n_img, DescConst k, bool want_half);

}  // namespace mods
