// Which copy of the input images a sampling kernel reads: the one place that decides it ("Input images";
// section 4, "Sampling from the 8-bit twin").
// The kernels that gather from the input image (orient_kernel, extract_small_kernel, big_fused_kernel, big_sample_kernel) exist for
// three pixel sources: fp32, row-major 8-bit grey, and 8-bit grey in 16-byte column strips (u8_strips.hpp).  The 8-bit forms give
// the same values from a quarter of the bytes; a call has them only when it came in as 8-bit (pair.hip: u8_sources_launch).
// common.hpp includes this header ahead of mods_ctx (whose replay key holds a PixelSources), so the functions here take the
// context's setting, mods_ctx::u8_kernels, rather than the context.
#pragma once
#include <type_traits>
#include "u8_strips.hpp"

namespace mods {

struct StripPx;      // device_util.hpp: the pixel type of a strip twin

// The copies of one call's images [n_img][h][w].  u8 and strips are null when the call has no such copy
struct PixelSources {
  const float *f32 = nullptr;
  const unsigned char *u8 = nullptr;       // row-major, packed rows
  const unsigned char *strips = nullptr;   // [n_img][strip_count(w)][h rounded up to 8][16]
  bool operator==(const PixelSources &o) const { return f32 == o.f32 && u8 == o.u8 && strips == o.strips; }
  PixelSources fp32_only() const { return {f32}; }
};

// One bit per kernel: bits 0-3, the kernel samples from the row-major 8-bit images when the call has them; bits 4-7, from the
// strip twin when the call has one, which goes before bits 0-3
enum { U8K_ORIENT = 1, U8K_EXTRACT_SMALL = 2, U8K_BIG_FUSED = 4, U8K_BIG_SAMPLE = 8, U8K_STRIPS_SHIFT = 4, U8K_ALL = 255 };
// The default keeps, for each kernel, the form that was faster at the benchmark's 32-image batch (DESIGN.md section 4;
// profiles/u8_sampling_*, profiles/strip_u8_*).  Times per batch:
//   row-major 8-bit against fp32
//     orient_kernel         1.853 against 1.861 ms, run-to-run deviation 0.067: no gain, stays on fp32
//     extract_small_kernel  3 x 0.985 against 3 x 1.036 ms: on
//     big_fused_kernel      2.67 against 2.88 ms: on
//     big_sample_kernel     no region of the benchmark's images reaches this kernel (P2 > 1024): not measured, stays on fp32
//   strips against the kernel's form above
//     orient_kernel         1.759 against 1.867 ms (fp32): on
//     extract_small_kernel  3 x 0.942 against 3 x 0.991 ms (row-major 8-bit): on
//     big_fused_kernel      2.36 against 2.68 ms (row-major 8-bit): on
//     big_sample_kernel     not measured, as above: stays on fp32
constexpr int kU8KernelsDefault = U8K_EXTRACT_SMALL | U8K_BIG_FUSED | ((U8K_ORIENT | U8K_EXTRACT_SMALL | U8K_BIG_FUSED) << U8K_STRIPS_SHIFT);
// the mask of a context's calls: the default, or the one it was given instead (mods_ctx_u8_kernels: the tests run the forms that the
// default leaves out)
inline int u8_kernel_mask(int setting) { return setting < 0 ? kU8KernelsDefault : setting; }
// whether a call with these 8-bit images gets a strip twin: a kernel of the mask samples from strips, the rows are packed and the
// size is one the layout's address arithmetic covers
inline bool u8_strips_wanted(int setting, int w, int h, int stride) {
  return (u8_kernel_mask(setting) >> U8K_STRIPS_SHIFT) != 0 && stride == w && strip_layout_ok(w, h);
}

// Calls launch(img) with the images `kernel` (one U8K_* bit) samples from in this call, as const StripPx *, const unsigned char * or
// const float *: strips if present and selected, else row-major 8-bit if present and selected, else fp32.  PixelOf<decltype(img)>
// names the kernel's instantiation
template <class P> using PixelOf = std::remove_const_t<std::remove_pointer_t<P>>;
template <class Launch> inline void with_pixel_source(int setting, const PixelSources &px, int kernel, Launch &&launch) {
  const int mask = u8_kernel_mask(setting);
  if (px.strips && (mask & (kernel << U8K_STRIPS_SHIFT))) launch((const StripPx *)px.strips);
  else if (px.u8 && (mask & kernel)) launch(px.u8);
  else launch(px.f32);
}

}  // namespace mods
