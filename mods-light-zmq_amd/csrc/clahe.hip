// CLAHE (contrast-limited adaptive histogram equalisation) of 8-bit grey images: the [Matching] doCLAHE branch of mods.cpp:133-189,
// which equalises both images with createCLAHE() + setClipLimit(4) (8 x 8 tiles) before they reach the ImageRepresentation.
// OpenCV is not part of this build, so the arithmetic restates the CPU path of OpenCV 3.x / 4.x imgproc/src/clahe.cpp for CV_8UC1
// (tests/clahe_ref.py is the same restatement in numpy):
//   - LUT source: the image, or - when w % tilesX or h % tilesY is nonzero - the image padded at the right by tilesX - w % tilesX
//     columns and at the bottom by tilesY - h % tilesY rows with BORDER_REFLECT_101 (both grow when either is indivisible);
//     the padding is never materialised, the LUT kernel maps its coordinates
//   - per tile: 256-bin histogram, clip at max((int)(clipLimit * total / 256), 1), redistribution of the clipped count
//     (clipped / 256 to every bin, the residual one by one to bins 0, step, 2 step, ...), lut = saturate(rint(cumsum * (255.f / total)))
//   - per pixel of the w x h image: bilinear blend of the four neighbouring tiles' LUTs in float32, one rounding per operation
//     (-ffp-contract=off), saturate(rint(.))
// Histograms are integer LDS atomics (order-free: exact).  Two launches per batch of images: clahe_lut_kernel (one workgroup per
// image and tile) and clahe_apply_kernel (one band of rows of one image per workgroup), u8 or fp32 out; the fp32 form takes the place
// of the pipeline's u8_to_f32_kernel.
#include "common.hpp"
#include <algorithm>
#include <climits>
#include <cmath>

namespace mods {

namespace {

constexpr int kLutThreads = 1024;                 // 16 waves, one sub-histogram each: a flat tile does not serialise on one bin
constexpr int kLutWaves = kLutThreads / 64;
constexpr int kApplyThreads = 256;
constexpr int kApplyBand = 16;                    // rows per workgroup (at most tile_h: a band then touches at most 3 tile rows)
constexpr int kApplyLutRows = 3;

struct ClaheGeom {
  int tiles_x, tiles_y, tile_w, tile_h;
  int clip;                                       // 0: no clipping
  float lut_scale, inv_tw, inv_th;
};

// cv::borderInterpolate(p, len, BORDER_REFLECT_101), repeated for pads longer than the image; p >= 0 here
__device__ inline int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// grid (tiles_x * tiles_y, n_img): histogram of one tile of the (virtually padded) image, clip + redistribute, 256-entry LUT
__global__ __launch_bounds__(kLutThreads) void clahe_lut_kernel(const unsigned char *__restrict__ src, int w, int h, int stride,
                                                                size_t img_stride, ClaheGeom g, unsigned char *__restrict__ lut) {
  __shared__ int hist[kLutWaves][256];
  __shared__ int scan[256];
  __shared__ int clipped_sh;
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int i = tid; i < kLutWaves * 256; i += kLutThreads) (&hist[0][0])[i] = 0;
  if (tid == 0) clipped_sh = 0;
  __syncthreads();
  const int tile = blockIdx.x, img = blockIdx.y;
  const int x0 = (tile % g.tiles_x) * g.tile_w, y0 = (tile / g.tiles_x) * g.tile_h;
  const unsigned char *base = src + (size_t)img * img_stride;
  const int total = g.tile_w * g.tile_h;
  // the tile in row-major order, kLutThreads pixels apart: (r, c) advances by (dr, dc) with a carry
  const int dr = kLutThreads / g.tile_w, dc = kLutThreads % g.tile_w;
  int r = tid / g.tile_w, c = tid % g.tile_w;
  for (int i = tid; i < total; i += kLutThreads) {
    const int y = reflect101(y0 + r, h), x = reflect101(x0 + c, w);
    atomicAdd(&hist[wave][base[(size_t)y * stride + x]], 1);
    c += dc; r += dr;
    if (c >= g.tile_w) { c -= g.tile_w; r++; }
  }
  __syncthreads();
  int v = 0;
  if (tid < 256)
    for (int k = 0; k < kLutWaves; k++) v += hist[k][tid];
  if (g.clip > 0) {
    if (tid < 256 && v > g.clip) atomicAdd(&clipped_sh, v - g.clip);
    __syncthreads();
    const int clipped = clipped_sh;
    const int batch = clipped / 256, residual = clipped - batch * 256;
    v = min(v, g.clip) + batch;
    if (residual != 0) {
      const int step = max(256 / residual, 1);
      if (tid % step == 0 && tid / step < residual) v++;
    }
  }
  if (tid < 256) scan[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int t = (tid < 256 && tid >= off) ? scan[tid - off] : 0;
    __syncthreads();
    if (tid < 256) scan[tid] += t;
    __syncthreads();
  }
  if (tid < 256) {
    const float q = rintf((float)scan[tid] * g.lut_scale);
    lut[((size_t)img * g.tiles_x * g.tiles_y + tile) * 256 + tid] = (unsigned char)fminf(fmaxf(q, 0.f), 255.f);
  }
}

template <bool F32> __device__ inline void put(void *dst, size_t i, float v) {
  if (F32) ((float *)dst)[i] = v;
  else ((unsigned char *)dst)[i] = (unsigned char)v;
}

// grid (ceil(h / band), n_img): rows [by * band, +band) of one image.  The LUT rows the band needs (at most 3, contiguous in the
// [tile][256] layout) are staged in LDS; every thread keeps the column weights of its 4-pixel groups in registers for the whole band.
// vec: rows, images and both buffers are 4-pixel aligned (4-byte loads, 16- / 4-byte stores).
// src and dst may be the same buffer (8-bit output in place, same stride): a thread stores only the pixels it has just loaded itself,
// so neither pointer is __restrict__
template <bool F32>
__global__ __launch_bounds__(kApplyThreads) void clahe_apply_kernel(const unsigned char *src, int w, int h, int src_stride,
                                                                    size_t src_img, ClaheGeom g, const unsigned char *__restrict__ lut,
                                                                    void *dst, int dst_stride, size_t dst_img, int band, int vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_lut[];      // [kApplyLutRows][tiles_x][256]
  const int img = blockIdx.y;
  const int y0 = blockIdx.x * band, y1 = min(y0 + band, h);
  if (y0 >= h) return;
  const int t_lo = max((int)floorf((float)y0 * g.inv_th - 0.5f), 0);
  const int t_hi = min((int)floorf((float)(y1 - 1) * g.inv_th - 0.5f) + 1, g.tiles_y - 1);
  const int n_rows = min(t_hi - t_lo + 1, kApplyLutRows);
  const size_t row_bytes = (size_t)g.tiles_x * 256;
  {
    const uint4 *s = (const uint4 *)(lut + ((size_t)img * g.tiles_y + t_lo) * row_bytes);
    uint4 *d = (uint4 *)lds_lut;
    const int n16 = (int)(n_rows * row_bytes / 16);
    for (int i = threadIdx.x; i < n16; i += kApplyThreads) d[i] = s[i];
  }
  __syncthreads();
  const unsigned char *sbase = src + (size_t)img * src_img;
  const size_t dbase = (size_t)img * dst_img;
  for (int x0 = 4 * threadIdx.x; x0 < w; x0 += 4 * kApplyThreads) {
    int i1[4], i2[4];
    float xa[4], xa1[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float txf = (float)(x0 + k) * g.inv_tw - 0.5f;
      const int tx1 = (int)floorf(txf);
      xa[k] = txf - (float)tx1;
      xa1[k] = 1.0f - xa[k];
      i1[k] = max(tx1, 0) * 256;
      i2[k] = min(tx1 + 1, g.tiles_x - 1) * 256;
    }
    const bool full = vec && x0 + 3 < w;
    for (int y = y0; y < y1; y++) {
      const float tyf = (float)y * g.inv_th - 0.5f;
      const int ty1 = (int)floorf(tyf);
      const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
      const int r1 = min(max(max(ty1, 0) - t_lo, 0), n_rows - 1);
      const int r2 = min(max(min(ty1 + 1, g.tiles_y - 1) - t_lo, 0), n_rows - 1);
      const unsigned char *L1 = lds_lut + r1 * row_bytes, *L2 = lds_lut + r2 * row_bytes;
      const unsigned char *srow = sbase + (size_t)y * src_stride;
      const size_t drow = dbase + (size_t)y * dst_stride;
      int px[4];
      if (full) {
        const uchar4 q = *(const uchar4 *)(srow + x0);
        px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) px[k] = x0 + k < w ? srow[x0 + k] : 0;
      }
      float out[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int v = px[k];
        const float res = ((float)L1[i1[k] + v] * xa1[k] + (float)L1[i2[k] + v] * xa[k]) * ya1 +
                          ((float)L2[i1[k] + v] * xa1[k] + (float)L2[i2[k] + v] * xa[k]) * ya;
        out[k] = fminf(fmaxf(rintf(res), 0.f), 255.f);
      }
      if (full) {
        if (F32) *(float4 *)((float *)dst + drow + x0) = make_float4(out[0], out[1], out[2], out[3]);
        else *(uchar4 *)((unsigned char *)dst + drow + x0) = make_uchar4((unsigned char)out[0], (unsigned char)out[1],
                                                                         (unsigned char)out[2], (unsigned char)out[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (x0 + k < w) put<F32>(dst, drow + x0 + k, out[k]);
      }
    }
  }
}

// the constants of clahe.cpp's CLAHE_Impl::apply for a w x h image
ClaheGeom clahe_geom(int w, int h, const mods_clahe_params *par) {
  ClaheGeom g;
  g.tiles_x = par->tiles_x; g.tiles_y = par->tiles_y;
  int pw = w, ph = h;
  if (w % g.tiles_x != 0 || h % g.tiles_y != 0) { pw = w + g.tiles_x - w % g.tiles_x; ph = h + g.tiles_y - h % g.tiles_y; }
  g.tile_w = pw / g.tiles_x; g.tile_h = ph / g.tiles_y;
  const int total = g.tile_w * g.tile_h;
  g.lut_scale = 255.0f / (float)total;
  g.clip = 0;
  if (par->clip_limit > 0.0) {
    const double c = par->clip_limit * total / 256;
    g.clip = std::max(c >= (double)INT_MAX ? INT_MAX : (int)c, 1);
  }
  g.inv_tw = 1.0f / (float)g.tile_w;
  g.inv_th = 1.0f / (float)g.tile_h;
  return g;
}

// argument checks of mods_clahe_dev / mods_clahe, before any device call (the context is looked at last)
int clahe_check(mods_ctx *c, const void *src, const void *dst, int n_img, int w, int h, int src_stride, int dst_stride,
                const mods_clahe_params *par, const char *fn) {
  if (!src || !dst) { set_error("%s: null image buffer", fn); return MODS_E_ARG; }
  if (!par) { set_error("%s: null CLAHE parameters", fn); return MODS_E_ARG; }
  if (n_img < 1) { set_error("%s: n_img %d < 1", fn, n_img); return MODS_E_ARG; }
  if (w < 1 || h < 1) { set_error("%s: image size %d x %d", fn, w, h); return MODS_E_ARG; }
  if (src_stride < w) { set_error("%s: source stride %d < width %d", fn, src_stride, w); return MODS_E_ARG; }
  if (dst_stride < w) { set_error("%s: destination stride %d < width %d", fn, dst_stride, w); return MODS_E_ARG; }
  if (par->tiles_x < 1 || par->tiles_x > 64 || par->tiles_y < 1 || par->tiles_y > 64) {
    set_error("%s: tile grid %d x %d outside [1, 64]", fn, par->tiles_x, par->tiles_y); return MODS_E_ARG;
  }
  if (!c) { set_error("%s: null context", fn); return MODS_E_ARG; }
  if ((size_t)w * h > (size_t)c->max_w * c->max_h) { set_error("%s: image %d x %d larger than the context", fn, w, h); return MODS_E_ARG; }
  return MODS_OK;
}

}  // namespace

// LUT scratch of n_img images on the given grid (a hipMalloc: called outside the pipeline's running path)
int clahe_reserve(mods_ctx *c, int n_img, const mods_clahe_params *par) {
  const size_t need = (size_t)n_img * par->tiles_x * par->tiles_y * 256;
  if (need <= c->clahe_lut.capacity()) return MODS_OK;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->clahe_lut, need, need));
  return MODS_OK;
}

// the two launches on the context's stream (no synchronisation; the LUT scratch must already hold n_img images)
int clahe_launch(mods_ctx *c, const unsigned char *src, int n_img, int w, int h, int src_stride, const mods_clahe_params *par,
                 void *dst, int dst_stride, int dst_f32) {
  const ClaheGeom g = clahe_geom(w, h, par);
  if ((size_t)n_img * g.tiles_x * g.tiles_y * 256 > c->clahe_lut.capacity()) { set_error("clahe: LUT scratch not reserved"); return MODS_E_ARG; }
  const size_t src_img = (size_t)h * src_stride, dst_img = (size_t)h * dst_stride;
  hipLaunchKernelGGL(clahe_lut_kernel, dim3(g.tiles_x * g.tiles_y, n_img), dim3(kLutThreads), 0, c->stream, src, w, h, src_stride,
                     src_img, g, c->clahe_lut);
  const int band = std::min(kApplyBand, g.tile_h);
  const dim3 grid((h + band - 1) / band, n_img);
  const size_t lds = (size_t)kApplyLutRows * g.tiles_x * 256;
  const bool src_vec = src_stride % 4 == 0 && (uintptr_t)src % 4 == 0;
  if (dst_f32) {
    const int vec = src_vec && dst_stride % 4 == 0 && (uintptr_t)dst % 16 == 0;
    hipLaunchKernelGGL(clahe_apply_kernel<true>, grid, dim3(kApplyThreads), lds, c->stream, src, w, h, src_stride, src_img, g,
                       c->clahe_lut, dst, dst_stride, dst_img, band, vec);
  } else {
    const int vec = src_vec && dst_stride % 4 == 0 && (uintptr_t)dst % 4 == 0;
    hipLaunchKernelGGL(clahe_apply_kernel<false>, grid, dim3(kApplyThreads), lds, c->stream, src, w, h, src_stride, src_img, g,
                       c->clahe_lut, dst, dst_stride, dst_img, band, vec);
  }
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_clahe_dev(mods_ctx *c, const unsigned char *src_dev, int n_img, int w, int h, int src_stride, const mods_clahe_params *par,
                   void *dst_dev, int dst_stride, int dst_f32) {
  int rc = clahe_check(c, src_dev, dst_dev, n_img, w, h, src_stride, dst_stride, par, "mods_clahe_dev");
  if (rc) return rc;
  if (!dst_f32 && dst_dev == (const void *)src_dev && dst_stride != src_stride) {
    set_error("mods_clahe_dev: in-place output needs the source stride"); return MODS_E_ARG;
  }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((rc = clahe_reserve(c, n_img, par))) return rc;
  if ((rc = clahe_launch(c, src_dev, n_img, w, h, src_stride, par, dst_dev, dst_stride, dst_f32))) return rc;
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

int mods_clahe(mods_ctx *c, const unsigned char *src_host, int w, int h, const mods_clahe_params *par, unsigned char *dst_host) {
  int rc = clahe_check(c, src_host, dst_host, 1, w, h, w, w, par, "mods_clahe");
  if (rc) return rc;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((rc = mods::u8_stage_ensure(c))) return rc;
  if ((rc = clahe_reserve(c, 1, par))) return rc;
  const size_t bytes = (size_t)w * h;
  MODS_HIP_CHECK(mods::copy_wait(c->stream, c->u8_stage_dev, src_host, bytes, hipMemcpyHostToDevice));
  if ((rc = clahe_launch(c, c->u8_stage_dev, 1, w, h, w, par, c->u8_stage_dev, w, 0))) return rc;     // in place
  MODS_HIP_CHECK(mods::copy_wait(c->stream, dst_host, c->u8_stage_dev, bytes, hipMemcpyDeviceToHost));
  return MODS_OK;
}

}  // extern "C"
