// Spatial selection of a count-limited detector's regions (mods_ctx_spatial_selection; contract in include/mods_hip.h, restated in
// tests/spatial_select_ref.py): adaptive non-maximal suppression, Brown, Szeliski and Winder, "Multi-image matching using
// multi-scale oriented patches", CVPR 2005.  No counterpart in the reference.
//
// After export_kernel an image's keys lie in keys_dev in the order the contract indexes them by: |response| descending.  Three
// launches then stand in the place of select_keys_kernel's prefix cut, none sized by a count the host would have to read:
//   spatial_radius_kernel   r2[i] = squared distance to the nearest key j with fl32(c a[j]) > a[i]; writes the selection key
//                           (~bits(r2) << 32) | i into sort_keys, whose sort keys the export has consumed
//   rank_keys_launch        the detector's own rank kernels over those keys: rank[i] = place of i by r2 descending, index ascending
//   spatial_compact_kernel  the keys with rank < keep, moved to the front of the list in index order; key_count = keep
// fl32(c a[j]) does not increase with j, so the suppressors of a key form a prefix of the list: a workgroup stops at the first tile
// whose strongest key suppresses none of its own.
#include "common.hpp"

namespace mods {

constexpr int SS_KEYS = 64;       // keys of a workgroup, one per lane; its four waves take a quarter of each tile
constexpr int SS_TILE = 1024;     // suppressor candidates staged in LDS at a time: {x, y, fl32(c a)}
constexpr int KEY_WORDS = sizeof(mods_affkey) / 8;
static_assert(sizeof(mods_affkey) % 8 == 0 && alignof(mods_affkey) == 8, "a key is moved as 64-bit words");

__device__ __forceinline__ int spatial_keep(int b, int n, int mode, int reg_number, float rel_reg_number, const int *keep_list) {
  const int keep = keep_list ? keep_list[b] : count_mode_keep(mode, n, reg_number, rel_reg_number);
  return max(0, min(keep, n));
}

// grid = (workgroups striding over the blocks of SS_KEYS keys, n_img), block = 256
__global__ __launch_bounds__(256) void spatial_radius_kernel(int max_cand, const mods_affkey *__restrict__ keys, const int *__restrict__ key_count,
                                                             int mode, int reg_number, float rel_reg_number, const int *__restrict__ keep_list,
                                                             float c, unsigned long long *__restrict__ sel_keys) {
  __shared__ float4 tile[SS_TILE];
  __shared__ float part[4][SS_KEYS];
  const int b = blockIdx.y;
  const int n = key_count[b];
  const int keep = spatial_keep(b, n, mode, reg_number, rel_reg_number, keep_list);
  if (keep <= 0 || keep >= n) return;            // the prefix cut: spatial_compact_kernel sets the count, no rank is read
  const mods_affkey *k = keys + (size_t)b * max_cand;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = (n + SS_KEYS - 1) / SS_KEYS;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int i = blk * SS_KEYS + lane;
    float x = 0.f, y = 0.f, a = INFINITY;        // a lane past the list: nothing suppresses it, nothing is written
    if (i < n) { x = (float)k[i].x; y = (float)k[i].y; a = fabsf((float)k[i].response); }
    const float a_min = fabsf((float)k[min(blk * SS_KEYS + SS_KEYS, n) - 1].response);   // the block's weakest key
    float m = INFINITY;
    for (int t0 = 0; t0 < n; t0 += SS_TILE) {
      if (!(__fmul_rn(c, fabsf((float)k[t0].response)) > a_min)) break;   // the tile's strongest suppresses none of the block: nor does a later key
      __syncthreads();
      for (int q = threadIdx.x; q < SS_TILE; q += 256) {
        const int j = t0 + q;
        tile[q] = j < n ? make_float4((float)k[j].x, (float)k[j].y, __fmul_rn(c, fabsf((float)k[j].response)), 0.f)
                        : make_float4(0.f, 0.f, 0.f, 0.f);                // fl32(c a) = 0 suppresses nothing
      }
      __syncthreads();
      const float4 *tw = tile + wave * (SS_TILE / 4);
#pragma unroll 4
      for (int q = 0; q < SS_TILE / 4; q++) {
        const float4 s = tw[q];
        const float dx = __fsub_rn(x, s.x), dy = __fsub_rn(y, s.y);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        m = (s.z > a && d2 < m) ? d2 : m;        // c <= 1: fl32(c a[i]) <= a[i], a key never suppresses itself
      }
    }
    __syncthreads();                             // (the last tile's readers, and part[]'s of the block before)
    part[wave][lane] = m;
    __syncthreads();
    if (wave == 0 && i < n) {
      m = fminf(fminf(part[0][lane], part[1][lane]), fminf(part[2][lane], part[3][lane]));
      sel_keys[(size_t)b * max_cand + i] = ((unsigned long long)(~__float_as_uint(m)) << 32) | (unsigned int)i;
    }
  }
}

// One workgroup per image: a stable compaction of the keys with rank < keep, in place - a chunk of 1024 keys is read whole before
// any of its keys is written, and a key never moves to a higher index, so no key is overwritten before it is read.
__global__ __launch_bounds__(1024) void spatial_compact_kernel(int max_cand, mods_affkey *__restrict__ keys, int *__restrict__ key_count,
                                                               int mode, int reg_number, float rel_reg_number, const int *__restrict__ keep_list,
                                                               const int *__restrict__ rank) {
  __shared__ int s_wave[16];
  const int b = blockIdx.x;
  const int n = key_count[b];
  const int keep = spatial_keep(b, n, mode, reg_number, rel_reg_number, keep_list);
  if (keep <= 0 || keep >= n) {                  // today's cut
    if (threadIdx.x == 0) key_count[b] = keep;
    return;
  }
  mods_affkey *k = keys + (size_t)b * max_cand;
  const int *r = rank + (size_t)b * max_cand;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + threadIdx.x;
    const bool kept = i < n && r[i] < keep;
    unsigned long long v[KEY_WORDS];             // (moved as words: a conditional struct copy goes through scratch memory)
    if (kept) {
      const unsigned long long *src = (const unsigned long long *)(k + i);
#pragma unroll
      for (int q = 0; q < KEY_WORDS; q++) v[q] = src[q];
    }
    const unsigned long long votes = __ballot(kept);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int at = base + __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < 16; w++) { const int cw = s_wave[w]; at += w < wave ? cw : 0; total += cw; }
    if (kept) {
      unsigned long long *dst = (unsigned long long *)(k + at);
#pragma unroll
      for (int q = 0; q < KEY_WORDS; q++) dst[q] = v[q];
    }
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) key_count[b] = keep;     // (= base: the ranks are a permutation of 0 .. n-1)
}

int spatial_select_launch(mods_ctx *ctx, int n_img, int *key_count, int mode, int reg_number, float rel_reg_number, float robustness,
                          const int *keep_list) {
  StageScope ts(ctx, MODS_STAGE_SPATIAL_SELECT);
  hipLaunchKernelGGL(spatial_radius_kernel, dim3(1024, n_img), dim3(256), 0, ctx->stream, ctx->max_cand, ctx->keys_dev.get(), key_count, mode,
                     reg_number, rel_reg_number, keep_list, robustness, ctx->sort_keys.get());
  const int rc = rank_keys_launch(ctx, n_img, key_count);
  if (rc) return rc;
  hipLaunchKernelGGL(spatial_compact_kernel, dim3(n_img), dim3(1024), 0, ctx->stream, ctx->max_cand, ctx->keys_dev.get(), key_count, mode,
                     reg_number, rel_reg_number, keep_list, ctx->rank_dev.get());
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

static int spatial_args(const char *who, int mode, double robustness) {
  if (mode < 0 || mode > 2) { set_error("%s: mode %d (0 off, 1 ANMS, 2 ANMS where the call's mode and detector allow it)", who, mode); return MODS_E_ARG; }
  if (!(robustness >= 0.0 && robustness <= 1.0)) { set_error("%s: robustness %g (0 <= robustness <= 1)", who, robustness); return MODS_E_ARG; }
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_ctx_spatial_selection(mods_ctx *c, int mode, double robustness) {
  const int rc = spatial_args("spatial_selection", mode, robustness);
  if (rc) return rc;
  if (!c) { set_error("spatial_selection: null context"); return MODS_E_ARG; }
  c->spatial_mode = mode;
  c->spatial_c = robustness;
  dev_state_changed(c);              // (recorded launch chains are not replayed across the change)
  return MODS_OK;
}

int mods_ctx_spatial_selection_get(const mods_ctx *c, int *mode, double *robustness) {
  if (!c) { set_error("spatial_selection_get: null context"); return MODS_E_ARG; }
  if (mode) *mode = c->spatial_mode;
  if (robustness) *robustness = c->spatial_c;
  return MODS_OK;
}

// n_img sorted lists [n_img][max_n] through the three launches as a detect call issues them; out_idx [n_img][max_n]: the indices of
// the keys each list keeps, n_out their counts.  The indices are read off the ranks, and the compacted lists are held against them.
int mods_test_spatial_select(mods_ctx *c, const mods_affkey *keys_host, int n_img, const int *n, int max_n, const int *keep, double robustness,
                             int *out_idx, int *n_out) {
  const int rc = spatial_args("test_spatial_select", 1, robustness);
  if (rc) return rc;
  if (!c || !keys_host || !n || !keep || !out_idx || !n_out) { set_error("test_spatial_select: null argument"); return MODS_E_ARG; }
  if (n_img < 1 || n_img > c->batch || max_n < 1 || max_n > c->max_cand) {
    set_error("test_spatial_select: %d lists of up to %d keys (the context holds %d of %d)", n_img, max_n, c->batch, c->max_cand);
    return MODS_E_ARG;
  }
  for (int b = 0; b < n_img; b++)
    if (n[b] < 0 || n[b] > max_n) { set_error("test_spatial_select: list %d has %d keys (0 .. %d)", b, n[b], max_n); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  int *keep_dev = c->cand_count + c->batch, *key_count = c->cand_count + 2 * c->batch;   // (the accepted counts' slots are free here)
  for (int b = 0; b < n_img; b++)
    if (n[b] > 0)
      MODS_HIP_CHECK(hipMemcpyAsync(c->keys_dev + (size_t)b * c->max_cand, keys_host + (size_t)b * max_n, sizeof(mods_affkey) * (size_t)n[b],
                                    hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(keep_dev, keep, sizeof(int) * n_img, hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(key_count, n, sizeof(int) * n_img, hipMemcpyHostToDevice, c->stream));
  const int lrc = spatial_select_launch(c, n_img, key_count, MODS_DET_FIXED_REG_NUMBER, 0, 0.f, (float)robustness, keep_dev);
  if (lrc) return lrc;
  std::vector<int> rank((size_t)max_n), count((size_t)n_img);
  std::vector<mods_affkey> got((size_t)max_n);
  MODS_HIP_CHECK(copy_wait(c->stream, count.data(), key_count, sizeof(int) * n_img, hipMemcpyDeviceToHost));
  for (int b = 0; b < n_img; b++) {
    const int kc = std::max(0, std::min(keep[b], n[b]));
    int *idx = out_idx + (size_t)b * max_n, m = 0;
    if (kc <= 0 || kc >= n[b]) for (; m < kc; m++) idx[m] = m;
    else {
      MODS_HIP_CHECK(copy_wait(c->stream, rank.data(), c->rank_dev + (size_t)b * c->max_cand, sizeof(int) * (size_t)n[b], hipMemcpyDeviceToHost));
      for (int i = 0; i < n[b]; i++) if (rank[i] < kc) { if (m < max_n) idx[m] = i; m++; }
    }
    n_out[b] = count[b];
    if (m != count[b] || m != kc) { set_error("test_spatial_select: list %d: %d ranks below keep = %d, key_count %d", b, m, kc, count[b]); return MODS_E_HIP; }
    if (m > 0) MODS_HIP_CHECK(copy_wait(c->stream, got.data(), c->keys_dev + (size_t)b * c->max_cand, sizeof(mods_affkey) * (size_t)m, hipMemcpyDeviceToHost));
    for (int q = 0; q < m; q++)
      if (memcmp(&got[q], keys_host + (size_t)b * max_n + idx[q], sizeof(mods_affkey)) != 0) {
        set_error("test_spatial_select: list %d: the compacted key %d is not key %d of the input", b, q, idx[q]);
        return MODS_E_HIP;
      }
  }
  return MODS_OK;
}

}  // extern "C"
