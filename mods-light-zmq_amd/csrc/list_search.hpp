// What the searches of two region lists under a known model share (guided.hip, overlap.hip, overlap_area.hip).
//
// Their shape: pack (208-byte regions -> small fp64 records), a sweep of the n_q x n_t pairs in which a thread owns a query (its
// record in registers) and the block walks the trains through LDS tiles that all lanes read at the same address (a broadcast), with
// the train range split over blockIdx.y, accept, and an ordered compaction: a count kernel leaves per-block counts, the emit kernel
// gives a block the sum of the counts before it and an item the emitted items before it in its block, and the last block writes
// the total.  Here live the constants of that shape, the compaction, the split plan of the sweeps and the staging of host lists.
// Kernels in a header are templates or static: the library is built without relocatable device code.
#pragma once
#include "common.hpp"
#include <algorithm>

namespace mods {

constexpr int LS_THREADS = 256;   // queries per block of a sweep, threads of every kernel of the searches
constexpr int LS_TILE = 256;      // trains per LDS tile
constexpr int LS_WAVES = LS_THREADS / 64;
constexpr unsigned long long LS_NONE = ~0ull;

// exclusive prefix of v over the block's threads and, in *total, the block's sum (s_wave: LS_WAVES ints of LDS)
__device__ __forceinline__ int block_scan(int v, int *s_wave, int *total) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  __syncthreads();
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < LS_WAVES; w++) { const int c = s_wave[w]; if (w < wv) before += c; all += c; }
  *total = all;
  return before + incl - v;
}

// the sum of counts[0 .. n) by the whole block (s_wave as above)
__device__ __forceinline__ int block_sum_before(const int *__restrict__ counts, int n, int *s_wave) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int part = 0;
  for (int b = tid; b < n; b += LS_THREADS) part += counts[b];
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  __syncthreads();
  if (lane == 0) s_wave[wv] = part;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < LS_WAVES; w++) t += s_wave[w];
  return t;
}

// The compaction's first kernel: block_counts[block] = the items of the block that `final` emits.  A search states its predicate
// once, as a struct of the few pointers it reads with a call operator on the item's index, and hands the same object to its emit
// kernel
template <class Final>
__global__ __launch_bounds__(LS_THREADS) void compact_count_kernel(Final final, int *__restrict__ block_counts) {
  const bool emit = final((int)(blockIdx.x * LS_THREADS + threadIdx.x));
  const int c = __syncthreads_count(emit ? 1 : 0);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

// ... and the emit kernel's half: the slot of the thread's item (when it is emitted) in the order of the items, and in *upto the
// items emitted up to the end of this block - the total in the last block
__device__ __forceinline__ int compact_slot(bool emit, const int *__restrict__ block_counts, int *s_wave, int *upto) {
  const int base = block_sum_before(block_counts, (int)blockIdx.x, s_wave);
  int total;
  const int slot = base + block_scan(emit ? 1 : 0, s_wave, &total);
  *upto = base + total;
  return slot;
}

// the trains [begin, end) that a block of a sweep walks (blockIdx.y = split)
struct TrainRange { int begin, end; };
__device__ __forceinline__ TrainRange train_range(int n_t, int tiles_per_split) {
  const int begin = min(n_t, (int)blockIdx.y * tiles_per_split * LS_TILE);
  return {begin, min(n_t, begin + tiles_per_split * LS_TILE)};
}

// The grid of a sweep: ceil(n_q / 256) query blocks times as many splits of the train tiles as bring the grid to target_blocks, so
// that the last round of blocks is a small part of the sweep even when the query list is short (profiles/overlap_timing.txt:
// 60 156 x 47 177 takes 2.7 ms unsplit, 1.3 ms with 16 splits).  forced_splits > 0 replaces the choice (mods_ctx_overlap_splits).
// The split count is the one the tiles per split leave: no split is empty
struct SweepGrid { int qblocks, splits, tiles_per_split; };
inline SweepGrid sweep_grid(int n_q, int n_t, int target_blocks, int forced_splits) {
  SweepGrid g;
  g.qblocks = (n_q + LS_THREADS - 1) / LS_THREADS;
  const int n_tiles = (n_t + LS_TILE - 1) / LS_TILE;
  int splits = std::max(1, std::min(n_tiles, (target_blocks + g.qblocks - 1) / std::max(g.qblocks, 1)));
  if (forced_splits > 0) splits = std::max(1, std::min(n_tiles, forced_splits));
  g.tiles_per_split = std::max(1, (n_tiles + splits - 1) / splits);
  g.splits = std::max(1, (n_tiles + g.tiles_per_split - 1) / g.tiles_per_split);
  return g;
}
constexpr int GUIDED_TARGET_BLOCKS = 2048;    // a few waves on every SIMD of the 256 CUs
constexpr int OVERLAP_TARGET_BLOCKS = 4096;   // some 16 blocks per CU (both overlap searches)

// The refusals of an entry point for host lists that concern the lists; `who` starts the message
inline int check_host_lists(const char *who, const void *q, int n_q, const void *t, int n_t) {
  if ((n_q > 0 && !q) || (n_t > 0 && !t)) { set_error("%s: null argument", who); return MODS_E_ARG; }
  if (n_q < 0 || n_t < 0) { set_error("%s: negative count (%d queries, %d trains)", who, n_q, n_t); return MODS_E_ARG; }
  return MODS_OK;
}

// Two host lists into the context's staging buffer, queries first; the searches run one after another on the context's stream,
// so one buffer serves them all
inline int stage_lists(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, const mods_region **q_dev,
                       const mods_region **t_dev) {
  const size_t n = (size_t)n_q + (size_t)n_t;
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->ls_regs, n + 1, n + n / 4 + 1));
  if (n_q) MODS_HIP_CHECK(hipMemcpyAsync(c->ls_regs, q, sizeof(mods_region) * (size_t)n_q, hipMemcpyHostToDevice, c->stream));
  if (n_t) MODS_HIP_CHECK(hipMemcpyAsync(c->ls_regs + n_q, t, sizeof(mods_region) * (size_t)n_t, hipMemcpyHostToDevice, c->stream));
  *q_dev = c->ls_regs; *t_dev = c->ls_regs + n_q;
  return MODS_OK;
}

}  // namespace mods
