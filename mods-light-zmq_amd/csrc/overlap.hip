// Overlap matching: which regions of image 1 have a geometric counterpart in image 2 under a known homography, and how
// repeatable the detector is on the pair.
//
// The reference reads [OverlapMatching] doOverlapMatch / overlapError (io_mods.cpp:685-687) and prints "Overlap matches with E <"
// (mods.cpp:522-523); the error is the linearised one of ellipseOverlapH / ellipseOverlapHPrep (matching/matching.hpp:170-253),
// not the area of intersection.  No descriptor takes part.  The contract (include/mods_hip.h: mods_match_overlap) is bit exact:
// fp64 with one rounding per operation, every reduction a minimum over a total order - so the result does not depend on the
// launch geometry, the train splits or the arrival order of the atomics.
//
// Shape, as guided.hip: pack (208-byte regions -> 48-byte fp64 records; a region outside the common area gets a record of NaNs,
// which matches nothing), one sweep of the n_q x n_t pairs, accept (+ one-to-one by two atomicMin per train: the error's bits, then
// the query index among the equal ones), ordered compaction and emit.  A thread owns a query (its record in registers), the block
// walks the trains through LDS tiles that all lanes read at the same address (a broadcast), four trains per branch on the centre
// term alone: the shape term is computed only for a pair whose centre term is below the best error the query has so far (at most
// max_error), which cannot change a minimum because the shape term is never negative.  Train splits run in blockIdx.y; each
// leaves its (E, t) per query in a table of its own and the accept kernel takes their minimum in split order, so no 96-bit
// atomic is needed.  VALU only, no matrix cores.
#include "overlap_common.hpp"
#include <cmath>

namespace mods {

struct OverlapConst {
  int n_q, n_t;
  double H[9], Hinv[9];   // row-major; Hinv = adjugate / determinant
  double max_error;
  int oriented, one_to_one;
  int area;               // the common-area test runs (all four sizes > 0)
  double w1, h1, w2, h2;
  int tiles_per_split;    // train tiles a block of the sweep walks (blockIdx.y = split)
};

constexpr int O_THREADS = 256;   // queries per block of the sweep, threads of every kernel here
constexpr int O_TILE = 256;      // trains per LDS tile (12 KB of records)
constexpr unsigned long long O_NONE = ~0ull;

// One list, a thread per region.  cnt[is_train] += the regions of the list that take part (all of them without the area test)
__global__ __launch_bounds__(O_THREADS) void overlap_pack_kernel(OverlapConst k, const mods_region *__restrict__ reg, int n, int is_train,
                                                                 OvRec *__restrict__ rec, int *__restrict__ cnt) {
  const int i = blockIdx.x * O_THREADS + threadIdx.x;
  bool part = false;
  if (i < n) {
    const OvRec f = overlap_frame(reg[i]);
    OvRec r;
    if (!is_train) {
      r = overlap_query_rec(k.H, f);
      part = !k.area || overlap_in_image(r.a, r.b, k.w2, k.h2);
    } else {                                             // x2 y2 I11 I12 I21 I22: the inverse of the frame
      const double d = 1.0 / (f.m11 * f.m22 - f.m12 * f.m21);
      r.a = f.a; r.b = f.b;
      r.m11 = f.m22 * d; r.m12 = -(f.m12 * d); r.m21 = -(f.m21 * d); r.m22 = f.m11 * d;
      part = !k.area || overlap_maps_into(k.Hinv, f.a, f.b, k.w1, k.h1);
    }
    rec[i] = part ? r : overlap_nan_rec();
  }
  const int c = __syncthreads_count(part ? 1 : 0);
  if (threadIdx.x == 0 && c) atomicAdd(&cnt[is_train], c);
}

// The two terms of a pair's error.  A record of NaNs gives NaN, which is below nothing
__device__ __forceinline__ double overlap_dist(const OvRec &r, const OvRec &t) {
  const double dx = r.a - t.a, dy = r.b - t.b;
  const double u = t.m11 * dx + t.m12 * dy, v = t.m21 * dx + t.m22 * dy;
  return u * u + v * v;
}
__device__ __forceinline__ double overlap_diff(const OvRec &r, const OvRec &t, bool oriented) {
  double G11 = t.m11 * r.m11 + t.m12 * r.m21, G12 = t.m11 * r.m12 + t.m12 * r.m22;
  double G21 = t.m21 * r.m11 + t.m22 * r.m21, G22 = t.m21 * r.m12 + t.m22 * r.m22;
  if (!oriented) {   // up is up: in-plane rotation of the frame does not count
    const double det = sqrt(fabs(G11 * G22 - G12 * G21));
    const double rr = sqrt(G12 * G12 + G11 * G11);
    const double g21 = (G22 * G12 + G21 * G11) / (rr * det);
    G11 = rr / det; G12 = 0.; G21 = g21; G22 = det / rr;
  }
  return 0.5 * ((((1. - G11) * (1. - G11) + G12 * G12) + G21 * G21) + (1. - G22) * (1. - G22));
}

// part_e / part_t [split][n_q]: the smallest (E, t) with E < max_error over the trains of the split (O_NONE: none).
// grid = (ceil(n_q / 256), splits)
template <bool ORIENTED>
__global__ __launch_bounds__(O_THREADS) void overlap_sweep_kernel(OverlapConst k, const OvRec *__restrict__ qrec, const OvRec *__restrict__ trec,
                                                                  unsigned long long *__restrict__ part_e, int *__restrict__ part_t) {
  __shared__ OvRec s_t[O_TILE];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * O_THREADS + tid;
  const OvRec none = overlap_nan_rec();
  OvRec r = none;                                        // lanes past the list
  if (q < k.n_q) r = qrec[q];
  const int t_begin = min(k.n_t, (int)blockIdx.y * k.tiles_per_split * O_TILE);
  const int t_end = min(k.n_t, t_begin + k.tiles_per_split * O_TILE);
  double best = k.max_error;                             // E >= 0: an error's order is the order of its bits
  int best_t = -1;
  for (int t0 = t_begin; t0 < t_end; t0 += O_TILE) {
    const int cnt = min(O_TILE, t_end - t0);             // the tail of the last tile holds records that match nothing
    __syncthreads();
    OvRec rec = none;
    if (tid < cnt) rec = trec[t0 + tid];
    s_t[tid] = rec;
    __syncthreads();
    for (int j4 = 0; j4 < cnt; j4 += 4) {
      // four trains at a time through the centre term: every lane reads the same addresses (broadcasts), one branch for the four
      const double d0 = overlap_dist(r, s_t[j4]), d1 = overlap_dist(r, s_t[j4 + 1]);
      const double d2 = overlap_dist(r, s_t[j4 + 2]), d3 = overlap_dist(r, s_t[j4 + 3]);
      if (!(d0 < best || d1 < best || d2 < best || d3 < best)) continue;
      auto full = [&](double d, int j) {
        if (!(d < best)) return;
        const double E = overlap_diff(r, s_t[j], ORIENTED) + d;
        if (E < best) { best = E; best_t = t0 + j; }       // strict: a tie stays with the lower train index
      };
      full(d0, j4); full(d1, j4 + 1); full(d2, j4 + 2); full(d3, j4 + 3);
    }
  }
  if (q < k.n_q) {
    const size_t at = (size_t)blockIdx.y * (size_t)k.n_q + (size_t)q;
    part_e[at] = best_t >= 0 ? (unsigned long long)__double_as_longlong(best) : O_NONE;
    part_t[at] = best_t;
  }
}

// best_e / best_t[q] = the minimum over the splits, in split order (= train order: ties stay with the lower train); with
// one_to_one an accepted query's error competes for its train
__global__ __launch_bounds__(O_THREADS) void overlap_accept_kernel(OverlapConst k, int splits, const unsigned long long *__restrict__ part_e,
                                                                   const int *__restrict__ part_t, unsigned long long *__restrict__ best_e,
                                                                   int *__restrict__ best_t, unsigned long long *__restrict__ train_e) {
  const int q = blockIdx.x * O_THREADS + threadIdx.x;
  if (q >= k.n_q) return;
  unsigned long long e = O_NONE;
  int t = -1;
  for (int s = 0; s < splits; s++) {
    const size_t at = (size_t)s * (size_t)k.n_q + (size_t)q;
    const unsigned long long es = part_e[at];
    if (es < e) { e = es; t = part_t[at]; }
  }
  best_e[q] = e; best_t[q] = t;
  if (t >= 0 && k.one_to_one) atomicMin(&train_e[t], e);
}

// ... and of the queries with that error on the train, the lowest index owns it
__global__ __launch_bounds__(O_THREADS) void overlap_owner_kernel(OverlapConst k, const unsigned long long *__restrict__ best_e,
                                                                  const int *__restrict__ best_t, const unsigned long long *__restrict__ train_e,
                                                                  int *__restrict__ train_q) {
  const int q = blockIdx.x * O_THREADS + threadIdx.x;
  if (q >= k.n_q) return;
  const int t = best_t[q];
  if (t >= 0 && train_e[t] == best_e[q]) atomicMin(&train_q[t], q);
}

__device__ __forceinline__ bool overlap_final(const OverlapConst &k, int q, const int *best_t, const int *train_q) {
  if (q >= k.n_q) return false;
  const int t = best_t[q];
  return t >= 0 && (!k.one_to_one || train_q[t] == q);
}

__global__ __launch_bounds__(O_THREADS) void overlap_count_kernel(OverlapConst k, const int *__restrict__ best_t, const int *__restrict__ train_q,
                                                                  int *__restrict__ block_counts) {
  const bool emit = overlap_final(k, blockIdx.x * O_THREADS + threadIdx.x, best_t, train_q);
  const int c = __syncthreads_count(emit ? 1 : 0);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

// Ordered compaction: a block's offset is the sum of the counts of the blocks before it, a query's slot the accepted queries before
// it in its block.  The two terms of the error are computed again from the records: the same operations, the same bits.
// counts_out (pinned): matches, queries and trains in the common area
__global__ __launch_bounds__(O_THREADS) void overlap_emit_kernel(OverlapConst k, const OvRec *__restrict__ qrec, const OvRec *__restrict__ trec,
                                                                 const unsigned long long *__restrict__ best_e, const int *__restrict__ best_t,
                                                                 const int *__restrict__ train_q, const int *__restrict__ block_counts,
                                                                 const int *__restrict__ cnt, mods_overlap_match *__restrict__ out,
                                                                 int *__restrict__ counts_out) {
  __shared__ int s_wave[O_THREADS / 64];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += O_THREADS) part += block_counts[b];
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) s_wave[wv] = part;
  __syncthreads();
  if (tid == 0) { int t = 0; for (int w = 0; w < O_THREADS / 64; w++) t += s_wave[w]; s_base = t; }
  __syncthreads();
  const int base = s_base;
  __syncthreads();
  const int q = blockIdx.x * O_THREADS + tid;
  const bool emit = overlap_final(k, q, best_t, train_q);
  const unsigned long long mm = __ballot(emit);
  if (lane == 0) s_wave[wv] = __popcll(mm);
  __syncthreads();
  int off = base;
  for (int w = 0; w < wv; w++) off += s_wave[w];
  if (emit) {
    const int slot = off + __popcll(mm & ((1ull << lane) - 1ull));
    const int t = best_t[q];
    const OvRec r = qrec[q], tr = trec[t];
    mods_overlap_match m;
    m.q = q; m.t = t;
    m.E = __longlong_as_double((long long)best_e[q]);
    m.dist = overlap_dist(r, tr);
    m.diff = overlap_diff(r, tr, k.oriented != 0);
    out[slot] = m;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {         // total = offset of the last block + its own count
    int t = base;
    for (int w = 0; w < O_THREADS / 64; w++) t += s_wave[w];
    counts_out[0] = t; counts_out[1] = cnt[0]; counts_out[2] = cnt[1];
  }
}

// an empty list on either side: no match, the common counts of the other side stand
__global__ void overlap_empty_kernel(const int *__restrict__ cnt, int *__restrict__ counts_out) {
  counts_out[0] = 0; counts_out[1] = cnt[0]; counts_out[2] = cnt[1];
}

// Every refusal of an overlap call that needs no device; fills the kernels' constants
static int overlap_check(const mods_overlap_params *par, OverlapConst *k) {
  if (!par) { set_error("match_overlap: null argument"); return MODS_E_ARG; }
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(par->H[i])) { set_error("match_overlap: H entry %d is not finite", i); return MODS_E_ARG; }
  if (!std::isfinite(par->max_error) || !(par->max_error > 0)) { set_error("match_overlap: max_error %g (finite, > 0)", par->max_error); return MODS_E_ARG; }
  if (par->oriented != 0 && par->oriented != 1) { set_error("match_overlap: oriented %d (0 or 1)", par->oriented); return MODS_E_ARG; }
  if (par->one_to_one != 0 && par->one_to_one != 1) { set_error("match_overlap: one_to_one %d (0 or 1)", par->one_to_one); return MODS_E_ARG; }
  if (par->w1 < 0 || par->h1 < 0 || par->w2 < 0 || par->h2 < 0) {
    set_error("match_overlap: negative image size (%d x %d, %d x %d)", par->w1, par->h1, par->w2, par->h2);
    return MODS_E_ARG;
  }
  double d;
  if (!invert3_adjugate(par->H, k->Hinv, &d)) { set_error("match_overlap: singular homography (determinant %g)", d); return MODS_E_ARG; }
  for (int i = 0; i < 9; i++) k->H[i] = par->H[i];
  k->n_q = k->n_t = 0;
  k->max_error = par->max_error;
  k->oriented = par->oriented; k->one_to_one = par->one_to_one;
  k->area = par->w1 > 0 && par->h1 > 0 && par->w2 > 0 && par->h2 > 0;
  k->w1 = (double)par->w1; k->h1 = (double)par->h1; k->w2 = (double)par->w2; k->h2 = (double)par->h2;
  k->tiles_per_split = 1;
  return MODS_OK;
}

// the refusals that concern the output, behind those of the parameters
static int overlap_check_out(const mods_overlap_match *out, int max_out, const int *n_out, const mods_overlap_counts *counts) {
  if (!n_out || !counts || max_out < 0 || (max_out > 0 && !out)) { set_error("match_overlap: null argument"); return MODS_E_ARG; }
  return MODS_OK;
}

// The search of device lists; leaves the matches in c->o_out and (matches, common queries, common trains) in c->o_count (pinned;
// valid after a stream wait).  The lists may be empty.
static int overlap_run(mods_ctx *c, const mods_region *q_dev, const mods_region *t_dev, OverlapConst k) {
  if (!c->o_count.get()) { MODS_HIP_CHECK(c->o_count.reserve(4)); }
  const size_t nq = (size_t)k.n_q, nt = (size_t)k.n_t, n = nq + nt;
  const int qblocks = (k.n_q + O_THREADS - 1) / O_THREADS;
  // splits of the train range: some 16 blocks per CU of the 256, so that the last round of blocks is a small part of the sweep even
  // when the query list is short (profiles/overlap_timing.txt: 60 156 x 47 177 takes 2.7 ms unsplit, 1.3 ms with 16 splits)
  const int n_tiles = (k.n_t + O_TILE - 1) / O_TILE;
  int splits = std::max(1, std::min(n_tiles, (4096 + qblocks - 1) / std::max(qblocks, 1)));
  if (c->o_splits > 0) splits = std::max(1, std::min(n_tiles, c->o_splits));
  k.tiles_per_split = std::max(1, (n_tiles + splits - 1) / splits);
  splits = std::max(1, (n_tiles + k.tiles_per_split - 1) / k.tiles_per_split);
  const size_t np = nq * (size_t)splits;
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->o_rec, 6 * (n + 1), 6 * (n + n / 4 + 1)));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->o_key, np + nq + nt + 1, np + nq + nt + n / 4 + 1));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->o_int, np + nq + nt + (size_t)qblocks + 2, np + nq + nt + n / 4 + (size_t)qblocks + 64));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->o_out, nq + 1, nq + nq / 4 + 1));
  OvRec *rec = (OvRec *)c->o_rec.get();
  unsigned long long *train_e = c->o_key, *best_e = train_e + nt, *part_e = best_e + nq;
  int *cnt = c->o_int, *train_q = cnt + 2, *best_t = train_q + nt, *block_counts = best_t + nq, *part_t = block_counts + qblocks;
  StageScope scope(c, MODS_STAGE_OVERLAP, (double)n * sizeof(mods_region));
  MODS_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * 2, c->stream));
  if (k.n_q)
    hipLaunchKernelGGL(overlap_pack_kernel, dim3(qblocks), dim3(O_THREADS), 0, c->stream, k, q_dev, k.n_q, 0, rec, cnt);
  if (k.n_t)
    hipLaunchKernelGGL(overlap_pack_kernel, dim3((k.n_t + O_THREADS - 1) / O_THREADS), dim3(O_THREADS), 0, c->stream, k, t_dev, k.n_t, 1,
                       rec + nq, cnt);
  if (k.n_q == 0 || k.n_t == 0) {
    hipLaunchKernelGGL(overlap_empty_kernel, dim3(1), dim3(1), 0, c->stream, cnt, c->o_count.get());
    MODS_HIP_CHECK(hipGetLastError());
    return MODS_OK;
  }
  if (k.one_to_one) {
    MODS_HIP_CHECK(hipMemsetAsync(train_e, 0xff, sizeof(unsigned long long) * nt, c->stream));
    MODS_HIP_CHECK(hipMemsetAsync(train_q, 0x7f, sizeof(int) * nt, c->stream));
  }
  const dim3 grid(qblocks, splits);
  if (k.oriented) hipLaunchKernelGGL((overlap_sweep_kernel<true>), grid, dim3(O_THREADS), 0, c->stream, k, rec, rec + nq, part_e, part_t);
  else hipLaunchKernelGGL((overlap_sweep_kernel<false>), grid, dim3(O_THREADS), 0, c->stream, k, rec, rec + nq, part_e, part_t);
  hipLaunchKernelGGL(overlap_accept_kernel, dim3(qblocks), dim3(O_THREADS), 0, c->stream, k, splits, part_e, part_t, best_e, best_t, train_e);
  if (k.one_to_one)
    hipLaunchKernelGGL(overlap_owner_kernel, dim3(qblocks), dim3(O_THREADS), 0, c->stream, k, best_e, best_t, train_e, train_q);
  hipLaunchKernelGGL(overlap_count_kernel, dim3(qblocks), dim3(O_THREADS), 0, c->stream, k, best_t, train_q, block_counts);
  hipLaunchKernelGGL(overlap_emit_kernel, dim3(qblocks), dim3(O_THREADS), 0, c->stream, k, rec, rec + nq, best_e, best_t, train_q, block_counts,
                     cnt, c->o_out.get(), c->o_count.get());
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// the counts and, when it fits, the list itself
static int overlap_fetch(mods_ctx *c, mods_overlap_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  const int n = read_slot(c->o_count, 0);
  counts->n_q_common = read_slot(c->o_count, 1);
  counts->n_t_common = read_slot(c->o_count, 2);
  counts->n_matches = n;
  const int lo = std::min(counts->n_q_common, counts->n_t_common);
  counts->repeatability = lo > 0 ? (double)n / (double)lo : 0.;
  *n_out = n;
  if (n > max_out) { set_error("match_overlap: output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
  if (n <= 0) return MODS_OK;
  MODS_HIP_CHECK(hipMemcpyAsync(out, c->o_out, sizeof(mods_overlap_match) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_match_overlap(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, const mods_overlap_params *par,
                       mods_overlap_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  if ((n_q > 0 && !q) || (n_t > 0 && !t)) { set_error("match_overlap: null argument"); return MODS_E_ARG; }
  if (n_q < 0 || n_t < 0) { set_error("match_overlap: negative count (%d queries, %d trains)", n_q, n_t); return MODS_E_ARG; }
  OverlapConst k;
  int rc = overlap_check(par, &k);
  if (rc) return rc;
  if ((rc = overlap_check_out(out, max_out, n_out, counts))) return rc;
  k.n_q = n_q; k.n_t = n_t;
  if (!c) { set_error("match_overlap: null context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const size_t n = (size_t)n_q + (size_t)n_t;
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->o_regs, n + 1, n + n / 4 + 1));
  if (n_q) MODS_HIP_CHECK(hipMemcpyAsync(c->o_regs, q, sizeof(mods_region) * (size_t)n_q, hipMemcpyHostToDevice, c->stream));
  if (n_t) MODS_HIP_CHECK(hipMemcpyAsync(c->o_regs + n_q, t, sizeof(mods_region) * (size_t)n_t, hipMemcpyHostToDevice, c->stream));
  if ((rc = overlap_run(c, c->o_regs, c->o_regs + n_q, k))) return rc;
  return overlap_fetch(c, out, max_out, n_out, counts);
}

int mods_match_overlap_reps(mods_ctx *c, const mods_imgrep *q, const mods_imgrep *t, const mods_overlap_params *par,
                            mods_overlap_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  if (!q || !t) { set_error("match_overlap: null argument"); return MODS_E_ARG; }
  OverlapConst k;
  int rc = overlap_check(par, &k);
  if (rc) return rc;
  if ((rc = overlap_check_out(out, max_out, n_out, counts))) return rc;
  if (!c) { set_error("match_overlap: null context"); return MODS_E_ARG; }
  k.n_q = mods_imgrep_count(q); k.n_t = mods_imgrep_count(t);   // (the banks are read only behind every refusal)
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((rc = overlap_run(c, mods_imgrep_regions_dev(q), mods_imgrep_regions_dev(t), k))) return rc;
  return overlap_fetch(c, out, max_out, n_out, counts);
}

int mods_ctx_overlap_splits(mods_ctx *c, int splits) {
  if (!c || splits < 0) { set_error("overlap_splits: null context or a negative count"); return MODS_E_ARG; }
  c->o_splits = splits;
  return MODS_OK;
}

}  // extern "C"
