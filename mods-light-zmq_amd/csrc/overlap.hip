// Overlap matching: which regions of image 1 have a geometric counterpart in image 2 under a known homography, and how
// repeatable the detector is on the pair.
//
// The reference reads [OverlapMatching] doOverlapMatch / overlapError (io_mods.cpp:685-687) and prints "Overlap matches with E <"
// (mods.cpp:522-523); the error is the linearised one of ellipseOverlapH / ellipseOverlapHPrep (matching/matching.hpp:170-253),
// not the area of intersection.  No descriptor takes part.  The contract (include/mods_hip.h: mods_match_overlap) is bit exact:
// fp64 with one rounding per operation, every reduction a minimum over a total order - so the result does not depend on the
// launch geometry, the train splits or the arrival order of the atomics.
//
// The shape is that of list_search.hpp, with the pack, the one-to-one rule (two atomicMin per train: the error's bits, then the
// query index among the equal ones) and the parameter checks of overlap_common.hpp; a train's 48-byte record holds the inverse
// of its frame (x2 y2 I11 I12 I21 I22).  The sweep takes four trains per branch on the centre term alone: the shape term is
// computed only for a pair whose centre term is below the best error the query has so far (at most max_error), which cannot
// change a minimum because the shape term is never negative.  Each train split leaves its (E, t) per query in a table of its own
// and the accept kernel takes their minimum in split order, so no 96-bit atomic is needed.  VALU only, no matrix cores.
#include "overlap_common.hpp"

namespace mods {

struct OverlapConst {
  int n_q, n_t;
  OvGeom geo;
  double max_error;
  int oriented, one_to_one;
  int tiles_per_split;    // train tiles a block of the sweep walks (blockIdx.y = split)
};

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

// part_e / part_t [split][n_q]: the smallest (E, t) with E < max_error over the trains of the split (LS_NONE: none).
// grid = (ceil(n_q / 256), splits)
template <bool ORIENTED>
__global__ __launch_bounds__(LS_THREADS) void overlap_sweep_kernel(OverlapConst k, const OvRec *__restrict__ qrec, const OvRec *__restrict__ trec,
                                                                  unsigned long long *__restrict__ part_e, int *__restrict__ part_t) {
  __shared__ OvRec s_t[LS_TILE];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * LS_THREADS + tid;
  const OvRec none = overlap_nan_rec();
  OvRec r = none;                                        // lanes past the list
  if (q < k.n_q) r = qrec[q];
  const TrainRange range = train_range(k.n_t, k.tiles_per_split);
  const int t_begin = range.begin, t_end = range.end;
  double best = k.max_error;                             // E >= 0: an error's order is the order of its bits
  int best_t = -1;
  for (int t0 = t_begin; t0 < t_end; t0 += LS_TILE) {
    const int cnt = min(LS_TILE, t_end - t0);             // the tail of the last tile holds records that match nothing
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
    part_e[at] = best_t >= 0 ? (unsigned long long)__double_as_longlong(best) : LS_NONE;
    part_t[at] = best_t;
  }
}

// best_e / best_t[q] = the minimum over the splits, in split order (= train order: ties stay with the lower train); with
// one_to_one an accepted query's error competes for its train
__global__ __launch_bounds__(LS_THREADS) void overlap_accept_kernel(OverlapConst k, int splits, const unsigned long long *__restrict__ part_e,
                                                                   const int *__restrict__ part_t, unsigned long long *__restrict__ best_e,
                                                                   int *__restrict__ best_t, unsigned long long *__restrict__ train_e) {
  const int q = blockIdx.x * LS_THREADS + threadIdx.x;
  if (q >= k.n_q) return;
  unsigned long long e = LS_NONE;
  int t = -1;
  for (int s = 0; s < splits; s++) {
    const size_t at = (size_t)s * (size_t)k.n_q + (size_t)q;
    const unsigned long long es = part_e[at];
    if (es < e) { e = es; t = part_t[at]; }
  }
  best_e[q] = e; best_t[q] = t;
  if (t >= 0 && k.one_to_one) atomicMin(&train_e[t], e);
}

// whether query q is emitted: it has a train and, with one_to_one, owns it
struct overlap_final {
  int n_q, one_to_one;
  const int *best_t, *train_q;
  __device__ bool operator()(int q) const {
    if (q >= n_q) return false;
    const int t = best_t[q];
    return t >= 0 && (!one_to_one || train_q[t] == q);
  }
};

// The emit kernel of the ordered compaction.  The two terms of the error are computed again from the records: the same operations,
// the same bits.  counts_out (pinned): matches, queries and trains in the common area
__global__ __launch_bounds__(LS_THREADS) void overlap_emit_kernel(overlap_final final, int oriented, const OvRec *__restrict__ qrec,
                                                                  const OvRec *__restrict__ trec, const unsigned long long *__restrict__ best_e,
                                                                  const int *__restrict__ block_counts, const int *__restrict__ cnt,
                                                                  mods_overlap_match *__restrict__ out, int *__restrict__ counts_out) {
  __shared__ int s_wave[LS_WAVES];
  const int q = blockIdx.x * LS_THREADS + threadIdx.x;
  const bool emit = final(q);
  int upto;
  const int slot = compact_slot(emit, block_counts, s_wave, &upto);
  if (emit) {
    const int t = final.best_t[q];
    const OvRec r = qrec[q], tr = trec[t];
    mods_overlap_match m;
    m.q = q; m.t = t;
    m.E = __longlong_as_double((long long)best_e[q]);
    m.dist = overlap_dist(r, tr);
    m.diff = overlap_diff(r, tr, oriented != 0);
    out[slot] = m;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { counts_out[0] = upto; counts_out[1] = cnt[0]; counts_out[2] = cnt[1]; }
}

// Every refusal of an overlap call that needs no device, the parameters before the output; fills the kernels' constants
static int overlap_check(const mods_overlap_params *par, const mods_overlap_match *out, int max_out, const int *n_out,
                         const mods_overlap_counts *counts, OverlapConst *k) {
  const int rc = overlap_check_geom("match_overlap", par, [par] {
    if (!std::isfinite(par->max_error) || !(par->max_error > 0)) { set_error("match_overlap: max_error %g (finite, > 0)", par->max_error); return MODS_E_ARG; }
    if (par->oriented != 0 && par->oriented != 1) { set_error("match_overlap: oriented %d (0 or 1)", par->oriented); return MODS_E_ARG; }
    if (par->one_to_one != 0 && par->one_to_one != 1) { set_error("match_overlap: one_to_one %d (0 or 1)", par->one_to_one); return MODS_E_ARG; }
    return MODS_OK;
  }, &k->geo);
  if (rc) return rc;
  k->n_q = k->n_t = 0;
  k->max_error = par->max_error;
  k->oriented = par->oriented; k->one_to_one = par->one_to_one;
  k->tiles_per_split = 1;
  return overlap_check_out("match_overlap", out, max_out, n_out, counts);
}

// The search of device lists; leaves the matches in c->o_out and (matches, common queries, common trains) in c->o_count (pinned;
// valid after a stream wait).  The lists may be empty.
static int overlap_run(mods_ctx *c, const mods_region *q_dev, const mods_region *t_dev, OverlapConst k) {
  if (!c->o_count.get()) { MODS_HIP_CHECK(c->o_count.reserve(4)); }
  const size_t nq = (size_t)k.n_q, nt = (size_t)k.n_t, n = nq + nt;
  const SweepGrid gr = sweep_grid(k.n_q, k.n_t, OVERLAP_TARGET_BLOCKS, c->o_splits);
  const int qblocks = gr.qblocks, splits = gr.splits;
  k.tiles_per_split = gr.tiles_per_split;
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
  overlap_pack<true>(c, k.geo, q_dev, k.n_q, t_dev, k.n_t, rec, cnt);
  if (k.n_q == 0 || k.n_t == 0) {
    hipLaunchKernelGGL(overlap_empty_kernel, dim3(1), dim3(1), 0, c->stream, cnt, c->o_count.get());
    MODS_HIP_CHECK(hipGetLastError());
    return MODS_OK;
  }
  if (k.one_to_one) MODS_HIP_CHECK(overlap_owner_reset(c, train_e, train_q, nt));
  const dim3 grid(qblocks, splits);
  if (k.oriented) hipLaunchKernelGGL((overlap_sweep_kernel<true>), grid, dim3(LS_THREADS), 0, c->stream, k, rec, rec + nq, part_e, part_t);
  else hipLaunchKernelGGL((overlap_sweep_kernel<false>), grid, dim3(LS_THREADS), 0, c->stream, k, rec, rec + nq, part_e, part_t);
  hipLaunchKernelGGL(overlap_accept_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, k, splits, part_e, part_t, best_e, best_t, train_e);
  if (k.one_to_one)
    hipLaunchKernelGGL(overlap_owner_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, k.n_q, best_e, best_t, train_e, train_q);
  const overlap_final final{k.n_q, k.one_to_one, best_t, train_q};
  hipLaunchKernelGGL(compact_count_kernel<overlap_final>, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, final, block_counts);
  hipLaunchKernelGGL(overlap_emit_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, final, k.oriented, rec, rec + nq, best_e, block_counts, cnt,
                     c->o_out.get(), c->o_count.get());
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// the counts and, when it fits, the list itself
static int overlap_fetch(mods_ctx *c, mods_overlap_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  const int n = read_slot(c->o_count, 0);
  overlap_fill_counts(c->o_count, n, counts);
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
  int rc = check_host_lists("match_overlap", q, n_q, t, n_t);
  if (rc) return rc;
  OverlapConst k;
  if ((rc = overlap_check(par, out, max_out, n_out, counts, &k))) return rc;
  k.n_q = n_q; k.n_t = n_t;
  if (!c) { set_error("match_overlap: null context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const mods_region *q_dev, *t_dev;
  if ((rc = stage_lists(c, q, n_q, t, n_t, &q_dev, &t_dev))) return rc;
  if ((rc = overlap_run(c, q_dev, t_dev, k))) return rc;
  return overlap_fetch(c, out, max_out, n_out, counts);
}

int mods_match_overlap_reps(mods_ctx *c, const mods_imgrep *q, const mods_imgrep *t, const mods_overlap_params *par,
                            mods_overlap_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  if (!q || !t) { set_error("match_overlap: null argument"); return MODS_E_ARG; }
  OverlapConst k;
  int rc = overlap_check(par, out, max_out, n_out, counts, &k);
  if (rc) return rc;
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

// the grid of a search's sweep (sweep_grid): host arithmetic only, no device, no launch
int mods_list_search_grid(int search, int n_q, int n_t, int forced_splits, int out[3]) {
  if (!out || (search != 0 && search != 1) || n_q < 0 || n_t < 0 || forced_splits < 0) {
    set_error("list_search_grid: null argument, a search other than 0 or 1 or a negative count");
    return MODS_E_ARG;
  }
  const SweepGrid gr = search == 0 ? sweep_grid(n_q, n_t, GUIDED_TARGET_BLOCKS, 0) : sweep_grid(n_q, n_t, OVERLAP_TARGET_BLOCKS, forced_splits);
  out[0] = gr.qblocks; out[1] = gr.splits; out[2] = gr.tiles_per_split;
  return MODS_OK;
}

}  // extern "C"
