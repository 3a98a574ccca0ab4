// Area-overlap matching: the question of overlap.hip - which regions of image 1 have a geometric counterpart in image 2 under a
// known homography - scored with the measure repeatability figures are quoted in (Mikolajczyk et al., IJCV 2005): one minus
// intersection over union of the two ellipses, the pair rescaled so that the image-1 region has the area of a circle of radius
// 30, the areas counted on the integer lattice.  The contract (include/mods_hip.h: mods_match_overlap_area) is exact: fp64 with one
// rounding per operation in front of three integer counts, so the result does not depend on the launch geometry, the train splits
// or the arrival order of the atomics.
//
// The shape is that of list_search.hpp, with the pack, the one-to-one rule and the parameter checks of overlap_common.hpp; a train
// keeps its frame, not the inverse: the pair's scale comes from the query.  The gate sweep of the n_q x n_t pairs runs twice - it
// counts the pairs to evaluate per (split, query), the host reads their total and sizes the list, it runs again and writes each
// pair to the place the counts give it, so the list is in (split, query, train) order whatever the blocks' order - then one wave
// per listed pair walks the lattice (lanes take consecutive points of the box row by row, three integers per lane, a wave
// reduction), and accept takes per query the minimum over its runs of the list in split order: no atomic on the way.  The
// compaction runs over the queries (modes 0, 1) or over the listed pairs (mode 2, whose sort and greedy pass run on the host).
// VALU only, no matrix cores.
#include "overlap_common.hpp"

namespace mods {

struct AreaConst {
  int n_q, n_t;
  OvGeom geo;
  double max_error;
  double g;               // 0.9 * (1.0 - max_error)
  int one_to_one;         // 0, 1, 2
  int tiles_per_split;    // train tiles a block of the sweep walks (blockIdx.y = split)
};

// query: px py C11 C12 C21 C22     train: x2 y2 M11 M12 M21 M22
using AreaRec = OvRec;

constexpr long long A_MAX_PAIRS = 1ll << 26;   // listed pairs a search may hold (28 bytes each, 60 with the output of mode 2)

// The query's half of a pair's set-up: the scale that gives its ellipse the area of a circle of radius 30, its frame and half
// box at that scale
struct AreaQuery { double px, py, f, Q11, Q12, Q21, Q22, qex, qey; };
__device__ __forceinline__ AreaQuery area_query(const AreaRec &r) {
  AreaQuery q;
  const double detC = r.m11 * r.m22 - r.m12 * r.m21;
  q.px = r.a; q.py = r.b;
  q.f = 30.0 / sqrt(fabs(detC));
  q.Q11 = q.f * r.m11; q.Q12 = q.f * r.m12; q.Q21 = q.f * r.m21; q.Q22 = q.f * r.m22;
  q.qex = sqrt(q.Q11 * q.Q11 + q.Q12 * q.Q12);
  q.qey = sqrt(q.Q21 * q.Q21 + q.Q22 * q.Q22);
  return q;
}

struct AreaPair { double T11, T12, T21, T22, dx, dy; int x0, x1, y0, y1; };
__device__ __forceinline__ double area_min(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double area_max(double a, double b) { return a > b ? a : b; }

// Whether the pair is evaluated; when it is, *p holds the train's frame at the query's scale, the centre offset and the box, which
// lies in [-256, 0] x [0, 256] on either axis.  The cheap area gate goes first; every test fails on NaN
__device__ __forceinline__ bool area_gate(double g, const AreaQuery &q, const AreaRec &t, AreaPair *p) {
  const double T11 = q.f * t.m11, T12 = q.f * t.m12, T21 = q.f * t.m21, T22 = q.f * t.m22;
  const double at = fabs(T11 * T22 - T12 * T21);
  if (!(at >= g * 900.0 && 900.0 >= g * at)) return false;
  const double dx = q.f * (q.px - t.a), dy = q.f * (q.py - t.b);
  const double tex = sqrt(T11 * T11 + T12 * T12);
  if (!(fabs(dx) <= q.qex + tex)) return false;
  const double tey = sqrt(T21 * T21 + T22 * T22);
  if (!(fabs(dy) <= q.qey + tey)) return false;
  const double x0 = floor(area_min(dx - q.qex, -tex)), x1 = ceil(area_max(dx + q.qex, tex));
  const double y0 = floor(area_min(dy - q.qey, -tey)), y1 = ceil(area_max(dy + q.qey, tey));
  if (!(-x0 <= 256.0 && x1 <= 256.0 && -y0 <= 256.0 && y1 <= 256.0)) return false;
  // tex and tey are not NaN and not negative here, so x0, y0 <= 0 <= x1, y1: the four are integers of [-256, 256]
  p->T11 = T11; p->T12 = T12; p->T21 = T21; p->T22 = T22; p->dx = dx; p->dy = dy;
  p->x0 = (int)x0; p->x1 = (int)x1; p->y0 = (int)y0; p->y1 = (int)y1;
  return true;
}

// The gate sweep.  grid = (ceil(n_q / 256), splits); a block's place in the list's order is blockIdx.y * gridDim.x + blockIdx.x.
// EMIT == false: cnt_sq[split][q] = the pairs of the query in the split that are evaluated, block_cnt[block] = their sum.
// EMIT == true (behind the other): off_sq[split][q] = where the query's run of the split starts in the list - the counts of the
// blocks before this one plus those of the block's threads before this one -, pair_q / pair_t = the run, trains ascending
template <bool EMIT>
__global__ __launch_bounds__(LS_THREADS) void area_sweep_kernel(AreaConst k, const AreaRec *__restrict__ qrec, const AreaRec *__restrict__ trec,
                                                               int *__restrict__ cnt_sq, int *__restrict__ block_cnt, int *__restrict__ off_sq,
                                                               int *__restrict__ pair_q, int *__restrict__ pair_t, int n_pairs) {
  __shared__ AreaRec s_t[LS_TILE];
  __shared__ int s_wave[LS_WAVES];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * LS_THREADS + tid;
  const size_t at = (size_t)blockIdx.y * (size_t)k.n_q + (size_t)q;
  AreaRec r = overlap_nan_rec();                            // lanes past the list
  if (q < k.n_q) r = qrec[q];
  const AreaQuery aq = area_query(r);
  int pos = 0, end = 0;
  if (EMIT) {
    const int base = block_sum_before(block_cnt, (int)(blockIdx.y * gridDim.x + blockIdx.x), s_wave);
    const int mine = q < k.n_q ? cnt_sq[at] : 0;
    int total;
    pos = base + block_scan(mine, s_wave, &total);
    end = min(pos + mine, n_pairs);                      // (the counts say it already: no store leaves the list)
    if (q < k.n_q) off_sq[at] = pos;
  }
  const TrainRange range = train_range(k.n_t, k.tiles_per_split);
  const int t_begin = range.begin, t_end = range.end;
  int c = 0;
  for (int t0 = t_begin; t0 < t_end; t0 += LS_TILE) {
    const int n = min(LS_TILE, t_end - t0);
    __syncthreads();
    if (tid < n) s_t[tid] = trec[t0 + tid];
    __syncthreads();
    for (int j = 0; j < n; j++) {
      AreaPair p;
      if (!area_gate(k.g, aq, s_t[j], &p)) continue;
      if (EMIT) {
        if (pos < end) { pair_q[pos] = q; pair_t[pos] = t0 + j; }
        pos++;
      } else c++;
    }
  }
  if (!EMIT) {
    if (q < k.n_q) cnt_sq[at] = c;
    int total;
    block_scan(c, s_wave, &total);
    if (tid == 0) block_cnt[blockIdx.y * gridDim.x + blockIdx.x] = total;
  }
}

// the list's length, as two halves of 64 bits, next to the common counts (pinned)
__global__ __launch_bounds__(LS_THREADS) void area_total_kernel(const int *__restrict__ block_cnt, int n_blocks, int *__restrict__ counts_out) {
  __shared__ unsigned long long s_wave[LS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long part = 0;
  for (int b = tid; b < n_blocks; b += LS_THREADS) part += (unsigned long long)block_cnt[b];
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) s_wave[wv] = part;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < LS_WAVES; w++) t += s_wave[w];
    counts_out[3] = (int)(unsigned)(t & 0xffffffffull); counts_out[4] = (int)(unsigned)(t >> 32);
  }
}

// One wave per listed pair.  The lanes take consecutive points of the box, row by row (a row is 1 .. 513 points); every point is
// decided by the contract's expression.  pair_key = the bits of E when E < max_error (E >= 0: an error's order is the order of
// its bits), LS_NONE otherwise; pair_px = n_q_px, n_t_px, n_both
__global__ __launch_bounds__(LS_THREADS) void area_lattice_kernel(AreaConst k, const AreaRec *__restrict__ qrec, const AreaRec *__restrict__ trec,
                                                                 const int *__restrict__ pair_q, const int *__restrict__ pair_t, int n_pairs,
                                                                 unsigned long long *__restrict__ pair_key, int *__restrict__ pair_px) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * LS_WAVES + (threadIdx.x >> 6);
  if (p >= n_pairs) return;                              // the whole wave
  const AreaQuery aq = area_query(qrec[pair_q[p]]);
  AreaPair g;
  int cq = 0, ct = 0, cb = 0;
  if (area_gate(k.g, aq, trec[pair_t[p]], &g)) {         // (the sweep listed it: the same operations, the same answer)
    const double dq = 1.0 / (aq.Q11 * aq.Q22 - aq.Q12 * aq.Q21);
    const double QI11 = aq.Q22 * dq, QI12 = -(aq.Q12 * dq), QI21 = -(aq.Q21 * dq), QI22 = aq.Q11 * dq;
    const double dt = 1.0 / (g.T11 * g.T22 - g.T12 * g.T21);
    const double TI11 = g.T22 * dt, TI12 = -(g.T12 * dt), TI21 = -(g.T21 * dt), TI22 = g.T11 * dt;
    const int W = g.x1 - g.x0 + 1;                       // 1 .. 513
    int X = g.x0 + lane, Y = g.y0;
    while (X > g.x1) { X -= W; Y++; }
    while (Y <= g.y1) {
      const double Xd = (double)X, Yd = (double)Y;
      const double a = Xd - g.dx, b = Yd - g.dy;
      const double u = QI11 * a + QI12 * b, v = QI21 * a + QI22 * b;
      const bool inQ = u * u + v * v <= 1.0;
      const double u2 = TI11 * Xd + TI12 * Yd, v2 = TI21 * Xd + TI22 * Yd;
      const bool inT = u2 * u2 + v2 * v2 <= 1.0;
      cq += inQ ? 1 : 0; ct += inT ? 1 : 0; cb += (inQ && inT) ? 1 : 0;
      X += 64;
      while (X > g.x1) { X -= W; Y++; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { cq += __shfl_xor(cq, off); ct += __shfl_xor(ct, off); cb += __shfl_xor(cb, off); }
  if (lane == 0) {
    unsigned long long key = LS_NONE;
    const int uni = cq + ct - cb;
    if (uni != 0) {
      const double E = 1.0 - (double)cb / (double)uni;
      if (E < k.max_error) key = (unsigned long long)__double_as_longlong(E);
    }
    pair_key[p] = key;
    pair_px[3 * (size_t)p] = cq; pair_px[3 * (size_t)p + 1] = ct; pair_px[3 * (size_t)p + 2] = cb;
  }
}

// best_e / best_p / best_t[q] = the smallest (E, t) of the query's accepted pairs, its place in the list and its train (-1: none):
// the runs in split order, a run in train order, strict comparisons - a tie stays with the lower train.  With one_to_one == 1 the
// error competes for the train
__global__ __launch_bounds__(LS_THREADS) void area_accept_kernel(AreaConst k, int splits, const int *__restrict__ cnt_sq, const int *__restrict__ off_sq,
                                                                 const unsigned long long *__restrict__ pair_key, const int *__restrict__ pair_t,
                                                                 int n_pairs, unsigned long long *__restrict__ best_e, int *__restrict__ best_p,
                                                                 int *__restrict__ best_t, unsigned long long *__restrict__ train_e) {
  const int q = blockIdx.x * LS_THREADS + threadIdx.x;
  if (q >= k.n_q) return;
  unsigned long long e = LS_NONE;
  int bp = -1;
  for (int s = 0; s < splits; s++) {
    const size_t at = (size_t)s * (size_t)k.n_q + (size_t)q;
    const int o = off_sq[at], end = min(o + cnt_sq[at], n_pairs);
    for (int p = o; p < end; p++) {
      const unsigned long long key = pair_key[p];
      if (key < e) { e = key; bp = p; }
    }
  }
  const int t = bp >= 0 ? pair_t[bp] : -1;
  best_e[q] = e; best_p[q] = bp; best_t[q] = t;
  if (t >= 0 && k.one_to_one == 1) atomicMin(&train_e[t], e);
}

// What the compaction runs over: the queries (modes 0 and 1: a query's chosen pair) or the listed pairs (mode 2: the accepted ones)
struct area_final {
  int n_items, one_to_one;
  const int *best_p, *best_t, *train_q;
  const unsigned long long *pair_key;
  // the list place of item i when it is emitted, -1 otherwise
  __device__ int place(int i) const {
    if (i >= n_items) return -1;
    if (one_to_one == 2) return pair_key[i] != LS_NONE ? i : -1;
    const int p = best_p[i];
    if (p < 0) return -1;
    return (one_to_one == 0 || train_q[best_t[i]] == i) ? p : -1;
  }
  __device__ bool operator()(int i) const { return place(i) >= 0; }
};

// The emit kernel of the ordered compaction.  counts_out (pinned): emitted items, queries and trains in the common area
__global__ __launch_bounds__(LS_THREADS) void area_emit_kernel(area_final final, const int *__restrict__ pair_q, const int *__restrict__ pair_t,
                                                               const int *__restrict__ pair_px, const int *__restrict__ block_counts,
                                                               const int *__restrict__ cnt, mods_overlap_area_match *__restrict__ out,
                                                               int *__restrict__ counts_out) {
  __shared__ int s_wave[LS_WAVES];
  const int p = final.place(blockIdx.x * LS_THREADS + threadIdx.x);
  int upto;
  const int slot = compact_slot(p >= 0, block_counts, s_wave, &upto);
  if (p >= 0) {
    mods_overlap_area_match m;
    m.q = pair_q[p]; m.t = pair_t[p];
    m.E = __longlong_as_double((long long)final.pair_key[p]);
    m.n_q_px = pair_px[3 * (size_t)p]; m.n_t_px = pair_px[3 * (size_t)p + 1]; m.n_both = pair_px[3 * (size_t)p + 2]; m.pad = 0;
    out[slot] = m;                                       // slot < the emitted items <= n_items, the room of `out`
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { counts_out[0] = upto; counts_out[1] = cnt[0]; counts_out[2] = cnt[1]; }
}

// Every refusal of an area-overlap call that needs no device, the parameters before the output; fills the kernels' constants
static int area_check(const mods_overlap_area_params *par, const mods_overlap_area_match *out, int max_out, const int *n_out,
                      const mods_overlap_counts *counts, AreaConst *k) {
  const int rc = overlap_check_geom("match_overlap_area", par, [par] {
    if (!(par->max_error > 0 && par->max_error <= 1)) { set_error("match_overlap_area: max_error %g (in (0, 1])", par->max_error); return MODS_E_ARG; }
    if (par->one_to_one < 0 || par->one_to_one > 2) { set_error("match_overlap_area: one_to_one %d (0, 1 or 2)", par->one_to_one); return MODS_E_ARG; }
    return MODS_OK;
  }, &k->geo);
  if (rc) return rc;
  k->n_q = k->n_t = 0;
  k->max_error = par->max_error;
  k->g = 0.9 * (1.0 - par->max_error);
  k->one_to_one = par->one_to_one;
  k->tiles_per_split = 1;
  return overlap_check_out("match_overlap_area", out, max_out, n_out, counts);
}

// The search of device lists; leaves the emitted items in c->oa_out and (items, common queries, common trains) in c->oa_count
// (pinned; valid after a stream wait).  The lists may be empty.  The stream is waited for once on the way: the second sweep's
// list is sized by what the first one counted
static int area_run(mods_ctx *c, const mods_region *q_dev, const mods_region *t_dev, AreaConst k) {
  if (!c->oa_count.get()) { MODS_HIP_CHECK(c->oa_count.reserve(8)); }
  const size_t nq = (size_t)k.n_q, nt = (size_t)k.n_t, n = nq + nt;
  const SweepGrid gr = sweep_grid(k.n_q, k.n_t, OVERLAP_TARGET_BLOCKS, c->o_splits);
  const int qblocks = gr.qblocks, splits = gr.splits;
  k.tiles_per_split = gr.tiles_per_split;
  const size_t np = nq * (size_t)splits, sblocks = (size_t)qblocks * (size_t)splits;
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->oa_rec, 6 * (n + 1), 6 * (n + n / 4 + 1)));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->oa_int, 2 + nt + 2 * nq + sblocks + 2 * np + 1, 2 + n + nq + n / 4 + sblocks + 2 * np + 64));
  AreaRec *rec = (AreaRec *)c->oa_rec.get();
  int *cnt = c->oa_int, *train_q = cnt + 2, *best_p = train_q + nt, *best_t = best_p + nq, *sweep_cnt = best_t + nq;
  int *cnt_sq = sweep_cnt + sblocks, *off_sq = cnt_sq + np;
  int *counts_out = c->oa_count.get();
  long long n_pairs = 0;
  {
    StageScope scope(c, MODS_STAGE_OVERLAP_AREA, (double)n * sizeof(mods_region));
    MODS_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * 2, c->stream));
    overlap_pack<false>(c, k.geo, q_dev, k.n_q, t_dev, k.n_t, rec, cnt);
    if (k.n_q && k.n_t) {
      hipLaunchKernelGGL((area_sweep_kernel<false>), dim3(qblocks, splits), dim3(LS_THREADS), 0, c->stream, k, rec, rec + nq, cnt_sq, sweep_cnt,
                         off_sq, (int *)nullptr, (int *)nullptr, 0);
      hipLaunchKernelGGL(area_total_kernel, dim3(1), dim3(LS_THREADS), 0, c->stream, sweep_cnt, (int)sblocks, counts_out);
      MODS_HIP_CHECK(hipGetLastError());
    }
  }
  if (k.n_q && k.n_t) {
    MODS_HIP_CHECK(mods::stream_wait(c->stream));
    n_pairs = (long long)(((unsigned long long)(unsigned)read_slot(counts_out, 4) << 32) | (unsigned long long)(unsigned)read_slot(counts_out, 3));
    if (n_pairs > A_MAX_PAIRS) {
      set_error("match_overlap_area: %lld pairs to evaluate, the list holds %lld", n_pairs, A_MAX_PAIRS);
      return MODS_E_CAPACITY;
    }
  }
  StageScope scope(c, MODS_STAGE_OVERLAP_AREA, 0.);
  if (n_pairs == 0) {
    hipLaunchKernelGGL(overlap_empty_kernel, dim3(1), dim3(1), 0, c->stream, cnt, counts_out);
    MODS_HIP_CHECK(hipGetLastError());
    return MODS_OK;
  }
  const int npairs = (int)n_pairs;
  const int n_items = k.one_to_one == 2 ? npairs : k.n_q;
  const int iblocks = (n_items + LS_THREADS - 1) / LS_THREADS;
  const size_t npz = (size_t)npairs;
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->oa_pair, 5 * npz + (size_t)iblocks + 1, 5 * (npz + npz / 4) + (size_t)iblocks + 64));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->oa_key, nt + nq + npz + 1, n + n / 4 + npz + npz / 4 + 1));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->oa_out, (size_t)n_items + 1, (size_t)n_items + (size_t)n_items / 4 + 1));
  int *pair_q = c->oa_pair, *pair_t = pair_q + npz, *pair_px = pair_t + npz, *block_counts = pair_px + 3 * npz;
  unsigned long long *train_e = c->oa_key, *best_e = train_e + nt, *pair_key = best_e + nq;
  MODS_HIP_CHECK(hipMemsetAsync(pair_q, 0, sizeof(int) * 2 * npz, c->stream));   // every place is written below; a valid pair all the same
  hipLaunchKernelGGL((area_sweep_kernel<true>), dim3(qblocks, splits), dim3(LS_THREADS), 0, c->stream, k, rec, rec + nq, cnt_sq, sweep_cnt, off_sq,
                     pair_q, pair_t, npairs);
  hipLaunchKernelGGL(area_lattice_kernel, dim3((npairs + LS_WAVES - 1) / LS_WAVES), dim3(LS_THREADS), 0, c->stream, k, rec, rec + nq, pair_q, pair_t,
                     npairs, pair_key, pair_px);
  if (k.one_to_one != 2) {
    if (k.one_to_one == 1) MODS_HIP_CHECK(overlap_owner_reset(c, train_e, train_q, nt));
    hipLaunchKernelGGL(area_accept_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, k, splits, cnt_sq, off_sq, pair_key, pair_t, npairs, best_e,
                       best_p, best_t, train_e);
    if (k.one_to_one == 1)
      hipLaunchKernelGGL(overlap_owner_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, k.n_q, best_e, best_t, train_e, train_q);
  }
  const area_final final{n_items, k.one_to_one, best_p, best_t, train_q, pair_key};
  hipLaunchKernelGGL(compact_count_kernel<area_final>, dim3(iblocks), dim3(LS_THREADS), 0, c->stream, final, block_counts);
  hipLaunchKernelGGL(area_emit_kernel, dim3(iblocks), dim3(LS_THREADS), 0, c->stream, final, pair_q, pair_t, pair_px, block_counts, cnt,
                     c->oa_out.get(), counts_out);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// The greedy assignment of mode 2 over the accepted pairs: by (E, q, t), a pair is taken when neither region is used yet; what is
// taken goes back into query order (a query is taken once)
static void area_greedy(std::vector<mods_overlap_area_match> &v, int n_q, int n_t) {
  std::sort(v.begin(), v.end(), [](const mods_overlap_area_match &a, const mods_overlap_area_match &b) {
    if (a.E != b.E) return a.E < b.E;
    if (a.q != b.q) return a.q < b.q;
    return a.t < b.t;
  });
  std::vector<unsigned char> used_q((size_t)n_q, 0), used_t((size_t)n_t, 0);
  size_t kept = 0;
  for (const mods_overlap_area_match &m : v)
    if (!used_q[m.q] && !used_t[m.t]) { used_q[m.q] = used_t[m.t] = 1; v[kept++] = m; }
  v.resize(kept);
  std::sort(v.begin(), v.end(), [](const mods_overlap_area_match &a, const mods_overlap_area_match &b) { return a.q < b.q; });
}

// the counts and, when it fits, the list itself
static int area_fetch(mods_ctx *c, const AreaConst &k, mods_overlap_area_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  int n = read_slot(c->oa_count, 0);
  const bool greedy = k.one_to_one == 2;
  if (greedy) {
    c->oa_host.resize((size_t)std::max(n, 0));
    if (n > 0) {
      MODS_HIP_CHECK(hipMemcpyAsync(c->oa_host.data(), c->oa_out, sizeof(mods_overlap_area_match) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
      MODS_HIP_CHECK(mods::stream_wait(c->stream));
      area_greedy(c->oa_host, k.n_q, k.n_t);
      n = (int)c->oa_host.size();
    }
  }
  overlap_fill_counts(c->oa_count, n, counts);
  *n_out = n;
  if (n > max_out) { set_error("match_overlap_area: output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
  if (n <= 0) return MODS_OK;
  if (greedy) { memcpy(out, c->oa_host.data(), sizeof(mods_overlap_area_match) * (size_t)n); return MODS_OK; }
  MODS_HIP_CHECK(hipMemcpyAsync(out, c->oa_out, sizeof(mods_overlap_area_match) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_match_overlap_area(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, const mods_overlap_area_params *par,
                            mods_overlap_area_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  int rc = check_host_lists("match_overlap_area", q, n_q, t, n_t);
  if (rc) return rc;
  AreaConst k;
  if ((rc = area_check(par, out, max_out, n_out, counts, &k))) return rc;
  k.n_q = n_q; k.n_t = n_t;
  if (!c) { set_error("match_overlap_area: null context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const mods_region *q_dev, *t_dev;
  if ((rc = stage_lists(c, q, n_q, t, n_t, &q_dev, &t_dev))) return rc;
  if ((rc = area_run(c, q_dev, t_dev, k))) return rc;
  return area_fetch(c, k, out, max_out, n_out, counts);
}

int mods_match_overlap_area_reps(mods_ctx *c, const mods_imgrep *q, const mods_imgrep *t, const mods_overlap_area_params *par,
                                 mods_overlap_area_match *out, int max_out, int *n_out, mods_overlap_counts *counts) {
  if (!q || !t) { set_error("match_overlap_area: null argument"); return MODS_E_ARG; }
  AreaConst k;
  int rc = area_check(par, out, max_out, n_out, counts, &k);
  if (rc) return rc;
  if (!c) { set_error("match_overlap_area: null context"); return MODS_E_ARG; }
  k.n_q = mods_imgrep_count(q); k.n_t = mods_imgrep_count(t);   // (the banks are read only behind every refusal)
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((rc = area_run(c, mods_imgrep_regions_dev(q), mods_imgrep_regions_dev(t), k))) return rc;
  return area_fetch(c, k, out, max_out, n_out, counts);
}

}  // extern "C"
