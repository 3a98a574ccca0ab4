// Local affine consistency of neighbouring tentatives (include/mods_hip.h: mods_filter_local_affine; no counterpart in the
// reference).  A tentative's two frames predict, through T = (s2 A2)(s1 A1)^-1, where the tentatives around it in image 1 land in
// image 2; it is kept when enough neighbours land there (strong), when a strong one confirms it (rescue), or when it has too few
// neighbours to be judged (keepSparse).  An O(n^2) sweep of fp64 comparisons with integer results, over the packed lists of
// common.hpp (mods_tentative[n] | u6[n][6] | laf[n][14]) - the lists of ALL pairs of a pipeline batch in the same launches
// (the last grid dimension = list), as dedup.hip does:
//   la_prep_kernel     one lane per tentative: T, dT and valid into an SoA scratch (x1 y1 x2 y2 | t00 t01 t10 t11 | dT valid), padded
//                      with NaN positions - nobody's neighbour - up to the launch's bound, a multiple of the tile: the sweeps have no
//                      tail branch and read nothing outside the scratch; and the bounding box of every tile's image-1 positions
//   la_sweep_kernel<1> block (row tile, column split): a lane keeps row i's ten values in registers and walks column tiles staged in
//                      LDS (every lane reads the same entry: a broadcast); a tile whose box is farther than the radius from the
//                      block's box is skipped whole, which pays when the list's order is spatially coherent and costs one test
//                      per tile when it is not.  The radius gate is evaluated for every pair, the rest of
//                      the predicate behind a branch that a wave skips when none of its 64 rows has a neighbour in column j.  A row's
//                      two counts go to neighbours[i] / support[i] with one integer atomicAdd each per block
//   la_sweep_kernel<2> the same walk for the blocks that hold a strong row: backed[j] += the strong rows of the wave that confirm
//                      column j (one ballot, one atomicAdd per wave and confirmed column)
//   la_keep_kernel     one workgroup per list: keep_i and the survivors' places in list order (ballot + prefix, as dup_resolve_kernel)
//   la_copy_kernel     the kept tentatives move to their places in the packed output
// Every output is an integer or a boolean and every comparison is the header's fp64 expression, one rounding per operation
// (-ffp-contract=off): the result cannot depend on the launch geometry, the grouping or the order of the walk.
#include "common.hpp"
#include <algorithm>

namespace mods {

// the bounding box of a tile's image-1 positions, NaN ignored (a tile of padding alone: +inf .. -inf, which is far from everything)
__device__ __forceinline__ double la_wave_min(double v) { for (int o = 32; o; o >>= 1) v = fmin(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ double la_wave_max(double v) { for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o)); return v; }

// grid = (tiles, lists), block LA_TILE
__global__ __launch_bounds__(LA_TILE) void la_prep_kernel(LaBatch b) {
  __shared__ double s_box[LA_TILE / 64][4];
  const LaJob &J = b.job[blockIdx.y];
  const int n = la_len(*J.n_src, b.max_n);
  const int i = blockIdx.x * LA_TILE + threadIdx.x;      // < max_n: the grid is the scratch's tiles
  double *s = b.soa + b.soa_stride * blockIdx.y;
  const size_t m = (size_t)b.max_n;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double x1 = nan, y1 = nan;
  if (i >= n) {          // padding: x1 = NaN makes r2 NaN, which fails r2 <= R2
    for (int q = 0; q < 10; q++) s[q * m + i] = q < 4 ? nan : 0.;
  } else {
    const double *f = (const double *)(J.src + tent_laf_off((size_t)n)) + (size_t)i * 14;
    const double s1 = f[6], s2 = f[13];
    const double m00 = s1 * f[2], m01 = s1 * f[3], m10 = s1 * f[4], m11 = s1 * f[5];
    const double n00 = s2 * f[9], n01 = s2 * f[10], n10 = s2 * f[11], n11 = s2 * f[12];
    const double det = m00 * m11 - m01 * m10;
    const double i00 = m11 / det, i01 = (-m01) / det, i10 = (-m10) / det, i11 = m00 / det;
    const double t00 = n00 * i00 + n01 * i10, t01 = n00 * i01 + n01 * i11, t10 = n10 * i00 + n11 * i10, t11 = n10 * i01 + n11 * i11;
    const double dT = t00 * t11 - t01 * t10;
    const bool valid = isfinite(t00) && isfinite(t01) && isfinite(t10) && isfinite(t11) && isfinite(dT) && dT != 0.;
    x1 = f[0]; y1 = f[1];
    s[0 * m + i] = x1; s[1 * m + i] = y1; s[2 * m + i] = f[7]; s[3 * m + i] = f[8];
    s[4 * m + i] = t00; s[5 * m + i] = t01; s[6 * m + i] = t10; s[7 * m + i] = t11;
    s[8 * m + i] = dT; s[9 * m + i] = valid ? 1. : 0.;
  }
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double x_lo = la_wave_min(fmin(x1, inf)), x_hi = la_wave_max(fmax(x1, -inf));
  const double y_lo = la_wave_min(fmin(y1, inf)), y_hi = la_wave_max(fmax(y1, -inf));
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_box[wv][0] = x_lo; s_box[wv][1] = x_hi; s_box[wv][2] = y_lo; s_box[wv][3] = y_hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double4 box = make_double4(s_box[0][0], s_box[0][1], s_box[0][2], s_box[0][3]);
    for (int q = 1; q < LA_TILE / 64; q++) {
      box.x = fmin(box.x, s_box[q][0]); box.y = fmax(box.y, s_box[q][1]); box.z = fmin(box.z, s_box[q][2]); box.w = fmax(box.w, s_box[q][3]);
    }
    ((double4 *)(s + 10 * m))[blockIdx.x] = box;
  }
}

// The squared distance between two boxes (x_lo x_hi y_lo y_hi).  A pair of positions out of the two boxes is at least that far apart;
// the sweep skips a column tile only when the distance exceeds R2 by more than the roundings of r2 can make up for
__device__ __forceinline__ bool la_boxes_apart(const double4 &a, const double4 &c, double R2) {
  const double gx = fmax(0., fmax(c.x - a.y, a.x - c.y)), gy = fmax(0., fmax(c.z - a.w, a.z - c.w));
  return gx * gx + gy * gy > R2 * (1. + 1e-9);
}

// grid = (row tiles, column splits, lists), block LA_ROWS = LA_TILE
template <int PASS>
__global__ __launch_bounds__(LA_ROWS) void la_sweep_kernel(LaBatch b) {
  __shared__ double4 s_xy[LA_TILE];
  __shared__ double2 s_d[LA_TILE];
  const LaJob &J = b.job[blockIdx.z];
  const int n = la_len(*J.n_src, b.max_n);
  const int i0 = blockIdx.x * LA_ROWS;
  if (i0 >= n) return;
  const LaConst k = b.k;
  const double *s = b.soa + b.soa_stride * blockIdx.z;
  const size_t m = (size_t)b.max_n;
  const int tid = threadIdx.x, i = i0 + tid;      // i < max_n: the scratch is padded to a multiple of the tile
  int *cnt = b.counters + (size_t)3 * b.max_n * blockIdx.z;
  const double x1 = s[0 * m + i], y1 = s[1 * m + i], x2 = s[2 * m + i], y2 = s[3 * m + i];
  const double t00 = s[4 * m + i], t01 = s[5 * m + i], t10 = s[6 * m + i], t11 = s[7 * m + i], dT = s[8 * m + i];
  const bool valid = s[9 * m + i] != 0.;
  const double adT = fabs(dT);
  bool strong = true;
  if (PASS == 2) {
    strong = i < n && cnt[b.max_n + i] >= k.minSupport;
    if (!__syncthreads_or(strong ? 1 : 0)) return;
  }
  int c_nb = 0, c_ok = 0;
  const double4 *box = (const double4 *)(s + 10 * m);
  const double4 my_box = box[blockIdx.x];
  for (int t0 = blockIdx.y * LA_TILE; t0 < n; t0 += gridDim.y * LA_TILE) {
    if (la_boxes_apart(my_box, box[t0 / LA_TILE], k.R2)) continue;       // (uniform) no row of the block has a neighbour in this tile
    __syncthreads();
    {
      const int j = t0 + tid;
      s_xy[tid] = make_double4(s[0 * m + j], s[1 * m + j], s[2 * m + j], s[3 * m + j]);
      s_d[tid] = make_double2(s[8 * m + j], s[9 * m + j]);      // (of a column's frame only dT and valid are read)
    }
    __syncthreads();
    for (int q = 0; q < LA_TILE; q++) {
      const double4 o = s_xy[q];
      const double dx = o.x - x1, dy = o.y - y1, r2 = dx * dx + dy * dy;
      const double gx = o.z - x2, gy = o.w - y2, q2 = gx * gx + gy * gy;
      const bool nb = r2 <= k.R2 && r2 >= k.D2 && q2 >= k.D2 && t0 + q != i;
      bool ok = false;
      if (nb && valid && strong) {
        const double mx = t00 * dx + t01 * dy, my = t10 * dx + t11 * dy;
        const double ex = gx - mx, ey = gy - my, e2 = ex * ex + ey * ey, m2 = mx * mx + my * my;
        ok = e2 <= k.A2 + k.L2 * m2;
        if (ok && k.areaTol != 0.) {
          const double2 d = s_d[q];
          const double adj = fabs(d.x);
          ok = d.y != 0. && dT * d.x > 0. && fmin(adT, adj) * k.areaTol >= fmax(adT, adj);
        }
      }
      if (PASS == 1) { c_nb += nb ? 1 : 0; c_ok += ok ? 1 : 0; }
      else {
        const unsigned long long mm = __ballot(ok);
        if (mm && (tid & 63) == __ffsll((long long)mm) - 1) atomicAdd(&cnt[2 * b.max_n + t0 + q], __popcll(mm));
      }
    }
  }
  if (PASS == 1 && i < n) {
    if (c_nb) atomicAdd(&cnt[i], c_nb);
    if (c_ok) atomicAdd(&cnt[b.max_n + i], c_ok);
  }
}

// grid = lists, one workgroup of 1024 threads each
__global__ __launch_bounds__(1024) void la_keep_kernel(LaBatch b) {
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const LaJob &J = b.job[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_src = *J.n_src;
  int *res = b.res + 2 * blockIdx.x;
  if (n_src > b.max_n) {               // (uniform) a list longer than the launch was sized for: reported, nothing is written
    if (tid == 0) { *J.n_dst = -1; res[0] = 0; }
    return;
  }
  const int n = max(n_src, 0);
  const LaConst k = b.k;
  const int *cnt = b.counters + (size_t)3 * b.max_n * blockIdx.x;
  int *slot_of = b.slots + (size_t)b.max_n * blockIdx.x;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int p0 = 0; p0 < n; p0 += 1024) {
    const int p = p0 + tid;
    bool keep = false;
    if (p < n) {
      const int nbs = cnt[p], sup = cnt[b.max_n + p], backed = cnt[2 * b.max_n + p];
      keep = sup >= k.minSupport || (k.rescue && backed > 0) || (k.keepSparse && nbs < k.minSupport);
    }
    const unsigned long long mm = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(mm);
    __syncthreads();
    int off = s_base;
    for (int q = 0; q < wv; q++) off += s_wave[q];
    if (p < n) slot_of[p] = keep ? off + __popcll(mm & ((1ull << lane) - 1ull)) : -1;
    __syncthreads();
    if (tid == 0) { int t = s_base; for (int q = 0; q < 16; q++) t += s_wave[q]; s_base = t; }
    __syncthreads();
  }
  if (tid == 0) { *J.n_dst = s_base; res[0] = s_base; }
}

// grid = (tiles, lists), block 256
__global__ __launch_bounds__(256) void la_copy_kernel(LaBatch b) {
  const LaJob &J = b.job[blockIdx.y];
  const int n = la_len(*J.n_src, b.max_n), total = b.res[2 * blockIdx.y];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int slot = b.slots[(size_t)b.max_n * blockIdx.y + p];
  if (slot < 0) return;
  const char *src = J.src; char *dst = J.dst;
  const mods_tentative *st = (const mods_tentative *)src;
  const double *su = (const double *)(src + tent_u6_off((size_t)n)), *sl = (const double *)(src + tent_laf_off((size_t)n));
  mods_tentative *dt = (mods_tentative *)dst;
  double *du = (double *)(dst + tent_u6_off((size_t)total)), *dl = (double *)(dst + tent_laf_off((size_t)total));
  dt[slot] = st[p];
#pragma unroll
  for (int q = 0; q < 6; q++) du[(size_t)slot * 6 + q] = su[(size_t)p * 6 + q];
#pragma unroll
  for (int q = 0; q < 14; q++) dl[(size_t)slot * 14 + q] = sl[(size_t)p * 14 + q];
}

// The parameters as the kernels take them; every rule of the header's list, before any device call
int la_check(const mods_local_affine_params *p, LaConst *k) {
  if (!p) { set_error("local_affine: null parameters"); return MODS_E_ARG; }
  if (!std::isfinite(p->radius) || !(p->radius > 0)) { set_error("local_affine: radius %g (finite and > 0)", p->radius); return MODS_E_ARG; }
  if (!(p->minDist >= 0)) { set_error("local_affine: minDist %g (>= 0)", p->minDist); return MODS_E_ARG; }
  if (!(p->absTol >= 0)) { set_error("local_affine: absTol %g (>= 0)", p->absTol); return MODS_E_ARG; }
  if (!(p->relTol >= 0)) { set_error("local_affine: relTol %g (>= 0)", p->relTol); return MODS_E_ARG; }
  if (!(p->areaTol >= 0)) { set_error("local_affine: areaTol %g (>= 0)", p->areaTol); return MODS_E_ARG; }
  if (p->minDist > p->radius) { set_error("local_affine: minDist %g > radius %g", p->minDist, p->radius); return MODS_E_ARG; }
  if (p->areaTol > 0 && p->areaTol < 1) { set_error("local_affine: areaTol %g (0 = no test, or >= 1)", p->areaTol); return MODS_E_ARG; }
  if (p->minSupport < 1) { set_error("local_affine: minSupport %d (>= 1)", p->minSupport); return MODS_E_ARG; }
  if (p->rescue != 0 && p->rescue != 1) { set_error("local_affine: rescue %d (0 or 1)", p->rescue); return MODS_E_ARG; }
  if (p->keepSparse != 0 && p->keepSparse != 1) { set_error("local_affine: keepSparse %d (0 or 1)", p->keepSparse); return MODS_E_ARG; }
  k->R2 = p->radius * p->radius; k->D2 = p->minDist * p->minDist; k->A2 = p->absTol * p->absTol; k->L2 = p->relTol * p->relTol;
  k->areaTol = p->areaTol; k->minSupport = p->minSupport; k->rescue = p->rescue; k->keepSparse = p->keepSparse;
  return MODS_OK;
}

static int la_pad(int n) { return (std::max(n, 1) + LA_TILE - 1) / LA_TILE * LA_TILE; }
// per list: ten SoA doubles, three counters and a place per (padded) position, and two result words
static size_t la_soa_stride(int max_n) { return (size_t)10 * max_n + (size_t)4 * (max_n / LA_TILE); }      // doubles: the SoA arrays, then a box per tile
static size_t la_bytes(int n_jobs, int max_n) { return (la_soa_stride(max_n) * sizeof(double) + (size_t)max_n * 4 * sizeof(int) + 2 * sizeof(int)) * n_jobs + 256; }

// scratch for n_jobs lists of up to grid_n tentatives (mods_ctx_warmup's place for a pipeline: a hipMalloc synchronises the device)
int la_reserve(mods_ctx *c, int n_jobs, int grid_n) {
  if (n_jobs < 1 || n_jobs > LA_MAX_JOBS) { set_error("local_affine: %d lists", n_jobs); return MODS_E_ARG; }
  const size_t bytes = la_bytes(n_jobs, la_pad(grid_n));
  MODS_HIP_CHECK(reserve_scratch(c, c->la_buf, bytes, bytes));
  MODS_HIP_CHECK(c->la_count.reserve(2 * LA_MAX_JOBS));
  return MODS_OK;
}

// Queues the filter behind whatever leaves the packed lists at job[i].src and their lengths at *job[i].n_src (device-readable): the
// kept tentatives go to job[i].dst (room for the source list), their number to *n_dst (-1: the list was longer than grid_n) - valid
// after the stream has been waited for.  grid_n: an upper bound of the list lengths.  diag, when given, receives the device arrays
// of list 0: neighbours | support | backed (3 runs of *diag_stride ints) and the places (-1 = dropped)
int la_filter_dev(mods_ctx *c, const LaJob *jobs, int n_jobs, int grid_n, const LaConst &k, const int **diag_counters,
                  const int **diag_slots, int *diag_stride) {
  { const int rc = la_reserve(c, n_jobs, grid_n); if (rc) return rc; }
  const int max_n = la_pad(grid_n);
  LaBatch b;
  b.n_jobs = n_jobs; b.max_n = max_n; b.k = k;
  b.soa = (double *)c->la_buf.get(); b.soa_stride = la_soa_stride(max_n);
  b.counters = (int *)(b.soa + b.soa_stride * n_jobs);
  b.slots = b.counters + (size_t)3 * max_n * n_jobs;
  b.res = b.slots + (size_t)max_n * n_jobs;
  for (int i = 0; i < n_jobs; i++) b.job[i] = jobs[i];
  if (diag_counters) *diag_counters = b.counters;
  if (diag_slots) *diag_slots = b.slots;
  if (diag_stride) *diag_stride = max_n;
  StageScope ts(c, MODS_STAGE_LOCAL_AFFINE);
  const int tiles = max_n / LA_TILE;
  // enough blocks for a short list to reach every compute unit, few enough atomics for a long one
  const int splits = std::max(1, std::min(tiles, 2048 / (tiles * n_jobs)));
  MODS_HIP_CHECK(hipMemsetAsync(b.counters, 0, sizeof(int) * 3 * (size_t)max_n * n_jobs, c->stream));
  hipLaunchKernelGGL(la_prep_kernel, dim3(tiles, n_jobs), dim3(LA_TILE), 0, c->stream, b);
  hipLaunchKernelGGL((la_sweep_kernel<1>), dim3(tiles, splits, n_jobs), dim3(LA_ROWS), 0, c->stream, b);
  hipLaunchKernelGGL((la_sweep_kernel<2>), dim3(tiles, splits, n_jobs), dim3(LA_ROWS), 0, c->stream, b);
  hipLaunchKernelGGL(la_keep_kernel, dim3(n_jobs), dim3(1024), 0, c->stream, b);
  hipLaunchKernelGGL(la_copy_kernel, dim3(tiles, n_jobs), dim3(256), 0, c->stream, b);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// The filter of the context on a host list that goes to the verification: DuplicateFiltering first when it runs ahead of RANSAC and
// the list has not been through it (`deduped`), then the host-list entry point
int local_affine_prefilter(mods_ctx *c, const mods_pair_params *par, TentList *list, bool deduped) {
  int n = (int)list->size(), rc;
  if (par->dup_before_ransac && !deduped && n > 0) {
    if ((rc = mods_duplicate_filter(list->tent.data(), list->u6.data(), list->laf.data(), n, par->dup_dist, par->dup_mode, &n))) return rc;
    list->truncate((size_t)n);
  }
  int m = n;
  if ((rc = mods_filter_local_affine(c, list->tent.data(), list->u6.data(), list->laf.data(), n, &c->la_par, &m, nullptr, nullptr, nullptr, nullptr))) return rc;
  list->truncate((size_t)m);
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

void mods_local_affine_defaults(mods_local_affine_params *p) {
  if (!p) return;
  p->radius = 160; p->minDist = 3; p->absTol = 4; p->relTol = 0.2; p->areaTol = 2; p->minSupport = 3; p->rescue = 1; p->keepSparse = 1;
}

void mods_local_affine_grid(int *rows, int *tile) {
  if (rows) *rows = LA_ROWS;
  if (tile) *tile = LA_TILE;
}

int mods_filter_local_affine(mods_ctx *c, mods_tentative *tent, double *u6, double *laf, int n, const mods_local_affine_params *par,
                             int *n_out, unsigned char *keep_out, int *neighbours_out, int *support_out, int *backed_out) {
  LaConst k;
  int rc = la_check(par, &k);
  if (rc) return rc;
  if (n < 0) { set_error("local_affine: n = %d", n); return MODS_E_ARG; }
  if (!c || !n_out || (n > 0 && (!tent || !u6 || !laf))) { set_error("local_affine: null argument"); return MODS_E_ARG; }
  *n_out = n;
  c->la_n_in = n; c->la_n_kept = n;
  if (n == 0) return MODS_OK;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((rc = la_reserve(c, 1, n))) return rc;
  const size_t bytes = tent_bytes((size_t)n);
  MODS_HIP_CHECK(reserve_scratch(c, c->la_io, 2 * bytes + 512, 2 * bytes + 512));
  char *src = c->la_io.get(), *dst = src + ((bytes + 255) & ~(size_t)255);
  static thread_local std::vector<char> stage;
  static thread_local std::vector<int> slots;
  stage.resize(bytes);
  tent_pack(stage.data(), (size_t)n, tent, u6, laf);
  MODS_HIP_CHECK(hipMemcpyAsync(src, stage.data(), bytes, hipMemcpyHostToDevice, c->stream));
  c->la_count[0] = n; c->la_count[LA_MAX_JOBS] = 0;
  const LaJob job = {src, dst, c->la_count.get(), c->la_count.get() + LA_MAX_JOBS};
  const int *d_cnt = nullptr, *d_slot = nullptr;
  int stride = 0;
  if ((rc = la_filter_dev(c, &job, 1, n, k, &d_cnt, &d_slot, &stride))) return rc;
  const size_t ib = sizeof(int) * (size_t)n;
  if (neighbours_out) MODS_HIP_CHECK(hipMemcpyAsync(neighbours_out, d_cnt, ib, hipMemcpyDeviceToHost, c->stream));
  if (support_out) MODS_HIP_CHECK(hipMemcpyAsync(support_out, d_cnt + stride, ib, hipMemcpyDeviceToHost, c->stream));
  if (backed_out) MODS_HIP_CHECK(hipMemcpyAsync(backed_out, d_cnt + 2 * (size_t)stride, ib, hipMemcpyDeviceToHost, c->stream));
  if (keep_out) { slots.resize(n); MODS_HIP_CHECK(hipMemcpyAsync(slots.data(), d_slot, ib, hipMemcpyDeviceToHost, c->stream)); }
  MODS_HIP_CHECK(stream_wait(c->stream));        // the one wait ahead of the final copy
  const int m = read_slot(c->la_count, LA_MAX_JOBS);
  if (m < 0 || m > n) { set_error("local_affine: the device returned %d of %d", m, n); return MODS_E_CAPACITY; }
  if (keep_out) for (int i = 0; i < n; i++) keep_out[i] = slots[i] >= 0 ? 1 : 0;
  if (m > 0 && m < n) {
    MODS_HIP_CHECK(copy_wait(c->stream, stage.data(), dst, tent_bytes((size_t)m), hipMemcpyDeviceToHost));
    tent_unpack(stage.data(), (size_t)m, tent, u6, laf);
  }
  *n_out = m;
  c->la_n_kept = m;
  return MODS_OK;
}

int mods_ctx_local_affine(mods_ctx *c, const mods_local_affine_params *par) {
  LaConst k;
  if (par) { const int rc = la_check(par, &k); if (rc) return rc; }
  if (!c) { set_error("local_affine: null context"); return MODS_E_ARG; }
  c->la_on = par != nullptr;
  if (par) c->la_par = *par;
  return MODS_OK;
}

int mods_local_affine_counts(mods_ctx *c, int *n_in, int *n_kept) {
  if (!c || !n_in || !n_kept) { set_error("local_affine_counts: null argument"); return MODS_E_ARG; }
  *n_in = c->la_n_in; *n_kept = c->la_n_kept;
  return MODS_OK;
}

}  // extern "C"
