// Match propagation (include/mods_hip.h: mods_propagate_matches[_dev]; no counterpart in the reference): refined correspondences
// grow into quasi-dense ones over a lattice of cells of image 1, round by round.  All geometry fp64, every decision an integer
// or a total order of integers, so nothing depends on launch geometry or timing.
//   prop_lsm_kernel<K>      the candidate rows of a round (and the seeds) through the shared row body of the least-squares refinement
//                           (lsm_row.hpp): one wave per row, as refine.hip launches it, rows and results in device memory.
//   prop_mark_kernel        round 0: the own cell of every OK seed; occupies it.
//   prop_propose_kernel     one thread per (front row, offset): a 64-bit atomicMin of (bits of (float)d2 << 32 | k) on the cell's key.
//   prop_list_*             the proposed cells in raster order -> candidate rows: per-workgroup counts (1024 cells a workgroup), one
//                           workgroup scans the counts, then every workgroup places its own cells (and clears their keys).
//   prop_gate_kernel        status + model test per candidate: cell state, the tried maps, the statistics, the accept flags and
//                           their per-workgroup counts; prop_scan_kernel again; prop_append_kernel places the accepted rows behind
//                           the output list in raster order.  The tail it wrote is the next front.
// The host waits once per round, behind the list, for the number of candidates (it sizes the LSM and gate launches; the proposal
// of the next round is sized by that bound and reads the front's true length on the device), and once at the end.  A buffer that
// has to grow waits for the stream first (reserve_scratch): the candidate buffer, sized by the front, does so in the early rounds
// of a context's first call and keeps its size; the host entry point waits once more for its image upload.
#include "common.hpp"
#include "lsm_row.hpp"
#include <algorithm>
#include <climits>

namespace mods {

constexpr unsigned long long PROP_NOKEY = ~0ull;
constexpr int PROP_BLOCK = 256, PROP_PER = 4, PROP_TILE = PROP_BLOCK * PROP_PER;   // a workgroup of the scans: 4 consecutive items a thread
constexpr int PROP_INACTIVE = INT_MIN;                                             // front_cell.x of a seed that does not propagate
constexpr int PROP_NS = MODS_PROP_STATUS_COUNT;
enum { PC_NCAND = 0, PC_NOUT = 1, PC_TRUNC = 2, PC_COUNT = 4 };

struct PropLattice { int Gx, Gy, cell, reach; };
struct PropModel { int type; double m[9]; double thr2; };

// inclusive sum over the lanes 0 .. lane of the wave
__device__ __forceinline__ int prop_wave_incl(int c, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(c, o); if (lane >= o) c += v; }
  return c;
}

// the sum of c over the threads before this one in the workgroup of PROP_BLOCK threads; *total = over all of them
__device__ __forceinline__ int prop_block_excl(int c, int *total) {
  __shared__ int ws[PROP_BLOCK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = prop_wave_incl(c, lane);
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < PROP_BLOCK / 64; i++) { if (i < w) off += ws[i]; tot += ws[i]; }
  __syncthreads();
  *total = tot;
  return off + inc - c;
}

__device__ __forceinline__ double prop_centre(int g, int cell) { return (double)(g * cell) + (double)(cell - 1) * 0.5; }

template <int K>
__global__ __launch_bounds__(64 * LSM_WAVES) void prop_lsm_kernel(LsmArgs A) {
  const int row = blockIdx.x * LSM_WAVES + (threadIdx.x >> 6);
  if (row >= A.n) return;
  lsm_row<K>(A, row, threadIdx.x & 63);
}

// grid = ceil(n / PROP_BLOCK).  laf = the seeds' round-0 output rows.  An OK row's x1, y1 lie inside image 1 (its window was sampled)
__global__ __launch_bounds__(PROP_BLOCK) void prop_mark_kernel(const double *laf, const int *status, int n, PropLattice L, unsigned char *state,
                                                               int2 *cellxy, int *stats) {
  __shared__ int hist[PROP_NS];
  if (threadIdx.x < PROP_NS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int k = blockIdx.x * PROP_BLOCK + threadIdx.x;
  if (k < n) {
    const int st = status[k];
    if (st >= 0 && st < PROP_NS) atomicAdd(&hist[st], 1);
    int2 c = make_int2(PROP_INACTIVE, 0);
    if (st == MODS_LSM_OK) {
      c.x = (int)floor(laf[(size_t)k * 14] / (double)L.cell); c.y = (int)floor(laf[(size_t)k * 14 + 1] / (double)L.cell);
      if (c.x >= 0 && c.y >= 0 && c.x < L.Gx && c.y < L.Gy) state[c.y * L.Gx + c.x] = 1;
    }
    cellxy[k] = c;
  }
  __syncthreads();
  if (threadIdx.x < PROP_NS && hist[threadIdx.x]) atomicAdd(&stats[threadIdx.x], hist[threadIdx.x]);
}

// grid = ceil(nf_bound (2 reach + 1)^2 / PROP_BLOCK).  The front has nf_bound rows, or, with n_out_ptr, *n_out_ptr - front_start (never
// more than nf_bound: the host sized the launch before the device knew)
__global__ __launch_bounds__(PROP_BLOCK) void prop_propose_kernel(const double *front_laf, const int2 *front_cell, int nf_bound, const int *n_out_ptr,
                                                                  int front_start, PropLattice L, const unsigned char *state, unsigned long long *key) {
  const int D = 2 * L.reach + 1, DD = D * D;
  int nf = nf_bound;
  if (n_out_ptr) nf = min(nf_bound, *n_out_ptr - front_start);
  const long long t = (long long)blockIdx.x * PROP_BLOCK + threadIdx.x;
  if (t >= (long long)nf * DD) return;
  const int k = (int)(t / DD), o = (int)(t % DD);
  const int2 c = front_cell[k];
  if (c.x == PROP_INACTIVE) return;
  const int gx = c.x + o % D - L.reach, gy = c.y + o / D - L.reach;
  if (gx < 0 || gy < 0 || gx >= L.Gx || gy >= L.Gy) return;
  const int idx = gy * L.Gx + gx;
  if (state[idx] != 0) return;
  const double dx = prop_centre(gx, L.cell) - front_laf[(size_t)k * 14], dy = prop_centre(gy, L.cell) - front_laf[(size_t)k * 14 + 1];
  const float d2 = (float)(dx * dx + dy * dy);
  atomicMin(&key[idx], (unsigned long long)__float_as_uint(d2) << 32 | (unsigned)k);
}

// grid = ceil(G / PROP_TILE): blk[b] = the proposed cells of tile b
__global__ __launch_bounds__(PROP_BLOCK) void prop_list_count_kernel(const unsigned long long *key, int G, int *blk) {
  const int base = blockIdx.x * PROP_TILE + threadIdx.x * PROP_PER;
  int c = 0;
#pragma unroll
  for (int j = 0; j < PROP_PER; j++) if (base + j < G && key[base + j] != PROP_NOKEY) c++;
  int tot;
  prop_block_excl(c, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// one workgroup: blk[0 .. nb) -> its exclusive prefix sums.  mode 0 (list): ctr[PC_NCAND] = the total.  mode 1 (gate): the list
// grows from base by the total, up to cap: ctr[PC_NOUT] = its new length, ctr[PC_TRUNC] = 1 when rows were cut
__global__ __launch_bounds__(PROP_BLOCK) void prop_scan_kernel(int *blk, int nb, int mode, int base, int cap, int *ctr) {
  const int per = (nb + PROP_BLOCK - 1) / PROP_BLOCK, lo = threadIdx.x * per, hi = min(lo + per, nb);
  int s = 0;
  for (int i = lo; i < hi; i++) s += blk[i];
  int tot, off = prop_block_excl(s, &tot);
  for (int i = lo; i < hi; i++) { const int v = blk[i]; blk[i] = off; off += v; }
  if (threadIdx.x != 0) return;
  if (mode == 0) { ctr[PC_NCAND] = tot; return; }
  long long e = (long long)base + tot;
  if (e > cap) { ctr[PC_TRUNC] = 1; e = cap; }
  ctr[PC_NOUT] = (int)e;
}

// grid = ceil(G / PROP_TILE), behind prop_scan_kernel: the candidate rows of the proposed cells, in raster order; their keys are
// cleared (reset) so that every key is PROP_NOKEY again when the next round proposes.  Never more than cand_cap rows
__global__ __launch_bounds__(PROP_BLOCK) void prop_list_kernel(unsigned long long *key, int G, const int *blk, const double *front_laf, int id_base, PropLattice L,
                                                               double *cand, int *cand_cell, int *cand_parent, int cand_cap, int reset) {
  const int base = blockIdx.x * PROP_TILE + threadIdx.x * PROP_PER;
  unsigned long long kk[PROP_PER];
  int c = 0;
#pragma unroll
  for (int j = 0; j < PROP_PER; j++) { kk[j] = base + j < G ? key[base + j] : PROP_NOKEY; if (kk[j] != PROP_NOKEY) c++; }
  int tot;
  int pos = blk[blockIdx.x] + prop_block_excl(c, &tot);
#pragma unroll
  for (int j = 0; j < PROP_PER; j++) {
    if (kk[j] == PROP_NOKEY) continue;
    const int idx = base + j, k = (int)(unsigned)(kk[j] & 0xffffffffull);
    if (reset) key[idx] = PROP_NOKEY;
    if (pos < cand_cap) {
      const double *f = front_laf + (size_t)k * 14;
      const double m00 = f[6] * f[2], m01 = f[6] * f[3], m10 = f[6] * f[4], m11 = f[6] * f[5];
      const double n00 = f[13] * f[9], n01 = f[13] * f[10], n10 = f[13] * f[11], n11 = f[13] * f[12];
      const double d1 = m00 * m11 - m01 * m10;
      const double i00 = m11 / d1, i01 = (-m01) / d1, i10 = (-m10) / d1, i11 = m00 / d1;
      const double b00 = n00 * i00 + n01 * i10, b01 = n00 * i01 + n01 * i11, b10 = n10 * i00 + n11 * i10, b11 = n10 * i01 + n11 * i11;
      const double dB = b00 * b11 - b01 * b10, s = sqrt(dB);
      const double px = prop_centre(idx % L.Gx, L.cell), py = prop_centre(idx / L.Gx, L.cell);
      const double dx = px - f[0], dy = py - f[1];
      double *r = cand + (size_t)pos * 14;
      r[0] = px; r[1] = py; r[2] = 1.; r[3] = 0.; r[4] = 0.; r[5] = 1.; r[6] = 1.;
      r[7] = f[7] + (b00 * dx + b01 * dy); r[8] = f[8] + (b10 * dx + b11 * dy);
      r[9] = b00 / s; r[10] = b01 / s; r[11] = b10 / s; r[12] = b11 / s; r[13] = s;
      cand_cell[pos] = idx; cand_parent[pos] = id_base + k;
    }
    pos++;
  }
}

__device__ __forceinline__ bool prop_on_model(const PropModel &M, double x1, double y1, double x2, double y2) {
  const double *m = M.m;
  if (M.type == 0) {
    const double X = (m[0] * x1 + m[1] * y1) + m[2], Y = (m[3] * x1 + m[4] * y1) + m[5], W = (m[6] * x1 + m[7] * y1) + m[8];
    if (!isfinite(W) || W == 0.) return false;
    const double ex = X / W - x2, ey = Y / W - y2;
    return ex * ex + ey * ey <= M.thr2;
  }
  // F as degensac stores it: Mij = m[3 j + i]
  const double l0 = (m[0] * x1 + m[3] * y1) + m[6], l1 = (m[1] * x1 + m[4] * y1) + m[7], l2 = (m[2] * x1 + m[5] * y1) + m[8];
  const double m0 = (m[0] * x2 + m[1] * y2) + m[2], m1 = (m[3] * x2 + m[4] * y2) + m[5];
  const double e = (l0 * x2 + l1 * y2) + l2, den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
  if (den == 0.) return false;
  return (e * e) / den <= M.thr2;
}

// grid = ceil(n_cand / PROP_TILE), behind the LSM launch of the round: the final status of every candidate, its cell's state and
// tried maps, the round's statistics, the accept flags and blk[b] = the accepted rows of tile b
__global__ __launch_bounds__(PROP_BLOCK) void prop_gate_kernel(const double *out, const int *status, const int *iters, const int *cand_cell, int n_cand,
                                                               PropModel M, unsigned char *state, int *tried_status, int *tried_iters, int *acc, int *blk,
                                                               int *stats) {
  __shared__ int hist[PROP_NS];
  if (threadIdx.x < PROP_NS) hist[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * PROP_TILE + threadIdx.x * PROP_PER;
  int c = 0;
#pragma unroll
  for (int j = 0; j < PROP_PER; j++) {
    const int i = base + j;
    if (i >= n_cand) continue;
    int st = status[i];
    if (st == MODS_LSM_OK && M.type >= 0) {
      const double *r = out + (size_t)i * 14;
      if (!prop_on_model(M, r[0], r[1], r[7], r[8])) st = MODS_PROP_OFF_MODEL;
    }
    const int a = st == MODS_LSM_OK, cell = cand_cell[i];
    state[cell] = a ? 1 : 2; tried_status[cell] = st; tried_iters[cell] = iters[i]; acc[i] = a;
    if (st >= 0 && st < PROP_NS) atomicAdd(&hist[st], 1);
    c += a;
  }
  int tot;
  prop_block_excl(c, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
  __syncthreads();
  if (threadIdx.x < PROP_NS && hist[threadIdx.x]) atomicAdd(&stats[threadIdx.x], hist[threadIdx.x]);
}

struct PropOut { double *laf, *zncc; int *iters, *round, *parent; int2 *cell; };

// grid = ceil(n_cand / PROP_TILE), behind prop_scan_kernel (mode 1): the accepted rows to base, base + 1, ... below cap
__global__ __launch_bounds__(PROP_BLOCK) void prop_append_kernel(const double *out, const double *za, const int *iters, const int *cand_cell, const int *cand_parent,
                                                                 const int *acc, int n_cand, const int *blk, int base, int cap, int round, int Gx, PropOut O) {
  const int first = blockIdx.x * PROP_TILE + threadIdx.x * PROP_PER;
  int a[PROP_PER], c = 0;
#pragma unroll
  for (int j = 0; j < PROP_PER; j++) { a[j] = first + j < n_cand ? acc[first + j] : 0; c += a[j]; }
  int tot;
  long long pos = (long long)base + blk[blockIdx.x] + prop_block_excl(c, &tot);
#pragma unroll
  for (int j = 0; j < PROP_PER; j++) {
    if (!a[j]) continue;
    if (pos < cap) {
      const int i = first + j;
#pragma unroll
      for (int q = 0; q < 14; q++) O.laf[(size_t)pos * 14 + q] = out[(size_t)i * 14 + q];
      O.zncc[pos] = za[i]; O.iters[pos] = iters[i]; O.round[pos] = round; O.parent[pos] = cand_parent[i];
      O.cell[pos] = make_int2(cand_cell[i] % Gx, cand_cell[i] / Gx);
    }
    pos++;
  }
}

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct PropGridLay {      // mods_ctx::prop_grid
  size_t state, key, tst, tit, ctr, stats, blk, bytes;
  int nb;
  PropGridLay(size_t G, int rounds) {
    nb = (int)((G + PROP_TILE - 1) / PROP_TILE) + 1;
    state = 0; key = up16(G); tst = key + G * sizeof(unsigned long long); tit = tst + G * sizeof(int);
    ctr = up16(tit + G * sizeof(int)); stats = ctr + PC_COUNT * sizeof(int); blk = up16(stats + (size_t)(rounds + 1) * PROP_NS * sizeof(int));
    bytes = blk + (size_t)nb * sizeof(int);
  }
};
struct PropRowLay {       // mods_ctx::prop_seed and prop_cand: rows in, rows out, zncc before and after, then five int arrays
  size_t in, out, zb, za, i0, i1, i2, i3, i4, bytes;
  explicit PropRowLay(size_t n) {
    in = 0; out = n * 14 * sizeof(double); zb = 2 * out; za = zb + n * sizeof(double); i0 = za + n * sizeof(double);
    i1 = i0 + n * sizeof(int2); i2 = i1 + n * sizeof(int); i3 = i2 + n * sizeof(int); i4 = i3 + n * sizeof(int); bytes = i4 + n * sizeof(int);
  }
};
struct PropOutLay {       // mods_ctx::prop_out
  size_t laf, zncc, cell, iters, round, parent, bytes;
  explicit PropOutLay(size_t n) {
    laf = 0; zncc = n * 14 * sizeof(double); cell = zncc + n * sizeof(double); iters = cell + n * sizeof(int2); round = iters + n * sizeof(int);
    parent = round + n * sizeof(int); bytes = parent + n * sizeof(int);
  }
};

static int prop_lsm_launch(mods_ctx *c, const LsmArgs &a, int radius) {
  const dim3 grid((unsigned)((a.n + LSM_WAVES - 1) / LSM_WAVES)), block(64 * LSM_WAVES);
  const int per_lane = lsm_per_lane(radius);
  if (per_lane <= 1) hipLaunchKernelGGL(prop_lsm_kernel<1>, grid, block, 0, c->stream, a);
  else if (per_lane <= 2) hipLaunchKernelGGL(prop_lsm_kernel<2>, grid, block, 0, c->stream, a);
  else if (per_lane <= 4) hipLaunchKernelGGL(prop_lsm_kernel<4>, grid, block, 0, c->stream, a);
  else if (per_lane <= 8) hipLaunchKernelGGL(prop_lsm_kernel<8>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(prop_lsm_kernel<16>, grid, block, 0, c->stream, a);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

static LsmArgs prop_lsm_args(const LsmImg &i1, const LsmImg &i2, const mods_lsm_params &p, char *rows, const PropRowLay &R, int n) {
  LsmArgs a;
  a.img[0] = i1; a.img[1] = i2;
  a.laf = (const double *)(rows + R.in); a.laf_out = (double *)(rows + R.out); a.zb = (double *)(rows + R.zb); a.za = (double *)(rows + R.za);
  a.dbg = nullptr; a.status = (int *)(rows + R.i1); a.iters = (int *)(rows + R.i2);
  a.n = n; a.R = p.radius; a.max_iter = p.max_iter; a.affine = p.affine;
  a.eps_shift = p.eps_shift; a.max_shift = p.max_shift; a.max_scale = p.max_scale_change; a.max_mag = p.max_magnification;
  a.min_zncc = p.min_zncc; a.lambda = p.lambda;
  return a;
}

static bool prop_lattice(int w1, int h1, int cell, int reach, PropLattice *L, const char *who) {
  if (cell < 2 || cell > 64) { set_error("%s: cell %d (2 .. 64)", who, cell); return false; }
  if (reach < 1 || reach > 4) { set_error("%s: reach %d (1 .. 4)", who, reach); return false; }
  if (w1 < cell || h1 < cell) { set_error("%s: image 1 of %d x %d holds no cell of %d px", who, w1, h1, cell); return false; }
  L->Gx = w1 / cell; L->Gy = h1 / cell; L->cell = cell; L->reach = reach;
  if ((long long)L->Gx * L->Gy > (1ll << 28)) { set_error("%s: a lattice of %d x %d cells (at most 2^28)", who, L->Gx, L->Gy); return false; }
  return true;
}

// the proposal of `front` and the list of its candidates into the candidate buffer (grown to cand_cap rows first); no wait
static int prop_propose_list(mods_ctx *c, const PropLattice &L, const PropGridLay &GL, const double *front_laf, const int2 *front_cell, int nf_bound,
                             const int *n_out_ptr, int front_start, int id_base, size_t cand_cap, int reset) {
  const int G = L.Gx * L.Gy, D = 2 * L.reach + 1;
  const PropRowLay CL(cand_cap);
  MODS_HIP_CHECK(reserve_scratch(c, c->prop_cand, CL.bytes, CL.bytes + CL.bytes / 4));
  char *g = c->prop_grid.get(), *cd = c->prop_cand.get();
  unsigned long long *key = (unsigned long long *)(g + GL.key);
  int *blk = (int *)(g + GL.blk), *ctr = (int *)(g + GL.ctr);
  const long long threads = (long long)nf_bound * D * D;
  const unsigned nbt = (unsigned)((G + PROP_TILE - 1) / PROP_TILE);
  hipLaunchKernelGGL(prop_propose_kernel, dim3((unsigned)((threads + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, c->stream, front_laf, front_cell,
                     nf_bound, n_out_ptr, front_start, L, (const unsigned char *)(g + GL.state), key);
  hipLaunchKernelGGL(prop_list_count_kernel, dim3(nbt), dim3(PROP_BLOCK), 0, c->stream, (const unsigned long long *)key, G, blk);
  hipLaunchKernelGGL(prop_scan_kernel, dim3(1), dim3(PROP_BLOCK), 0, c->stream, blk, (int)nbt, 0, 0, 0, ctr);
  hipLaunchKernelGGL(prop_list_kernel, dim3(nbt), dim3(PROP_BLOCK), 0, c->stream, key, G, (const int *)blk, front_laf, id_base, L, (double *)(cd + CL.in),
                     (int *)(cd + CL.i3), (int *)(cd + CL.i4), (int)cand_cap, reset);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// how many candidates a front of nf rows can propose: its offsets (the seam's own cells may be free), never more than there are cells
static size_t prop_cand_bound(const PropLattice &L, size_t nf) {
  const size_t D = 2 * (size_t)L.reach + 1;
  return std::max<size_t>(1, std::min((size_t)L.Gx * L.Gy, nf * (D * D)));
}

static int prop_fetch_ctr(mods_ctx *c, const int *ctr_dev, int *ctr) {
  MODS_HIP_CHECK(c->prop_ctr.reserve(PC_COUNT));
  MODS_HIP_CHECK(copy_wait(c->stream, c->prop_ctr.get(), ctr_dev, PC_COUNT * sizeof(int), hipMemcpyDeviceToHost));
  memcpy(ctr, c->prop_ctr.get(), PC_COUNT * sizeof(int));
  return MODS_OK;
}

struct PropResult {
  int max_out;
  double *laf, *u6, *zncc;
  int *iters, *round, *cell, *parent, *n_out, *truncated, *seed_status, *stats, *tried_status, *tried_iters;
};

static int prop_run(mods_ctx *c, const LsmImg &i1, const LsmImg &i2, const double *laf14, int n, const mods_propagate_params &p, const PropLattice &L,
                    const PropResult &res) {
  const size_t G = (size_t)L.Gx * L.Gy, out_cap = std::min<size_t>((size_t)res.max_out, G);
  const PropGridLay GL(G, p.rounds);
  const PropRowLay SL((size_t)n);
  const PropOutLay OL(std::max<size_t>(out_cap, 1));
  MODS_HIP_CHECK(reserve_scratch(c, c->prop_grid, GL.bytes, GL.bytes));
  MODS_HIP_CHECK(reserve_scratch(c, c->prop_seed, SL.bytes, SL.bytes + SL.bytes / 4));
  MODS_HIP_CHECK(reserve_scratch(c, c->prop_out, OL.bytes, OL.bytes));
  char *g = c->prop_grid.get(), *sd = c->prop_seed.get(), *od = c->prop_out.get();
  unsigned char *state = (unsigned char *)(g + GL.state);
  int *tst = (int *)(g + GL.tst), *tit = (int *)(g + GL.tit), *ctr = (int *)(g + GL.ctr), *stats = (int *)(g + GL.stats), *blk = (int *)(g + GL.blk);
  PropOut O;
  O.laf = (double *)(od + OL.laf); O.zncc = (double *)(od + OL.zncc); O.cell = (int2 *)(od + OL.cell); O.iters = (int *)(od + OL.iters);
  O.round = (int *)(od + OL.round); O.parent = (int *)(od + OL.parent);
  PropModel M;
  M.type = p.model_type; M.thr2 = p.model_thr * p.model_thr;
  for (int i = 0; i < 9; i++) M.m[i] = p.model[i];

  MODS_HIP_CHECK(hipMemsetAsync(g + GL.state, 0, G, c->stream));
  MODS_HIP_CHECK(hipMemsetAsync(g + GL.key, 0xff, GL.tit + G * sizeof(int) - GL.key, c->stream));      // keys and both tried maps
  MODS_HIP_CHECK(hipMemsetAsync(g + GL.ctr, 0, GL.blk - GL.ctr, c->stream));                           // counters and statistics
  MODS_HIP_CHECK(hipMemcpyAsync(sd + SL.in, laf14, SL.out, hipMemcpyHostToDevice, c->stream));
  int rc;
  {
    StageScope ts(c, MODS_STAGE_PROPAGATE);
    if ((rc = prop_lsm_launch(c, prop_lsm_args(i1, i2, p.lsm, sd, SL, n), p.lsm.radius))) return rc;
    hipLaunchKernelGGL(prop_mark_kernel, dim3((unsigned)((n + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, c->stream, (const double *)(sd + SL.out),
                       (const int *)(sd + SL.i1), n, L, state, (int2 *)(sd + SL.i0), stats);
    MODS_HIP_CHECK(hipGetLastError());
  }
  // the front: the seeds in round 1, then the tail of the output list from `base`
  const double *front_laf = (const double *)(sd + SL.out);
  const int2 *front_cell = (const int2 *)(sd + SL.i0);
  const int *n_out_ptr = nullptr;
  int nf_bound = n, base = 0, id_base = 0, h[PC_COUNT] = {0, 0, 0, 0};
  for (int r = 1; r <= p.rounds; r++) {
    const size_t cand_cap = prop_cand_bound(L, (size_t)nf_bound);
    {
      StageScope ts(c, MODS_STAGE_PROPAGATE);
      if ((rc = prop_propose_list(c, L, GL, front_laf, front_cell, nf_bound, n_out_ptr, base, id_base, cand_cap, 1))) return rc;
    }
    if ((rc = prop_fetch_ctr(c, ctr, h))) return rc;            // the round's one wait
    const int n_cand = std::min<long long>(h[PC_NCAND], (long long)cand_cap);
    if (h[PC_TRUNC] || n_cand == 0) break;
    base = h[PC_NOUT];                                          // the list's length behind round r - 1
    const PropRowLay CL(cand_cap);
    char *cd = c->prop_cand.get();
    StageScope ts(c, MODS_STAGE_PROPAGATE);
    const LsmArgs a = prop_lsm_args(i1, i2, p.lsm, cd, CL, n_cand);
    if ((rc = prop_lsm_launch(c, a, p.lsm.radius))) return rc;
    const unsigned nbt = (unsigned)((n_cand + PROP_TILE - 1) / PROP_TILE);
    int *acc = (int *)(cd + CL.i0);
    hipLaunchKernelGGL(prop_gate_kernel, dim3(nbt), dim3(PROP_BLOCK), 0, c->stream, (const double *)a.laf_out, (const int *)a.status, (const int *)a.iters,
                       (const int *)(cd + CL.i3), n_cand, M, state, tst, tit, acc, blk, stats + (size_t)r * PROP_NS);
    hipLaunchKernelGGL(prop_scan_kernel, dim3(1), dim3(PROP_BLOCK), 0, c->stream, blk, (int)nbt, 1, base, (int)out_cap, ctr);
    hipLaunchKernelGGL(prop_append_kernel, dim3(nbt), dim3(PROP_BLOCK), 0, c->stream, (const double *)a.laf_out, (const double *)a.za, (const int *)a.iters,
                       (const int *)(cd + CL.i3), (const int *)(cd + CL.i4), (const int *)acc, n_cand, (const int *)blk, base, (int)out_cap, r, L.Gx, O);
    MODS_HIP_CHECK(hipGetLastError());
    front_laf = O.laf + (size_t)base * 14; front_cell = O.cell + base; n_out_ptr = ctr + PC_NOUT;
    nf_bound = (int)std::min<size_t>((size_t)n_cand, out_cap - (size_t)base); id_base = n + base;
    if (nf_bound == 0) break;
  }
  if ((rc = prop_fetch_ctr(c, ctr, h))) return rc;
  const size_t n_out = (size_t)h[PC_NOUT];
  if (n_out && (res.laf || res.u6)) {
    std::vector<double> stage;                                  // only when the caller wants u6 without laf
    double *lo = res.laf;
    if (!lo) { stage.resize(n_out * 14); lo = stage.data(); }
    MODS_HIP_CHECK(copy_wait(c->stream, lo, O.laf, n_out * 14 * sizeof(double), hipMemcpyDeviceToHost));
    if (res.u6) for (size_t i = 0; i < n_out; i++) {
      double *u = res.u6 + 6 * i;
      u[0] = lo[14 * i]; u[1] = lo[14 * i + 1]; u[2] = 1.; u[3] = lo[14 * i + 7]; u[4] = lo[14 * i + 8]; u[5] = 1.;
    }
  }
  if (n_out && res.zncc) MODS_HIP_CHECK(copy_wait(c->stream, res.zncc, O.zncc, n_out * sizeof(double), hipMemcpyDeviceToHost));
  if (n_out && res.cell) MODS_HIP_CHECK(copy_wait(c->stream, res.cell, O.cell, n_out * sizeof(int2), hipMemcpyDeviceToHost));
  if (n_out && res.iters) MODS_HIP_CHECK(copy_wait(c->stream, res.iters, O.iters, n_out * sizeof(int), hipMemcpyDeviceToHost));
  if (n_out && res.round) MODS_HIP_CHECK(copy_wait(c->stream, res.round, O.round, n_out * sizeof(int), hipMemcpyDeviceToHost));
  if (n_out && res.parent) MODS_HIP_CHECK(copy_wait(c->stream, res.parent, O.parent, n_out * sizeof(int), hipMemcpyDeviceToHost));
  if (res.seed_status) MODS_HIP_CHECK(copy_wait(c->stream, res.seed_status, sd + SL.i1, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  if (res.stats) MODS_HIP_CHECK(copy_wait(c->stream, res.stats, stats, (size_t)(p.rounds + 1) * PROP_NS * sizeof(int), hipMemcpyDeviceToHost));
  if (res.tried_status) MODS_HIP_CHECK(copy_wait(c->stream, res.tried_status, tst, G * sizeof(int), hipMemcpyDeviceToHost));
  if (res.tried_iters) MODS_HIP_CHECK(copy_wait(c->stream, res.tried_iters, tit, G * sizeof(int), hipMemcpyDeviceToHost));
  if (res.n_out) *res.n_out = (int)n_out;
  if (res.truncated) *res.truncated = h[PC_TRUNC] ? 1 : 0;
  return MODS_OK;
}

// every refusal of the header's list; *p = the parameters the call runs with, *L = its lattice
static int prop_check_call(const mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2,
                           const double *laf14, int n, const mods_propagate_params *par, int max_out, mods_propagate_params *p, PropLattice *L) {
  const char *who = "propagate_matches";
  if (par) *p = *par; else mods_propagate_defaults(p);
  const int rc = lsm_check(&p->lsm, who);
  if (rc) return rc;
  if (n < 0) { set_error("%s: n = %d", who, n); return MODS_E_ARG; }
  if (max_out < 0) { set_error("%s: max_out = %d", who, max_out); return MODS_E_ARG; }
  if (w1 < 2 || h1 < 2 || w2 < 2 || h2 < 2) { set_error("%s: image size %d x %d, %d x %d (at least 2 x 2)", who, w1, h1, w2, h2); return MODS_E_ARG; }
  if (stride1 < w1 || stride2 < w2) { set_error("%s: stride %d, %d below the width %d, %d", who, stride1, stride2, w1, w2); return MODS_E_ARG; }
  if (p->rounds < 1 || p->rounds > 64) { set_error("%s: rounds %d (1 .. 64)", who, p->rounds); return MODS_E_ARG; }
  if (!prop_lattice(w1, h1, p->cell, p->reach, L, who)) return MODS_E_ARG;
  if (p->model_type < -1 || p->model_type > 1) { set_error("%s: model_type %d (-1 none, 0 = H, 1 = F)", who, p->model_type); return MODS_E_ARG; }
  if (p->model_type >= 0) {
    for (int i = 0; i < 9; i++) if (!std::isfinite(p->model[i])) { set_error("%s: model entry %d is not finite", who, i); return MODS_E_ARG; }
    if (!std::isfinite(p->model_thr) || !(p->model_thr > 0)) { set_error("%s: model_thr %g (finite and > 0)", who, p->model_thr); return MODS_E_ARG; }
  }
  if (!c || !img1 || !img2 || (n > 0 && !laf14)) { set_error("%s: null argument", who); return MODS_E_ARG; }
  return MODS_OK;
}

static PropResult prop_result(int max_out, double *laf_out, double *u6_out, double *zncc_out, int *iters_out, int *round_out, int *cell_out, int *parent_out,
                              int *n_out, int *truncated, int *seed_status, int *stats, int *tried_status, int *tried_iters) {
  return PropResult{max_out, laf_out, u6_out, zncc_out, iters_out, round_out, cell_out, parent_out, n_out, truncated, seed_status, stats, tried_status, tried_iters};
}

}  // namespace mods

using namespace mods;

extern "C" {

void mods_propagate_defaults(mods_propagate_params *p) {
  if (!p) return;
  p->cell = 4; p->reach = 1; p->rounds = 8; p->model_type = -1;
  mods_lsm_defaults(&p->lsm);
  p->lsm.radius = 5;
  for (int i = 0; i < 9; i++) p->model[i] = 0.;
  p->model_thr = 2.0;
}

int mods_propagate_matches_dev(mods_ctx *c, const float *img1_dev, int w1, int h1, int stride1, const float *img2_dev, int w2, int h2, int stride2,
                               const double *laf14, int n, const mods_propagate_params *par, int max_out, double *laf_out, double *u6_out,
                               double *zncc_out, int *iters_out, int *round_out, int *cell_out, int *parent_out, int *n_out, int *truncated,
                               int *seed_status, int *stats, int *tried_status, int *tried_iters) {
  mods_propagate_params p;
  PropLattice L;
  const int rc = prop_check_call(c, img1_dev, w1, h1, stride1, img2_dev, w2, h2, stride2, laf14, n, par, max_out, &p, &L);
  if (rc) return rc;
  if (n == 0) { if (n_out) *n_out = 0; if (truncated) *truncated = 0; return MODS_OK; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  return prop_run(c, LsmImg{img1_dev, w1, h1, stride1}, LsmImg{img2_dev, w2, h2, stride2}, laf14, n, p, L,
                  prop_result(max_out, laf_out, u6_out, zncc_out, iters_out, round_out, cell_out, parent_out, n_out, truncated, seed_status, stats,
                              tried_status, tried_iters));
}

int mods_propagate_matches(mods_ctx *c, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2, int stride2,
                           const double *laf14, int n, const mods_propagate_params *par, int max_out, double *laf_out, double *u6_out,
                           double *zncc_out, int *iters_out, int *round_out, int *cell_out, int *parent_out, int *n_out, int *truncated,
                           int *seed_status, int *stats, int *tried_status, int *tried_iters) {
  mods_propagate_params p;
  PropLattice L;
  int rc = prop_check_call(c, img1, w1, h1, stride1, img2, w2, h2, stride2, laf14, n, par, max_out, &p, &L);
  if (rc) return rc;
  if (n == 0) { if (n_out) *n_out = 0; if (truncated) *truncated = 0; return MODS_OK; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  LsmImg i1, i2;
  if ((rc = lsm_upload(c, c->prop_img, img1, w1, h1, stride1, img2, w2, h2, stride2, &i1, &i2))) return rc;
  return prop_run(c, i1, i2, laf14, n, p, L,
                  prop_result(max_out, laf_out, u6_out, zncc_out, iters_out, round_out, cell_out, parent_out, n_out, truncated, seed_status, stats,
                              tried_status, tried_iters));
}

int mods_test_propagate_round(mods_ctx *c, int w1, int h1, int cell, int reach, const double *front_laf, const int *front_cell, int nf,
                              const unsigned char *state_in, int *winner_out, unsigned long long *key_out, int *cand_cell_out, double *cand_laf_out,
                              int *n_cand_out) {
  const char *who = "propagate_matches";
  PropLattice L;
  if (!prop_lattice(w1, h1, cell, reach, &L, who)) return MODS_E_ARG;
  if (nf < 1) { set_error("%s: a front of %d rows", who, nf); return MODS_E_ARG; }
  if (!c || !front_laf) { set_error("%s: null argument", who); return MODS_E_ARG; }
  const size_t G = (size_t)L.Gx * L.Gy;
  std::vector<int2> cells((size_t)nf);
  for (int k = 0; k < nf; k++) {
    const double x = front_laf[(size_t)k * 14], y = front_laf[(size_t)k * 14 + 1];
    if (!std::isfinite(x) || !std::isfinite(y)) { set_error("%s: front row %d is not finite", who, k); return MODS_E_ARG; }
    const double gx = front_cell ? (double)front_cell[2 * k] : std::floor(x / (double)cell), gy = front_cell ? (double)front_cell[2 * k + 1] : std::floor(y / (double)cell);
    if (!(std::fabs(gx) < 1e6 && std::fabs(gy) < 1e6)) { set_error("%s: front row %d lies in cell (%g, %g)", who, k, gx, gy); return MODS_E_ARG; }
    cells[k] = make_int2((int)gx, (int)gy);
  }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const PropGridLay GL(G, 1);
  const PropRowLay SL((size_t)nf);
  MODS_HIP_CHECK(reserve_scratch(c, c->prop_grid, GL.bytes, GL.bytes));
  MODS_HIP_CHECK(reserve_scratch(c, c->prop_seed, SL.bytes, SL.bytes + SL.bytes / 4));
  char *g = c->prop_grid.get(), *sd = c->prop_seed.get();
  if (state_in) MODS_HIP_CHECK(hipMemcpyAsync(g + GL.state, state_in, G, hipMemcpyHostToDevice, c->stream));
  else MODS_HIP_CHECK(hipMemsetAsync(g + GL.state, 0, G, c->stream));
  MODS_HIP_CHECK(hipMemsetAsync(g + GL.key, 0xff, G * sizeof(unsigned long long), c->stream));
  MODS_HIP_CHECK(hipMemsetAsync(g + GL.ctr, 0, PC_COUNT * sizeof(int), c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(sd + SL.out, front_laf, (size_t)nf * 14 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(hipMemcpyAsync(sd + SL.i0, cells.data(), (size_t)nf * sizeof(int2), hipMemcpyHostToDevice, c->stream));
  MODS_HIP_CHECK(stream_wait(c->stream));                       // `cells` and the caller's arrays are pageable
  const size_t cand_cap = prop_cand_bound(L, (size_t)nf);
  int rc = prop_propose_list(c, L, GL, (const double *)(sd + SL.out), (const int2 *)(sd + SL.i0), nf, nullptr, 0, 0, cand_cap, 0);
  if (rc) return rc;
  int h[PC_COUNT];
  if ((rc = prop_fetch_ctr(c, (const int *)(g + GL.ctr), h))) return rc;
  const size_t n_cand = (size_t)std::min<long long>(h[PC_NCAND], (long long)cand_cap);
  std::vector<unsigned long long> keys(G);
  MODS_HIP_CHECK(copy_wait(c->stream, keys.data(), g + GL.key, G * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < G; i++) {
    if (key_out) key_out[i] = keys[i];
    if (winner_out) winner_out[i] = keys[i] == PROP_NOKEY ? -1 : (int)(unsigned)(keys[i] & 0xffffffffull);
  }
  const PropRowLay CL(cand_cap);
  char *cd = c->prop_cand.get();
  if (n_cand && cand_cell_out) MODS_HIP_CHECK(copy_wait(c->stream, cand_cell_out, cd + CL.i3, n_cand * sizeof(int), hipMemcpyDeviceToHost));
  if (n_cand && cand_laf_out) MODS_HIP_CHECK(copy_wait(c->stream, cand_laf_out, cd + CL.in, n_cand * 14 * sizeof(double), hipMemcpyDeviceToHost));
  if (n_cand_out) *n_cand_out = (int)n_cand;
  return MODS_OK;
}

}  // extern "C"
