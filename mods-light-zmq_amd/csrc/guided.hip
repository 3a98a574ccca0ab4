// Guided matching: a second, model-guided search of two region lists under a verified homography or fundamental matrix.
//
// No counterpart in the reference: its step loop stops at the verified list of the global FGINN search.  Here every query is
// matched again, but only against the trains its position predicts under the model (a symmetric transfer gate for H, a symmetric
// point-to-epipolar-line gate for F), with the FGINN idea kept for the ratio test: the second neighbour is the nearest gated train
// that lies farther than contradDist from the first.  The contract (include/mods_hip.h: mods_match_guided) is bit exact: fp64
// geometry with one rounding per operation, integer descriptor distances, every reduction a minimum over a total order - so the
// result does not depend on the launch geometry, the train splits or the arrival order of the atomics.
//
// The shape is that of list_search.hpp: the pack gives 32-byte fp64 gate records + dense 128-byte descriptor rows (an 8 KB tile
// of records), there are two sweeps of the n_q x n_t gate (nearest gated train, then nearest gated train inconsistent with it),
// accept settles one-to-one by one atomicMin per train, and the emit is in the packed layout of common.hpp.  The sweep takes four
// trains per branch, and the few pairs that pass the gate get their descriptor distance from the whole wave: 32 lanes per
// 128-byte row, two rows at a time.  VALU only, no matrix cores.
#include "list_search.hpp"
#include <cmath>

namespace mods {

struct GuidedConst {
  int n_q, n_t;
  int mode;               // 0 homography, 1 fundamental matrix
  double M[9];            // M[3 * i + j] = entry (i, j) of the model
  double Minv[9];         // mode 0: adjugate / determinant
  double r2, rho2, c2;    // radius^2, ratio^2, contradDist^2
  int max_dist, one_to_one;
  int tiles_per_split;    // train tiles a block of the sweep walks (blockIdx.y = split)
};

__device__ __forceinline__ void guided_project(const double *M, double x, double y, double *px, double *py) {
  const double X = (M[0] * x + M[1] * y) + M[2];
  const double Y = (M[3] * x + M[4] * y) + M[5];
  const double W = (M[6] * x + M[7] * y) + M[8];
  *px = X / W; *py = Y / W;
}

// One list: thread (8 i + c) copies 16-byte chunk c of region i's descriptor, chunk 0's thread also writes the gate record.
//   H, query: px py x1 y1      H, train: x2 y2 bx by
//   F, query: a b c0 gq        F, train: x2 y2 gt 0
__global__ __launch_bounds__(LS_THREADS) void guided_pack_kernel(GuidedConst k, const mods_region *__restrict__ reg, int n, int is_train,
                                                                double4 *__restrict__ rec, uint4 *__restrict__ desc) {
  const size_t gid = (size_t)blockIdx.x * LS_THREADS + threadIdx.x;
  const size_t i = gid >> 3;
  const int ch = (int)(gid & 7);
  if (i >= (size_t)n) return;
  desc[i * 8 + ch] = ((const uint4 *)reg[i].desc)[ch];
  if (ch) return;
  const double x = reg[i].x, y = reg[i].y;
  double4 r;
  if (k.mode == 0) {
    double u, v;
    guided_project(is_train ? k.Minv : k.M, x, y, &u, &v);
    r = is_train ? make_double4(x, y, u, v) : make_double4(u, v, x, y);
  } else if (!is_train) {
    const double a = (k.M[0] * x + k.M[1] * y) + k.M[2];
    const double b = (k.M[3] * x + k.M[4] * y) + k.M[5];
    const double c0 = (k.M[6] * x + k.M[7] * y) + k.M[8];
    r = make_double4(a, b, c0, k.r2 * (a * a + b * b));
  } else {
    const double a = (k.M[0] * x + k.M[3] * y) + k.M[6];
    const double b = (k.M[1] * x + k.M[4] * y) + k.M[7];
    r = make_double4(x, y, k.r2 * (a * a + b * b), 0.);
  }
  rec[i] = r;
}

// The test of one (query record, train record) pair.  A record of NaNs passes nothing: the sweep pads its tiles and its unused
// lanes with them instead of masking.  gate_first is the cheap necessary half that the sweep tries on four trains at a time
// (H: the forward transfer; F: the whole test), gate_rest the remainder
template <int MODE> __device__ __forceinline__ bool gate_first(const double4 r, const double4 tr, double r2) {
  if (MODE == 0) {
    const double dx = r.x - tr.x, dy = r.y - tr.y;
    return dx * dx + dy * dy <= r2;
  }
  const double e = (r.x * tr.x + r.y * tr.y) + r.z;
  const double e2 = e * e;
  return e2 <= r.w && e2 <= tr.z;
}
template <int MODE> __device__ __forceinline__ bool gate_rest(const double4 r, const double4 tr, double r2) {
  if (MODE != 0) return true;
  const double ex = tr.z - r.z, ey = tr.w - r.w;
  return ex * ex + ey * ey <= r2;
}

// The gate sweep.  SECOND = false: out[q] = min (d, t) over the gated trains.  SECOND = true: the same minimum over the gated trains
// other than t1 = the train of best[q] whose centre lies farther than contradDist from t1's.  grid = (ceil(n_q / 256), splits).
template <int MODE, bool SECOND>
__global__ __launch_bounds__(LS_THREADS) void guided_sweep_kernel(GuidedConst k, const double4 *__restrict__ qrec, const double4 *__restrict__ trec,
                                                                 const unsigned int *__restrict__ qdesc, const unsigned int *__restrict__ tdesc,
                                                                 const unsigned long long *__restrict__ best, unsigned long long *__restrict__ out) {
  __shared__ double4 s_t[LS_TILE];
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 31;
  const int q = blockIdx.x * LS_THREADS + tid;
  const int qw = q - lane;                               // the wave's first query
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double4 none = make_double4(nan, nan, nan, nan);
  double4 r = none;                                      // lanes past the list, and (SECOND) queries without a first neighbour
  int t1 = -1;
  double t1x = 0., t1y = 0.;
  if (q < k.n_q) {
    if (SECOND) {
      const unsigned long long k1 = best[q];
      if (k1 != LS_NONE) { r = qrec[q]; t1 = (int)(unsigned int)k1; const double4 c = trec[t1]; t1x = c.x; t1y = c.y; }
    } else r = qrec[q];
  }
  const TrainRange range = train_range(k.n_t, k.tiles_per_split);
  const int t_begin = range.begin, t_end = range.end;
  unsigned long long mine = LS_NONE;
  for (int t0 = t_begin; t0 < t_end; t0 += LS_TILE) {
    const int cnt = min(LS_TILE, t_end - t0);             // the tail of the last tile holds records that pass nothing
    __syncthreads();
    double4 rec = none;
    if (tid < cnt) rec = trec[t0 + tid];
    s_t[tid] = rec;
    __syncthreads();
    for (int j4 = 0; j4 < cnt; j4 += 4) {
      // four trains at a time through the cheap half: every lane reads the same addresses (broadcasts), one branch for the four
      const bool f0 = gate_first<MODE>(r, s_t[j4], k.r2), f1 = gate_first<MODE>(r, s_t[j4 + 1], k.r2);
      const bool f2 = gate_first<MODE>(r, s_t[j4 + 2], k.r2), f3 = gate_first<MODE>(r, s_t[j4 + 3], k.r2);
      if (!__ballot((int)f0 | (int)f1 | (int)f2 | (int)f3)) continue;
#pragma unroll 1
      for (int j = j4; j < j4 + 4; j++) {
        const double4 tr = s_t[j];
        const int t = t0 + j;
        bool pass = gate_first<MODE>(r, tr, k.r2) && gate_rest<MODE>(r, tr, k.r2);
        if (SECOND) {
          const double cx = tr.x - t1x, cy = tr.y - t1y;
          pass = pass && t != t1 && (cx * cx + cy * cy > k.c2);
        }
        unsigned long long m = __ballot(pass);
        if (!m) continue;
        // descriptor distances of the wave's gated pairs: lanes 0..31 take one pair, lanes 32..63 the next, four bytes per lane
        unsigned int d = 0;
        const unsigned int tb = tdesc[(size_t)t * 32 + sub];
        const unsigned int tt = __builtin_amdgcn_udot4(tb, tb, 0u, false);
        while (m) {
          const int l0 = __ffsll((long long)m) - 1;
          m &= m - 1;
          int l1 = l0;
          if (m) { l1 = __ffsll((long long)m) - 1; m &= m - 1; }
          const int src = lane < 32 ? l0 : l1;
          const unsigned int qb = qdesc[(size_t)(qw + src) * 32 + sub];
          // sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a b, exact in 32 bits
          unsigned int s = __builtin_amdgcn_udot4(qb, qb, tt, false) - 2u * __builtin_amdgcn_udot4(qb, tb, 0u, false);
          for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off);
          const unsigned int da = __shfl(s, 0), db = __shfl(s, 32);
          if (lane == l0) d = da;
          if (lane == l1) d = db;
        }
        if (pass) {
          const unsigned long long key = ((unsigned long long)d << 32) | (unsigned int)t;
          if (key < mine) mine = key;
        }
      }
    }
  }
  if (mine != LS_NONE) atomicMin(&out[q], mine);
}

// acc[q] = the query passes the distance cap and the ratio test; with one_to_one its (d1, q) competes for its train
__global__ __launch_bounds__(LS_THREADS) void guided_accept_kernel(GuidedConst k, const unsigned long long *__restrict__ best,
                                                                  const unsigned long long *__restrict__ second, int *__restrict__ acc,
                                                                  unsigned long long *__restrict__ train_best) {
  const int q = blockIdx.x * LS_THREADS + threadIdx.x;
  if (q >= k.n_q) return;
  const unsigned long long k1 = best[q], k2 = second[q];
  bool ok = k1 != LS_NONE;
  if (ok) {
    const int d1 = (int)(k1 >> 32);
    ok = k.max_dist == 0 || d1 <= k.max_dist;
    if (k2 != LS_NONE) ok = ok && ((double)d1 < k.rho2 * (double)(int)(k2 >> 32));
    if (ok && k.one_to_one) atomicMin(&train_best[(unsigned int)k1], (k1 & 0xffffffff00000000ull) | (unsigned int)q);
  }
  acc[q] = ok ? 1 : 0;
}

// whether query q is emitted: it was accepted and, with one_to_one, owns its train
struct guided_final {
  int n_q, one_to_one;
  const unsigned long long *best, *train_best;
  const int *acc;
  __device__ bool operator()(int q) const {
    if (q >= n_q || !acc[q]) return false;
    return !one_to_one || (unsigned int)train_best[(unsigned int)best[q]] == (unsigned int)q;
  }
};

// The emit kernel of the ordered compaction.  Output in the packed layout of common.hpp (tentatives | correspondences | frames),
// whose parts lie where the total count puts them: every block sums all the block counts before it writes
__global__ __launch_bounds__(LS_THREADS) void guided_emit_kernel(guided_final final, const unsigned long long *__restrict__ second,
                                                                 const int *__restrict__ block_counts, const mods_region *__restrict__ qreg,
                                                                 const mods_region *__restrict__ treg, char *__restrict__ out,
                                                                 int *__restrict__ out_count) {
  __shared__ int s_wave[LS_WAVES];
  const size_t n_out = (size_t)block_sum_before(block_counts, (int)gridDim.x, s_wave);   // at most n_q, which the output buffer holds
  mods_tentative *tent = (mods_tentative *)out;
  double *u6 = (double *)(out + tent_u6_off(n_out)), *laf = (double *)(out + tent_laf_off(n_out));
  const int q = blockIdx.x * LS_THREADS + threadIdx.x;
  const bool emit = final(q);
  int upto;
  const int slot = compact_slot(emit, block_counts, s_wave, &upto);
  if (emit) {
    const unsigned long long k1 = final.best[q], k2 = second[q];
    const int d1 = (int)(k1 >> 32), d2 = k2 != LS_NONE ? (int)(k2 >> 32) : 0;
    mods_tentative tc;
    tc.q = q; tc.t = (int)(unsigned int)k1; tc.t_bad = k2 != LS_NONE ? (int)(unsigned int)k2 : -1; tc.t_2nd = -1;
    tc.d1 = (float)d1; tc.d2 = (float)d2; tc.d2nd = 0.f; tc.pad = 0.f;
    tc.ratio = k2 != LS_NONE ? sqrt((double)d1 / (double)d2) : 0.;
    tent[slot] = tc;
    const mods_region &r1 = qreg[tc.q], &r2 = treg[tc.t];
    double *u = u6 + (size_t)slot * 6;
    u[0] = r1.x; u[1] = r1.y; u[2] = 1.; u[3] = r2.x; u[4] = r2.y; u[5] = 1.;
    double *f = laf + (size_t)slot * 14;
    f[0] = r1.x; f[1] = r1.y; f[2] = r1.a11; f[3] = r1.a12; f[4] = r1.a21; f[5] = r1.a22; f[6] = r1.s;
    f[7] = r2.x; f[8] = r2.y; f[9] = r2.a11; f[10] = r2.a12; f[11] = r2.a21; f[12] = r2.a22; f[13] = r2.s;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *out_count = upto;
}

// Every refusal of a guided call that needs no device, the parameters before the output; fills the kernels' constants
static int guided_check(const mods_guided_params *par, const mods_tentative *out, int max_out, GuidedConst *k) {
  if (!par) { set_error("match_guided: null argument"); return MODS_E_ARG; }
  if (par->model_type != 0 && par->model_type != 1) { set_error("match_guided: model_type %d (0 or 1)", par->model_type); return MODS_E_ARG; }
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(par->model[i])) { set_error("match_guided: model entry %d is not finite", i); return MODS_E_ARG; }
  if (!std::isfinite(par->radius) || !(par->radius > 0)) { set_error("match_guided: radius %g (finite, > 0)", par->radius); return MODS_E_ARG; }
  if (!(par->ratio > 0 && par->ratio <= 1)) { set_error("match_guided: ratio %g outside (0, 1]", par->ratio); return MODS_E_ARG; }
  if (!std::isfinite(par->contradDist) || par->contradDist < 0) { set_error("match_guided: contradDist %g (finite, >= 0)", par->contradDist); return MODS_E_ARG; }
  if (par->max_dist < 0) { set_error("match_guided: max_dist %d < 0", par->max_dist); return MODS_E_ARG; }
  k->n_q = k->n_t = 0; k->mode = par->model_type;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) k->M[3 * r + c] = par->model_type == 0 ? par->model[3 * r + c] : par->model[3 * c + r];
  for (int i = 0; i < 9; i++) k->Minv[i] = 0;
  if (par->model_type == 0) {
    double d;
    if (!invert3_adjugate(k->M, k->Minv, &d)) { set_error("match_guided: singular homography (determinant %g)", d); return MODS_E_ARG; }
  }
  k->r2 = par->radius * par->radius;
  k->rho2 = par->ratio * par->ratio;
  k->c2 = par->contradDist * par->contradDist;
  k->max_dist = par->max_dist; k->one_to_one = par->one_to_one ? 1 : 0;
  k->tiles_per_split = 1;
  if (max_out < 0 || (max_out > 0 && !out)) { set_error("match_guided: null argument"); return MODS_E_ARG; }
  return MODS_OK;
}

template <int MODE, bool SECOND>
static void launch_sweep(mods_ctx *c, dim3 grid, const GuidedConst &k, const double4 *rec, const unsigned int *desc,
                         const unsigned long long *best, unsigned long long *out) {
  hipLaunchKernelGGL((guided_sweep_kernel<MODE, SECOND>), grid, dim3(LS_THREADS), 0, c->stream, k, rec, rec + k.n_q, desc,
                     desc + (size_t)k.n_q * 32, best, out);
}

// The search of device lists; leaves the packed result in c->g_tent and its length in c->g_count[0] (pinned; valid after a
// stream wait).  The lists may be empty.
static int guided_run(mods_ctx *c, const mods_region *q_dev, const mods_region *t_dev, GuidedConst k) {
  if (!c->g_count.get()) { MODS_HIP_CHECK(c->g_count.reserve(4)); }
  if (k.n_q == 0 || k.n_t == 0) {
    MODS_HIP_CHECK(mods::stream_wait(c->stream));
    c->g_count[0] = 0;
    return MODS_OK;
  }
  const size_t nq = (size_t)k.n_q, nt = (size_t)k.n_t, n = nq + nt;
  const SweepGrid gr = sweep_grid(k.n_q, k.n_t, GUIDED_TARGET_BLOCKS, 0);
  const int qblocks = gr.qblocks;
  k.tiles_per_split = gr.tiles_per_split;
  const dim3 grid(qblocks, gr.splits);
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->g_rec, n, n + n / 4));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->g_desc, n * 128, (n + n / 4) * 128));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->g_key, 2 * nq + nt, 2 * nq + nt + n / 4));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->g_int, nq + (size_t)qblocks, nq + nq / 4 + (size_t)qblocks + 64));
  MODS_HIP_CHECK(mods::reserve_scratch(c, c->g_tent, tent_bytes(nq), tent_bytes(nq + nq / 4)));
  double4 *rec = c->g_rec;
  uint4 *desc = (uint4 *)c->g_desc.get();
  unsigned long long *best = c->g_key, *second = best + nq, *train_best = second + nq;
  int *acc = c->g_int, *block_counts = acc + nq;
  StageScope scope(c, MODS_STAGE_GUIDED, (double)n * sizeof(mods_region));
  MODS_HIP_CHECK(hipMemsetAsync(best, 0xff, sizeof(unsigned long long) * (2 * nq + nt), c->stream));
  hipLaunchKernelGGL(guided_pack_kernel, dim3((unsigned)((nq * 8 + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, c->stream, k, q_dev,
                     k.n_q, 0, rec, desc);
  hipLaunchKernelGGL(guided_pack_kernel, dim3((unsigned)((nt * 8 + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, c->stream, k, t_dev,
                     k.n_t, 1, rec + nq, desc + nq * 8);
  const unsigned int *d32 = (const unsigned int *)desc;
  if (k.mode == 0) { launch_sweep<0, false>(c, grid, k, rec, d32, best, best); launch_sweep<0, true>(c, grid, k, rec, d32, best, second); }
  else { launch_sweep<1, false>(c, grid, k, rec, d32, best, best); launch_sweep<1, true>(c, grid, k, rec, d32, best, second); }
  hipLaunchKernelGGL(guided_accept_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, k, best, second, acc, train_best);
  const guided_final final{k.n_q, k.one_to_one, best, train_best, acc};
  hipLaunchKernelGGL(compact_count_kernel<guided_final>, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, final, block_counts);
  hipLaunchKernelGGL(guided_emit_kernel, dim3(qblocks), dim3(LS_THREADS), 0, c->stream, final, second, block_counts, q_dev, t_dev,
                     c->g_tent.get(), c->g_count.get());
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// the length and, when it fits, the list itself: one device-to-host copy of the packed form
static int guided_fetch(mods_ctx *c, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out) {
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  const int n = read_slot(c->g_count, 0);
  *n_out = n;
  if (n > max_out) { set_error("match_guided: tentative output overflow: %d > %d", n, max_out); return MODS_E_CAPACITY; }
  if (n <= 0) return MODS_OK;
  static thread_local std::vector<char> stage;
  stage.resize(tent_bytes((size_t)n));
  MODS_HIP_CHECK(hipMemcpyAsync(stage.data(), c->g_tent, stage.size(), hipMemcpyDeviceToHost, c->stream));
  MODS_HIP_CHECK(mods::stream_wait(c->stream));
  tent_unpack(stage.data(), (size_t)n, out, u6_out, laf_out);
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_match_guided(mods_ctx *c, const mods_region *q, int n_q, const mods_region *t, int n_t, const mods_guided_params *par,
                      mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out) {
  if (!n_out) { set_error("match_guided: null argument"); return MODS_E_ARG; }
  int rc = check_host_lists("match_guided", q, n_q, t, n_t);
  if (rc) return rc;
  GuidedConst k;
  if ((rc = guided_check(par, out, max_out, &k))) return rc;
  k.n_q = n_q; k.n_t = n_t;
  if (!c) { set_error("match_guided: null context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const mods_region *q_dev, *t_dev;
  if ((rc = stage_lists(c, q, n_q, t, n_t, &q_dev, &t_dev))) return rc;
  if ((rc = guided_run(c, q_dev, t_dev, k))) return rc;
  return guided_fetch(c, out, u6_out, laf_out, max_out, n_out);
}

int mods_match_guided_reps(mods_ctx *c, const mods_imgrep *q, const mods_imgrep *t, const mods_guided_params *par, mods_tentative *out,
                           double *u6_out, double *laf_out, int max_out, int *n_out) {
  if (!n_out || !q || !t) { set_error("match_guided: null argument"); return MODS_E_ARG; }
  GuidedConst k;
  int rc = guided_check(par, out, max_out, &k);
  if (rc) return rc;
  if (!c) { set_error("match_guided: null context"); return MODS_E_ARG; }
  k.n_q = mods_imgrep_count(q); k.n_t = mods_imgrep_count(t);   // (the banks are read only behind every refusal)
  MODS_HIP_CHECK(hipSetDevice(c->device));
  if ((rc = guided_run(c, mods_imgrep_regions_dev(q), mods_imgrep_regions_dev(t), k))) return rc;
  return guided_fetch(c, out, u6_out, laf_out, max_out, n_out);
}

}  // extern "C"
