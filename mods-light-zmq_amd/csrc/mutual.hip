// Mutual nearest-neighbour check of the FGINN matcher (mods_ctx_match_mutual; contract in include/mods_hip.h).
//
// No counterpart in the reference: its matcher is one-directional.  Here a forward tentative (q, t) with d1 = d(q, t) is dropped when
//   mode 1, 2   some other query r of the list lies before q in (d(r, t), r) order, or
//   mode 2      some other query r farther than contradDist from q fails the forward ratio test with the roles swapped:
//               fl32(d1 / d(r, t)) <= ratio^2 is false.  The quotient is monotone in d(r, t), so that is d(r, t) < D*, the smallest
//               integer distance passing the test against d1 - the dstar that match_mid_kernel left in the query's QueryMid.
// Both are OR-predicates over the query list: nothing is ordered or reduced, so the result cannot depend on the launch geometry.
//
// The stage runs between match_fginn_kernel and the emit kernels, on what the forward search left in the matcher's scratch buffers:
// mutual_list_kernel evaluates fginn_accept for every query and collects the accepted ones as (q, t, d1, D*), mutual_sweep_kernel
// checks them against all queries and stores bad[q] = 1 for the ones that fail; the emit kernels then pass those by.  A thread of
// the sweep owns a candidate (its train's 128 int8 in 32 registers), the block walks its share of the packed query list through LDS
// tiles that every lane reads at the same address (a broadcast), the distance is cq + ct - 2 dot by v_dot4 - the integers of the
// forward search.  VALU only, no matrix cores.
#include "match_types.hpp"

namespace mods {

constexpr int MU_THREADS = 256;      // candidates per block of the sweep, threads of both kernels
constexpr int MU_TILE = 64;          // queries per LDS tile (8 KB of descriptors + norms + centres)
constexpr int MU_MIN_TPS = 4;        // a block of the sweep walks at least this many tiles (256 queries) ...
constexpr int MU_MAX_SPLITS = 64;    // ... and the query list is cut into at most this many shares (blockIdx.y)

// the sweep's share count for a query list (the grid's y extent; a group takes its longest list's)
static int mutual_splits(int n_q) {
  const int n_tiles = (n_q + MU_TILE - 1) / MU_TILE;
  return std::max(1, std::min(MU_MAX_SPLITS, (n_tiles + MU_MIN_TPS - 1) / MU_MIN_TPS));
}

// The accepted queries of every search, in any order.  grid = (ceil(max n_q / 256), searches), block 256; count[search] zeroed before
__global__ __launch_bounds__(MU_THREADS) void mutual_list_kernel(MatchJobs J, MatchConst k, const QueryMid *__restrict__ mid,
                                                                 const unsigned long long *__restrict__ key_ge,
                                                                 const unsigned long long *__restrict__ key_lt, const int *__restrict__ n_lt,
                                                                 const int *__restrict__ bad, int4 *__restrict__ cand, size_t s_cand,
                                                                 int *__restrict__ count) {
  const int job = blockIdx.y;
  k.n_q = J.n_q[job]; k.n_t = J.n_t[job];
  if ((int)blockIdx.x * MU_THREADS >= k.n_q) return;
  mid = set_el(mid, job, J.s_mid); key_ge = set_el(key_ge, job, J.s_u64); key_lt = set_el(key_lt, job, J.s_u64);
  n_lt = set_el(n_lt, job, J.s_int); bad = set_el(bad, job, J.s_int); cand = set_el(cand, job, s_cand);
  const int j = blockIdx.x * MU_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  mods_tentative tc;
  const bool acc = fginn_accept(k, j, mid, key_ge, key_lt, n_lt, bad, &tc);
  const unsigned long long m = __ballot(acc);
  if (!m) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(&count[job], __popcll(m));     // one atomic per wave
  base = __shfl(base, 0);
  if (acc) cand[base + __popcll(m & ((1ull << lane) - 1ull))] = make_int4(j, tc.t, mid[j].d0, mid[j].dstar);
}

// Candidates x all queries.  grid = (ceil(max n_q / 256), splits, searches): x covers the worst case of every query accepted, blocks
// past the device-side count exit.  MODE: 1 or 2
template <int MODE>
__global__ __launch_bounds__(MU_THREADS) void mutual_sweep_kernel(MatchJobs J, double contr_sq, const int4 *__restrict__ cand, size_t s_cand,
                                                                  const int *__restrict__ count, int *__restrict__ count_host,
                                                                  const int8_t *__restrict__ qdesc, const int *__restrict__ qc,
                                                                  const double2 *__restrict__ qxy, const int8_t *__restrict__ tdesc,
                                                                  const int *__restrict__ tc, int *__restrict__ bad) {
  __shared__ uint4 s_d[MU_TILE * 8];
  __shared__ int s_c[MU_TILE];
  __shared__ double2 s_xy[MU_TILE];
  const int job = blockIdx.z, tid = threadIdx.x;
  const int n_c = count[job];
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) count_host[job] = n_c;      // pinned: mods_match_mutual_counts
  if ((int)blockIdx.x * MU_THREADS >= n_c) return;
  const int n_q = J.n_q[job];
  const int n_tiles = (n_q + MU_TILE - 1) / MU_TILE;
  const int tps = (n_tiles + (int)gridDim.y - 1) / (int)gridDim.y;      // (the grid is sized for the longest list of the group)
  const int tile0 = blockIdx.y * tps, tile1 = min(n_tiles, tile0 + tps);
  if (tile0 >= tile1) return;
  cand = set_el(cand, job, s_cand);
  qdesc = set_by(qdesc, job, J.s_desc); tdesc = set_by(tdesc, job, J.s_desc); qc = set_el(qc, job, J.s_c); tc = set_el(tc, job, J.s_c);
  qxy = set_el(qxy, job, J.s_xy); bad = set_el(bad, job, J.s_int);
  // this thread's candidate (threads past the list take the last one and store nothing)
  const int ci = blockIdx.x * MU_THREADS + tid;
  const bool valid = ci < n_c;
  const int4 cd = cand[valid ? ci : n_c - 1];
  const int q = cd.x, d1 = cd.z, dstar = cd.w;
  uint4 tr[8];
#pragma unroll
  for (int e = 0; e < 8; e++) tr[e] = ((const uint4 *)(tdesc + (size_t)cd.y * 128))[e];
  const int ct = tc[cd.y] - 4194304;         // d = cq + ct - 2 dot with the packed norms, as in match_fix_kernel
  double2 own = make_double2(0., 0.);
  if (MODE == 2) own = qxy[q];
  bool fail = false;
  // the staging of a tile: two 16-byte chunks of descriptor per thread, norm and centre by the first 64 threads; rows past the end
  // of the list are zero and never read
  uint4 pd[2]; int pc = 0; double2 pxy = make_double2(0., 0.);
  auto fetch = [&](int tile) {
    const int r0 = tile * MU_TILE;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int ch = tid + e * MU_THREADS, r = r0 + (ch >> 3);
      pd[e] = r < n_q ? ((const uint4 *)(qdesc + (size_t)r * 128))[ch & 7] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (tid < MU_TILE) {
      const int r = r0 + tid;
      pc = r < n_q ? qc[r] : 0;
      if (MODE == 2) pxy = r < n_q ? qxy[r] : make_double2(0., 0.);
    }
  };
  fetch(tile0);
  for (int tile = tile0; tile < tile1; tile++) {
    __syncthreads();
    s_d[tid] = pd[0]; s_d[tid + MU_THREADS] = pd[1];
    if (tid < MU_TILE) { s_c[tid] = pc; if (MODE == 2) s_xy[tid] = pxy; }
    __syncthreads();
    if (tile + 1 < tile1) fetch(tile + 1);             // in flight during this tile's dot products
    if (!__ballot(valid && !fail)) continue;           // every candidate of the wave has already failed
    const int r0 = tile * MU_TILE, cnt = min(MU_TILE, n_q - r0);
#pragma unroll 2
    for (int j = 0; j < cnt; j++) {
      int dot = 0;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const uint4 a = s_d[j * 8 + e];
        dot = __builtin_amdgcn_sdot4((int)a.x, (int)tr[e].x, dot, false); dot = __builtin_amdgcn_sdot4((int)a.y, (int)tr[e].y, dot, false);
        dot = __builtin_amdgcn_sdot4((int)a.z, (int)tr[e].z, dot, false); dot = __builtin_amdgcn_sdot4((int)a.w, (int)tr[e].w, dot, false);
      }
      const int r = r0 + j;
      const int d = s_c[j] + ct - 2 * dot;
      // (r == q gives d == d1 and r == q: neither compare fires)
      fail |= d < d1 || (d == d1 && r < q);
      if (MODE == 2 && d < dstar && r != q) {
        const double2 p = s_xy[j];
        const double dx = p.x - own.x, dy = p.y - own.y;
        fail |= dx * dx + dy * dy > contr_sq;
      }
    }
  }
  if (valid && fail) bad[q] = 1;     // (every share that finds a rival stores the same word)
}

// The stage of one grouped launch, queued on ctx->stream between pass 2 and the emit kernels (match.hip: match_run_group); qd .. bad
// are the pointers of set 0 there.  The scratch - candidate lists of the context's sets behind their counters - and the pinned
// counters are reserved on the first search with a mode set.
int mutual_stage(mods_ctx *ctx, const MatchJobs &J, const MatchConst &k, int max_q, size_t pad, const void *mid, const unsigned long long *key_ge,
                 const unsigned long long *key_lt, const int *n_lt, int *bad, const int8_t *qd, const int *qc, const double2 *qxy,
                 const int8_t *td, const int *tc) {
  const int mode = ctx->mutual_mode;
  const size_t need = 4 + (size_t)ctx->m_sets * pad;          // 16 counters | m_sets lists of `pad` candidates
  MODS_HIP_CHECK(reserve_scratch(ctx, ctx->mu_cand, need, need));
  MODS_HIP_CHECK(ctx->mu_count.reserve(MATCH_MAX_JOBS));
  int *count = (int *)ctx->mu_cand.get();
  int4 *cand = ctx->mu_cand + 4;
  StageScope ts(ctx, MODS_STAGE_MATCH_MUTUAL);
  MODS_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int) * MATCH_MAX_JOBS, ctx->stream));
  const unsigned G = (unsigned)J.n_jobs, xb = (unsigned)((max_q + MU_THREADS - 1) / MU_THREADS);
  hipLaunchKernelGGL(mutual_list_kernel, dim3(xb, G), dim3(MU_THREADS), 0, ctx->stream, J, k, (const QueryMid *)mid, key_ge, key_lt, n_lt,
                     (const int *)bad, cand, pad, count);
  const dim3 grid(xb, (unsigned)mutual_splits(max_q), G);
  if (mode == 1)
    hipLaunchKernelGGL((mutual_sweep_kernel<1>), grid, dim3(MU_THREADS), 0, ctx->stream, J, k.contr_sq, (const int4 *)cand, pad, (const int *)count,
                       ctx->mu_count.get(), qd, qc, qxy, td, tc, bad);
  else
    hipLaunchKernelGGL((mutual_sweep_kernel<2>), grid, dim3(MU_THREADS), 0, ctx->stream, J, k.contr_sq, (const int4 *)cand, pad, (const int *)count,
                       ctx->mu_count.get(), qd, qc, qxy, td, tc, bad);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_ctx_match_mutual(mods_ctx *c, int mode) {
  if (mode < 0 || mode > 2) { set_error("match_mutual: mode %d (0 off, 1 mutual nearest neighbour, 2 with the backward ratio test)", mode); return MODS_E_ARG; }
  if (!c) { set_error("match_mutual: null context"); return MODS_E_ARG; }
  c->mutual_mode = mode;
  dev_state_changed(c);              // (recorded launch chains are not replayed across the change)
  return MODS_OK;
}

int mods_match_mutual_counts(mods_ctx *c, int *n_forward, int *n_kept) {
  if (!c || !n_forward || !n_kept) { set_error("match_mutual_counts: null argument"); return MODS_E_ARG; }
  if (!c->m_count.get()) { set_error("match_mutual_counts: no search has run on this context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(stream_wait(c->stream));
  *n_kept = read_slot(c->m_count, count_slot());
  *n_forward = c->mu_last_checked ? read_slot(c->mu_count, 0) : *n_kept;
  return MODS_OK;
}

}  // extern "C"
