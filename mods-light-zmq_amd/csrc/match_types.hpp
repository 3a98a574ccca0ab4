// What the matcher's kernels share across files (match.hip, mutual.hip): the constants of a search, the job table of a grouped
// launch, the per-query state between the passes and the acceptance decision of the emit stage.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace mods {

struct MatchConst {
  int n_q, n_t;
  int nn;
  double sqminratio, contr_sq;
  int tiles_per_split;
  int max_distance;       // >= 0: MatchFLANNDistance (Hamming) decisions in the emit stage; -1: FGINN
};

// The searches of one grouped launch: blockIdx.y (blockIdx.z in the pack kernel) = search.  Every scratch buffer of the context
// exists once per search of a group ("set"): set j = set 0 + j * stride, so a kernel takes the pointers of set 0 and moves them.
// The pairs of a pipeline batch are matched in ONE set of launches (a 10 k x 9 k search fills 40 of the 256 CUs on its own, and
// every dispatch costs the host a completion interrupt); a single search is a group of one.
constexpr int MATCH_MAX_JOBS = 16;
struct MatchJobs {
  int n_jobs;
  int n_q[MATCH_MAX_JOBS], n_t[MATCH_MAX_JOBS];
  int tps[MATCH_MAX_JOBS], qblocks[MATCH_MAX_JOBS], splits[MATCH_MAX_JOBS];     // pass-1 geometry (nn1_grid)
  int eblocks[MATCH_MAX_JOBS];                                                   // blocks of the emit stage
  const mods_region *q_reg[MATCH_MAX_JOBS], *t_reg[MATCH_MAX_JOBS];
  mods_tentative *tent_out[MATCH_MAX_JOBS];
  int *count_out[MATCH_MAX_JOBS];
  size_t s_desc, s_p2;                       // set strides in bytes (m_desc, m_p2)
  size_t s_c, s_xy, s_u64, s_int, s_mid;     // set strides in elements of the buffer's type (m_c, m_xy, m_u64, m_int, m_mid)
};
template <class T> __device__ __forceinline__ T *set_el(T *p, int job, size_t stride) { return p + (size_t)job * stride; }
template <class T> __device__ __forceinline__ T *set_by(T *p, int job, size_t stride_bytes) {
  typedef typename std::conditional<std::is_const<T>::value, const char, char>::type C;
  return (T *)((C *)p + (size_t)job * stride_bytes);
}

// Accumulator seed of a train row: acc = dot - floor(ct/2) + MATCH_BIAS.  dot lies in [-2^21, 2^21] and ct in [2^21, 2^22], so the
// seeded accumulators of real rows lie in [1, 5*2^20 + 1] (23 bits, never negative); the rows past the end of the list inside the last
// tile carry zero descriptors and the seed 0: their accumulators are exactly 0, below every real one.
constexpr int MATCH_BIAS = (1 << 22) + 1;

// where match_pack2_kernel leaves one packed list: int8 descriptors (v - 128), c = sum v^2 - 256 * sum (v - 128), the accumulator
// seeds, one parity word (c & 1) per 32-row tile, the centres
struct PackList { const mods_region *reg; int n; int8_t *desc; int *cvec; int *c2neg; unsigned int *parity; double2 *xy; };
void match_pack_lists(mods_ctx *ctx, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, const PackList &lq, const PackList &lt,
                      int *counters);   // match.hip

struct QueryMid {        // per query state between the passes
  int i0, d0, dstar, pad;
  double x0, y0;
};

// fl32(d0/d) <= ratio^2, evaluated as the reference does (float quotient promoted to double)
__device__ __forceinline__ bool ratio_ok(int d0, int d, double sqmin) {
  const double ratio = (double)((float)d0 / (float)d);
  return ratio <= sqmin;
}

// the emit stage's decision for query j, and its tentative (match_emit_count_kernel, match_emit_kernel, mutual_list_kernel)
__device__ __forceinline__ bool fginn_accept(const MatchConst &k, int j, const QueryMid *__restrict__ mid,
                                             const unsigned long long *__restrict__ key_ge, const unsigned long long *__restrict__ key_lt,
                                             const int *__restrict__ n_lt, const int *__restrict__ bad, mods_tentative *tc) {
  if (j >= k.n_q) return false;
  if (k.max_distance >= 0) {   // MatchFLANNDistance, matching.cpp:612-627: mid = nearest, key_ge = second nearest
    const QueryMid m = mid[j];
    if (m.d0 > k.max_distance) return false;
    const unsigned long long k2 = key_ge[j];
    tc->q = j; tc->t = m.i0; tc->t_bad = tc->t_2nd = (int)(unsigned int)k2;
    tc->d1 = (float)m.d0; tc->d2 = tc->d2nd = (float)(int)(k2 >> 32); tc->pad = 0;
    tc->ratio = (double)tc->d1 / (double)tc->d2;
    return true;
  }
  const int K = min(k.nn, k.n_t);
  const unsigned long long kg = key_ge[j];
  const int c = n_lt[j];
  if (bad[j] || kg == ~0ull || c + 1 > K - 1) return false;
  const QueryMid m = mid[j];
  const unsigned long long k2 = c > 0 ? key_lt[j] : kg;
  const int d2 = (int)(kg >> 32);
  tc->q = j; tc->t = m.i0; tc->t_bad = (int)(unsigned int)kg; tc->t_2nd = (int)(unsigned int)k2;
  tc->d1 = (float)m.d0; tc->d2 = (float)d2; tc->d2nd = (float)(int)(k2 >> 32); tc->pad = 0;
  tc->ratio = sqrt((double)((float)m.d0 / (float)d2));
  return true;
}

// mutual.hip: the mutual check of one grouped launch, between pass 2 and the emit kernels (the pointers are those of set 0)
int mutual_stage(mods_ctx *ctx, const MatchJobs &J, const MatchConst &k, int max_q, size_t pad, const void *mid, const unsigned long long *key_ge,
                 const unsigned long long *key_lt, const int *n_lt, int *bad, const int8_t *qd, const int *qc, const double2 *qxy,
                 const int8_t *td, const int *tc);

}  // namespace mods
