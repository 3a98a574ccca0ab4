// Exact k-nearest-neighbour search over 128-byte descriptors on the gfx950 matrix cores (mods_match_knn, mods_match_knn_dev,
// mods_match_knn_reps): for every query the K = min(k, n_t) trains with the smallest keys (d, t), d the exact integer squared L2
// distance and t the train's index, in increasing key order.  No n_q x n_t matrix is written.
//
// The lists are packed by the matcher's kernel (match_pack_lists) into buffers of this search, so distances are the matcher's:
// seeded int8 MFMA accumulators acc = dot - floor(ct/2) + MATCH_BIAS, d = cq + (ct & 1) - 2 * (acc - MATCH_BIAS).
//
//   knn_sweep_kernel   trains stream through LDS in 32-row tiles (a ring of three images, three tiles ahead in registers), a wave keeps two
//                      blocks of 32 queries resident; every (query block, train split) leaves its K best keys, sorted
//   knn_merge_kernel   one wave per query merges the splits' sorted lists by rank and writes the padded rows
//
// The selection inside the sweep is the buffered one ("k-NN structure").  A lane owns one query column and half of
// a tile's rows.  It keeps the query's current K-th best key in registers; a tile is looked at element by element only when the
// largest of the lane's 16 accumulators reaches that bound.  An element whose key beats the bound is appended, unsorted, to the
// lane's own queue in LDS (two lanes serve one query, each has a queue, so no location has two writers).  When a queue is full
// the wave merges every queue into the sorted list of its query (a lane per query while most queries have keys queued, else the
// whole wave on one query at a time with an entry of the list per lane: knn_flush), and every lane reads the new K-th key back.
// All comparisons are on whole keys, nothing depends on the order in which trains arrive.
#include "match_types.hpp"
#include <algorithm>
#include <climits>
#include <type_traits>

namespace mods {

typedef int kv4i __attribute__((ext_vector_type(4)));
typedef int kv16i __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int KNN_MAX_K = 64;
constexpr int KNN_MAX_SPLITS = 64;
constexpr int KNN_QB = 2;                          // query blocks (of 32) per wave: at K = 64 the lists of 128 * QB queries take 65 * QB KiB of LDS
constexpr int KNN_QPW = 32 * KNN_QB;               // queries per wave
constexpr int KNN_QPB = 4 * KNN_QPW;               // ... and per workgroup (four waves, one per SIMD)
constexpr int KNN_QUEUE_MIN = 4, KNN_QUEUE_MAX = 16;   // queue entries per lane and query block: what the LDS leaves beside the lists (knn_queue_len)
constexpr int KNN_LDS_MAX = 160 * 1024;
constexpr int KNN_NBUF = 3;                        // tiles on their way in registers, and images of the ring (two would do: knn_sweep_kernel)
constexpr int KNN_IMG = 4096 + 128;                // rows | seeds
constexpr u64 KNN_NONE = ~0ull;

struct KnnConst { int n_q, n_t, K, qblocks, splits, tiles_per_split, queue; };

__host__ __device__ inline int knn_list_stride(int K) { return K | 1; }   // odd: the same position of 32 queries' lists falls into 32 different bank pairs
inline size_t knn_lds_bytes(int K, int Q) { return (size_t)KNN_NBUF * KNN_IMG + (size_t)KNN_QPB * (knn_list_stride(K) + 2 * Q) * sizeof(u64); }
// a bound is as fresh as the last merge: where merging is cheap (short lists, the lane-per-query form) short queues keep it fresh,
// longer lists get what the LDS leaves beside them
inline int knn_queue_len(int K) {
  if (K <= 16) return KNN_QUEUE_MIN;
  const int room = (int)((KNN_LDS_MAX - (int)knn_lds_bytes(K, 0)) / (KNN_QPB * 2 * (int)sizeof(u64)));
  return room < KNN_QUEUE_MIN ? KNN_QUEUE_MIN : room > KNN_QUEUE_MAX ? KNN_QUEUE_MAX : room;
}
static_assert((size_t)KNN_NBUF * KNN_IMG + (size_t)KNN_QPB * ((KNN_MAX_K | 1) + 2 * KNN_QUEUE_MIN) * sizeof(u64) <= (size_t)KNN_LDS_MAX, "the lists of k = 64 and the shortest queues fit the LDS");

// the whole register file of the wave's SIMD (the co-residency rule, match.hip): the workgroup is four waves of 512 registers
__device__ __forceinline__ void knn_own_simd() { asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a255, 0" ::: "v255", "a255"); }

__device__ __forceinline__ int knn_max16(const kv16i &acc) {
  int m = max(max(acc[0], acc[1]), acc[2]);
  m = max(max(m, acc[3]), acc[4]);
  m = max(max(m, acc[5]), acc[6]);
  m = max(max(m, acc[7]), acc[8]);
  m = max(max(m, acc[9]), acc[10]);
  m = max(max(m, acc[11]), acc[12]);
  m = max(max(m, acc[13]), acc[14]);
  return max(m, acc[15]);
}

// One train tile (32 rows x 128 B) and its 32 seeds on their way from global memory to an LDS image: 16 bytes per thread (and a seed
// for the first 32 threads) wait in registers while earlier tiles are multiplied.  The 16-byte chunk c of row r lands at chunk
// position c ^ ((r >> 1) & 7) (swizzled on the source side: the operand reads of 16 rows then fall into 16 different slots of a
// bank row).  (global_load_lds would save the registers, but behind such a fetch the compiler puts s_waitcnt vmcnt(0) in front of
// every LDS access - the queues and lists of the selection included - i.e. a wait for the tile requested a moment ago; with
// registers its count of the fetches in flight is exact.  DESIGN.md 4, "k-NN structure".)
struct KnnTileRegs { kv4i a; int s; };
__device__ __forceinline__ KnnTileRegs knn_tile_fetch(const int8_t *__restrict__ tdesc, const int *__restrict__ tc2n, int tt) {
  KnnTileRegs r;
  const int row = threadIdx.x >> 3, c = threadIdx.x & 7;
  r.a = *(const kv4i *)(tdesc + (size_t)tt * 4096 + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
  r.s = tc2n[tt * 32 + (threadIdx.x & 31)];
  return r;
}
__device__ __forceinline__ void knn_tile_store(char *img, const KnnTileRegs &r) {
  *(kv4i *)(img + threadIdx.x * 16) = r.a;
  if (threadIdx.x < 32) ((int *)(img + 4096))[threadIdx.x] = r.s;
}

__device__ __forceinline__ void knn_wave_sync() {      // LDS written by one lane of the wave is read by another
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ u64 knn_readlane64(u64 v, int l) {
  return ((u64)(unsigned int)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned int)__builtin_amdgcn_readlane((int)v, l);
}
// lane j takes the value of lane j - 1 (DPP wave_shr:1: one VALU instruction per half, no LDS); lane 0 keeps its own
__device__ __forceinline__ u64 knn_from_lane_below(u64 v) {
  const int lo = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(v >> 32), (int)(v >> 32), 0x138, 0xf, 0xf, false);
  return ((u64)(unsigned int)hi << 32) | (unsigned int)lo;
}

// The merge of the wave's queues into its lists.  Its wave-wide form takes one query with a non-empty queue after the other: lane j holds
// entry j of the query's sorted list, lanes 0 .. 2Q-1 the entries of its two queues.  A key goes in at the position the ballot of
// "my entry is below the key" counts; the lanes above it take their lower neighbour's entry, the last entry falls out - a compare,
// a ballot and two DPP moves per key, whatever K is.  Then every lane takes the K-th key of its two queries back as its bound, and
// the queues are empty.
__device__ __forceinline__ void knn_flush(u64 *list_w, const u64 *queue_w, int K, int Q, int lane, int (&qcnt)[KNN_QB], u64 (&kth)[KNN_QB],
                                          int (&thr)[KNN_QB], const int (&cq)[KNN_QB]) {
  static_assert(KNN_QB == 2, "in the lane-per-query form a lane of half g merges the queues of query block g");
  const int g = lane >> 5, col = lane & 31, LS = knn_list_stride(K);
  // the lane (g, col) speaks for the query (block g, column col): what its two queues hold
  const int own = g ? qcnt[1] : qcnt[0];
  const int oth = __shfl_xor(g ? qcnt[0] : qcnt[1], 32);
  const int busy = __popcll(__ballot(own + oth > 0));          // queries of the wave with something queued
  knn_wave_sync();
  // Two forms.  While most queries have keys queued (a split's first tiles, small K) a lane merges its own query, all lanes at
  // once: an insertion costs a walk over the list in LDS, ~65 clocks an entry, but 64 queries share it.  Later few queries have
  // any, and the whole wave takes them one after the other at ~100 clocks a key whatever K is.  The rule below is where the two
  // estimates cross (busy * Q * 50 against Q * (100 + 65 K): never the first form from K = 47 on, which is what was measured -
  // profiles/knn_timing.txt); the result does not depend on it.
  if (3 * busy > 6 + 4 * K) {
    u64 *lst = list_w + (g * 32 + col) * LS;
    const u64 *qu = queue_w + (g * 32 + col) * 2 * Q;
    for (int h = 0; h < 2; h++) {
      const int cnt = h == g ? own : oth;
      for (int e = 0; e < cnt; e++) {
        const u64 key = qu[h * Q + e];
        if (key >= lst[K - 1]) continue;
        int j = K - 1;
        while (j > 0) {
          const u64 p = lst[j - 1];
          if (p < key) break;
          lst[j] = p;
          j--;
        }
        lst[j] = key;
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < KNN_QB; b++) {
      const u64 m = __ballot(qcnt[b] > 0);
      unsigned int qm = (unsigned int)m | (unsigned int)(m >> 32);       // the block's queries with something queued
      while (qm) {
        const int c = __builtin_ctz(qm);
        qm &= qm - 1;
        const int n0 = __builtin_amdgcn_readlane(qcnt[b], c), n1 = __builtin_amdgcn_readlane(qcnt[b], c + 32);
        u64 *lst = list_w + (b * 32 + c) * LS;
        const u64 *qu = queue_w + (b * 32 + c) * 2 * Q;
        u64 e = lane < K ? lst[lane] : KNN_NONE;
        const u64 mine = lane < 2 * Q ? qu[lane] : KNN_NONE;             // (slots past a queue's count hold stale keys: not read below)
        for (int i = 0; i < n0 + n1; i++) {
          const u64 key = knn_readlane64(mine, i < n0 ? i : Q + i - n0);
          const int pos = __popcll(__ballot(e < key));                   // entries below the key: a prefix of the lanes
          if (pos < K) {
            const u64 up = knn_from_lane_below(e);
            e = lane < pos ? e : (lane == pos ? key : up);
            if (lane >= K) e = KNN_NONE;
          }
        }
        if (lane < K) lst[lane] = e;
      }
    }
  }
  knn_wave_sync();
#pragma unroll
  for (int b = 0; b < KNN_QB; b++) {
    kth[b] = list_w[(b * 32 + col) * LS + K - 1];
    thr[b] = kth[b] == KNN_NONE ? INT_MAX : (int)(kth[b] >> 32) - cq[b];
    qcnt[b] = 0;
  }
}

// grid = qblocks * splits workgroups of 256 threads (four waves, each the owner of its SIMD), LDS: the static ring and,
// dynamic, lists [256][K | 1] | queues [256][2][k.queue].  part: [split][qblocks * 256][K] sorted keys (d << 32 | t), KNN_NONE
// where a split holds fewer than K trains.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void knn_sweep_kernel(KnnConst k, const int8_t *__restrict__ qdesc,
                                                        const int *__restrict__ qc, const int8_t *__restrict__ tdesc,
                                                        const int *__restrict__ tc2n, const unsigned int *__restrict__ tpar,
                                                        u64 *__restrict__ part) {
  constexpr int QB = KNN_QB;
  __shared__ __attribute__((aligned(16))) char s_ring[KNN_NBUF * KNN_IMG];      // the tile images (a static object of its own: the
  extern __shared__ __attribute__((aligned(16))) char s_mem[];                  // lists and queues behind it never alias a tile fetch)
  knn_own_simd();
  const int lane = threadIdx.x & 63, g = lane >> 5, col = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qb = blockIdx.x % k.qblocks, sp = blockIdx.x / k.qblocks;
  const int n_tiles = (k.n_t + 31) / 32;
  const int t0 = sp * k.tiles_per_split;
  const int n = max(0, min(n_tiles, t0 + k.tiles_per_split) - t0);      // tiles of this workgroup
  const int K = k.K, LS = knn_list_stride(K), Q = k.queue;
  u64 *list_w = (u64 *)s_mem + (size_t)w * KNN_QPW * LS;
  u64 *queue_w = (u64 *)s_mem + (size_t)KNN_QPB * LS + (size_t)w * KNN_QPW * 2 * Q;
  if (n == 0) {      // an empty trailing split of a forced split count: its lists stay empty
    u64 *out = part + ((size_t)sp * k.qblocks * KNN_QPB + (size_t)(qb * 4 + w) * KNN_QPW) * K;
    for (int e = lane; e < KNN_QPW * K; e += 64) out[e] = KNN_NONE;
    return;
  }
  // tiles past the end of the split are fetched as its last tile again and never multiplied: no branch around a fetch
  const int t_last = t0 + n - 1;
  KnnTileRegs fetched[KNN_NBUF];
#pragma unroll
  for (int d = 0; d < KNN_NBUF; d++) fetched[d] = knn_tile_fetch(tdesc, tc2n, min(t0 + d, t_last));
  for (int e = lane; e < KNN_QPW * LS; e += 64) list_w[e] = KNN_NONE;
  const int jwave = (qb * 4 + w) * KNN_QPW;
  kv4i bq[QB][4];
  int cq[QB], thr[QB], qcnt[QB];
  u64 kth[QB];
  u64 *qq[QB];
#pragma unroll
  for (int b = 0; b < QB; b++) {
    const int j = jwave + 32 * b + col;
    const int jc = j < k.n_q ? j : k.n_q - 1;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) bq[b][ks] = *(const kv4i *)(qdesc + (size_t)jc * 128 + ks * 32 + g * 16);
    cq[b] = qc[jc] - 4194304 + 2 * MATCH_BIAS;   // d = cq + (ct & 1) - 2 * (seeded accumulator)
    kth[b] = KNN_NONE; thr[b] = INT_MAX; qcnt[b] = 0;
    qq[b] = queue_w + ((b * 32 + col) * 2 + g) * Q;
  }
  int aoff[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) aoff[ks] = col * 128 + (((2 * ks + g) ^ ((col >> 1) & 7)) << 4);
  knn_tile_store(s_ring, fetched[0]);
  fetched[0] = knn_tile_fetch(tdesc, tc2n, min(t0 + KNN_NBUF, t_last));
  __syncthreads();
  // One tile step: tile i is multiplied and examined from image i mod 3; then tile i + 1, fetched three steps ago, goes from its
  // registers to the next image, and the registers take tile i + 4.  Image and register numbers are compile-time constants (the
  // loop is unrolled by three).  The prefetch depth is the three register sets; the protocol itself needs two images only (the
  // store follows the barrier that ended step i - 1, the last reader of the other image) - the ring has a third so that images
  // and register sets share one index.
  auto step = [&](auto slot_c, int i) __attribute__((always_inline)) {
    constexpr int SLOT = decltype(slot_c)::value, NEXT = (SLOT + 1) % KNN_NBUF;
    const char *img = s_ring + SLOT * KNN_IMG;
    kv4i a[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) a[ks] = *(const kv4i *)(img + aoff[ks]);
    kv16i acc[QB];
    {
      // seeds of this lane's rows (r & 3) + 8 * (r >> 2) + 4 * g
      const int *sd = (const int *)(img + 4096) + 4 * g;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int4 c = *(const int4 *)(sd + 8 * q);
        acc[0][4 * q + 0] = c.x; acc[0][4 * q + 1] = c.y; acc[0][4 * q + 2] = c.z; acc[0][4 * q + 3] = c.w;
      }
#pragma unroll
      for (int b = 1; b < QB; b++) acc[b] = acc[0];
    }
#pragma unroll
    for (int ks = 0; ks < 4; ks++)
#pragma unroll
      for (int b = 0; b < QB; b++) acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ks], bq[b][ks], acc[b], 0, 0, 0);
    const int tbase = (t0 + i) * 32;
    const unsigned int par = tpar[t0 + i];   // wave-uniform: ct & 1 of the 32 train rows
    unsigned int done[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) done[b] = 0u;
    for (;;) {
      bool ovf = false;
#pragma unroll
      for (int b = 0; b < QB; b++) {
        if (-2 * knn_max16(acc[b]) > thr[b]) continue;            // d - cq >= -2 * acc: nothing of this half tile can beat the bound
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m2 = -2 * acc[b][r];
          if (m2 > thr[b] || ((done[b] >> r) & 1u)) continue;
          const int row = (r & 3) + 8 * (r >> 2) + 4 * g;
          const int t = tbase + row;
          if (t >= k.n_t) continue;                                // rows past the end of the list
          const int d = cq[b] + (int)((par >> row) & 1u) + m2;
          const u64 key = ((u64)(unsigned int)d << 32) | (unsigned int)t;
          if (!(key < kth[b])) continue;
          if (qcnt[b] < Q) { qq[b][qcnt[b]] = key; qcnt[b]++; done[b] |= 1u << r; }
          else ovf = true;      // the queue is full: the element waits for the merge below and is examined again
        }
      }
      if (!__any(ovf ? 1 : 0)) break;
      knn_flush(list_w, queue_w, K, Q, lane, qcnt, kth, thr, cq);
    }
    knn_tile_store(s_ring + NEXT * KNN_IMG, fetched[NEXT]);
    fetched[NEXT] = knn_tile_fetch(tdesc, tc2n, min(t0 + i + 1 + KNN_NBUF, t_last));
    __syncthreads();
  };
  static_assert(KNN_NBUF == 3, "the tile loop is unrolled for a ring of three images");
  int i = 0;
  for (; i + 2 < n; i += 3) {      // (whole triples without a condition inside: the compiler's count of the fetches in flight stays exact)
    step(std::integral_constant<int, 0>(), i);
    step(std::integral_constant<int, 1>(), i + 1);
    step(std::integral_constant<int, 2>(), i + 2);
  }
  if (i < n) step(std::integral_constant<int, 0>(), i);
  if (i + 1 < n) step(std::integral_constant<int, 1>(), i + 1);
  knn_flush(list_w, queue_w, K, Q, lane, qcnt, kth, thr, cq);
  // the wave's 64 lists are 64 * K consecutive keys of the output
  u64 *out = part + ((size_t)sp * k.qblocks * KNN_QPB + jwave) * K;
  for (int e = lane; e < KNN_QPW * K; e += 64) out[e] = list_w[(e / K) * LS + e % K];
}

// entries of the sorted list p[0 .. K) below key
__device__ __forceinline__ int knn_count_below(const u64 *__restrict__ p, int K, u64 key) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave per query: the rank of a key among the keys of all splits is its position in its own list plus the entries below it in
// every other list (keys are distinct: a train belongs to one split).  Ranks below K are the result, the row's tail is padded
// with (index -1, distance INT_MAX).  out_d2 / out_idx: [n_q][k].  grid = ceil(n_q / 4), block 256
__global__ __launch_bounds__(256) void knn_merge_kernel(KnnConst k, int k_out, const u64 *__restrict__ part, int *__restrict__ out_d2,
                                                        int *__restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= k.n_q) return;
  const int K = k.K;
  const size_t n_qpad = (size_t)k.qblocks * KNN_QPB;
  int finite = 0;
  for (int e = lane; e < k.splits * K; e += 64) {
    const int s = e / K, i = e % K;
    const u64 key = part[((size_t)s * n_qpad + j) * K + i];
    if (key == KNN_NONE) continue;
    finite++;
    int rank = i;
    for (int s2 = 0; s2 < k.splits && rank < K; s2++)
      if (s2 != s) rank += knn_count_below(part + ((size_t)s2 * n_qpad + j) * K, K, key);
    if (rank < K) {
      out_d2[(size_t)j * k_out + rank] = (int)(key >> 32);
      out_idx[(size_t)j * k_out + rank] = (int)(unsigned int)key;
    }
  }
  for (int off = 32; off > 0; off >>= 1) finite += __shfl_xor(finite, off);
  for (int e = min(finite, K) + lane; e < k_out; e += 64) {
    out_d2[(size_t)j * k_out + e] = INT_MAX;
    out_idx[(size_t)j * k_out + e] = -1;
  }
}

// The grid of the sweep.  A workgroup owns its compute unit, so the launch runs in rounds of one workgroup per CU: the train list
// is split until the grid has a workgroup for each of the 256 CUs (ceil(256 / query blocks) splits: where the query blocks do not
// divide 256 the grid overshoots a round - 235 x 2 = 470 workgroups at 60 156 x 47 177 are 1.84 rounds; a split count that makes
// whole rounds was not tried), but a split starts from an empty list and its first K trains are all hits, so it keeps at least
// 8 + k tiles.  forced_splits > 0 replaces the choice (mods_ctx_knn_splits; trailing splits may then be empty).
struct KnnGrid { int qblocks, splits, tiles_per_split; };
static KnnGrid knn_grid(int n_q, int n_t, int k, int forced_splits) {
  KnnGrid gr;
  const int n_tiles = (n_t + 31) / 32;
  gr.qblocks = (n_q + KNN_QPB - 1) / KNN_QPB;
  int splits = (256 + std::max(gr.qblocks, 1) - 1) / std::max(gr.qblocks, 1);
  splits = std::min(splits, n_tiles / (8 + k));
  if (forced_splits > 0) splits = std::min(forced_splits, n_tiles);
  gr.splits = std::max(1, std::min(splits, KNN_MAX_SPLITS));
  gr.tiles_per_split = (n_tiles + gr.splits - 1) / gr.splits;
  return gr;
}

static size_t knn_pad(int n) { return (((size_t)n + 31) & ~(size_t)31) + 32; }   // list stride: the last tile's tail and a spare tile

// n_q, n_t >= 1: leaves the rows in ctx->kn_out (d2 [n_q][k] | idx [n_q][k])
static int knn_run(mods_ctx *ctx, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, int k) {
  const KnnGrid gr = knn_grid(n_q, n_t, k, ctx->kn_splits);
  KnnConst kc;
  kc.n_q = n_q; kc.n_t = n_t; kc.K = std::min(k, n_t);
  kc.qblocks = gr.qblocks; kc.splits = gr.splits; kc.tiles_per_split = gr.tiles_per_split; kc.queue = knn_queue_len(kc.K);
  const size_t pq = knn_pad(n_q), pt = knn_pad(n_t), n = pq + pt;
  const size_t n_part = (size_t)gr.splits * gr.qblocks * KNN_QPB * kc.K, n_out = 2 * (size_t)n_q * k;
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->kn_desc, n * 128, (n + n / 4) * 128));
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->kn_c, 2 * n + n / 32 + 4, 2 * (n + n / 4) + (n + n / 4) / 32 + 4));
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->kn_xy, n, n + n / 4));
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->kn_part, n_part, n_part + n_part / 4));
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->kn_out, n_out, n_out + n_out / 4));
  int8_t *qd = ctx->kn_desc, *td = qd + pq * 128;
  int *qc = ctx->kn_c, *tc = qc + pq, *qc2 = tc + pt, *tc2 = qc2 + pq;
  unsigned int *qpar = (unsigned int *)(tc2 + pt), *tpar = qpar + pq / 32;
  int *counters = (int *)(tpar + pt / 32);
  double2 *qxy = ctx->kn_xy, *txy = qxy + pq;
  const size_t lds = knn_lds_bytes(kc.K, kc.queue) - (size_t)KNN_NBUF * KNN_IMG;      // the dynamic part
  static DynLdsOnce lds_once;
  MODS_HIP_CHECK(dyn_lds_once(lds_once, (const void *)knn_sweep_kernel, KNN_LDS_MAX - KNN_NBUF * KNN_IMG, ctx->device));
  StageScope ts(ctx, MODS_STAGE_KNN);
  const PackList lq = {nullptr, 0, qd, qc, qc2, qpar, qxy}, lt = {nullptr, 0, td, tc, tc2, tpar, txy};
  match_pack_lists(ctx, q_dev, n_q, t_dev, n_t, lq, lt, counters);
  {
    StageScope ts1(ctx, MODS_STAGE_KNN_SWEEP);
    hipLaunchKernelGGL(knn_sweep_kernel, dim3(gr.qblocks * gr.splits), dim3(256), lds, ctx->stream, kc, qd, qc, td, tc2, tpar, ctx->kn_part.get());
  }
  int *out = ctx->kn_out;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((n_q + 3) / 4), dim3(256), 0, ctx->stream, kc, k, (const u64 *)ctx->kn_part.get(), out, out + (size_t)n_q * k);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

int knn_check(const char *who, int k, const int *idx_out, const int *d2_out) {
  if (!idx_out && !d2_out) { set_error("%s: both outputs are null", who); return MODS_E_ARG; }
  if (k < 1 || k > KNN_MAX_K) { set_error("%s: k = %d (1 .. %d)", who, k, KNN_MAX_K); return MODS_E_ARG; }
  return MODS_OK;
}

int knn_search(mods_ctx *ctx, const char *who, const mods_region *q_dev, int n_q, const mods_region *t_dev, int n_t, int k, int *idx_out,
               int *d2_out) {
  int rc = knn_check(who, k, idx_out, d2_out);
  if (rc) return rc;
  if (n_q > ctx->max_cand || n_t > ctx->max_cand) { set_error("%s: list larger than the context capacity", who); return MODS_E_CAPACITY; }
  if (n_q <= 0) return MODS_OK;
  const size_t rows = (size_t)n_q * k;
  if (n_t <= 0) {
    for (size_t e = 0; e < rows; e++) { if (idx_out) idx_out[e] = -1; if (d2_out) d2_out[e] = INT_MAX; }
    return MODS_OK;
  }
  if ((rc = knn_run(ctx, q_dev, n_q, t_dev, n_t, k))) return rc;
  // the rows come back through pinned memory, one transfer per array, behind one wait
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->kn_host, 2 * rows, 2 * rows + rows / 2));
  int *host = ctx->kn_host;
  if (d2_out) MODS_HIP_CHECK(hipMemcpyAsync(host, ctx->kn_out, sizeof(int) * rows, hipMemcpyDeviceToHost, ctx->stream));
  if (idx_out) MODS_HIP_CHECK(hipMemcpyAsync(host + rows, ctx->kn_out + rows, sizeof(int) * rows, hipMemcpyDeviceToHost, ctx->stream));
  MODS_HIP_CHECK(mods::stream_wait(ctx->stream));
  if (d2_out) memcpy(d2_out, host, sizeof(int) * rows);
  if (idx_out) memcpy(idx_out, host + rows, sizeof(int) * rows);
  return MODS_OK;
}

}  // namespace mods

extern "C" {

// the grid of an n_q x n_t sweep (knn_grid): host arithmetic only, no device, no launch
int mods_match_knn_grid(int n_q, int n_t, int k, int forced_splits, int out[3]) {
  if (!out || n_q < 0 || n_t < 0 || k < 1 || k > mods::KNN_MAX_K || forced_splits < 0) {
    mods::set_error("match_knn_grid: null argument, a negative count or k = %d outside 1 .. %d", k, mods::KNN_MAX_K);
    return MODS_E_ARG;
  }
  const mods::KnnGrid gr = mods::knn_grid(n_q, n_t, k, forced_splits);
  out[0] = gr.qblocks; out[1] = gr.splits; out[2] = gr.tiles_per_split;
  return MODS_OK;
}

int mods_ctx_knn_splits(mods_ctx *c, int splits) {
  if (!c || splits < 0) { mods::set_error("knn_splits: null context or a negative count"); return MODS_E_ARG; }
  c->kn_splits = splits;
  return MODS_OK;
}

}  // extern "C"
