// Distractor descriptor database of the FGINN ratio test (mods_descdb_*, mods_ctx_distractor_db; contract in include/mods_hip.h).
//
// Reference behaviour: MatchFlannFGINNPlusDB, matching/matching.cpp:461-572 - defined there, declared nowhere and never called.  A
// forward tentative (q, t) with d0 = d(q, t) gets a second rival, the nearest row of a fixed database of unrelated descriptors at
// dDB = min_b d(q, b): the quotient it has to pass becomes max(d0 / dj, d0 / dDB).
//
// The database is packed once, when it is made, into what the distance kernels of the matcher stream (match_types.hpp): int8 rows
// v - 128 in 32-row tiles of 4096 bytes, the accumulator seeds MATCH_BIAS - (c >> 1), one parity word (c & 1) per tile, rows past the
// end with zero descriptor and zero seed.  A search never packs it again.
//
// The veto of a search runs on what the forward search left in the matcher's scratch buffers, around the emit kernels:
//   descdb_gather_kernel   evaluates fginn_accept for every query and copies the packed descriptors of the accepted ones - the only
//                          queries that need dDB - to a compact list (any order), its length stays on the device
//   descdb_sweep_kernel    the compact list against the database on the matrix cores: queries resident as B operands (four blocks
//                          of 32 per wave, 512 per workgroup), database tiles through LDS (a ring of three images, three tiles ahead
//                          in registers, as knn_sweep_kernel), v_mfma_i32_32x32x32_i8; per lane and query block ONE running value
//                          2 * acc - parity, and a tile is looked at element by element only where its largest accumulator can
//                          still raise that value; the grid covers the worst case, idle workgroups exit
//   descdb_fold_kernel     rDB against ratio^2: a vetoed query is marked in bad[], which the emit kernels pass by
//   (match_emit_count_kernel, match_emit_kernel: unchanged)
//   descdb_ratio_kernel    the survivors' ratio = sqrt(max(r, rDB)) and their dDB, in list order
// With a seeded accumulator acc = dot - floor(ct / 2) + MATCH_BIAS the distance is d = cq + (ct & 1) - 2 * (acc - MATCH_BIAS): the
// minimum distance is cq' - max(2 * acc - (ct & 1)), a maximum of integers.  Partial results are combined across the half-waves, the
// splits of the database and the workgroups by integer min: nothing depends on the order rows arrive in.
#include "match_types.hpp"
#include <algorithm>
#include <atomic>
#include <climits>
#include <vector>

struct mods_descdb {
  int device = 0;
  long n = 0;                        // rows
  int n_tiles = 0;                   // 32-row tiles
  mods::Buf<int8_t> desc;            // [(n_tiles + 1) * 32][128]: the last tile's tail and a spare tile are zero
  mods::Buf<int> seed;               // [(n_tiles + 1) * 32]
  mods::Buf<unsigned int> parity;    // [n_tiles + 1]
  std::atomic<int> refs{1};          // the creator's reference + one per context slot
};

namespace mods {

typedef int dv4i __attribute__((ext_vector_type(4)));
typedef int dv16i __attribute__((ext_vector_type(16)));

constexpr long DESCDB_MAX_ROWS = 1l << 24;        // 2 GiB of rows; row and tile indices stay far inside an int
constexpr int DB_QB = 4;                          // query blocks (of 32) per wave: 16 MFMAs per database tile read from LDS
constexpr int DB_QPW = 32 * DB_QB;                // queries per wave
constexpr int DB_QPB = 4 * DB_QPW;                // ... and per workgroup (four waves, one per SIMD)
constexpr int DB_NBUF = 3;                        // tiles on their way in registers, and images of the ring
constexpr int DB_IMG = 4096 + 128;                // rows | seeds
constexpr int DB_ROW = 256;                       // workgroups of a sweep whose query count lives on the device: one per compute unit
constexpr int DB_MIN_TPS = 16;                    // a split keeps at least this many tiles (a workgroup first loads 64 KiB of queries)
constexpr int DB_MAX_SPLITS = 4096;
constexpr int DB_CHUNK = 1 << 17;                 // rows per staging step of the host entry points (16 MiB)
constexpr int DB_THREADS = 256;

// Packs rows of 128 bytes (dense, on the device) as match_pack2_kernel packs a region list: a wave takes the 32 rows of a tile, two
// lanes per row.  Rows row0 .. row0 + n of the output (row0 a multiple of 32); cvec, seed, parity and fill may be null (a query list
// needs c, a database its seeds and parity words; fill: INT_MAX per row, the start of an integer min).  grid = ceil(n / 32 / 4)
__global__ __launch_bounds__(DB_THREADS) void descdb_pack_kernel(const unsigned char *__restrict__ src, int n, long row0, int8_t *__restrict__ desc,
                                                                 int *__restrict__ cvec, int *__restrict__ seed, unsigned int *__restrict__ parity,
                                                                 int *__restrict__ fill) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile * 32 >= n) return;
  const int i = tile * 32 + (lane >> 1), half = lane & 1;
  unsigned int n2 = 0, sb = 0;
  uint4 *dst = (uint4 *)(desc + (size_t)(row0 + i) * 128 + 64 * half);
  if (i < n) {
    const uint4 *s = (const uint4 *)(src + (size_t)i * 128 + 64 * half);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint4 v = s[q];
      n2 = __builtin_amdgcn_udot4(v.x, v.x, n2, false); n2 = __builtin_amdgcn_udot4(v.y, v.y, n2, false);
      n2 = __builtin_amdgcn_udot4(v.z, v.z, n2, false); n2 = __builtin_amdgcn_udot4(v.w, v.w, n2, false);
      sb = __builtin_amdgcn_udot4(v.x, 0x01010101u, sb, false); sb = __builtin_amdgcn_udot4(v.y, 0x01010101u, sb, false);
      sb = __builtin_amdgcn_udot4(v.z, 0x01010101u, sb, false); sb = __builtin_amdgcn_udot4(v.w, 0x01010101u, sb, false);
      dst[q] = make_uint4(v.x ^ 0x80808080u, v.y ^ 0x80808080u, v.z ^ 0x80808080u, v.w ^ 0x80808080u);   // v - 128 as int8
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) dst[q] = make_uint4(0u, 0u, 0u, 0u);
    if (half == 0 && seed) seed[row0 + i] = 0;
  }
  n2 += __shfl_xor(n2, 1); sb += __shfl_xor(sb, 1);
  const int c = (int)n2 - 256 * ((int)sb - 128 * 128);        // sum v^2 - 256 * sum (v - 128)
  if (i < n && half == 0) {
    if (cvec) cvec[row0 + i] = c;
    if (seed) seed[row0 + i] = MATCH_BIAS - (c >> 1);
    if (fill) fill[row0 + i] = INT_MAX;
  }
  unsigned long long m = __ballot(i < n && half == 0 && (c & 1));
  m = (m | (m >> 1)) & 0x3333333333333333ull;
  m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
  m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
  m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
  m = (m | (m >> 16)) & 0x00000000ffffffffull;
  if (lane == 0 && parity) parity[row0 / 32 + tile] = (unsigned int)m;
}

// the whole register file of the wave's SIMD (the co-residency rule, match.hip): the workgroup is four waves of 512 registers
__device__ __forceinline__ void db_own_simd() { asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a255, 0" ::: "v255", "a255"); }

__device__ __forceinline__ int db_max16(const dv16i &acc) {
  int m = max(max(acc[0], acc[1]), acc[2]);
  m = max(max(m, acc[3]), acc[4]);
  m = max(max(m, acc[5]), acc[6]);
  m = max(max(m, acc[7]), acc[8]);
  m = max(max(m, acc[9]), acc[10]);
  m = max(max(m, acc[11]), acc[12]);
  m = max(max(m, acc[13]), acc[14]);
  return max(m, acc[15]);
}

// a database tile on its way to an LDS image, 16 bytes per thread and a seed for the first 32 (knn_tile_fetch: the chunk c of row r
// lands at chunk position c ^ ((r >> 1) & 7), swizzled on the source side)
struct DbTileRegs { dv4i a; int s; };
__device__ __forceinline__ DbTileRegs db_tile_fetch(const int8_t *__restrict__ tdesc, const int *__restrict__ tseed, int tt) {
  DbTileRegs r;
  const int row = threadIdx.x >> 3, c = threadIdx.x & 7;
  r.a = *(const dv4i *)(tdesc + (size_t)tt * 4096 + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
  r.s = tseed[(size_t)tt * 32 + (threadIdx.x & 31)];
  return r;
}
__device__ __forceinline__ void db_tile_store(char *img, const DbTileRegs &r) {
  *(dv4i *)(img + threadIdx.x * 16) = r.a;
  if (threadIdx.x < 32) ((int *)(img + 4096))[threadIdx.x] = r.s;
}

// n_tiles: of the database; splits > 0: the split count (the grid's x extent is query blocks * splits at least), 0: as many splits
// as the row of workgroups leaves for the query blocks the list fills; n_fixed: the list's length where n_dev is null; strides of
// the sets (searches of a group) in bytes / elements
struct DbSweepConst { int n_tiles, splits, n_fixed; size_t s_desc, s_int; };

__host__ __device__ inline int db_auto_splits(int row, int n_qb, int n_tiles) {
  int s = row / (n_qb < 1 ? 1 : n_qb);
  if (s > n_tiles / DB_MIN_TPS) s = n_tiles / DB_MIN_TPS;
  if (s > DB_MAX_SPLITS) s = DB_MAX_SPLITS;
  return s < 1 ? 1 : s;
}

// grid = (workgroups, searches), block 256 (four waves, each the owner of its SIMD).  qdesc / qc: the packed query list of a set,
// n_dev[set] its length (null: k.n_fixed); the minimum distance of list entry j goes to ddb[out_index ? out_index[j] : j] by
// atomicMin (INT_MAX before the launch).
__global__ __launch_bounds__(DB_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void descdb_sweep_kernel(
    DbSweepConst k, const int *__restrict__ n_dev, const int8_t *__restrict__ qdesc, const int *__restrict__ qc, const int *__restrict__ out_index,
    int *__restrict__ ddb, const int8_t *__restrict__ tdesc, const int *__restrict__ tseed, const unsigned int *__restrict__ tpar) {
  constexpr int QB = DB_QB;
  __shared__ __attribute__((aligned(16))) char s_ring[DB_NBUF * DB_IMG];
  db_own_simd();
  const int job = blockIdx.y;
  const int n_q = n_dev ? n_dev[job] : k.n_fixed;
  const int n_qb = (n_q + DB_QPB - 1) / DB_QPB;
  if (n_qb <= 0) return;
  const int splits = k.splits > 0 ? k.splits : db_auto_splits((int)gridDim.x, n_qb, k.n_tiles);
  const int qb = blockIdx.x % n_qb, sp = blockIdx.x / n_qb;
  if (sp >= splits) return;
  const int tps = (k.n_tiles + splits - 1) / splits;
  const int t0 = sp * tps;
  const int n = min(k.n_tiles, t0 + tps) - t0;       // tiles of this workgroup
  if (n <= 0) return;                                // an empty trailing split of a forced split count
  qdesc += (size_t)job * k.s_desc; qc += (size_t)job * k.s_int; ddb += (size_t)job * k.s_int;
  if (out_index) out_index += (size_t)job * k.s_int;
  const int lane = threadIdx.x & 63, g = lane >> 5, col = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // tiles past the end of the split are fetched as its last tile again and never multiplied: no branch around a fetch
  const int t_last = t0 + n - 1;
  DbTileRegs fetched[DB_NBUF];
#pragma unroll
  for (int d = 0; d < DB_NBUF; d++) fetched[d] = db_tile_fetch(tdesc, tseed, min(t0 + d, t_last));
  const int jwave = (qb * 4 + w) * DB_QPW;
  dv4i bq[QB][4];
  int best[QB];           // max over the rows seen of 2 * acc - (ct & 1); 0: none (a real row's accumulator is at least 1)
#pragma unroll
  for (int b = 0; b < QB; b++) {
    const int j = jwave + 32 * b + col;
    const int jc = j < n_q ? j : n_q - 1;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) bq[b][ks] = *(const dv4i *)(qdesc + (size_t)jc * 128 + ks * 32 + g * 16);
    best[b] = 0;
  }
  int aoff[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) aoff[ks] = col * 128 + (((2 * ks + g) ^ ((col >> 1) & 7)) << 4);
  db_tile_store(s_ring, fetched[0]);
  fetched[0] = db_tile_fetch(tdesc, tseed, min(t0 + DB_NBUF, t_last));
  __syncthreads();
  // One tile step (knn_sweep_kernel's): tile i is multiplied from image i mod 3; then tile i + 1, fetched three steps ago, goes from
  // its registers to the next image and the registers take tile i + 4.  The store follows the barrier that ended step i - 1, the
  // last reader of that image.
  auto step = [&](auto slot_c, int i) __attribute__((always_inline)) {
    constexpr int SLOT = decltype(slot_c)::value, NEXT = (SLOT + 1) % DB_NBUF;
    const char *img = s_ring + SLOT * DB_IMG;
    dv4i a[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) a[ks] = *(const dv4i *)(img + aoff[ks]);
    dv16i acc[QB];
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
    const unsigned int par = tpar[t0 + i];   // wave-uniform: ct & 1 of the 32 rows
#pragma unroll
    for (int b = 0; b < QB; b++) {
      // the parity bit only orders equal accumulators: a half tile whose largest accumulator m has 2 m <= best holds nothing better
      if (2 * db_max16(acc[b]) > best[b]) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * g;
          best[b] = max(best[b], 2 * acc[b][r] - (int)((par >> row) & 1u));
        }
      }
    }
    db_tile_store(s_ring + NEXT * DB_IMG, fetched[NEXT]);
    fetched[NEXT] = db_tile_fetch(tdesc, tseed, min(t0 + i + 1 + DB_NBUF, t_last));
    __syncthreads();
  };
  static_assert(DB_NBUF == 3, "the tile loop is unrolled for a ring of three images");
  int i = 0;
  for (; i + 2 < n; i += 3) {
    step(std::integral_constant<int, 0>(), i);
    step(std::integral_constant<int, 1>(), i + 1);
    step(std::integral_constant<int, 2>(), i + 2);
  }
  if (i < n) step(std::integral_constant<int, 0>(), i);
  if (i + 1 < n) step(std::integral_constant<int, 1>(), i + 1);
#pragma unroll
  for (int b = 0; b < QB; b++) {
    const int j = jwave + 32 * b + col;
    const int m = max(best[b], __shfl_xor(best[b], 32));      // the two half-waves hold the two halves of every tile
    if (g == 0 && j < n_q && m > 0) {
      const int d = qc[j] - 4194304 + 2 * MATCH_BIAS - m;     // d = cq + (ct & 1) - 2 * (seeded accumulator)
      atomicMin(&ddb[out_index ? out_index[j] : j], d);
    }
  }
}

// The veto's scratch of one set inside mods_ctx::dr_int: dDB per survivor (set 0's is what mods_distractor_fetch reads) | norms of
// the compact list | its query indices | dDB per query, `pad` ints each; 16 counters (the compact lists' lengths) follow the sets
struct DrPtrs { int8_t *desc; int *qc, *list, *ddb_q, *ddb_out, *count; size_t s_desc, s_int; };

// The accepted queries of every search, in any order, with their packed descriptors and norms; every query's dDB starts at INT_MAX.
// grid = (ceil(max n_q / 256), searches), block 256; count[search] zeroed before
__global__ __launch_bounds__(DB_THREADS) void descdb_gather_kernel(MatchJobs J, MatchConst k, const QueryMid *__restrict__ mid,
                                                                   const unsigned long long *__restrict__ key_ge,
                                                                   const unsigned long long *__restrict__ key_lt, const int *__restrict__ n_lt,
                                                                   const int *__restrict__ bad, const int8_t *__restrict__ qdesc,
                                                                   const int *__restrict__ qc, DrPtrs S) {
  const int job = blockIdx.y;
  k.n_q = J.n_q[job]; k.n_t = J.n_t[job];
  if ((int)blockIdx.x * DB_THREADS >= k.n_q) return;
  mid = set_el(mid, job, J.s_mid); key_ge = set_el(key_ge, job, J.s_u64); key_lt = set_el(key_lt, job, J.s_u64);
  n_lt = set_el(n_lt, job, J.s_int); bad = set_el(bad, job, J.s_int);
  qdesc = set_by(qdesc, job, J.s_desc); qc = set_el(qc, job, J.s_c);
  int8_t *desc2 = S.desc + (size_t)job * S.s_desc;
  int *qc2 = S.qc + (size_t)job * S.s_int, *list = S.list + (size_t)job * S.s_int, *ddb_q = S.ddb_q + (size_t)job * S.s_int;
  const int j = blockIdx.x * DB_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  mods_tentative tc;
  const bool acc = fginn_accept(k, j, mid, key_ge, key_lt, n_lt, bad, &tc);
  if (j < k.n_q) ddb_q[j] = INT_MAX;
  const unsigned long long m = __ballot(acc);
  if (!m) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(&S.count[job], __popcll(m));     // one atomic per wave
  base = __shfl(base, 0);
  if (acc) {
    const int i = base + __popcll(m & ((1ull << lane) - 1ull));
    list[i] = j; qc2[i] = qc[j];
    const uint4 *src = (const uint4 *)(qdesc + (size_t)j * 128);
    uint4 *dst = (uint4 *)(desc2 + (size_t)i * 128);
    uint4 row[8];
#pragma unroll
    for (int q = 0; q < 8; q++) row[q] = src[q];
#pragma unroll
    for (int q = 0; q < 8; q++) dst[q] = row[q];
  }
}

// rDB = fl32(d0 / dDB) against ratio^2 for every query that has a dDB: a vetoed one is marked in bad[].  A NaN quotient (0 / 0)
// vetoes nothing, an infinite one (dDB = 0 < d0) does.  Thread 0 of a search leaves the forward list's length in pinned memory.
// grid = (ceil(max n_q / 256), searches), block 256
__global__ __launch_bounds__(DB_THREADS) void descdb_fold_kernel(MatchJobs J, double sqminratio, const QueryMid *__restrict__ mid, int *__restrict__ bad,
                                                                 DrPtrs S, int *__restrict__ count_host) {
  const int job = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) count_host[job] = S.count[job];
  const int j = blockIdx.x * DB_THREADS + threadIdx.x;
  if (j >= J.n_q[job]) return;
  const int d = (S.ddb_q + (size_t)job * S.s_int)[j];
  if (d == INT_MAX) return;
  const double rdb = (double)((float)set_el(mid, job, J.s_mid)[j].d0 / (float)d);
  if (rdb > sqminratio) set_el(bad, job, J.s_int)[j] = 1;
}

// The survivors, in list order: ratio = sqrt(r') with r' = (r < rDB) ? rDB : r, and their dDB for mods_distractor_fetch.
// grid = (ceil(max n_q / 256), searches), block 256; the list's length is what the emit kernel left in pinned memory
__global__ __launch_bounds__(DB_THREADS) void descdb_ratio_kernel(MatchJobs J, DrPtrs S, int max_out) {
  const int job = blockIdx.y;
  const int n = min(*(const volatile int *)J.count_out[job], max_out);
  const int i = blockIdx.x * DB_THREADS + threadIdx.x;
  if (i >= n) return;
  mods_tentative *t = J.tent_out[job] + i;
  const int d = (S.ddb_q + (size_t)job * S.s_int)[t->q];
  (S.ddb_out + (size_t)job * S.s_int)[i] = d;
  const float d1 = t->d1;
  const double r = (double)(d1 / t->d2), rdb = (double)(d1 / (float)d);
  if (r < rdb) t->ratio = sqrt(rdb);
}

const mods_descdb *distractor_db_of(const mods_ctx *ctx) { return ctx->dr_db[ctx->dr_half_search ? 1 : 0]; }

static void descdb_unref(const mods_descdb *db) {
  if (!db) return;
  mods_descdb *d = const_cast<mods_descdb *>(db);
  if (d->refs.fetch_sub(1) == 1) {
    // the buffers are freed on the database's device; the caller's current device is put back
    int prev = -1;
    const bool have = hipGetDevice(&prev) == hipSuccess;
    (void)hipSetDevice(d->device);
    delete d;
    if (have && prev != d->device) (void)hipSetDevice(prev);
  }
}

void distractor_release(mods_ctx *ctx) {
  for (int s = 0; s < 2; s++) { descdb_unref(ctx->dr_db[s]); ctx->dr_db[s] = nullptr; }
}

static DrPtrs dr_carve(mods_ctx *ctx, size_t pad) {
  DrPtrs S;
  S.s_desc = pad * 128; S.s_int = 4 * pad;
  S.desc = ctx->dr_desc;
  S.ddb_out = ctx->dr_int; S.qc = S.ddb_out + pad; S.list = S.ddb_out + 2 * pad; S.ddb_q = S.ddb_out + 3 * pad;
  S.count = ctx->dr_int + (size_t)ctx->m_sets * S.s_int;
  return S;
}

// the grid of a sweep: query blocks, splits, tiles per split (forced_splits > 0 replaces the choice; trailing splits may be empty)
struct DbGrid { int qblocks, splits, tiles_per_split; };
static DbGrid descdb_grid(long m, int n_queries, int forced_splits) {
  DbGrid gr;
  const int n_tiles = (int)((m + 31) / 32);
  gr.qblocks = (n_queries + DB_QPB - 1) / DB_QPB;
  gr.splits = forced_splits > 0 ? std::max(1, std::min(std::min(forced_splits, DB_MAX_SPLITS), n_tiles))
                                : db_auto_splits(std::max(DB_ROW, gr.qblocks), gr.qblocks, n_tiles);
  gr.tiles_per_split = (n_tiles + gr.splits - 1) / gr.splits;
  return gr;
}

// Between pass 2 (and the mutual check) and the emit kernels, on ctx->stream, no host wait
int distractor_stage(mods_ctx *ctx, const mods_descdb *db, const MatchJobs &J, const MatchConst &k, int max_q, size_t pad, const void *mid,
                     const unsigned long long *key_ge, const unsigned long long *key_lt, const int *n_lt, int *bad, const int8_t *qd,
                     const int *qc) {
  const size_t sets = (size_t)ctx->m_sets;
  MODS_HIP_CHECK(reserve_scratch(ctx, ctx->dr_desc, sets * pad * 128, sets * pad * 128));
  MODS_HIP_CHECK(reserve_scratch(ctx, ctx->dr_int, sets * 4 * pad + MATCH_MAX_JOBS, sets * 4 * pad + MATCH_MAX_JOBS));
  MODS_HIP_CHECK(ctx->dr_count.reserve(MATCH_MAX_JOBS));
  const DrPtrs S = dr_carve(ctx, pad);
  StageScope ts(ctx, MODS_STAGE_DISTRACTOR);
  MODS_HIP_CHECK(hipMemsetAsync(S.count, 0, sizeof(int) * MATCH_MAX_JOBS, ctx->stream));
  const unsigned G = (unsigned)J.n_jobs, xb = (unsigned)((max_q + DB_THREADS - 1) / DB_THREADS);
  hipLaunchKernelGGL(descdb_gather_kernel, dim3(xb, G), dim3(DB_THREADS), 0, ctx->stream, J, k, (const QueryMid *)mid, key_ge, key_lt, n_lt,
                     (const int *)bad, qd, qc, S);
  {
    // the worst case is every query accepted; the searches of a group share the chip
    const int qblocks = (max_q + DB_QPB - 1) / DB_QPB;
    DbSweepConst sc;
    sc.n_tiles = db->n_tiles; sc.n_fixed = 0; sc.s_desc = S.s_desc; sc.s_int = S.s_int;
    sc.splits = ctx->dr_splits > 0 ? std::max(1, std::min(std::min(ctx->dr_splits, DB_MAX_SPLITS), db->n_tiles)) : 0;
    const int row = sc.splits > 0 ? qblocks * sc.splits : std::max(std::max(DB_ROW / J.n_jobs, 64), qblocks);
    StageScope ts1(ctx, MODS_STAGE_DISTRACTOR_SWEEP);
    hipLaunchKernelGGL(descdb_sweep_kernel, dim3(row, G), dim3(DB_THREADS), 0, ctx->stream, sc, (const int *)S.count, (const int8_t *)S.desc,
                       (const int *)S.qc, (const int *)S.list, S.ddb_q, (const int8_t *)db->desc.get(), (const int *)db->seed.get(),
                       (const unsigned int *)db->parity.get());
  }
  hipLaunchKernelGGL(descdb_fold_kernel, dim3(xb, G), dim3(DB_THREADS), 0, ctx->stream, J, k.sqminratio, (const QueryMid *)mid, bad, S,
                     ctx->dr_count.get());
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// behind the emit kernels
int distractor_finish(mods_ctx *ctx, const MatchJobs &J, int max_q, size_t pad) {
  const DrPtrs S = dr_carve(ctx, pad);
  StageScope ts(ctx, MODS_STAGE_DISTRACTOR);
  hipLaunchKernelGGL(descdb_ratio_kernel, dim3((max_q + DB_THREADS - 1) / DB_THREADS, J.n_jobs), dim3(DB_THREADS), 0, ctx->stream, J, S, ctx->max_cand);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// rows [row0, row0 + n) of a database from n dense rows on the device (row0 a multiple of 32), on stream s
static void descdb_pack_rows(mods_descdb *db, hipStream_t s, const unsigned char *raw_dev, int n, long row0) {
  hipLaunchKernelGGL(descdb_pack_kernel, dim3((n + 127) / 128), dim3(DB_THREADS), 0, s, raw_dev, n, row0, db->desc.get(), (int *)nullptr,
                     db->seed.get(), db->parity.get(), (int *)nullptr);
}

// the device arrays of a database of n rows, zeroed where the pack kernel does not write (on the current device, waits)
static int descdb_alloc(mods_descdb *db, long n, hipStream_t s) {
  db->n = n; db->n_tiles = (int)((n + 31) / 32);
  if (n == 0) return MODS_OK;
  const size_t rows = ((size_t)db->n_tiles + 1) * 32;
  MODS_HIP_CHECK(db->desc.reserve(rows * 128));
  MODS_HIP_CHECK(db->seed.reserve(rows));
  MODS_HIP_CHECK(db->parity.reserve((size_t)db->n_tiles + 1));
  MODS_HIP_CHECK(hipMemsetAsync(db->desc.get() + (rows - 32) * 128, 0, 32 * 128, s));
  MODS_HIP_CHECK(hipMemsetAsync(db->seed.get(), 0, rows * sizeof(int), s));
  MODS_HIP_CHECK(hipMemsetAsync(db->parity.get(), 0, ((size_t)db->n_tiles + 1) * sizeof(unsigned int), s));
  return MODS_OK;
}

// dDB of n host rows (n >= 1, db->n >= 1) into out, in steps of DB_CHUNK rows through the context's staging; waits
static int descdb_min_dist_run(mods_ctx *ctx, const mods_descdb *db, const unsigned char *rows_host, int n, int *out) {
  const int step = std::min(n, DB_CHUNK);
  const size_t pad = (((size_t)step + 31) & ~(size_t)31) + 32;
  MODS_HIP_CHECK(reserve_scratch(ctx, ctx->dr_stage, (size_t)step * 128, (size_t)step * 128));
  MODS_HIP_CHECK(reserve_scratch(ctx, ctx->dr_out, pad * 128 / sizeof(int) + 2 * pad, pad * 128 / sizeof(int) + 2 * pad));
  MODS_HIP_CHECK(reserve_scratch(ctx, ctx->dr_host, (size_t)step, (size_t)step));
  int8_t *qd = (int8_t *)ctx->dr_out.get();
  int *qc = ctx->dr_out + pad * 128 / sizeof(int), *ddb = qc + pad;
  for (int b = 0; b < n; b += step) {
    const int m = std::min(step, n - b);
    const DbGrid gr = descdb_grid(db->n, m, ctx->dr_splits);
    MODS_HIP_CHECK(hipMemcpyAsync(ctx->dr_stage, rows_host + (size_t)b * 128, (size_t)m * 128, hipMemcpyHostToDevice, ctx->stream));
    StageScope ts(ctx, MODS_STAGE_DISTRACTOR);
    hipLaunchKernelGGL(descdb_pack_kernel, dim3((m + 127) / 128), dim3(DB_THREADS), 0, ctx->stream, (const unsigned char *)ctx->dr_stage.get(), m, 0l,
                       qd, qc, (int *)nullptr, (unsigned int *)nullptr, ddb);
    {
      DbSweepConst sc;
      sc.n_tiles = db->n_tiles; sc.splits = gr.splits; sc.n_fixed = m; sc.s_desc = 0; sc.s_int = 0;
      StageScope ts1(ctx, MODS_STAGE_DISTRACTOR_SWEEP);
      hipLaunchKernelGGL(descdb_sweep_kernel, dim3(gr.qblocks * gr.splits, 1), dim3(DB_THREADS), 0, ctx->stream, sc, (const int *)nullptr,
                         (const int8_t *)qd, (const int *)qc, (const int *)nullptr, ddb, (const int8_t *)db->desc.get(),
                         (const int *)db->seed.get(), (const unsigned int *)db->parity.get());
    }
    MODS_HIP_CHECK(hipGetLastError());
    MODS_HIP_CHECK(hipMemcpyAsync(ctx->dr_host, ddb, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    MODS_HIP_CHECK(stream_wait(ctx->stream));
    memcpy(out + b, ctx->dr_host.get(), sizeof(int) * (size_t)m);
  }
  return MODS_OK;
}

static int descdb_check_pair(const char *who, const mods_ctx *c, const mods_descdb *db) {
  if (!c || !db) { set_error("%s: null context or database", who); return MODS_E_ARG; }
  if (db->device != c->device) { set_error("%s: the database lives on device %d, the context on device %d", who, db->device, c->device); return MODS_E_ARG; }
  return MODS_OK;
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_descdb_create(int device, const uint8_t *desc_host, long n, mods_descdb **out) {
  if (!out || n < 0 || device < 0 || (n > 0 && !desc_host)) { set_error("descdb_create: null argument, a negative count or a negative device"); return MODS_E_ARG; }
  if (n > DESCDB_MAX_ROWS) { set_error("descdb_create: %ld rows, the capacity is %ld", n, DESCDB_MAX_ROWS); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipSetDevice(device));
  mods_descdb *db = new mods_descdb;
  db->device = device;
  hipStream_t s = thread_stream(device);
  int rc = descdb_alloc(db, n, s);
  Buf<unsigned char> stage;
  if (!rc && n > 0 && stage.reserve((size_t)std::min<long>(n, DB_CHUNK) * 128) != hipSuccess) { set_error("descdb_create: no memory for the staging buffer"); rc = MODS_E_HIP; }
  for (long b = 0; !rc && b < n; b += DB_CHUNK) {
    const int m = (int)std::min<long>(DB_CHUNK, n - b);
    // (the copy waits: the staging buffer is free again when the next step overwrites it only after this step's kernel, same stream)
    if (copy_wait(s, stage.get(), desc_host + (size_t)b * 128, (size_t)m * 128, hipMemcpyHostToDevice) != hipSuccess) { set_error("descdb_create: upload failed"); rc = MODS_E_HIP; break; }
    descdb_pack_rows(db, s, stage.get(), m, b);
    if (hipGetLastError() != hipSuccess || stream_wait(s) != hipSuccess) { set_error("descdb_create: the pack launch failed"); rc = MODS_E_HIP; }
  }
  if (rc) { delete db; return rc; }
  *out = db;
  return MODS_OK;
}

int mods_descdb_create_from_reps(mods_ctx *c, const mods_imgrep *const *reps, int n_reps, mods_descdb **out) {
  if (!c || !out || n_reps < 0 || (n_reps > 0 && !reps)) { set_error("descdb_create_from_reps: null argument or a negative count"); return MODS_E_ARG; }
  long total = 0;
  for (int r = 0; r < n_reps; r++) {
    if (!reps[r]) { set_error("descdb_create_from_reps: bank %d is null", r); return MODS_E_ARG; }
    const mods_region *reg; int n, dev; hipStream_t s;
    imgrep_view(reps[r], &reg, &n, &dev, &s);
    if (dev != c->device) { set_error("descdb_create_from_reps: bank %d lives on device %d, the context on device %d", r, dev, c->device); return MODS_E_ARG; }
    total += n;
  }
  if (total > DESCDB_MAX_ROWS) { set_error("descdb_create_from_reps: %ld rows, the capacity is %ld", total, DESCDB_MAX_ROWS); return MODS_E_CAPACITY; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  mods_descdb *db = new mods_descdb;
  db->device = c->device;
  int rc = descdb_alloc(db, total, c->stream);
  Buf<unsigned char> raw;
  if (!rc && total > 0 && raw.reserve((size_t)total * 128) != hipSuccess) { set_error("descdb_create_from_reps: no memory for the staging buffer"); rc = MODS_E_HIP; }
  long at = 0;
  for (int r = 0; !rc && r < n_reps; r++) {
    const mods_region *reg; int n, dev; hipStream_t s;
    imgrep_view(reps[r], &reg, &n, &dev, &s);
    if (n == 0) continue;
    // a bank is appended to on its owner's stream
    if (s != c->stream && stream_wait(s) != hipSuccess) { set_error("descdb_create_from_reps: waiting for bank %d failed", r); rc = MODS_E_HIP; break; }
    if (hipMemcpy2DAsync(raw.get() + (size_t)at * 128, 128, (const unsigned char *)reg + offsetof(mods_region, desc), sizeof(mods_region), 128, (size_t)n,
                         hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { set_error("descdb_create_from_reps: copying bank %d failed", r); rc = MODS_E_HIP; }
    at += n;
  }
  for (long b = 0; !rc && b < total; b += DB_CHUNK) descdb_pack_rows(db, c->stream, raw.get() + (size_t)b * 128, (int)std::min<long>(DB_CHUNK, total - b), b);
  if (!rc && (hipGetLastError() != hipSuccess || stream_wait(c->stream) != hipSuccess)) { set_error("descdb_create_from_reps: the pack launch failed"); rc = MODS_E_HIP; }
  if (rc) { (void)stream_wait(c->stream); delete db; return rc; }
  *out = db;
  return MODS_OK;
}

long mods_descdb_count(const mods_descdb *db) { return db ? db->n : 0; }

void mods_descdb_destroy(mods_descdb *db) { descdb_unref(db); }

int mods_descdb_min_dist(mods_ctx *c, const mods_descdb *db, const uint8_t *desc_host, int n, int *d2_out) {
  int rc = descdb_check_pair("descdb_min_dist", c, db);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!desc_host || !d2_out))) { set_error("descdb_min_dist: null argument or a negative count"); return MODS_E_ARG; }
  if (n == 0) return MODS_OK;
  if (db->n == 0) { for (int i = 0; i < n; i++) d2_out[i] = INT_MAX; return MODS_OK; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  return descdb_min_dist_run(c, db, desc_host, n, d2_out);
}

int mods_filter_distractor(mods_ctx *c, const mods_descdb *db, const mods_region *q, int n_q, double ratio, mods_tentative *tent, double *u6,
                           double *laf, int n, int *d_db_out, int *n_out) {
  int rc = descdb_check_pair("filter_distractor", c, db);
  if (rc) return rc;
  if (!n_out || n < 0 || n_q < 0 || (n > 0 && (!tent || !q))) { set_error("filter_distractor: null argument or a negative count"); return MODS_E_ARG; }
  const double sq = ratio * ratio;
  if (!(sq < 1.0)) { set_error("filter_distractor: ratio %g, below 1 expected", ratio); return MODS_E_ARG; }
  for (int i = 0; i < n; i++)
    if (tent[i].q < 0 || tent[i].q >= n_q) { set_error("filter_distractor: tentative %d names query %d of %d", i, tent[i].q, n_q); return MODS_E_ARG; }
  *n_out = n;
  if (n == 0) return MODS_OK;
  std::vector<int> ddb((size_t)n, INT_MAX);
  if (db->n > 0) {
    std::vector<unsigned char> rows((size_t)n * 128);
    for (int i = 0; i < n; i++) memcpy(&rows[(size_t)i * 128], q[tent[i].q].desc, 128);
    MODS_HIP_CHECK(hipSetDevice(c->device));
    if ((rc = descdb_min_dist_run(c, db, rows.data(), n, ddb.data()))) return rc;
  }
  int kept = 0;
  for (int i = 0; i < n; i++) {
    const float d1 = tent[i].d1;
    const double r = (double)(d1 / tent[i].d2);
    const double rdb = db->n > 0 ? (double)(d1 / (float)ddb[i]) : r;
    const double r2 = (r < rdb) ? rdb : r;
    if (!(r2 <= sq)) continue;
    if (kept != i) {
      tent[kept] = tent[i];
      if (u6) memcpy(u6 + (size_t)kept * 6, u6 + (size_t)i * 6, 6 * sizeof(double));
      if (laf) memcpy(laf + (size_t)kept * 14, laf + (size_t)i * 14, 14 * sizeof(double));
    }
    if (r < rdb) tent[kept].ratio = sqrt(rdb);
    if (d_db_out) d_db_out[kept] = ddb[i];
    kept++;
  }
  *n_out = kept;
  return MODS_OK;
}

int mods_ctx_distractor_db(mods_ctx *c, const mods_descdb *full, const mods_descdb *half) {
  if (!c) { set_error("distractor_db: null context"); return MODS_E_ARG; }
  const mods_descdb *want[2] = {full, half};
  for (int s = 0; s < 2; s++)
    if (want[s] && want[s]->device != c->device) {
      set_error("distractor_db: the %s database lives on device %d, the context on device %d", s ? "half" : "full", want[s]->device, c->device);
      return MODS_E_ARG;
    }
  for (int s = 0; s < 2; s++) {
    const mods_descdb *w = want[s] && want[s]->n > 0 ? want[s] : nullptr;      // an empty database equals none
    if (w) const_cast<mods_descdb *>(w)->refs.fetch_add(1);
    // a search queued on the stream may still read the database that goes
    if (c->dr_db[s] && c->stream) { (void)hipSetDevice(c->device); (void)stream_wait(c->stream); }
    descdb_unref(c->dr_db[s]);
    c->dr_db[s] = w;
  }
  dev_state_changed(c);              // (recorded launch chains are not replayed across the change)
  return MODS_OK;
}

int mods_distractor_counts(mods_ctx *c, int *n_forward, int *n_kept) {
  if (!c || !n_forward || !n_kept) { set_error("distractor_counts: null argument"); return MODS_E_ARG; }
  if (!c->m_count.get()) { set_error("distractor_counts: no search has run on this context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(stream_wait(c->stream));
  *n_kept = read_slot(c->m_count, count_slot());
  *n_forward = c->dr_last_vetoed ? read_slot(c->dr_count, 0) : *n_kept;
  return MODS_OK;
}

int mods_distractor_fetch(mods_ctx *c, int *d_db_out, int max, int *n) {
  if (!c || !n || max < 0 || (max > 0 && !d_db_out)) { set_error("distractor_fetch: null argument or a negative count"); return MODS_E_ARG; }
  *n = 0;
  if (!c->m_count.get()) { set_error("distractor_fetch: no search has run on this context"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(stream_wait(c->stream));
  if (!c->dr_last_vetoed) return MODS_OK;
  const int m = std::min(read_slot(c->m_count, count_slot()), c->max_cand);
  *n = m;
  if (m > max) { set_error("distractor_fetch: %d survivors, room for %d", m, max); return MODS_E_CAPACITY; }
  if (m == 0) return MODS_OK;
  MODS_HIP_CHECK(copy_wait(c->stream, d_db_out, c->dr_int.get(), sizeof(int) * (size_t)m, hipMemcpyDeviceToHost));
  return MODS_OK;
}

int mods_descdb_grid(long m, int n_queries, int forced_splits, int out[3]) {
  if (!out || m < 0 || m > DESCDB_MAX_ROWS || n_queries < 0 || forced_splits < 0) {
    set_error("descdb_grid: null argument, a negative count or more than %ld rows", DESCDB_MAX_ROWS);
    return MODS_E_ARG;
  }
  const DbGrid gr = descdb_grid(m, n_queries, forced_splits);
  out[0] = gr.qblocks; out[1] = gr.splits; out[2] = gr.tiles_per_split;
  return MODS_OK;
}

int mods_ctx_descdb_splits(mods_ctx *c, int splits) {
  if (!c || splits < 0) { set_error("descdb_splits: null context or a negative count"); return MODS_E_ARG; }
  c->dr_splits = splits;
  return MODS_OK;
}

}  // extern "C"
