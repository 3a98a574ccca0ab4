// Match and region images: an RGB8 canvas in HBM and a tile rasteriser (the contract: include/mods_hip.h, "match and region
// images"; restated in tests/draw_ref.py).  Three kinds of element - solid disc, one-pixel line in closed form, anti-aliased thick
// segment whose runs form polylines - are drawn in list order, everything in 64-bit integers.
//
// Shape: one workgroup per 16 x 16 tile, one pixel per lane, the pixel's R G B in registers from the first element to the last.
// The workgroup walks the list in chunks of 256: each lane tests one element's inflated box against the tile, the hits are
// compacted in list order into LDS (ballot + popcount per wave, the waves' counts through LDS - the idiom of match.hip and
// detect.hip), then every lane runs the hits, all lanes reading one LDS address at a time.  A lane keeps the 16-bit subsample mask
// of the open polyline, ORs its capsules into it and blends when the run changes; the mask lives in a register, so it survives a
// chunk boundary.  No atomics and no sort: the order is the list's by construction.  The run of a polyline is made unique when the
// list is staged (host lists) or built (region contours), so that a tile which sees only two runs' members with an element between
// them culled never joins them.  VALU only.
#include "common.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

struct mods_canvas {
  mods_ctx *ctx = nullptr;
  int w = 0, h = 0;
  mods::Buf<unsigned char> px;          // [h][w][3]
  mods::Buf<mods_draw_elem> elems;      // the staged / built list of the last draw call
  mods::Buf<unsigned char> stage;       // a host image on its way in
  mods::Buf<int> dropped_dev;           // the contour builder's count
};

namespace mods {

constexpr int D_TILE = 16;
constexpr int D_THREADS = D_TILE * D_TILE;
constexpr int D_CHUNK = D_THREADS;       // elements tested per round, one per lane
constexpr int D_WAVES = D_THREADS / 64;
constexpr int D_COORD_MAX = 32767, D_SEG_MAX = 2047, D_T_MAX = 255, D_SAT = 40000, D_CANVAS_MAX = 16384;
constexpr int D_SEGS = 21;               // segments of a region's contour (22 points)

struct DrawTables { double C[D_SEGS + 1], S[D_SEGS + 1]; };

__host__ __device__ __forceinline__ long long draw_floor_div(long long a, long long b) {   // b > 0
  long long q = a / b;
  if (a % b < 0) q--;
  return q;
}

// whether the element can touch the tile with corner (tx0, ty0): its box, a SEG's inflated by half its thickness and the reach of a
// subsample (t / 2 + 3 sqrt(2) / 8 < (t + 1) / 2 + 1)
__device__ __forceinline__ bool draw_hits_tile(const mods_draw_elem &e, int tx0, int ty0) {
  int x0, x1, y0, y1;
  if (e.kind == MODS_DRAW_DISC) { x0 = e.ax - e.t; x1 = e.ax + e.t; y0 = e.ay - e.t; y1 = e.ay + e.t; }
  else if (e.kind == MODS_DRAW_LINE || e.kind == MODS_DRAW_SEG) {
    const int m = e.kind == MODS_DRAW_SEG ? (e.t + 1) / 2 + 1 : 0;
    x0 = min(e.ax, e.bx) - m; x1 = max(e.ax, e.bx) + m; y0 = min(e.ay, e.by) - m; y1 = max(e.ay, e.by) + m;
  } else return false;
  return x0 <= tx0 + D_TILE - 1 && x1 >= tx0 && y0 <= ty0 + D_TILE - 1 && y1 >= ty0;
}

__device__ __forceinline__ bool draw_line_covers(const mods_draw_elem &e, int x, int y) {
  int ax = e.ax, ay = e.ay, bx = e.bx, by = e.by;
  const int adx = abs(bx - ax), ady = abs(by - ay);
  if (adx >= ady) {
    if (bx < ax) { int t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; }
    const long long D = (long long)bx - ax;
    if (D == 0) return x == ax && y == ay;
    if (x < ax || x > bx) return false;
    return (long long)y == (long long)ay + draw_floor_div(2ll * (x - ax) * ((long long)by - ay) + D, 2ll * D);
  }
  if (by < ay) { int t = ax; ax = bx; bx = t; t = ay; ay = by; by = t; }
  const long long D = (long long)by - ay;
  if (y < ay || y > by) return false;
  return (long long)x == (long long)ax + draw_floor_div(2ll * (y - ay) * ((long long)bx - ax) + D, 2ll * D);
}

// the 16 subsamples of pixel (x, y) inside the capsule, bit 4 * j + i for the offsets (2 i - 3, 2 j - 3) eighths
__device__ __forceinline__ unsigned draw_seg_mask(const mods_draw_elem &e, int x, int y) {
  const long long Ax = 8ll * e.ax, Ay = 8ll * e.ay, Bx = 8ll * e.bx, By = 8ll * e.by;
  const long long dx = Bx - Ax, dy = By - Ay, L2 = dx * dx + dy * dy;
  const long long h = 4ll * e.t, h2 = h * h, h2L2 = h2 * L2;
  unsigned mask = 0;
  for (int j = 0; j < 4; j++) {
    const long long py = 8ll * y + (2 * j - 3);
    for (int i = 0; i < 4; i++) {
      const long long px = 8ll * x + (2 * i - 3);
      const long long wx = px - Ax, wy = py - Ay;
      const long long s = wx * dx + wy * dy;
      bool in;
      if (L2 == 0 || s <= 0) in = wx * wx + wy * wy <= h2;
      else if (s >= L2) { const long long ux = px - Bx, uy = py - By; in = ux * ux + uy * uy <= h2; }
      else { const long long cr = wx * dy - wy * dx; in = cr * cr <= h2L2; }
      mask |= (in ? 1u : 0u) << (4 * j + i);
    }
  }
  return mask;
}

__device__ __forceinline__ void draw_blend(int &r, int &g, int &b, unsigned rgb, unsigned mask) {
  const int c = __popc(mask);
  if (!c) return;
  r = (r * (16 - c) + (int)((rgb >> 16) & 255u) * c + 8) >> 4;
  g = (g * (16 - c) + (int)((rgb >> 8) & 255u) * c + 8) >> 4;
  b = (b * (16 - c) + (int)(rgb & 255u) * c + 8) >> 4;
}

// grid = (ceil(w / 16), ceil(h / 16)).  el[i].group is unique per polyline; kind MODS_DRAW_NONE is skipped
__global__ __launch_bounds__(D_THREADS) void draw_tiles_kernel(unsigned char *__restrict__ px, int w, int h, const mods_draw_elem *__restrict__ el,
                                                               int n) {
  __shared__ mods_draw_elem s_hit[D_CHUNK];
  __shared__ int s_wave[D_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tx0 = blockIdx.x * D_TILE, ty0 = blockIdx.y * D_TILE;
  const int x = tx0 + (tid & (D_TILE - 1)), y = ty0 + tid / D_TILE;
  const bool live = x < w && y < h;
  const size_t at = ((size_t)y * (size_t)w + (size_t)x) * 3;
  int r = 0, g = 0, b = 0;
  if (live) { r = px[at]; g = px[at + 1]; b = px[at + 2]; }
  bool open = false;
  int run = 0;
  unsigned run_rgb = 0, mask = 0;
  for (int base = 0; base < n; base += D_CHUNK) {
    const int i = base + tid;
    mods_draw_elem e;
    bool hit = false;
    if (i < n) { e = el[i]; hit = draw_hits_tile(e, tx0, ty0); }
    const unsigned long long bal = __ballot(hit);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();                                     // the hits of the chunk before this one are consumed
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
    for (int k = 0; k < D_WAVES; k++) { const int c = s_wave[k]; if (k < wv) off += c; total += c; }
    if (hit) s_hit[off + before] = e;                    // off + before < total <= D_CHUNK
    __syncthreads();
    for (int j = 0; j < total; j++) {
      const mods_draw_elem q = s_hit[j];
      if (q.kind == MODS_DRAW_SEG) {
        if (!open || q.group != run) {
          if (open) draw_blend(r, g, b, run_rgb, mask);
          open = true; run = q.group; run_rgb = q.rgb; mask = 0;
        }
        mask |= draw_seg_mask(q, x, y);
      } else {
        if (open) { draw_blend(r, g, b, run_rgb, mask); open = false; }
        bool in;
        if (q.kind == MODS_DRAW_DISC) {
          const long long ddx = (long long)x - q.ax, ddy = (long long)y - q.ay;
          in = ddx * ddx + ddy * ddy <= (long long)q.t * q.t;
        } else in = draw_line_covers(q, x, y);
        if (in) { r = (int)((q.rgb >> 16) & 255u); g = (int)((q.rgb >> 8) & 255u); b = (int)(q.rgb & 255u); }
      }
    }
  }
  if (open) draw_blend(r, g, b, run_rgb, mask);
  if (live) { px[at] = (unsigned char)r; px[at + 1] = (unsigned char)g; px[at + 2] = (unsigned char)b; }
}

// One thread per region: its 22 contour points (fp64, one rounding per operation, in the contract's order) and 21 SEG of group i.
// A point outside the coordinate range or a segment that is too long drops the polyline: its 21 members become MODS_DRAW_NONE
__global__ __launch_bounds__(D_THREADS) void draw_contours_kernel(const mods_region *__restrict__ reg, int begin, int count, DrawTables tab, int dx,
                                                                  int dy, int t, unsigned rgb, mods_draw_elem *__restrict__ out,
                                                                  int *__restrict__ n_dropped) {
  const int i = blockIdx.x * D_THREADS + threadIdx.x;
  bool bad = false;
  if (i < count) {
    const mods_region rg = reg[(size_t)begin + i];
    const double s3 = __dmul_rn(3.0, rg.s);
    const double A11 = __dmul_rn(s3, rg.a11), A12 = __dmul_rn(s3, rg.a12), A21 = __dmul_rn(s3, rg.a21), A22 = __dmul_rn(s3, rg.a22);
    mods_draw_elem *o = out + (size_t)D_SEGS * i;
    int px = 0, py = 0;
    for (int k = 0; k <= D_SEGS; k++) {
      const double vx = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(A11, tab.C[k]), __dmul_rn(A12, tab.S[k])), rg.x), (double)dx);
      const double vy = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(A21, tab.C[k]), __dmul_rn(A22, tab.S[k])), rg.y), (double)dy);
      const double fx = floor(vx), fy = floor(vy);
      int qx = 0, qy = 0;
      if (fx >= -(double)D_COORD_MAX && fx <= (double)D_COORD_MAX && fy >= -(double)D_COORD_MAX && fy <= (double)D_COORD_MAX) {
        qx = (int)fx; qy = (int)fy;
      } else bad = true;                                 // NaN fails every comparison
      if (k > 0) {
        if (abs(qx - px) > D_SEG_MAX || abs(qy - py) > D_SEG_MAX) bad = true;
        mods_draw_elem e;
        e.kind = MODS_DRAW_SEG; e.ax = px; e.ay = py; e.bx = qx; e.by = qy; e.t = t; e.rgb = rgb; e.group = i;
        o[k - 1] = e;
      }
      px = qx; py = qy;
    }
    if (bad)
      for (int k = 0; k < D_SEGS; k++) { o[k].kind = MODS_DRAW_NONE; o[k].ax = o[k].ay = o[k].bx = o[k].by = 0; }
  }
  const int c = __syncthreads_count(bad ? 1 : 0);
  if (threadIdx.x == 0 && c) atomicAdd(n_dropped, D_SEGS * c);
}

__global__ __launch_bounds__(D_THREADS) void draw_fill_kernel(unsigned char *__restrict__ px, size_t n_px, unsigned rgb) {
  const size_t i = (size_t)blockIdx.x * D_THREADS + threadIdx.x;
  if (i >= n_px) return;
  px[3 * i] = (unsigned char)(rgb >> 16); px[3 * i + 1] = (unsigned char)(rgb >> 8); px[3 * i + 2] = (unsigned char)rgb;
}

__device__ __forceinline__ unsigned char draw_f32_to_u8(float v) {
  return (unsigned char)rintf(fminf(fmaxf(v, 0.f), 255.f));   // fmaxf(NaN, 0) = 0
}

// source pixel (sx, sy) goes to (x0 + sx, y0 + sy) when that lies on the canvas.  SRC: 1 = grey bytes, 3 = R G B bytes, 4 = fp32 grey.
// stride in elements of the source's rows
template <int SRC>
__global__ __launch_bounds__(D_THREADS) void draw_blit_kernel(unsigned char *__restrict__ px, int w, int h, const void *__restrict__ src, int sw, int sh,
                                                              size_t stride, int x0, int y0) {
  const int sx = blockIdx.x * D_TILE + (threadIdx.x & (D_TILE - 1)), sy = blockIdx.y * D_TILE + threadIdx.x / D_TILE;
  if (sx >= sw || sy >= sh) return;
  const long long x = (long long)x0 + sx, y = (long long)y0 + sy;
  if (x < 0 || y < 0 || x >= w || y >= h) return;
  const size_t at = ((size_t)y * (size_t)w + (size_t)x) * 3, from = (size_t)sy * stride;
  unsigned char r, g, b;
  if (SRC == 3) { const unsigned char *s = (const unsigned char *)src + from + 3 * (size_t)sx; r = s[0]; g = s[1]; b = s[2]; }
  else if (SRC == 1) r = g = b = ((const unsigned char *)src)[from + sx];
  else r = g = b = draw_f32_to_u8(((const float *)src)[from + sx]);
  px[at] = r; px[at + 1] = g; px[at + 2] = b;
}

static int draw_blit(mods_canvas *cv, int kind, const void *src_dev, int sw, int sh, size_t stride, int x0, int y0) {
  const dim3 grid((sw + D_TILE - 1) / D_TILE, (sh + D_TILE - 1) / D_TILE);
  hipStream_t st = cv->ctx->stream;
  if (kind == 3) hipLaunchKernelGGL((draw_blit_kernel<3>), grid, dim3(D_THREADS), 0, st, cv->px.get(), cv->w, cv->h, src_dev, sw, sh, stride, x0, y0);
  else if (kind == 1) hipLaunchKernelGGL((draw_blit_kernel<1>), grid, dim3(D_THREADS), 0, st, cv->px.get(), cv->w, cv->h, src_dev, sw, sh, stride, x0, y0);
  else hipLaunchKernelGGL((draw_blit_kernel<4>), grid, dim3(D_THREADS), 0, st, cv->px.get(), cv->w, cv->h, src_dev, sw, sh, stride, x0, y0);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

static bool draw_in_range(int v) { return v >= -D_COORD_MAX && v <= D_COORD_MAX; }

// The drop rule over a host list, in place: members of one polyline get one run number (unique in the list) for a group, what is
// dropped becomes MODS_DRAW_NONE.  MODS_E_ARG for what is no coordinate's fault
static int draw_validate(std::vector<mods_draw_elem> &v, int *n_dropped) {
  int dropped = 0, run = 0;
  size_t i = 0;
  while (i < v.size()) {
    mods_draw_elem &e = v[i];
    if (e.kind != MODS_DRAW_DISC && e.kind != MODS_DRAW_LINE && e.kind != MODS_DRAW_SEG) { set_error("canvas_draw: element %zu has kind %d", i, e.kind); return MODS_E_ARG; }
    if (e.t < 0 && e.kind != MODS_DRAW_LINE) { set_error("canvas_draw: element %zu has t = %d", i, e.t); return MODS_E_ARG; }
    if (e.kind == MODS_DRAW_DISC) {
      if (e.t > D_COORD_MAX) { set_error("canvas_draw: disc %zu has radius %d (at most %d)", i, e.t, D_COORD_MAX); return MODS_E_ARG; }
      if (!draw_in_range(e.ax) || !draw_in_range(e.ay)) { e.kind = MODS_DRAW_NONE; dropped++; }
      i++;
    } else if (e.kind == MODS_DRAW_LINE) {
      if (!draw_in_range(e.ax) || !draw_in_range(e.ay) || !draw_in_range(e.bx) || !draw_in_range(e.by)) { e.kind = MODS_DRAW_NONE; dropped++; }
      i++;
    } else {
      size_t j = i;
      bool bad = false;
      while (j < v.size() && v[j].kind == MODS_DRAW_SEG && v[j].group == e.group && v[j].rgb == e.rgb) {
        const mods_draw_elem &s = v[j];
        if (s.t < 0 || s.t > D_T_MAX) { set_error("canvas_draw: segment %zu has thickness %d (0 .. %d)", j, s.t, D_T_MAX); return MODS_E_ARG; }
        if (!draw_in_range(s.ax) || !draw_in_range(s.ay) || !draw_in_range(s.bx) || !draw_in_range(s.by)) bad = true;
        else if (std::abs(s.bx - s.ax) > D_SEG_MAX || std::abs(s.by - s.ay) > D_SEG_MAX) bad = true;
        j++;
      }
      for (size_t k = i; k < j; k++) { v[k].group = run; if (bad) v[k].kind = MODS_DRAW_NONE; }
      if (bad) dropped += (int)(j - i);
      run++;
      i = j;
    }
  }
  *n_dropped = dropped;
  return MODS_OK;
}

static int draw_launch_tiles(mods_canvas *cv, const mods_draw_elem *el_dev, int n) {
  if (n <= 0) return MODS_OK;
  hipLaunchKernelGGL(draw_tiles_kernel, dim3((cv->w + D_TILE - 1) / D_TILE, (cv->h + D_TILE - 1) / D_TILE), dim3(D_THREADS), 0, cv->ctx->stream,
                     cv->px.get(), cv->w, cv->h, el_dev, n);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

static DrawTables draw_tables(int table) {
  DrawTables t;
  for (int l = 0; l <= D_SEGS; l++) { t.C[l] = cos(l * M_PI / 10); t.S[l] = sin(l * M_PI / 10); }
  if (table == MODS_DRAW_TABLE_MATCHES) t.C[D_SEGS] = t.S[D_SEGS] = 0;
  return t;
}

// the contours of a bank's regions into cv->elems; *n_dropped after a stream wait
static int draw_build_contours(mods_canvas *cv, const mods_imgrep *rep, int begin, int count, int dx, int dy, int thickness, unsigned rgb, int table,
                               int *n_dropped) {
  if (!cv || !rep || !n_dropped) { set_error("canvas_draw_regions: null argument"); return MODS_E_ARG; }
  if (table != MODS_DRAW_TABLE_REGIONS && table != MODS_DRAW_TABLE_MATCHES) { set_error("canvas_draw_regions: table %d", table); return MODS_E_ARG; }
  if (thickness < 0 || thickness > D_T_MAX) { set_error("canvas_draw_regions: thickness %d (0 .. %d)", thickness, D_T_MAX); return MODS_E_ARG; }
  if (!draw_in_range(dx) || !draw_in_range(dy)) { set_error("canvas_draw_regions: offset (%d, %d)", dx, dy); return MODS_E_ARG; }
  const int n_rep = mods_imgrep_count(rep);
  if (begin < 0 || count < 0 || begin > n_rep || count > n_rep - begin) {
    set_error("canvas_draw_regions: regions [%d, %d + %d) of %d", begin, begin, count, n_rep);
    return MODS_E_ARG;
  }
  if (count > (1 << 26)) { set_error("canvas_draw_regions: %d regions in one call", count); return MODS_E_ARG; }
  *n_dropped = 0;
  if (count == 0) return MODS_OK;
  mods_ctx *c = cv->ctx;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const size_t n = (size_t)D_SEGS * (size_t)count;
  MODS_HIP_CHECK(mods::reserve_scratch(c, cv->elems, n, n + n / 4));
  if (!cv->dropped_dev.get()) MODS_HIP_CHECK(cv->dropped_dev.reserve(1));
  MODS_HIP_CHECK(hipMemsetAsync(cv->dropped_dev.get(), 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(draw_contours_kernel, dim3((count + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, c->stream, mods_imgrep_regions_dev(rep), begin,
                     count, draw_tables(table), dx, dy, thickness, rgb, cv->elems.get(), cv->dropped_dev.get());
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

// ---- DrawMatches' element lists (host) ----------------------------------------------------------------------------

static int draw_sat(double v) { return (v >= -(double)D_SAT && v <= (double)D_SAT) ? (int)v : D_SAT; }   // NaN: D_SAT

struct DrawList {
  std::vector<mods_draw_elem> v;
  int next_group = 0;
  void add(int kind, int ax, int ay, int bx, int by, int t, unsigned rgb, int group) {
    mods_draw_elem e;
    e.kind = kind; e.ax = ax; e.ay = ay; e.bx = bx; e.by = by; e.t = t; e.rgb = rgb; e.group = group;
    v.push_back(e);
  }
  void polyline(const int *px, const int *py, int t, unsigned rgb) {
    for (int k = 0; k < D_SEGS; k++) add(MODS_DRAW_SEG, px[k], py[k], px[k + 1], py[k + 1], t, rgb, next_group);
    next_group++;
  }
};

// frame f = x y a11 a12 a21 a22 s
static void draw_contour_plain(DrawList &l, const DrawTables &tab, const double *f, int dx, int dy, int t, unsigned rgb) {
  const double s3 = 3.0 * f[6];
  const double A11 = s3 * f[2], A12 = s3 * f[3], A21 = s3 * f[4], A22 = s3 * f[5];
  int px[D_SEGS + 1], py[D_SEGS + 1];
  for (int k = 0; k <= D_SEGS; k++) {
    const double p1 = A11 * tab.C[k], p2 = A12 * tab.S[k], p3 = A21 * tab.C[k], p4 = A22 * tab.S[k];
    const double sx = p1 + p2, sy = p3 + p4;
    const double vx = (sx + f[0]) + (double)dx, vy = (sy + f[1]) + (double)dy;
    px[k] = draw_sat(floor(vx)); py[k] = draw_sat(floor(vy));
  }
  l.polyline(px, py, t, rgb);
}

static void draw_contour_through(DrawList &l, const DrawTables &tab, const double *G, const double *f, int t, unsigned rgb) {
  const double s3 = 3.0 * f[6];
  const double B[9] = {s3 * f[2], s3 * f[3], f[0], s3 * f[4], s3 * f[5], f[1], 0., 0., 1.};
  double P[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      const double a = G[3 * r] * B[c], b = G[3 * r + 1] * B[3 + c], d = G[3 * r + 2] * B[6 + c];
      const double ab = a + b;
      P[3 * r + c] = ab + d;
    }
  int px[D_SEGS + 1], py[D_SEGS + 1];
  for (int k = 0; k <= D_SEGS; k++) {
    double X[3];
    for (int r = 0; r < 3; r++) {
      const double a = P[3 * r] * tab.C[k], b = P[3 * r + 1] * tab.S[k], d = P[3 * r + 2] * 1.0;
      const double ab = a + b;
      X[r] = ab + d;
    }
    px[k] = draw_sat(floor(X[0] / X[2])); py[k] = draw_sat(floor(X[1] / X[2]));   // X[2] = 0: inf or NaN, saturated
  }
  l.polyline(px, py, t, rgb);
}

static void draw_project(const double *G, double x, double y, double *xa, double *ya) {
  const double den = (G[6] * x + G[7] * y) + G[8];
  *xa = ((G[0] * x + G[1] * y) + G[2]) / den;
  *ya = ((G[3] * x + G[4] * y) + G[5]) / den;
}

// GetEpipolarLineF: the line of pt = (px, py, 1) under G (read column-wise) as y = k x + b
static void draw_epipolar_kb(const double *G, double px, double py, double *k, double *b) {
  double l[3];
  for (int j = 0; j < 3; j++) l[j] = (px * G[j] + py * G[3 + j]) + G[6 + j];
  const double xc = (-l[2]) / l[0];
  *b = (-l[2]) / l[1];
  *k = (0. - *b) / (xc - 0.);
}

// the minor coordinate of the closed-form line a -> b (ordered, D > 0) at major coordinate m
static long long draw_line_minor(long long am, long long an, long long dn, long long D, long long m) {
  return an + draw_floor_div(2 * (m - am) * dn + D, 2 * D);
}

// the LINE (ax, ay) -> (bx, by) clipped to the rectangle [rx, rx + rw) x [ry, ry + rh) by the contract's rule
static void draw_clipped_line(DrawList &l, int ax, int ay, int bx, int by, int rx, int ry, int rw, int rh, unsigned rgb) {
  if (!draw_in_range(ax) || !draw_in_range(ay) || !draw_in_range(bx) || !draw_in_range(by)) { l.add(MODS_DRAW_LINE, ax, ay, bx, by, 0, rgb, 0); return; }
  const bool xmajor = std::abs(bx - ax) >= std::abs(by - ay);
  long long am = xmajor ? ax : ay, an = xmajor ? ay : ax, bm = xmajor ? bx : by, bn = xmajor ? by : bx;
  if (bm < am) { std::swap(am, bm); std::swap(an, bn); }
  const long long D = bm - am, dn = bn - an;
  const long long m_lo = xmajor ? rx : ry, m_hi = m_lo + (xmajor ? rw : rh) - 1, n_lo = xmajor ? ry : rx, n_hi = n_lo + (xmajor ? rh : rw) - 1;
  bool any = false;
  long long fm = 0, fn = 0, lm = 0, ln = 0;
  for (long long m = std::max(am, m_lo); m <= std::min(bm, m_hi); m++) {
    const long long nn = D == 0 ? an : draw_line_minor(am, an, dn, D, m);
    if (nn < n_lo || nn > n_hi) continue;
    if (!any) { fm = m; fn = nn; any = true; }
    lm = m; ln = nn;
  }
  if (!any) return;
  if (xmajor) l.add(MODS_DRAW_LINE, (int)fm, (int)fn, (int)lm, (int)ln, 0, rgb, 0);
  else l.add(MODS_DRAW_LINE, (int)fn, (int)fm, (int)ln, (int)lm, 0, rgb, 0);
}

constexpr unsigned D_COLOUR1 = 0x0000ffu, D_COLOUR2 = 0x00ff00u, D_COLOUR_EPI = 0x00ffffu;
constexpr int D_SEP = 20;

static int draw_matches_check(const double *laf14, int n, const mods_draw_matches_params *par, double *Hinv) {
  if (!par || n < 0 || (n > 0 && !laf14)) { set_error("draw_matches: null argument"); return MODS_E_ARG; }
  if (par->r1 < 0 || par->r2 < 0 || par->r1 > D_T_MAX || par->r2 > D_T_MAX) { set_error("draw_matches: r1 = %d, r2 = %d (0 .. %d)", par->r1, par->r2, D_T_MAX); return MODS_E_ARG; }
  if (par->reproject_to_one_image) {
    double d;
    if (!invert3_adjugate(par->M, Hinv, &d)) { set_error("draw_matches: singular homography (determinant %g)", d); return MODS_E_ARG; }
  }
  return MODS_OK;
}

static void draw_matches_list(int which, int w1, int h1, int w2, int h2, const double *laf14, int n, const mods_draw_matches_params *par,
                              const double *Hinv, DrawList &l) {
  const DrawTables tab = draw_tables(MODS_DRAW_TABLE_MATCHES);
  const int r1 = par->r1, r2 = par->r2;
  if (par->reproject_to_one_image) {
    const double *G = which == 0 ? Hinv : par->M;
    const int own = which == 0 ? 0 : 7, other = which == 0 ? 7 : 0;
    if (!par->draw_only_centers)
      for (int m = 0; m < n; m++) {
        const double *f = laf14 + 14 * (size_t)m;
        draw_contour_plain(l, tab, f + own, 0, 0, r1, D_COLOUR1);
        draw_contour_through(l, tab, G, f + other, r2, D_COLOUR2);
      }
    for (int m = 0; m < n; m++) {
      const double *f = laf14 + 14 * (size_t)m;
      const int cx = draw_sat(f[own]), cy = draw_sat(f[own + 1]);
      double xa, ya;
      draw_project(G, f[other], f[other + 1], &xa, &ya);
      l.add(MODS_DRAW_DISC, cx, cy, 0, 0, r1 + 2, D_COLOUR1, 0);
      l.add(MODS_DRAW_DISC, draw_sat(xa), draw_sat(ya), 0, 0, r2, D_COLOUR2, 0);
      l.add(MODS_DRAW_LINE, draw_sat(xa), draw_sat(ya), cx, cy, 0, D_COLOUR2, 0);
    }
    return;
  }
  const int ox = which == 0 ? w1 + D_SEP : 0, oy = which == 0 ? 0 : h1 + D_SEP;
  if (!par->draw_only_centers)
    for (int m = 0; m < n; m++) {
      const double *f = laf14 + 14 * (size_t)m;
      draw_contour_plain(l, tab, f, 0, 0, r1, D_COLOUR2);
      draw_contour_plain(l, tab, f + 7, ox, oy, r2, D_COLOUR2);
    }
  double Mt[9];
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Mt[3 * r + c] = par->M[3 * c + r];
  for (int m = 0; m < n; m++) {
    const double *f = laf14 + 14 * (size_t)m;
    const int cx = draw_sat(f[0]), cy = draw_sat(f[1]);
    const int xa = draw_sat((double)ox + f[7]), ya = draw_sat((double)oy + f[8]);
    l.add(MODS_DRAW_DISC, cx, cy, 0, 0, r1 + 2, D_COLOUR1, 0);
    l.add(MODS_DRAW_DISC, xa, ya, 0, 0, r1 + 2, D_COLOUR1, 0);
    if (par->draw_epipolar_lines) {
      double k, b, k2, b2;
      draw_epipolar_kb(par->M, f[7], f[8], &k, &b);
      draw_epipolar_kb(Mt, f[0], f[1], &k2, &b2);
      draw_clipped_line(l, 0, draw_sat(b), w1, draw_sat(k * (double)w1 + b), 0, 0, w1, h1, D_COLOUR_EPI);
      draw_clipped_line(l, ox, draw_sat(b2) + oy, ox + w2, draw_sat(k2 * (double)w2 + b2) + oy, ox, oy, w2, h2, D_COLOUR_EPI);
    }
    l.add(MODS_DRAW_LINE, xa, ya, cx, cy, 0, D_COLOUR2, 0);
  }
}

}  // namespace mods

using namespace mods;

extern "C" {

int mods_canvas_create(mods_ctx *c, int w, int h, mods_canvas **out) {
  if (!c || !out) { set_error("canvas_create: null argument"); return MODS_E_ARG; }
  if (w < 1 || h < 1 || w > D_CANVAS_MAX || h > D_CANVAS_MAX) { set_error("canvas_create: %d x %d (1 .. %d)", w, h, D_CANVAS_MAX); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(c->device));
  mods_canvas *cv = new mods_canvas;
  cv->ctx = c; cv->w = w; cv->h = h;
  const hipError_t e = cv->px.reserve((size_t)w * (size_t)h * 3);
  if (e != hipSuccess) { delete cv; set_error("canvas_create: %s", hipGetErrorString(e)); return MODS_E_HIP; }
  *out = cv;
  return MODS_OK;
}

void mods_canvas_destroy(mods_canvas *cv) {
  if (!cv) return;
  (void)hipSetDevice(cv->ctx->device);
  (void)mods::stream_wait(cv->ctx->stream);
  delete cv;
}

int mods_canvas_width(const mods_canvas *cv) { return cv ? cv->w : 0; }
int mods_canvas_height(const mods_canvas *cv) { return cv ? cv->h : 0; }

int mods_canvas_fill(mods_canvas *cv, unsigned rgb) {
  if (!cv) { set_error("canvas_fill: null argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(cv->ctx->device));
  const size_t n = (size_t)cv->w * (size_t)cv->h;
  hipLaunchKernelGGL(draw_fill_kernel, dim3((unsigned)((n + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, cv->ctx->stream, cv->px.get(), n, rgb);
  MODS_HIP_CHECK(hipGetLastError());
  return MODS_OK;
}

int mods_canvas_blit_u8(mods_canvas *cv, const unsigned char *img, int w, int h, int channels, int x0, int y0) {
  if (!cv || !img) { set_error("canvas_blit_u8: null argument"); return MODS_E_ARG; }
  if (w < 1 || h < 1 || w > D_CANVAS_MAX || h > D_CANVAS_MAX || (channels != 1 && channels != 3)) {
    set_error("canvas_blit_u8: %d x %d, %d channels", w, h, channels);
    return MODS_E_ARG;
  }
  if (!draw_in_range(x0) || !draw_in_range(y0)) { set_error("canvas_blit_u8: offset (%d, %d)", x0, y0); return MODS_E_ARG; }
  mods_ctx *c = cv->ctx;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  const size_t bytes = (size_t)w * (size_t)h * (size_t)channels;
  MODS_HIP_CHECK(mods::reserve_scratch(c, cv->stage, bytes, bytes));
  MODS_HIP_CHECK(mods::copy_wait(c->stream, cv->stage.get(), img, bytes, hipMemcpyHostToDevice));
  return draw_blit(cv, channels, cv->stage.get(), w, h, (size_t)w * (size_t)channels, x0, y0);
}

int mods_canvas_blit_f32_dev(mods_canvas *cv, const float *img_dev, int w, int h, int stride, int x0, int y0) {
  if (!cv || !img_dev) { set_error("canvas_blit_f32_dev: null argument"); return MODS_E_ARG; }
  if (w < 1 || h < 1 || w > D_CANVAS_MAX || h > D_CANVAS_MAX || stride < w) { set_error("canvas_blit_f32_dev: %d x %d, stride %d", w, h, stride); return MODS_E_ARG; }
  if (!draw_in_range(x0) || !draw_in_range(y0)) { set_error("canvas_blit_f32_dev: offset (%d, %d)", x0, y0); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(cv->ctx->device));
  return draw_blit(cv, 4, img_dev, w, h, (size_t)stride, x0, y0);
}

int mods_canvas_blit_canvas(mods_canvas *cv, const mods_canvas *src, int x0, int y0) {
  if (!cv || !src || cv == src) { set_error("canvas_blit_canvas: null argument or the canvas itself"); return MODS_E_ARG; }
  if (cv->ctx != src->ctx) { set_error("canvas_blit_canvas: canvases of two contexts"); return MODS_E_ARG; }
  if (!draw_in_range(x0) || !draw_in_range(y0)) { set_error("canvas_blit_canvas: offset (%d, %d)", x0, y0); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(cv->ctx->device));
  return draw_blit(cv, 3, src->px.get(), src->w, src->h, (size_t)src->w * 3, x0, y0);
}

int mods_canvas_fetch(mods_canvas *cv, unsigned char *rgb_out) {
  if (!cv || !rgb_out) { set_error("canvas_fetch: null argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(cv->ctx->device));
  MODS_HIP_CHECK(mods::copy_wait(cv->ctx->stream, rgb_out, cv->px.get(), (size_t)cv->w * (size_t)cv->h * 3, hipMemcpyDeviceToHost));
  return MODS_OK;
}

int mods_canvas_draw(mods_canvas *cv, const mods_draw_elem *elems, int n, int *n_dropped) {
  if (!cv || !n_dropped || n < 0 || (n > 0 && !elems)) { set_error("canvas_draw: null argument"); return MODS_E_ARG; }
  *n_dropped = 0;
  if (n == 0) return MODS_OK;
  std::vector<mods_draw_elem> v(elems, elems + n);
  const int rc = draw_validate(v, n_dropped);
  if (rc) return rc;
  mods_ctx *c = cv->ctx;
  MODS_HIP_CHECK(hipSetDevice(c->device));
  MODS_HIP_CHECK(mods::reserve_scratch(c, cv->elems, (size_t)n, (size_t)n + (size_t)n / 4));
  MODS_HIP_CHECK(mods::copy_wait(c->stream, cv->elems.get(), v.data(), sizeof(mods_draw_elem) * (size_t)n, hipMemcpyHostToDevice));
  return draw_launch_tiles(cv, cv->elems.get(), n);
}

int mods_canvas_draw_regions(mods_canvas *cv, const mods_imgrep *rep, int begin, int count, int dx, int dy, int thickness, unsigned rgb, int table,
                             int *n_dropped) {
  int rc = draw_build_contours(cv, rep, begin, count, dx, dy, thickness, rgb, table, n_dropped);
  if (rc || count == 0) return rc;
  if ((rc = draw_launch_tiles(cv, cv->elems.get(), D_SEGS * count))) return rc;
  MODS_HIP_CHECK(mods::copy_wait(cv->ctx->stream, n_dropped, cv->dropped_dev.get(), sizeof(int), hipMemcpyDeviceToHost));
  return MODS_OK;
}

int mods_canvas_regions_elems(mods_canvas *cv, const mods_imgrep *rep, int begin, int count, int dx, int dy, int thickness, unsigned rgb, int table,
                              mods_draw_elem *out, int *n_dropped) {
  if (!out && count > 0) { set_error("canvas_regions_elems: null argument"); return MODS_E_ARG; }
  const int rc = draw_build_contours(cv, rep, begin, count, dx, dy, thickness, rgb, table, n_dropped);
  if (rc || count == 0) return rc;
  MODS_HIP_CHECK(mods::copy_wait(cv->ctx->stream, out, cv->elems.get(), sizeof(mods_draw_elem) * (size_t)D_SEGS * (size_t)count, hipMemcpyDeviceToHost));
  MODS_HIP_CHECK(mods::copy_wait(cv->ctx->stream, n_dropped, cv->dropped_dev.get(), sizeof(int), hipMemcpyDeviceToHost));
  return MODS_OK;
}

int mods_draw_matches_elems(int which, int w1, int h1, int w2, int h2, const double *laf14, int n, const mods_draw_matches_params *par,
                            mods_draw_elem *out, int max_out, int *n_out) {
  if (!n_out || max_out < 0 || (max_out > 0 && !out)) { set_error("draw_matches_elems: null argument"); return MODS_E_ARG; }
  if ((which != 0 && which != 1) || w1 < 1 || h1 < 1 || w2 < 1 || h2 < 1 || w1 > D_CANVAS_MAX || h1 > D_CANVAS_MAX || w2 > D_CANVAS_MAX || h2 > D_CANVAS_MAX) {
    set_error("draw_matches_elems: image %d, %d x %d, %d x %d", which, w1, h1, w2, h2);
    return MODS_E_ARG;
  }
  double Hinv[9];
  const int rc = draw_matches_check(laf14, n, par, Hinv);
  if (rc) return rc;
  DrawList l;
  draw_matches_list(which, w1, h1, w2, h2, laf14, n, par, Hinv, l);
  *n_out = (int)l.v.size();
  if (*n_out > max_out) { set_error("draw_matches_elems: output overflow: %d > %d", *n_out, max_out); return MODS_E_CAPACITY; }
  if (*n_out) memcpy(out, l.v.data(), sizeof(mods_draw_elem) * l.v.size());
  return MODS_OK;
}

int mods_draw_matches(mods_ctx *c, const mods_canvas *src1, const mods_canvas *src2, const double *laf14, int n,
                      const mods_draw_matches_params *par, mods_canvas **out1, mods_canvas **out2, int *n_dropped2) {
  if (!c || !src1 || !src2 || !out1 || !out2 || !n_dropped2) { set_error("draw_matches: null argument"); return MODS_E_ARG; }
  if (src1->ctx != c || src2->ctx != c) { set_error("draw_matches: a source canvas of another context"); return MODS_E_ARG; }
  double Hinv[9];
  int rc = draw_matches_check(laf14, n, par, Hinv);
  if (rc) return rc;
  const int w1 = src1->w, h1 = src1->h, w2 = src2->w, h2 = src2->h;
  const bool one = par->reproject_to_one_image != 0;
  const int ow[2] = {one ? w1 : w1 + w2 + D_SEP, one ? w2 : std::max(w1, w2)};
  const int oh[2] = {one ? h1 : std::max(h1, h2), one ? h2 : h1 + h2 + D_SEP};
  if (ow[0] > D_CANVAS_MAX || oh[1] > D_CANVAS_MAX) { set_error("draw_matches: composed image %d x %d / %d x %d (at most %d)", ow[0], oh[0], ow[1], oh[1], D_CANVAS_MAX); return MODS_E_ARG; }
  mods_canvas *o[2] = {nullptr, nullptr};
  for (int i = 0; i < 2 && !rc; i++) {
    rc = mods_canvas_create(c, ow[i], oh[i], &o[i]);
    if (rc) break;
    if (one) rc = mods_canvas_blit_canvas(o[i], i == 0 ? src1 : src2, 0, 0);
    else {
      rc = mods_canvas_fill(o[i], 0xffffffu);
      if (!rc) rc = mods_canvas_blit_canvas(o[i], src1, 0, 0);
      if (!rc) rc = mods_canvas_blit_canvas(o[i], src2, i == 0 ? w1 + D_SEP : 0, i == 0 ? 0 : h1 + D_SEP);
    }
    if (rc) break;
    DrawList l;
    draw_matches_list(i, w1, h1, w2, h2, laf14, n, par, Hinv, l);
    rc = mods_canvas_draw(o[i], l.v.data(), (int)l.v.size(), &n_dropped2[i]);
  }
  if (rc) { mods_canvas_destroy(o[0]); mods_canvas_destroy(o[1]); return rc; }
  *out1 = o[0]; *out2 = o[1];
  return MODS_OK;
}

int mods_ctx_verified_lafs(mods_ctx *c, double *laf14, int max, int *n) {
  if (!c || !n || max < 0 || (max > 0 && !laf14)) { set_error("ctx_verified_lafs: null argument"); return MODS_E_ARG; }
  const int have = (int)std::min((size_t)std::max(c->h_verified, 0), c->h_list.size());
  *n = have;
  const int m = std::min(have, max);
  if (m > 0) memcpy(laf14, c->h_list.laf.data(), sizeof(double) * 14 * (size_t)m);
  return MODS_OK;
}

}  // extern "C"
