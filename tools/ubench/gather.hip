// micro-benchmark: cost of an 8-byte gather per wave instruction and CU as a function of how the 64 lanes' addresses fall
// into cache lines.  The image (8 MB) stays L2 / MALL resident.  pattern: lane l of wave-instruction i reads pixel
//   base(wave, i) + f(l):  0: l * 1 px (coalesced)  1: l * 2 px  2: (l & 3) * 1 + (l >> 2) * 64 px (quads share a line)
//   3: l * 64 px (every lane its own line, one row)  4: l * 1920 px (every lane its own row)  5: (l&7)*1 + (l>>3)*1920 (8 x 8 block)
//   6: the 8 x 8 block of 5, but the 8 loads of an iteration walk 8 px to the right each (the same rows: L1 reuse, as a row of tiles does)
// 8-bit section (2-byte pair loads, as pix_pair of an 8-bit image issues them): the same 8 x 8 block of samples in a 1920 x 1080
// 8-bit image laid out row-major, in 16-byte column strips (15 columns + the first of the next strip, rows consecutive: a 128-byte
// line is 8 rows of a strip) and in 32-byte strips (31 + 1 columns, 4 rows per line).  The block's origin is one per wave and
// instruction (scalar), random, or placed so that the block does / does not cross a strip seam or a line boundary of the strips;
// "walk" = pattern 6's eight loads that step 8 px to the right.  Beside each time: the distinct 128-byte lines the 64 lanes touch.
#include <hip/hip_runtime.h>
#include <cstdio>
struct __attribute__((packed, aligned(4))) PixPair { float a, b; };
template <int PAT>
__global__ __launch_bounds__(256) void k(const float *img, float *out, int iters, int npx) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * 4 + (threadIdx.x >> 6));
  int off;
  if (PAT == 0) off = lane; else if (PAT == 1) off = lane * 2; else if (PAT == 2) off = (lane & 3) + (lane >> 2) * 64;
  else if (PAT == 3) off = lane * 64; else if (PAT == 4) off = lane * 1920; else off = (lane & 7) + (lane >> 3) * 1920;
  unsigned walk = 0;
  float acc = 0;
  unsigned base = (unsigned)gw * 7919u;
  for (int it = 0; it < iters; it++) {
    PixPair v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      if (PAT != 6 || q == 0) { base = base * 1664525u + 1013904223u; walk = 0; } else walk += 8;
      const unsigned p = ((base >> 8) % (unsigned)(npx - 64 * 1920 - 80)) + off + walk;
      v[q] = *(const PixPair *)(img + p);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) acc += v[q].a + v[q].b;
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc;
}
// layouts of the 8-bit section: 0 row-major, 1 16-byte strips, 2 32-byte strips
constexpr int kW = 1920, kH = 1080;
template <int LAY> __host__ __device__ inline unsigned u8_offset(unsigned x, unsigned y) {
  if (LAY == 0) return y * kW + x;
  if (LAY == 1) { const unsigned s = (x * 0x8889u) >> 19; return s * (16u * kH) + 16u * y + (x - 15u * s); }       // x / 15, exact below 74 909
  const unsigned s = (x * 0x10843u) >> 21; return s * (32u * kH) + 32u * y + (x - 31u * s);                         // x / 31, exact below 2 332
}
template <int LAY> constexpr unsigned u8_bytes() {
  return LAY == 0 ? kW * kH : LAY == 1 ? ((kW - 1 + 14) / 15) * 16u * kH : ((kW - 1 + 30) / 31) * 32u * kH;
}
// origin of the 8 x 8 block from a random word.  ORG 0: anywhere; 1: inside one strip and one line run (32-byte strips: two 4-row
// lines, the fewest an 8-row block can have); 2: across a strip seam; 3: across a line boundary; 4: both
template <int LAY, int ORG> __host__ __device__ inline void u8_origin(unsigned r, unsigned &ox, unsigned &oy) {
  constexpr unsigned SW = LAY == 2 ? 31 : 15, LR = LAY == 2 ? 4 : 8;
  const unsigned a = (r >> 8) & 0xfff, b = (r >> 20) & 0xfff;
  if (ORG == 0) { ox = (a * (kW - 1 - 64 - 8)) >> 12; oy = (b * (kH - 1 - 8)) >> 12; return; }
  ox = ((a * ((kW - 64 - 8) / SW - 1)) >> 12) * SW + ((ORG == 2 || ORG == 4) ? SW - 4 : 0);
  oy = ((b * ((kH - 8) / LR - 1)) >> 12) * LR + ((ORG == 3 || ORG == 4) ? LR / 2 : 0);
}
struct __attribute__((packed, aligned(1))) PixPairU8 { unsigned char a, b; };
template <int LAY, int ORG, bool WALK>
__global__ __launch_bounds__(256) void k8(const unsigned char *img, float *out, int iters) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  float acc = 0;
  unsigned base = gw * 7919u, ox = 0, oy = 0;
  for (int it = 0; it < iters; it++) {
    PixPairU8 v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      if (!WALK || q == 0) { base = base * 1664525u + 1013904223u; u8_origin<LAY, ORG>(base, ox, oy); } else ox += 8;
      v[q] = *(const PixPairU8 *)(img + u8_offset<LAY>(ox + (lane & 7), oy + (lane >> 3)));
    }
#pragma unroll
    for (int q = 0; q < 8; q++) acc += (float)v[q].a + (float)v[q].b;
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc;
}
// host: mean number of distinct 128-byte lines per wave-load, and the largest offset (+ 1 for the pair's second byte) against the buffer
template <int LAY, int ORG, bool WALK> static double u8_lines(bool &inside) {
  unsigned base = 7919u, ox = 0, oy = 0; double sum = 0; int n = 0; inside = true;
  for (int it = 0; it < 2000; it++)
    for (int q = 0; q < 8; q++) {
      if (!WALK || q == 0) { base = base * 1664525u + 1013904223u; u8_origin<LAY, ORG>(base, ox, oy); } else ox += 8;
      unsigned lines[64]; int nl = 0;
      for (unsigned l = 0; l < 64; l++) {
        const unsigned x = ox + (l & 7), y = oy + (l >> 3), o = u8_offset<LAY>(x, y);
        if (x > kW - 2 || y > kH - 2 || o + 1 >= u8_bytes<LAY>()) inside = false;
        for (unsigned e = o; e <= o + 1; e++) { int j = 0; while (j < nl && lines[j] != e / 128) j++; if (j == nl) lines[nl++] = e / 128; }
      }
      sum += nl; n++;
    }
  return sum / n;
}
template <int LAY, int ORG, bool WALK> static int run8(const char *name, const unsigned char *img, float *out, int iters) {
  bool inside; const double lines = u8_lines<LAY, ORG, WALK>(inside);
  if (!inside) { printf("%s: offsets leave the buffer, not run\n", name); return 1; }
  for (int bpc : {2, 4}) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int grid = 256 * bpc;
    hipLaunchKernelGGL((k8<LAY, ORG, WALK>), dim3(grid), dim3(256), 0, 0, img, out, iters); 
    if (hipDeviceSynchronize() != hipSuccess) { printf("%s: kernel failed\n", name); return 1; }
    hipEventRecord(e0); hipLaunchKernelGGL((k8<LAY, ORG, WALK>), dim3(grid), dim3(256), 0, 0, img, out, iters); hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: kernel failed\n", name); return 1; }
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double ops_per_cu = (double)iters * 8 * 4 * bpc;
    printf("u8 %-44s %4.1f lines  %2d waves/CU: %.3f ms, %.1f ns = %.0f cycles (2.1 GHz) per wave-load per CU\n", name, lines, 4 * bpc, ms,
           ms * 1e6 / ops_per_cu, ms * 1e6 / ops_per_cu * 2.1);
  }
  return 0;
}
int main() {
  const int npx = 1920 * 1080;
  float *img, *out;
  hipMalloc(&img, npx * 4); hipMalloc(&out, 4 * 256 * 4096); hipMemset(img, 0, npx * 4);
  const int iters = 400;
  for (int pat = 0; pat < 7; pat++)
    for (int bpc : {2, 4}) {
      hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
      const int grid = 256 * bpc;
      auto launch = [&] {
        switch (pat) {
          case 0: hipLaunchKernelGGL(k<0>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
          case 1: hipLaunchKernelGGL(k<1>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
          case 2: hipLaunchKernelGGL(k<2>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
          case 3: hipLaunchKernelGGL(k<3>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
          case 4: hipLaunchKernelGGL(k<4>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
          case 5: hipLaunchKernelGGL(k<5>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
          default: hipLaunchKernelGGL(k<6>, dim3(grid), dim3(256), 0, 0, img, out, iters, npx); break;
        }
      };
      launch(); hipDeviceSynchronize();
      hipEventRecord(e0); launch(); hipEventRecord(e1); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1);
      const double ops_per_cu = (double)iters * 8 * 4 * bpc;
      printf("pattern %d  %2d waves/CU: %.3f ms, %.1f ns = %.0f cycles (2.1 GHz) per wave-load per CU\n", pat, 4 * bpc, ms, ms * 1e6 / ops_per_cu, ms * 1e6 / ops_per_cu * 2.1);
    }
  for (unsigned x = 0; x < 74909; x++) if (((x * 0x8889u) >> 19) != x / 15) { printf("x / 15 multiply-shift wrong at %u\n", x); return 1; }
  for (unsigned x = 0; x < 2332; x++) if (((x * 0x10843u) >> 21) != x / 31) { printf("x / 31 multiply-shift wrong at %u\n", x); return 1; }
  unsigned char *img8;
  const size_t nb = u8_bytes<1>() > u8_bytes<2>() ? u8_bytes<1>() : u8_bytes<2>();     // (both above the row-major size)
  hipMalloc(&img8, nb); hipMemset(img8, 0, nb);
  int bad = 0;
  bad |= run8<0, 0, false>("row-major, random origin", img8, out, iters);
  bad |= run8<1, 0, false>("16-byte strips, random origin", img8, out, iters);
  bad |= run8<1, 1, false>("16-byte strips, one strip, one line", img8, out, iters);
  bad |= run8<1, 2, false>("16-byte strips, across a seam", img8, out, iters);
  bad |= run8<1, 3, false>("16-byte strips, across a line boundary", img8, out, iters);
  bad |= run8<1, 4, false>("16-byte strips, across both", img8, out, iters);
  bad |= run8<2, 0, false>("32-byte strips, random origin", img8, out, iters);
  bad |= run8<2, 1, false>("32-byte strips, one strip, two lines", img8, out, iters);
  bad |= run8<2, 2, false>("32-byte strips, across a seam", img8, out, iters);
  bad |= run8<2, 3, false>("32-byte strips, across a line boundary", img8, out, iters);
  bad |= run8<2, 4, false>("32-byte strips, across both", img8, out, iters);
  bad |= run8<0, 0, true>("row-major, walk to the right", img8, out, iters);
  bad |= run8<1, 0, true>("16-byte strips, walk to the right", img8, out, iters);
  bad |= run8<2, 0, true>("32-byte strips, walk to the right", img8, out, iters);
  return bad;
}
