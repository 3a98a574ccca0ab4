// The bf16 matrix-core mode of AffNet, OriNet and HardNet (MODS_NET_BF16, include/mods_hip.h "bf16 mode"): stages 2..6 (the convolution
// blocks behind the first; stage 0 is the normalisation, 1..6 the six blocks, 7 the head, as in mods_test_net_stage) as implicit
// GEMMs and HardNet's 8 x 8 head as a GEMM on v_mfma_f32_16x16x32_bf16, stage 1 and the small
// heads with the fp32 mode's arithmetic on bf16 activations.  One launch per layer, as in nets.hip.
//
// Activations are bf16, channels last: [n][h][w][c].  A convolution is D[cout][pixel] = sum_k W[cout][k] X[k][pixel] with
// k = tap * cin + input channel: the weights are the A operand (a lane holds 8 consecutive k of one output channel), the
// activations the B operand (8 consecutive channels of one tap of one pixel: 16 bytes of the zero-padded input map in LDS), and a
// lane of the result holds 4 consecutive output channels of one pixel: one 8-byte store, channels last again.  K is padded to the
// instruction's 32 with zero weights (9 x 16 = 144 -> 160); the activations read there are those of tap 0 (finite), their
// products are zeros.  The weights lie in memory in the order the lanes hold them ([cout / 16][k-step][lane][8],
// mfma_w_index): a wave's load of a fragment reads 1 KB of consecutive bytes.  (Row-major [cout][k] made every such load touch 16
// rows, and the layers ran at the L1's rate of tag lookups: 6000 HardNet patches took 2.9 ms instead of 1.9, measured while this was written.)
//
//   net_conv3_mfma_kernel   a workgroup = the output map of one patch (32 x 32, 16 x 16) or the 8 x 8 maps of two patches, and
//                           ALL output channels: its input map with every input channel goes to LDS once (26 to 92 KB), a
//                           wave takes a quarter of the pixels (MT tiles of 16) times all NT = cout / 16 channel tiles.  Per
//                           k-step a lane reads NT weight fragments from global memory (L2: every workgroup reads the same
//                           bytes) and MT activation fragments from LDS for MT x NT MFMAs.  The weight fragments of KG k-steps
//                           share a register set; three sets, so two groups are on their way while one is multiplied, and
//                           the first three are requested before the tile is filled (layers of up to three groups: all).
//   net_head_hard_mfma_kernel  16 patches x 128 outputs x K = 8192; the four waves take a quarter of K each (both operands straight
//                           from global memory, three register sets of two k-steps) and are added in the fixed order
//                           ((w0 + w1) + w2) + w3 through LDS; the tail (bias, L2 norm, quantisation) is the fp32 head's.
//
// Co-residency (match.hip, DESIGN.md "Matrix-core kernels own their SIMDs"): both MFMA kernels run as one workgroup of four waves
// per CU, each wave the owner of its SIMD's 512 registers, no scratch.  With one wave per SIMD nothing else hides a latency, hence
// the register prefetch of the weights and the single LDS fill per workgroup.
// The order of every sum is fixed by the tiling: k ascending inside the matrix unit's step, k-steps ascending, (head) the four
// K quarters in wave order.  No patch's arithmetic reads another patch's data; padded rows and patches are zeros or copies that
// are never written back.
#include "common.hpp"
#include "nets_mfma.hpp"

namespace mods {
namespace {

typedef __bf16 bfx8 __attribute__((ext_vector_type(8)));
typedef float fx4 __attribute__((ext_vector_type(4)));
typedef int ix4 __attribute__((ext_vector_type(4)));

// the whole register file of the wave's SIMD (the co-residency rule, match.hip): the workgroup is four waves of 512 registers
__device__ __forceinline__ void nets_own_simd() { asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a255, 0" ::: "v255", "a255"); }

// fp32 -> nearest bf16, ties to even (finite input), as 16 bits
__device__ __forceinline__ unsigned bf16_bits(float x) {
  unsigned u = __float_as_uint(x);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ float bf16_widen(bf16_t h) { return __uint_as_float((unsigned)h << 16); }

__device__ __forceinline__ fx4 mfma_bf16(const ix4 &a, const ix4 &b, const fx4 &c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfx8, a), __builtin_bit_cast(bfx8, b), c, 0, 0, 0);
}

__device__ inline float wave_sum(float v) {
  // xor butterfly: both partners add the same two numbers, so all 64 lanes end with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// k-steps per register set of weight fragments: the largest divisor of the layer's k-steps that keeps a set within 24 fragments
// (three sets: 288 registers beside at most 128 accumulators), 16 at eight channel tiles: load destinations live in the 256
// architectural registers, and with 24 the stride-2 block of HardNet spilled to scratch, which the co-residency rule forbids
constexpr int pick_group(int ks, int nt) {
  int g = 1;
  for (int d = 1; d <= ks; d++)
    if (ks % d == 0 && d * nt <= (nt >= 8 ? 16 : 24)) g = d;
  return g;
}

template <int CIN, int COUT, int HIN, int STRIDE>
struct ConvGeom {
  static constexpr int HOUT = HIN / STRIDE, PIX = HOUT * HOUT;
  static constexpr int TP = PIX;                                   // pixels of one patch in a workgroup: the whole map
  static constexpr int PPB = PIX == 64 ? kMfmaPatches8 : 1;        // patches per workgroup
  static constexpr int IR = (HOUT - 1) * STRIDE + 3, IW = HIN + 2; // rows and columns of the zero-padded input map in LDS
  static constexpr int CS = CIN + 8;                               // elements between two pixels in LDS: 16 bytes of padding spread the banks
  static constexpr int UPP = CIN / 8;                              // 16-byte units of a pixel
  static constexpr int NU = PPB * IR * IW * UPP;                   // ... of the tile
  static constexpr int MT = TP * PPB / 64;                         // 16-pixel tiles of a wave
  static constexpr int NT = COUT / 16;                             // 16-channel tiles (every wave has all)
  static constexpr int KP = (9 * CIN + 31) / 32 * 32, KS = KP / 32;
  static constexpr int KG = pick_group(KS, NT), NG = KS / KG;      // k-steps whose weight fragments share a register set; sets of the layer
  static constexpr int LDS_BYTES = PPB * IR * IW * CS * 2;
  static_assert(CIN % 8 == 0 && COUT % 16 == 0 && (TP * PPB) % 64 == 0 && LDS_BYTES <= 160 * 1024, "tiling");
};

// stage 1: conv3x3(1 -> C) + folded BatchNorm + ReLU with the arithmetic of net_conv3_kernel<1, C, 32, 1> (nets.hip: one fmaf
// chain over the taps 0..8 from 0, then + bias, then the ReLU), stored as bf16 [n][32][32][C].  A block = 8 rows of one patch.
template <int C>
__global__ __launch_bounds__(256) void net_conv1_bf16_kernel(const float *__restrict__ in, bf16_t *__restrict__ out, const float *__restrict__ wt,
                                                             const float *__restrict__ bias, int n) {
  __shared__ float tile[10 * 34];
  const int t = threadIdx.x, patch = blockIdx.x >> 2, band = blockIdx.x & 3;
  if (patch >= n) return;
  for (int e = t; e < 10 * 34; e += 256) {
    const int gy = band * 8 - 1 + e / 34, gx = e % 34 - 1;
    tile[e] = gy >= 0 && gy < 32 && gx >= 0 && gx < 32 ? in[(size_t)patch * 1024 + gy * 32 + gx] : 0.f;
  }
  __syncthreads();
  const int oy = t >> 5, ox = t & 31;
  float v[9];
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] = tile[(oy + k / 3) * 34 + ox + k % 3];
  bf16_t *o = out + ((size_t)patch * 1024 + band * 256 + t) * C;
#pragma unroll
  for (int cg = 0; cg < C / 16; cg++) {
    const float *wc = wt + cg * 9 * 16;                              // wave-uniform: scalar loads
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; k++)
#pragma unroll
      for (int j = 0; j < 16; j++) acc[j] = fmaf(v[k], wc[k * 16 + j], acc[j]);
    unsigned pk[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
      pk[j] = bf16_bits(fmaxf(acc[2 * j] + bias[cg * 16 + 2 * j], 0.f)) | (bf16_bits(fmaxf(acc[2 * j + 1] + bias[cg * 16 + 2 * j + 1], 0.f)) << 16);
    uint4 *o4 = (uint4 *)(o + cg * 16);
    o4[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    o4[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
  }
}

// stages 2..6: conv3x3 (pad 1, stride STRIDE) + folded BatchNorm + ReLU, bf16 [n][HIN][HIN][CIN] -> bf16 [n][HOUT][HOUT][COUT].
// grid = ceil(n / PPB) workgroups of 256 threads, dynamic LDS = ConvGeom::LDS_BYTES.
template <int CIN, int COUT, int HIN, int STRIDE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void net_conv3_mfma_kernel(
    const bf16_t *__restrict__ in, bf16_t *__restrict__ out, const bf16_t *__restrict__ wt, const float *__restrict__ bias, int n) {
  typedef ConvGeom<CIN, COUT, HIN, STRIDE> G;
  constexpr int MT = G::MT, NT = G::NT, IW = G::IW, IR = G::IR, CS = G::CS, KG = G::KG, NG = G::NG;
  extern __shared__ __attribute__((aligned(16))) char s_tile[];
  nets_own_simd();
  const int t = threadIdx.x, lane = t & 63, g = lane >> 4, r16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int pg = blockIdx.x;                                         // the workgroup's group of PPB patches
  // the weight fragments of k-step ks (rows nt * 16 + r16, elements ks * 32 + 8 g .. + 7) are stored in the order the lanes hold
  // them (mfma_w_index): a load instruction of the wave reads 1 KB of consecutive bytes
  constexpr int KS = G::KS;
  const bf16_t *wl = wt + lane * 8;
  auto load_a = [&](int gi, ix4 (&a)[KG][NT]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < KG; j++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++) a[j][nt] = *(const ix4 *)(wl + ((size_t)nt * KS + gi * KG + j) * 512);
  };
  // three register sets of KG k-steps each: the first three groups are requested before the tile is filled
  ix4 s0[KG][NT], s1[KG][NT], s2[KG][NT];
  load_a(0, s0);
  if (NG > 1) load_a(1, s1);
  if (NG > 2) load_a(2, s2);
  // the input maps of the workgroup's patches, every channel, zero padded
  {
    constexpr int ST = 8;
    for (int e0 = t; e0 < G::NU; e0 += 256 * ST) {
      ix4 v[ST];
#pragma unroll
      for (int i = 0; i < ST; i++) {
        const int e = e0 + i * 256;
        const int c8 = e % G::UPP, x = (e / G::UPP) % IW, r = (e / (G::UPP * IW)) % IR, p = e / (G::UPP * IW * IR);
        const int gy = r - 1, gx = x - 1, gp = pg * G::PPB + p;
        v[i] = ix4{0, 0, 0, 0};
        if (e < G::NU && gy >= 0 && gy < HIN && gx >= 0 && gx < HIN && gp < n)
          v[i] = *(const ix4 *)(in + (((size_t)gp * HIN + gy) * HIN + gx) * CIN + c8 * 8);
      }
#pragma unroll
      for (int i = 0; i < ST; i++) {
        const int e = e0 + i * 256;
        if (e < G::NU) *(ix4 *)(s_tile + ((size_t)(e / G::UPP) * CS + (e % G::UPP) * 8) * 2) = v[i];
      }
    }
  }
  // the lane's pixel of tile m: workgroup pixel q = (w MT + m) 16 + r16 -> (patch of the workgroup, row, column)
  int base[MT];
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int q = (w * MT + m) * 16 + r16, pl = q / G::TP, pix = q % G::TP;
    base[m] = (((pl * IR + (pix / G::HOUT) * STRIDE) * IW + (pix % G::HOUT) * STRIDE) * CS + 8 * g) * 2;
  }
  fx4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[m][nt] = fx4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  // group gi = k-steps gi KG .. + KG - 1 from the set `cur`; in step ks the lane's 8 k are channels ci .. ci + 7 of tap `tap`.  The
  // set is then refilled with group gi + 3: two groups are always on their way while one is multiplied.
  auto step = [&](int gi, ix4 (&cur)[KG][NT]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < KG; j++) {
      const int k0 = (gi * KG + j) * 32 + 8 * g;
      int tap = k0 / CIN;
      const int ci = k0 % CIN - 8 * g;                              // (8 g is in base[])
      if (9 * CIN % 32 != 0) tap = tap < 9 ? tap : 0;                // the padded k: zero weights
      const int off = (((tap / 3) * IW + tap % 3) * CS + ci) * 2;
      ix4 b[MT];
#pragma unroll
      for (int m = 0; m < MT; m++) b[m] = *(const ix4 *)(s_tile + base[m] + off);
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[m][nt] = mfma_bf16(cur[j][nt], b[m], acc[m][nt]);
    }
    if (gi + 3 < NG) load_a(gi + 3, cur);
  };
  int gi = 0;
#pragma unroll 1
  for (; gi + 2 < NG; gi += 3) {
    step(gi, s0);
    step(gi + 1, s1);
    step(gi + 2, s2);
  }
  if (gi < NG) step(gi, s0);
  if (gi + 1 < NG) step(gi + 1, s1);
  // + bias, ReLU, bf16: the lane has channels nt * 16 + 4 g .. + 3 of its pixel
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int q = (w * MT + m) * 16 + r16, pl = q / G::TP, pix = q % G::TP;
    const int patch = pg * G::PPB + pl;
    if (patch >= n) continue;
    bf16_t *o = out + ((size_t)patch * G::PIX + pix) * COUT + 4 * g;
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      const float4 bv = *(const float4 *)(bias + nt * 16 + 4 * g);
      const fx4 c = acc[m][nt];
      uint2 pk;
      pk.x = bf16_bits(fmaxf(c[0] + bv.x, 0.f)) | (bf16_bits(fmaxf(c[1] + bv.y, 0.f)) << 16);
      pk.y = bf16_bits(fmaxf(c[2] + bv.z, 0.f)) | (bf16_bits(fmaxf(c[3] + bv.w, 0.f)) << 16);
      *(uint2 *)(o + nt * 16) = pk;
    }
  }
}

// AffNet head on [n][64 pixels][64 channels] bf16: net_head_aff_kernel's sums (a lane is a pixel and adds its channels in
// ascending order, then the butterfly), w [3][64 channels][64 pixels] fp32; one wave per patch
__global__ __launch_bounds__(256) void net_head_aff_bf16_kernel(const bf16_t *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                                                                float *__restrict__ out, int n) {
  const int lane = threadIdx.x & 63, patch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= n) return;
  const bf16_t *p = in + (size_t)patch * 4096 + lane * 64;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int i = 0; i < 64; i++) {
    const int k = i * 64 + lane;
    const float v = bf16_widen(p[i]);
    a0 = fmaf(v, w[k], a0); a1 = fmaf(v, w[4096 + k], a1); a2 = fmaf(v, w[8192 + k], a2);
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
  if (lane == 0) {
    out[(size_t)patch * 3 + 0] = tanhf(a0 + bias[0]) + 1.f;
    out[(size_t)patch * 3 + 1] = tanhf(a1 + bias[1]);
    out[(size_t)patch * 3 + 2] = tanhf(a2 + bias[2]) + 1.f;
  }
}

// OriNet head on bf16 [n][64 pixels][64 channels]: net_head_ori_kernel's sums, w [2][64][8][8] fp32; one wave per patch
__global__ __launch_bounds__(256) void net_head_ori_bf16_kernel(const bf16_t *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                                                                float *__restrict__ out, int n) {
  const int lane = threadIdx.x & 63, patch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= n) return;
  const int y = lane >> 3, x = lane & 7;
  int off[9];
  bool ok[9];
#pragma unroll
  for (int q = 0; q < 9; q++) {
    const int ky = y - q / 3 + 1, kx = x - q % 3 + 1;       // input (y, x) = output (py, px) + (ky, kx) - 1
    ok[q] = ky >= 0 && ky < 8 && kx >= 0 && kx < 8;
    off[q] = ok[q] ? ky * 8 + kx : 0;
  }
  float acc[18];
#pragma unroll
  for (int q = 0; q < 18; q++) acc[q] = 0.f;
  const bf16_t *p = in + (size_t)patch * 4096 + lane * 64;
  for (int c = 0; c < 64; c++) {
    const float v = bf16_widen(p[c]);
#pragma unroll
    for (int o = 0; o < 2; o++)
#pragma unroll
      for (int q = 0; q < 9; q++) {
        const float wv = ok[q] ? w[(o * 64 + c) * 64 + off[q]] : 0.f;
        acc[o * 9 + q] = fmaf(v, wv, acc[o * 9 + q]);
      }
  }
#pragma unroll
  for (int o = 0; o < 2; o++) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 9; q++) s += tanhf(wave_sum(acc[o * 9 + q]) + bias[o]);
    if (lane == 0) out[(size_t)patch * 2 + o] = s / 9.f;
  }
}

// HardNet head: in [n][8192] bf16 (k = pixel * 128 + channel) x wt [128][8192] bf16 (BatchNorm folded), + bias, L2 normalisation,
// the daemon's quantisation.  A workgroup = 16 patches (columns of the result; rows past n repeat patch n - 1 and are not written).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void net_head_hard_mfma_kernel(
    const bf16_t *__restrict__ in, const bf16_t *__restrict__ wt, const float *__restrict__ bias, float *__restrict__ out, int n) {
  constexpr int P = kMfmaHeadPatches, NT = 8, KQ = 2048, KS = KQ / 32, KG = 2, NG = KS / KG;
  static_assert(NG > 3, "three register sets of KG k-steps");
  static_assert(P == 16, "a column tile of the instruction");
  __shared__ float part[4][128][P + 1];
  __shared__ float norm2[P][2];
  nets_own_simd();
  const int t = threadIdx.x, lane = t & 63, g = lane >> 4, r16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int p0 = blockIdx.x * P;
  const bf16_t *bp = in + (size_t)min(p0 + r16, n - 1) * 8192 + w * KQ + 8 * g;
  const bf16_t *ap = wt + ((size_t)w * KS * 64 + lane) * 8;           // fragment order (mfma_w_index): 1 KB per load instruction
  struct Frag { ix4 a[KG][NT]; ix4 b[KG]; };
  auto load = [&](int gi, Frag &f) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < KG; j++) {
#pragma unroll
      for (int nt = 0; nt < NT; nt++) f.a[j][nt] = *(const ix4 *)(ap + ((size_t)nt * (8192 / 32) + gi * KG + j) * 512);
      f.b[j] = *(const ix4 *)(bp + (gi * KG + j) * 32);
    }
  };
  Frag s0, s1, s2;
  load(0, s0);
  load(1, s1);
  load(2, s2);
  fx4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) acc[nt] = fx4{0.f, 0.f, 0.f, 0.f};
  // a set of KG k-steps is multiplied, then refilled with the group three ahead
  auto step = [&](int gi, Frag &cur) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < KG; j++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++) acc[nt] = mfma_bf16(cur.a[j][nt], cur.b[j], acc[nt]);
    if (gi + 3 < NG) load(gi + 3, cur);
  };
  int gi = 0;
#pragma unroll 1
  for (; gi + 2 < NG; gi += 3) {
    step(gi, s0);
    step(gi + 1, s1);
    step(gi + 2, s2);
  }
  if (gi < NG) step(gi, s0);
  if (gi + 1 < NG) step(gi + 1, s1);
#pragma unroll
  for (int nt = 0; nt < NT; nt++)
#pragma unroll
    for (int r = 0; r < 4; r++) part[w][nt * 16 + 4 * g + r][r16] = acc[nt][r];
  __syncthreads();
  // thread = (half of the patches, output channel), as net_head_hard_kernel's tail
  const int c = t & 127, h = t >> 7;
  float y[P / 2];
#pragma unroll
  for (int p = 0; p < P / 2; p++) {
    const int pp = h * (P / 2) + p;
    y[p] = (((part[0][c][pp] + part[1][c][pp]) + part[2][c][pp]) + part[3][c][pp]) + bias[c];
    const float s = wave_sum(y[p] * y[p]);
    if (lane == 0) norm2[pp][c >> 6] = s;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < P / 2; p++) {
    const int pp = h * (P / 2) + p;
    if (p0 + pp >= n) break;
    const float d = y[p] / sqrtf((norm2[pp][0] + norm2[pp][1]) + 1e-10f);
    double q = 210.0 * ((double)d + 0.45);                  // desc_server.py:44, then the cast to 8 bits truncates
    q = q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q);
    out[(size_t)(p0 + pp) * 128 + c] = (float)(int)q;
  }
}

template <int CIN, int COUT, int HIN, int STRIDE>
hipError_t launch_conv3(hipStream_t s, int device, const bf16_t *in, bf16_t *out, const bf16_t *w, const float *b, int n) {
  typedef ConvGeom<CIN, COUT, HIN, STRIDE> G;
  static DynLdsOnce site;
  const hipError_t e = dyn_lds_once(site, (const void *)net_conv3_mfma_kernel<CIN, COUT, HIN, STRIDE>, G::LDS_BYTES, device);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((n + G::PPB - 1) / G::PPB);
  hipLaunchKernelGGL((net_conv3_mfma_kernel<CIN, COUT, HIN, STRIDE>), dim3(grid), dim3(256), G::LDS_BYTES, s, in, out, w, b, n);
  return hipSuccess;
}

template <int C>
hipError_t launch_block(hipStream_t s, int device, int l /* stage - 1 */, const bf16_t *in, bf16_t *out, const bf16_t *w, const float *b, int n) {
  switch (l) {
    case 1: return launch_conv3<C, C, 32, 1>(s, device, in, out, w, b, n);
    case 2: return launch_conv3<C, 2 * C, 32, 2>(s, device, in, out, w, b, n);
    case 3: return launch_conv3<2 * C, 2 * C, 16, 1>(s, device, in, out, w, b, n);
    case 4: return launch_conv3<2 * C, 4 * C, 16, 2>(s, device, in, out, w, b, n);
    case 5: return launch_conv3<4 * C, 4 * C, 8, 1>(s, device, in, out, w, b, n);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t mfma_launch_conv1(hipStream_t s, int device, int C, const float *in, bf16_t *out, const float *w, const float *bias, int n) {
  (void)device;
  if (C == 16) hipLaunchKernelGGL(net_conv1_bf16_kernel<16>, dim3((unsigned)n * 4), dim3(256), 0, s, in, out, w, bias, n);
  else hipLaunchKernelGGL(net_conv1_bf16_kernel<32>, dim3((unsigned)n * 4), dim3(256), 0, s, in, out, w, bias, n);
  return hipSuccess;
}

hipError_t mfma_launch_conv3(hipStream_t s, int device, int C, int l, const bf16_t *in, bf16_t *out, const bf16_t *w, const float *bias, int n) {
  return C == 16 ? launch_block<16>(s, device, l, in, out, w, bias, n) : launch_block<32>(s, device, l, in, out, w, bias, n);
}

hipError_t mfma_launch_head_aff(hipStream_t s, const bf16_t *in, const float *w, const float *bias, float *out, int n) {
  hipLaunchKernelGGL(net_head_aff_bf16_kernel, dim3((n + 3) / 4), dim3(256), 0, s, in, w, bias, out, n);
  return hipSuccess;
}

hipError_t mfma_launch_head_ori(hipStream_t s, const bf16_t *in, const float *w, const float *bias, float *out, int n) {
  hipLaunchKernelGGL(net_head_ori_bf16_kernel, dim3((n + 3) / 4), dim3(256), 0, s, in, w, bias, out, n);
  return hipSuccess;
}

hipError_t mfma_launch_head_hard(hipStream_t s, const bf16_t *in, const bf16_t *w, const float *bias, float *out, int n) {
  hipLaunchKernelGGL(net_head_hard_mfma_kernel, dim3((n + kMfmaHeadPatches - 1) / kMfmaHeadPatches), dim3(256), 0, s, in, w, bias, out, n);
  return hipSuccess;
}

}  // namespace mods
