// AffNet, OriNet and HardNet (the reference's affnet_server.py / orinet_server.py / desc_server.py networks) as HIP kernels:
// inference mode, 32 x 32 patches, fp32 with fp32 accumulation on the VALU (fp32-input MFMA has no rate advantage on gfx950 and
// would put the library's fp64 RANSAC kernels at risk, match.hip).
//
//   input  (x - mean) / (std + 1e-7) per patch, std with the N - 1 divisor                                   net_norm_kernel
//   6 x    conv3x3(pad 1) -> BatchNorm(running statistics, no affine) -> ReLU; channels C, C, 2C (stride 2),
//          2C, 4C (stride 2), 4C; C = 16 (AffNet, OriNet) or 32 (HardNet)                                    net_conv3_kernel
//   head   AffNet  conv8x8(64 -> 3) + bias -> tanh, (y0 + 1, y1, y2 + 1)                                     net_head_aff_kernel
//          OriNet  conv8x8(64 -> 2, pad 1) + bias -> tanh -> mean of the 3 x 3 map                           net_head_ori_kernel
//          HardNet conv8x8(128 -> 128) -> BatchNorm -> L2 normalisation -> trunc(clip(210 (y + 0.45)))       net_head_hard_kernel
//
// BatchNorm is folded into the weights and a bias when the network is created.  One launch per layer over a chunk of at most
// kChunk patches; the activations of a chunk ping-pong between two scratch buffers (2 x 32 MB for C = 16, 2 x 64 MB for C = 32:
// they live in the caches, the layers are bound by the FMA rate).  In the convolutions a lane is an output pixel, so a weight is
// the same for the whole wave: it arrives through scalar loads and is an SGPR operand of the FMA, and every activation read from
// LDS feeds 16 output channels held in registers.
// Every sum runs in an order fixed by the architecture alone (input channel, then tap; fixed trees across lanes), and no patch's
// arithmetic touches another patch's data: a patch's output does not depend on the call's size, order or chunking.
//
// That is the fp32 mode (MODS_NET_FP32, the default).  A network created with MODS_NET_BF16 keeps this file's normalisation and
// its host code (creation, scratch, chunking, the test hook) and runs everything behind the normalisation through the kernels of
// nets_mfma.hip: stages 2..6 (the convolution blocks behind the first; stage = block index l + 1, as in mods_test_net_stage)
// and HardNet's head on the matrix cores with bf16 operands and fp32 accumulators (which do have a rate advantage: 16 x the
// fp32 vector rate), stage 1 and the small heads with this file's arithmetic, activations bf16 channels
// last in half the scratch.  The contract of that mode is in include/mods_hip.h; the matrix-core kernels own their SIMDs
// (match.hip), which is what keeps the fp64 RANSAC kernels safe beside them.
#include "common.hpp"
#include "nets_mfma.hpp"
#include <algorithm>
#include <cmath>
#include <mutex>

using mods::set_error;

namespace {

constexpr int kPP = 32 * 32;          // pixels of a patch
constexpr int kChunk = 512;           // patches per set of launches (what the scratch buffers hold)
constexpr int kCoutT = 16;            // output channels a thread of the convolution holds

// fp32 mode: a | b, the two activation buffers.  bf16 mode: a = the normalised patches (fp32), h0 | h1 the bf16 activations
struct NetScratch { float *a = nullptr, *b = nullptr; mods::bf16_t *h0 = nullptr, *h1 = nullptr; hipEvent_t done = nullptr; };

}  // namespace

struct mods_net {
  int device = 0, kind = 0, C = 16, dim = 0, precision = MODS_NET_FP32;
  float *params = nullptr;                       // every folded tensor, one allocation
  // bf16 mode: the folded weights of stages 2..6 (l = 1..5) rounded to bf16, cout x mfma_conv_kp(cin) with k = tap * cin + input channel,
  // and HardNet's head 128 x 8192 with k = pixel * 128 + channel, both in fragment order (mods::mfma_w_index) (params then holds stage 1, the biases and the small heads)
  mods::bf16_t *params16 = nullptr;
  size_t w16_off[6] = {0}, head_w16 = 0;
  size_t w_off[6] = {0}, b_off[6] = {0};         // per block: weights [cout / 16][cin][9][16], bias [cout]
  size_t head_w = 0, head_b = 0;
  // scratch of calls in flight: a call takes a pair of buffers (or makes one), and hands it back with an event that the next
  // taker's stream waits for - the network itself stays immutable and can serve several streams and threads at once
  std::mutex mu;
  std::vector<NetScratch> idle;
};

namespace {

__device__ inline float wave_sum(float v) {
  // xor butterfly: both partners add the same two numbers, so all 64 lanes end with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// [n][1024] -> normalised [n][1024]; one wave per patch, 4 patches per block
__global__ __launch_bounds__(256) void net_norm_kernel(const float *__restrict__ in, float *__restrict__ out, int n, int q8) {
  const int lane = threadIdx.x & 63, patch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= n) return;
  const float *p = in + (size_t)patch * kPP;
  float v[16], s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    float x = p[i * 64 + lane];
    if (q8) x = fminf(fmaxf(rintf(x), 0.f), 255.f);      // cv convertTo(CV_8U): round half to even, saturate
    v[i] = x; s += x;
  }
  const float mean = wave_sum(s) / 1024.f;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) { v[i] -= mean; ss = fmaf(v[i], v[i], ss); }
  const float sd = sqrtf(wave_sum(ss) / 1023.f) + 1e-7f;
  float *o = out + (size_t)patch * kPP;
#pragma unroll
  for (int i = 0; i < 16; i++) o[i * 64 + lane] = v[i] / sd;
}

// conv3x3 (pad 1, stride STRIDE) + folded BatchNorm + ReLU: in [n][CIN][HIN][HIN] -> out [n][COUT][HOUT][HOUT].
// A block of 256 threads = 256 output pixels: a band of 8 rows of one 32 x 32 map, one 16 x 16 map, or the 8 x 8 maps of four
// patches; blockIdx.y = the group of 16 output channels.  The input channels pass through LDS a few at a time, zero padded.
template <int CIN, int COUT, int HIN, int STRIDE>
__global__ __launch_bounds__(256) void net_conv3_kernel(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ wt,
                                                        const float *__restrict__ bias, int n) {
  constexpr int HOUT = HIN / STRIDE, PIX = HOUT * HOUT;
  constexpr int TP = PIX < 256 ? PIX : 256;            // pixels of one patch in a block
  constexpr int PPB = 256 / TP;                        // patches per block
  constexpr int BANDS = PIX / TP;                      // blocks per patch
  constexpr int TROWS = TP / HOUT;                     // output rows of a block
  constexpr int IR = (TROWS - 1) * STRIDE + 3, IW = HIN + 2;
  constexpr int CC = CIN < 8 ? CIN : (STRIDE == 2 ? 4 : 8);
  constexpr int TILE = CC * PPB * IR * IW;
  __shared__ float tile[TILE];
  const int t = threadIdx.x;
  const int pl = t / TP, pix = t % TP;
  const int band = blockIdx.x % BANDS, pg = blockIdx.x / BANDS;
  const int patch = pg * PPB + pl;
  const int oy = pix / HOUT, ox = pix % HOUT;
  const int cg = blockIdx.y;
  const int row0 = band * TROWS * STRIDE - 1;          // input row of the tile's first row
  float acc[kCoutT];
#pragma unroll
  for (int j = 0; j < kCoutT; j++) acc[j] = 0.f;
  const float *w = wt + (size_t)cg * CIN * 9 * kCoutT;
  for (int c0 = 0; c0 < CIN; c0 += CC) {
    __syncthreads();
    // (unrolled in groups, loads first: the global loads of a group are in flight together)
    constexpr int ST = 6;
    for (int e0 = t; e0 < TILE; e0 += 256 * ST) {
      float v[ST];
#pragma unroll
      for (int i = 0; i < ST; i++) {
        const int e = e0 + i * 256;
        const int x = e % IW, r = (e / IW) % IR, p = (e / (IW * IR)) % PPB, c = e / (IW * IR * PPB);
        const int gy = row0 + r, gx = x - 1, gp = pg * PPB + p;
        v[i] = 0.f;
        if (e < TILE && gy >= 0 && gy < HIN && gx >= 0 && gx < HIN && gp < n) v[i] = in[((size_t)gp * CIN + c0 + c) * (HIN * HIN) + gy * HIN + gx];
      }
#pragma unroll
      for (int i = 0; i < ST; i++)
        if (e0 + i * 256 < TILE) tile[e0 + i * 256] = v[i];
    }
    __syncthreads();
    for (int c = 0; c < CC; c++) {
      const float *tp = tile + ((c * PPB + pl) * IR + oy * STRIDE) * IW + ox * STRIDE;
      const float *wc = w + (size_t)(c0 + c) * 9 * kCoutT;      // wave-uniform: scalar loads
#pragma unroll
      for (int k = 0; k < 9; k++) {
        const float v = tp[(k / 3) * IW + (k % 3)];
#pragma unroll
        for (int j = 0; j < kCoutT; j++) acc[j] = fmaf(v, wc[k * kCoutT + j], acc[j]);
      }
    }
  }
  if (patch < n) {
    float *o = out + ((size_t)patch * COUT + cg * kCoutT) * PIX + band * TP + pix;
#pragma unroll
    for (int j = 0; j < kCoutT; j++) o[(size_t)j * PIX] = fmaxf(acc[j] + bias[cg * kCoutT + j], 0.f);
  }
}

// AffNet head: in [n][4096], w [3][4096]; one wave per patch
__global__ __launch_bounds__(256) void net_head_aff_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                                                           float *__restrict__ out, int n) {
  const int lane = threadIdx.x & 63, patch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= n) return;
  const float *p = in + (size_t)patch * 4096;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int i = 0; i < 64; i++) {
    const int k = i * 64 + lane;
    const float v = p[k];
    a0 = fmaf(v, w[k], a0); a1 = fmaf(v, w[4096 + k], a1); a2 = fmaf(v, w[8192 + k], a2);
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
  if (lane == 0) {
    out[(size_t)patch * 3 + 0] = tanhf(a0 + bias[0]) + 1.f;
    out[(size_t)patch * 3 + 1] = tanhf(a1 + bias[1]);
    out[(size_t)patch * 3 + 2] = tanhf(a2 + bias[2]) + 1.f;
  }
}

// OriNet head: conv8x8 with padding 1 over the 8 x 8 map = a 3 x 3 map of 2 channels, tanh, mean.  in [n][64][8][8],
// w [2][64][8][8]; one wave per patch, a lane is the input pixel (y, x) and adds to the output positions whose window holds it
__global__ __launch_bounds__(256) void net_head_ori_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
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
  const float *p = in + (size_t)patch * 4096;
  for (int c = 0; c < 64; c++) {
    const float v = p[c * 64 + lane];
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

// HardNet head: in [n][8192] x wt [8192][128] (BatchNorm folded), + bias, L2 normalisation, the daemon's quantisation.
// A block = 8 patches: thread = (half of K, output channel); the activations are wave-uniform (scalar loads), the weights
// stream from L2 coalesced.  The two halves of K are added in a fixed order through LDS.
constexpr int kHeadP = 8;
__global__ __launch_bounds__(256) void net_head_hard_kernel(const float *__restrict__ in, const float *__restrict__ wt, const float *__restrict__ bias,
                                                            float *__restrict__ out, int n) {
  __shared__ float part[kHeadP][128];
  __shared__ float norm2[kHeadP][2];
  const int t = threadIdx.x, c = t & 127, kh = t >> 7, lane = t & 63;
  const int p0 = blockIdx.x * kHeadP;
  const float *a[kHeadP];
#pragma unroll
  for (int p = 0; p < kHeadP; p++) a[p] = in + (size_t)min(p0 + p, n - 1) * 8192 + kh * 4096;
  const float *wk = wt + (size_t)kh * 4096 * 128 + c;
  float acc[kHeadP];
#pragma unroll
  for (int p = 0; p < kHeadP; p++) acc[p] = 0.f;
  for (int k0 = 0; k0 < 4096; k0 += 4) {
    float wv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) wv[i] = wk[(size_t)(k0 + i) * 128];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int p = 0; p < kHeadP; p++) acc[p] = fmaf(a[p][k0 + i], wv[i], acc[p]);
  }
  if (kh == 1)
#pragma unroll
    for (int p = 0; p < kHeadP; p++) part[p][c] = acc[p];
  __syncthreads();
  float y[kHeadP];
  if (kh == 0) {
#pragma unroll
    for (int p = 0; p < kHeadP; p++) {
      y[p] = (acc[p] + part[p][c]) + bias[c];
      const float s = wave_sum(y[p] * y[p]);
      if (lane == 0) norm2[p][c >> 6] = s;
    }
  }
  __syncthreads();
  if (kh == 0) {
#pragma unroll
    for (int p = 0; p < kHeadP; p++) {
      if (p0 + p >= n) break;
      const float d = y[p] / sqrtf((norm2[p][0] + norm2[p][1]) + 1e-10f);
      double q = 210.0 * ((double)d + 0.45);                  // desc_server.py:44, then the cast to 8 bits truncates
      q = q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q);
      out[(size_t)(p0 + p) * 128 + c] = (float)(int)q;
    }
  }
}

template <int CIN, int COUT, int HIN, int STRIDE>
void launch_conv(hipStream_t s, const float *in, float *out, const float *w, const float *b, int n) {
  constexpr int PIX = (HIN / STRIDE) * (HIN / STRIDE);
  constexpr int TP = PIX < 256 ? PIX : 256, PPB = 256 / TP, BANDS = PIX / TP;
  const dim3 grid((unsigned)((n + PPB - 1) / PPB * BANDS), COUT / kCoutT);
  hipLaunchKernelGGL((net_conv3_kernel<CIN, COUT, HIN, STRIDE>), grid, dim3(256), 0, s, in, out, w, b, n);
}

// block l of the six: conv l of a network of width C on n patches
template <int C>
void launch_block(const mods_net *net, hipStream_t s, int l, const float *in, float *out, int n) {
  const float *w = net->params + net->w_off[l], *b = net->params + net->b_off[l];
  switch (l) {
    case 0: launch_conv<1, C, 32, 1>(s, in, out, w, b, n); break;
    case 1: launch_conv<C, C, 32, 1>(s, in, out, w, b, n); break;
    case 2: launch_conv<C, 2 * C, 32, 2>(s, in, out, w, b, n); break;
    case 3: launch_conv<2 * C, 2 * C, 16, 1>(s, in, out, w, b, n); break;
    case 4: launch_conv<2 * C, 4 * C, 16, 2>(s, in, out, w, b, n); break;
    default: launch_conv<4 * C, 4 * C, 8, 1>(s, in, out, w, b, n); break;
  }
}

void launch_block(const mods_net *net, hipStream_t s, int l, const float *in, float *out, int n) {
  if (net->C == 16) launch_block<16>(net, s, l, in, out, n);
  else launch_block<32>(net, s, l, in, out, n);
}

void launch_norm(hipStream_t s, const float *in, float *out, int n, int quantise_u8) {
  hipLaunchKernelGGL(net_norm_kernel, dim3((n + 3) / 4), dim3(256), 0, s, in, out, n, quantise_u8 ? 1 : 0);
}

void launch_head(const mods_net *net, hipStream_t s, const float *in, float *out, int n) {
  const float *w = net->params + net->head_w, *b = net->params + net->head_b;
  if (net->kind == MODS_NET_AFFNET) hipLaunchKernelGGL(net_head_aff_kernel, dim3((n + 3) / 4), dim3(256), 0, s, in, w, b, out, n);
  else if (net->kind == MODS_NET_ORINET) hipLaunchKernelGGL(net_head_ori_kernel, dim3((n + 3) / 4), dim3(256), 0, s, in, w, b, out, n);
  else hipLaunchKernelGGL(net_head_hard_kernel, dim3((n + kHeadP - 1) / kHeadP), dim3(256), 0, s, in, w, b, out, n);
}

// the blocks (l = stage - 1) and the head of a bf16 network (nets_mfma.hip); l = 0 reads the fp32 normalised patches
hipError_t launch_block16(const mods_net *net, hipStream_t s, int l, const void *in, mods::bf16_t *out, int n) {
  const float *b = net->params + net->b_off[l];
  if (l == 0) return mods::mfma_launch_conv1(s, net->device, net->C, (const float *)in, out, net->params + net->w_off[0], b, n);
  return mods::mfma_launch_conv3(s, net->device, net->C, l, (const mods::bf16_t *)in, out, net->params16 + net->w16_off[l], b, n);
}

hipError_t launch_head16(const mods_net *net, hipStream_t s, const mods::bf16_t *in, float *out, int n) {
  const float *w = net->params + net->head_w, *b = net->params + net->head_b;
  if (net->kind == MODS_NET_AFFNET) return mods::mfma_launch_head_aff(s, in, w, b, out, n);
  if (net->kind == MODS_NET_ORINET) return mods::mfma_launch_head_ori(s, in, w, b, out, n);
  return mods::mfma_launch_head_hard(s, in, net->params16 + net->head_w16, b, out, n);
}

// floats of one patch at the input (out = false) or the output of stage 0 (normalisation), 1..6 (blocks), 7 (head)
size_t stage_elems(const mods_net *net, int stage, bool out) {
  const int C = net->C;
  const int ch[7] = {1, C, C, 2 * C, 2 * C, 4 * C, 4 * C}, size[7] = {32, 32, 32, 16, 16, 8, 8};   // the maps between the stages
  if (stage == 7 && out) return net->dim;
  const int m = stage == 0 ? 0 : stage - 1 + (out ? 1 : 0);
  return (size_t)ch[m] * size[m] * size[m];
}

// expected element counts of the tensors of `kind`, network order
std::vector<size_t> net_tensor_sizes(int kind) {
  const int C = kind == MODS_NET_HARDNET ? 32 : 16;
  const int cin[6] = {1, C, C, 2 * C, 2 * C, 4 * C}, cout[6] = {C, C, 2 * C, 2 * C, 4 * C, 4 * C};
  std::vector<size_t> v;
  for (int l = 0; l < 6; l++) { v.push_back((size_t)cout[l] * cin[l] * 9); v.push_back(cout[l]); v.push_back(cout[l]); }
  if (kind == MODS_NET_HARDNET) { v.push_back((size_t)128 * 128 * 64); v.push_back(128); v.push_back(128); }
  else { const size_t o = kind == MODS_NET_AFFNET ? 3 : 2; v.push_back(o * 64 * 64); v.push_back(o); }
  return v;
}

const char *net_name(int kind) { return kind == MODS_NET_AFFNET ? "AffNet" : kind == MODS_NET_ORINET ? "OriNet" : "HardNet"; }

int scratch_take(mods_net *net, hipStream_t s, NetScratch *out) {
  {
    std::lock_guard<std::mutex> g(net->mu);
    if (!net->idle.empty()) { *out = net->idle.back(); net->idle.pop_back(); }
  }
  if (out->a) { MODS_HIP_CHECK(hipStreamWaitEvent(s, out->done, 0)); return MODS_OK; }
  const size_t elems = (size_t)kChunk * net->C * kPP;       // the widest activation: C x 32 x 32 per patch
  if (net->precision == MODS_NET_BF16) {
    MODS_HIP_CHECK(hipMalloc(&out->a, (size_t)kChunk * kPP * sizeof(float) + 2 * elems * sizeof(mods::bf16_t)));
    out->h0 = (mods::bf16_t *)(out->a + (size_t)kChunk * kPP);
    out->h1 = out->h0 + elems;
  } else {
    MODS_HIP_CHECK(hipMalloc(&out->a, 2 * elems * sizeof(float)));
    out->b = out->a + elems;
  }
  MODS_HIP_CHECK(hipEventCreateWithFlags(&out->done, hipEventDisableTiming));
  return MODS_OK;
}

}  // namespace

extern "C" {

int mods_net_create(int device, int kind, const float *const *tensors, const size_t *n_floats, int n_tensors, mods_net **out) {
  return mods_net_create_ex(device, kind, tensors, n_floats, n_tensors, MODS_NET_FP32, out);
}

int mods_net_create_ex(int device, int kind, const float *const *tensors, const size_t *n_floats, int n_tensors, int precision, mods_net **out) {
  if (!out) { set_error("net_create: null output"); return MODS_E_ARG; }
  *out = nullptr;
  if (kind != MODS_NET_AFFNET && kind != MODS_NET_ORINET && kind != MODS_NET_HARDNET) { set_error("net_create: unknown kind %d", kind); return MODS_E_ARG; }
  if (precision != MODS_NET_FP32 && precision != MODS_NET_BF16) {
    set_error("net_create: unknown precision %d (MODS_NET_FP32 = %d, MODS_NET_BF16 = %d)", precision, MODS_NET_FP32, MODS_NET_BF16);
    return MODS_E_ARG;
  }
  const std::vector<size_t> want = net_tensor_sizes(kind);
  if (!tensors || !n_floats || n_tensors != (int)want.size()) {
    set_error("net_create: %s takes %d tensors, %d given", net_name(kind), (int)want.size(), n_tensors);
    return MODS_E_ARG;
  }
  for (int i = 0; i < n_tensors; i++)
    if (!tensors[i] || n_floats[i] != want[i]) {
      set_error("net_create: tensor %d of %s has %zu elements, %zu expected", i, net_name(kind), tensors[i] ? n_floats[i] : (size_t)0, want[i]);
      return MODS_E_ARG;
    }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
    (void)hipGetLastError();
    set_error("net_create: no HIP device %d (%d visible); there is no CPU path", device, n_dev);
    return MODS_E_NODEVICE;
  }
  const int C = kind == MODS_NET_HARDNET ? 32 : 16;
  const int cin[6] = {1, C, C, 2 * C, 2 * C, 4 * C}, cout[6] = {C, C, 2 * C, 2 * C, 4 * C, 4 * C};
  const bool bf = precision == MODS_NET_BF16;
  std::vector<float> host;
  std::vector<mods::bf16_t> host16;
  mods_net *net = new mods_net;
  net->device = device; net->kind = kind; net->precision = precision; net->C = C; net->dim = kind == MODS_NET_AFFNET ? 3 : kind == MODS_NET_ORINET ? 2 : 128;
  auto reserve = [&](size_t n) { const size_t o = (host.size() + 15) & ~(size_t)15; host.resize(o + n, 0.f); return o; };   // 64-byte aligned
  auto reserve16 = [&](size_t n) { const size_t o = (host16.size() + 31) & ~(size_t)31; host16.resize(o + n, 0); return o; };
  for (int l = 0; l < 6; l++) {
    const float *W = tensors[3 * l], *mean = tensors[3 * l + 1], *var = tensors[3 * l + 2];
    const bool w16 = bf && l >= 1;                            // bf16 mode, stages 2..6: the folded weight rounded once more
    const int kp = mods::mfma_conv_kp(cin[l]);
    const size_t wo = w16 ? reserve16((size_t)cout[l] * kp) : reserve((size_t)cout[l] * cin[l] * 9), bo = reserve(cout[l]);
    (w16 ? net->w16_off[l] : net->w_off[l]) = wo; net->b_off[l] = bo;
    for (int co = 0; co < cout[l]; co++) {
      const double inv = 1.0 / sqrt((double)var[co] + 1e-5);
      host[bo + co] = (float)(-(double)mean[co] * inv);
      for (int ci = 0; ci < cin[l]; ci++)
        for (int k = 0; k < 9; k++) {
          const float wf = (float)((double)W[((size_t)co * cin[l] + ci) * 9 + k] * inv);
          if (w16) host16[wo + mods::mfma_w_index(co, k * cin[l] + ci, kp / 32)] = mods::bf16_round_host(wf);
          else host[wo + (((size_t)(co / kCoutT) * cin[l] + ci) * 9 + k) * kCoutT + co % kCoutT] = wf;
        }
    }
  }
  if (kind == MODS_NET_HARDNET && bf) {
    const float *W = tensors[18], *mean = tensors[19], *var = tensors[20];
    net->head_w16 = reserve16((size_t)128 * 8192); net->head_b = reserve(128);
    for (int co = 0; co < 128; co++) {
      const double inv = 1.0 / sqrt((double)var[co] + 1e-5);
      host[net->head_b + co] = (float)(-(double)mean[co] * inv);
      for (int c = 0; c < 128; c++)
        for (int px = 0; px < 64; px++)
          host16[net->head_w16 + mods::mfma_w_index(co, px * 128 + c, 8192 / 32)] = mods::bf16_round_host((float)((double)W[(size_t)co * 8192 + c * 64 + px] * inv));
    }
  } else if (kind == MODS_NET_HARDNET) {
    const float *W = tensors[18], *mean = tensors[19], *var = tensors[20];
    net->head_w = reserve((size_t)8192 * 128); net->head_b = reserve(128);
    for (int co = 0; co < 128; co++) {
      const double inv = 1.0 / sqrt((double)var[co] + 1e-5);
      host[net->head_b + co] = (float)(-(double)mean[co] * inv);
      for (int k = 0; k < 8192; k++) host[net->head_w + (size_t)k * 128 + co] = (float)((double)W[(size_t)co * 8192 + k] * inv);
    }
  } else {
    net->head_w = reserve(want[18]); net->head_b = reserve(want[19]);
    memcpy(&host[net->head_w], tensors[18], want[18] * sizeof(float));
    memcpy(&host[net->head_b], tensors[19], want[19] * sizeof(float));
  }
  int prev = 0;
  (void)hipGetDevice(&prev);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc(&net->params, host.size() * sizeof(float));
  if (e == hipSuccess) e = mods::copy_wait(mods::thread_stream(device), net->params, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && bf) e = hipMalloc(&net->params16, host16.size() * sizeof(mods::bf16_t));
  if (e == hipSuccess && bf) e = mods::copy_wait(mods::thread_stream(device), net->params16, host16.data(), host16.size() * sizeof(mods::bf16_t), hipMemcpyHostToDevice);
  (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    set_error("net_create: %s", hipGetErrorString(e));
    if (net->params) (void)hipFree(net->params);
    if (net->params16) (void)hipFree(net->params16);
    delete net;
    return MODS_E_HIP;
  }
  *out = net;
  return MODS_OK;
}

void mods_net_destroy(mods_net *net) {
  if (!net) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(net->device);
  for (NetScratch &s : net->idle) { (void)hipEventSynchronize(s.done); (void)hipEventDestroy(s.done); (void)hipFree(s.a); }
  (void)hipFree(net->params);
  if (net->params16) (void)hipFree(net->params16);
  (void)hipSetDevice(prev);
  delete net;
}

int mods_net_dim(const mods_net *net) { return net ? net->dim : 0; }
int mods_net_precision(const mods_net *net) { return net ? net->precision : MODS_NET_FP32; }
int mods_net_chunk(void) { return kChunk; }

// the launches of one call; `marks` (the timing hook): an event in front of every stage of every chunk and one behind the last
static int forward_launches(mods_net *net, hipStream_t s, const float *patches_dev, int n, int quantise_u8, float *out_dev, std::vector<hipEvent_t> *marks) {
  NetScratch sc;
  int rc = scratch_take(net, s, &sc);
  if (rc) { if (sc.a) (void)hipFree(sc.a); return rc; }
  // the first host-side failure of the call: a kernel's LDS attribute could not be set (bf16 mode), or an event of the timing hook
  // could not be made or recorded.  After one, the remaining bf16 launches and marks are skipped and the call reports it.
  hipError_t e_host = hipSuccess;
  auto mark = [&]() {
    if (!marks || e_host != hipSuccess) return;
    hipEvent_t ev = nullptr;
    e_host = hipEventCreate(&ev);
    if (e_host == hipSuccess) { marks->push_back(ev); e_host = hipEventRecord(ev, s); }
  };
  for (int i0 = 0; i0 < n; i0 += kChunk) {
    const int m = std::min(kChunk, n - i0);
    if (net->precision == MODS_NET_BF16) {
      mark();
      launch_norm(s, patches_dev + (size_t)i0 * kPP, sc.a, m, quantise_u8);
      mark();
      if (e_host == hipSuccess) e_host = launch_block16(net, s, 0, sc.a, sc.h0, m);
      for (int l = 1; l < 6 && e_host == hipSuccess; l++) { mark(); e_host = launch_block16(net, s, l, l % 2 ? sc.h0 : sc.h1, l % 2 ? sc.h1 : sc.h0, m); }
      mark();
      if (e_host == hipSuccess) e_host = launch_head16(net, s, sc.h1, out_dev + (size_t)i0 * net->dim, m);
      continue;
    }
    mark();
    launch_norm(s, patches_dev + (size_t)i0 * kPP, sc.b, m, quantise_u8);
    for (int l = 0; l < 6; l++) { mark(); launch_block(net, s, l, l % 2 ? sc.a : sc.b, l % 2 ? sc.b : sc.a, m); }
    mark();
    launch_head(net, s, sc.b, out_dev + (size_t)i0 * net->dim, m);
  }
  mark();
  const hipError_t e_launch = e_host != hipSuccess ? e_host : hipGetLastError();
  const hipError_t e_rec = hipEventRecord(sc.done, s);
  {
    std::lock_guard<std::mutex> g(net->mu);
    net->idle.push_back(sc);
  }
  MODS_HIP_CHECK(e_launch);
  MODS_HIP_CHECK(e_rec);
  return MODS_OK;
}

int mods_net_forward_dev(mods_net *net, void *hip_stream, const float *patches_dev, int n, int quantise_u8, float *out_dev) {
  if (!net || n < 0 || (n > 0 && (!patches_dev || !out_dev))) { set_error("net_forward: null argument"); return MODS_E_ARG; }
  if (n == 0) return MODS_OK;
  MODS_HIP_CHECK(hipSetDevice(net->device));
  return forward_launches(net, (hipStream_t)hip_stream, patches_dev, n, quantise_u8, out_dev, nullptr);
}

int mods_test_net_stage_times(mods_net *net, void *hip_stream, const float *patches_dev, int n, int quantise_u8, float *out_dev, float *stage_ms) {
  if (!net || n < 1 || !patches_dev || !out_dev || !stage_ms) { set_error("net_stage_times: bad argument"); return MODS_E_ARG; }
  MODS_HIP_CHECK(hipSetDevice(net->device));
  hipStream_t s = (hipStream_t)hip_stream;
  std::vector<hipEvent_t> marks;
  int rc = forward_launches(net, s, patches_dev, n, quantise_u8, out_dev, &marks);
  hipError_t e = hipStreamSynchronize(s);
  for (int i = 0; i < 8; i++) stage_ms[i] = 0.f;
  const size_t chunks = ((size_t)n + kChunk - 1) / kChunk;
  if (rc == MODS_OK && e == hipSuccess && marks.size() == 8 * chunks + 1) {
    // events 8 c .. 8 c + 7 stand in front of the stages of chunk c; the event behind a chunk's head is the next chunk's first
    for (size_t i = 0; i + 1 < marks.size() && e == hipSuccess; i++) {
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, marks[i], marks[i + 1]);
      stage_ms[i % 8] += ms;
    }
  } else if (rc == MODS_OK && e == hipSuccess) {
    set_error("net_stage_times: %zu events for %zu chunks", marks.size(), chunks);
    rc = MODS_E_HIP;
  }
  for (hipEvent_t ev : marks) (void)hipEventDestroy(ev);
  if (rc) return rc;
  MODS_HIP_CHECK(e);
  return MODS_OK;
}

int mods_net_forward(mods_net *net, const float *patches_host, int n, int quantise_u8, float *out_host) {
  if (!net || n < 0 || (n > 0 && (!patches_host || !out_host))) { set_error("net_forward: null argument"); return MODS_E_ARG; }
  if (n == 0) return MODS_OK;
  MODS_HIP_CHECK(hipSetDevice(net->device));
  hipStream_t s = mods::thread_stream(net->device);
  mods::Buf<float> in_dev;
  const size_t in_elems = (size_t)n * kPP, out_elems = (size_t)n * net->dim;
  MODS_HIP_CHECK(in_dev.reserve(in_elems + out_elems));
  hipError_t e = mods::copy_wait(s, in_dev, patches_host, in_elems * sizeof(float), hipMemcpyHostToDevice);
  int rc = MODS_OK;
  if (e == hipSuccess) rc = mods_net_forward_dev(net, s, in_dev, n, quantise_u8, in_dev + in_elems);
  if (e == hipSuccess && rc == MODS_OK) e = mods::copy_wait(s, out_host, in_dev + in_elems, out_elems * sizeof(float), hipMemcpyDeviceToHost);
  if (rc) return rc;
  MODS_HIP_CHECK(e);
  return MODS_OK;
}

int mods_test_net_stage(mods_net *net, int stage, const float *in_host, int n, int quantise_u8, float *out_host, int *guard_ok) {
  if (!net || !in_host || !out_host || !guard_ok || stage < 0 || stage > 7 || n < 1 || n > kChunk) { set_error("net_stage: bad argument"); return MODS_E_ARG; }
  *guard_ok = 0;
  MODS_HIP_CHECK(hipSetDevice(net->device));
  hipStream_t s = mods::thread_stream(net->device);
  const size_t in_elems = n * stage_elems(net, stage, false), per_out = stage_elems(net, stage, true), out_elems = (n + 1) * per_out;
  if (net->precision == MODS_NET_BF16 && stage >= 1) {
    // bf16 mode: the activations between the stages are bf16, channels last.  The host's [n][c][h][w] floats are rounded and
    // transposed on their way in (stages 2..7), the outputs of stages 1..6 widened and transposed back.
    const bool in16 = stage >= 2, out16 = stage <= 6;
    const size_t per_in = stage_elems(net, stage, false);
    const int C = net->C;
    const int ch[7] = {1, C, C, 2 * C, 2 * C, 4 * C, 4 * C};                    // channels of the maps between the stages
    const size_t cin = ch[stage - 1], hw_in = per_in / cin, cout = out16 ? ch[stage] : 1, hw_out = per_out / cout;
    mods::Buf<float> in_dev, out_dev;                                          // (bf16 data takes half of the words)
    MODS_HIP_CHECK(mods::reserve_group(in_dev, in_elems, out_dev, out_elems));
    if (in16) {
      std::vector<mods::bf16_t> h(in_elems);
      for (int p = 0; p < n; p++)
        for (size_t c = 0; c < cin; c++)
          for (size_t i = 0; i < hw_in; i++) h[(p * hw_in + i) * cin + c] = mods::bf16_round_host(in_host[(p * cin + c) * hw_in + i]);
      MODS_HIP_CHECK(mods::copy_wait(s, in_dev, h.data(), in_elems * sizeof(mods::bf16_t), hipMemcpyHostToDevice));
    } else {
      MODS_HIP_CHECK(mods::copy_wait(s, in_dev, in_host, in_elems * sizeof(float), hipMemcpyHostToDevice));
    }
    const size_t out_bytes = out_elems * (out16 ? sizeof(mods::bf16_t) : sizeof(float));
    MODS_HIP_CHECK(mods::fill_wait(s, out_dev, 0xA5, out_bytes));
    if (out16) MODS_HIP_CHECK(launch_block16(net, s, stage - 1, (const float *)in_dev, (mods::bf16_t *)(float *)out_dev, n));
    else MODS_HIP_CHECK(launch_head16(net, s, (const mods::bf16_t *)(const float *)in_dev, out_dev, n));
    MODS_HIP_CHECK(hipGetLastError());
    std::vector<unsigned char> host(out_bytes);
    MODS_HIP_CHECK(mods::copy_wait(s, host.data(), out_dev, out_bytes, hipMemcpyDeviceToHost));
    if (out16) {
      const mods::bf16_t *h = (const mods::bf16_t *)host.data();
      for (int p = 0; p < n; p++)
        for (size_t c = 0; c < cout; c++)
          for (size_t i = 0; i < hw_out; i++) out_host[(p * cout + c) * hw_out + i] = mods::bf16_widen_host(h[(p * hw_out + i) * cout + c]);
    } else {
      memcpy(out_host, host.data(), n * per_out * sizeof(float));
    }
    int ok = 1;
    for (size_t i = n * per_out * (out16 ? sizeof(mods::bf16_t) : sizeof(float)); i < out_bytes; i++)
      if (host[i] != 0xA5) ok = 0;
    *guard_ok = ok;
    return MODS_OK;
  }
  mods::Buf<float> in_dev, out_dev;
  MODS_HIP_CHECK(mods::reserve_group(in_dev, in_elems, out_dev, out_elems));
  MODS_HIP_CHECK(mods::copy_wait(s, in_dev, in_host, in_elems * sizeof(float), hipMemcpyHostToDevice));
  MODS_HIP_CHECK(mods::fill_wait(s, out_dev, 0xA5, out_elems * sizeof(float)));       // every word 0xA5A5A5A5 (-2.9e-16f)
  if (stage == 0) launch_norm(s, in_dev, out_dev, n, quantise_u8);
  else if (stage <= 6) launch_block(net, s, stage - 1, in_dev, out_dev, n);
  else launch_head(net, s, in_dev, out_dev, n);
  MODS_HIP_CHECK(hipGetLastError());
  std::vector<float> host(out_elems);
  MODS_HIP_CHECK(mods::copy_wait(s, host.data(), out_dev, out_elems * sizeof(float), hipMemcpyDeviceToHost));
  memcpy(out_host, host.data(), n * per_out * sizeof(float));
  int ok = 1;
  for (size_t i = n * per_out; i < out_elems; i++) {
    unsigned bits;
    memcpy(&bits, &host[i], 4);
    if (bits != 0xA5A5A5A5u) ok = 0;
  }
  *guard_ok = ok;
  return MODS_OK;
}

static int slot_check(mods_ctx *c, const mods_net *net, int kind, const char *slot) {
  if (!c) { set_error("built-in %s: null context", slot); return MODS_E_ARG; }
  if (!net) return MODS_OK;
  if (net->kind != kind) { set_error("built-in %s takes an %s, the network given is a %s", slot, net_name(kind), net_name(net->kind)); return MODS_E_ARG; }
  if (net->device != c->device) { set_error("built-in %s: the network lives on device %d, the context on %d", slot, net->device, c->device); return MODS_E_ARG; }
  return MODS_OK;
}

int mods_ctx_set_builtin_shape(mods_ctx *c, mods_net *net, double mrSize, int quantise_u8) {
  const int rc = slot_check(c, net, MODS_NET_AFFNET, "shape");
  if (rc) return rc;
  if (net) { c->shape_fn = nullptr; c->shape_user = nullptr; c->shape_mr = mrSize; c->shape_ps = 32; }
  c->shape_net = net; c->shape_q8 = quantise_u8 ? 1 : 0;
  mods::dev_state_changed(c);
  return MODS_OK;
}

int mods_ctx_set_builtin_orientation(mods_ctx *c, mods_net *net, double mrSize, int quantise_u8) {
  const int rc = slot_check(c, net, MODS_NET_ORINET, "orientation");
  if (rc) return rc;
  if (net) { c->ori_fn = nullptr; c->ori_user = nullptr; c->ori_mr = mrSize; c->ori_ps = 32; }
  c->ori_net = net; c->ori_q8 = quantise_u8 ? 1 : 0;
  mods::dev_state_changed(c);
  return MODS_OK;
}

int mods_ctx_set_builtin_descriptor(mods_ctx *c, mods_net *net, double mrSize, int quantise_u8) {
  const int rc = slot_check(c, net, MODS_NET_HARDNET, "descriptor");
  if (rc) return rc;
  if (net) { c->ext_fn = nullptr; c->ext_user = nullptr; c->ext_mr = mrSize; c->ext_ps = 32; }
  c->ext_net = net; c->ext_q8 = quantise_u8 ? 1 : 0;
  mods::dev_state_changed(c);
  return MODS_OK;
}

}  // extern "C"

namespace mods {

int net_run_to_host(mods_ctx *ctx, mods_net *net, const float *patches_dev, int n, int quantise_u8, float *out_host) {
  if (n <= 0) return MODS_OK;
  const size_t need = (size_t)n * net->dim;
  MODS_HIP_CHECK(mods::reserve_scratch(ctx, ctx->net_out_dev, need, std::max<size_t>(need + need / 2, 1 << 16)));
  const int rc = mods_net_forward_dev(net, ctx->stream, patches_dev, n, quantise_u8, ctx->net_out_dev);
  if (rc) return rc;
  MODS_HIP_CHECK(mods::copy_wait(ctx->stream, out_host, ctx->net_out_dev, need * sizeof(float), hipMemcpyDeviceToHost));
  return MODS_OK;
}

}  // namespace mods
