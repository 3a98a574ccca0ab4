// The bf16 matrix-core mode of the built-in networks (nets_mfma.hip): launch functions that nets.hip calls for a network created
// with MODS_NET_BF16, and the host-side rounding both files share.  Activations are bf16 in [n][h][w][channels] order
// ("channels last": the 8 values of a matrix-core operand are 8 channels of one pixel, one 16-byte read).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

namespace mods {

typedef uint16_t bf16_t;   // the upper half of a float

// fp32 -> nearest bf16, ties to even (finite input)
inline bf16_t bf16_round_host(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}
inline float bf16_widen_host(bf16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// (stages as in mods_test_net_stage: 0 normalisation, 1..6 the convolution blocks, 7 the head; the launch functions take
// l = stage - 1, the block's index in the state dict's order)
// K of a block of stages 2..6 padded to the k-step of the matrix-core instruction: elements of one output channel's row of the bf16 weights
inline int mfma_conv_kp(int cin) { return (9 * cin + 31) / 32 * 32; }
// where element (output channel co, k) of a weight matrix of `ksteps` k-steps lies: fragment order [co / 16][k-step][lane][8], the
// lane (k % 32 / 8) * 16 + co % 16 holding k % 8 = 0..7 of its row - what a wave reads with one 16-byte load per lane
inline size_t mfma_w_index(int co, int k, int ksteps) {
  return ((((size_t)(co / 16) * ksteps + k / 32) * 64) + (size_t)((k % 32) / 8) * 16 + co % 16) * 8 + k % 8;
}
// patches whose 8 x 8 output maps share a workgroup (stages 5 and 6), and patches of one workgroup of HardNet's head
constexpr int kMfmaPatches8 = 2;
constexpr int kMfmaHeadPatches = 16;

// stage 1 (conv 1 -> C, the fp32 kernel's arithmetic and fp32 weights [C / 16][1][9][16]) with bf16 output [n][32][32][C]
hipError_t mfma_launch_conv1(hipStream_t s, int device, int C, const float *in, bf16_t *out, const float *w, const float *bias, int n);
// stage l + 1 = 2..6 (l = 1..5) of a network of width C: in [n][hin][hin][cin] -> out [n][hout][hout][cout], weights bf16, cout x mfma_conv_kp(cin)
// in fragment order (mfma_w_index) with k = tap * cin + input channel, zero behind 9 cin; bias fp32
hipError_t mfma_launch_conv3(hipStream_t s, int device, int C, int l, const bf16_t *in, bf16_t *out, const bf16_t *w, const float *bias, int n);
// heads on [n][8][8][4C]: AffNet / OriNet with their fp32 weights in the state dict's order, HardNet with bf16 weights
// 128 x 8192 in fragment order, k = pixel * 128 + channel
hipError_t mfma_launch_head_aff(hipStream_t s, const bf16_t *in, const float *w, const float *bias, float *out, int n);
hipError_t mfma_launch_head_ori(hipStream_t s, const bf16_t *in, const float *w, const float *bias, float *out, int n);
hipError_t mfma_launch_head_hard(hipStream_t s, const bf16_t *in, const bf16_t *w, const float *bias, float *out, int n);

}  // namespace mods
