// What the exact-f32 kernels of the ResNet x-vector extractor share between their per-call form (csrc/conv2d.hip) and their form per segment
// of a ragged batch (csrc/ragged2d/resnet_ragged.hip): ONE copy of each body.  The kernels only say which image, or which row, a block or
// wave works on; every load, operation and store is issued by the shared text, so a segment of a ragged batch has the bits of the single
// call by construction.  An image is [C][H][pitch] with columns 0 .. W - 1 of every row its own: a call of its own has pitch = W, a segment
// of a packed time axis has the pitch of the whole rows.
//
// The two conv bodies are STATEMENTS in headers of their own, #included inside the kernels, not functions: csrc/conv2d_tile_body.h and
// csrc/conv2d_stem_body.h.  As __forceinline__ functions they compiled to other code than the same statements in the kernel: hipcc
// optimises a callee, and the `fetch` lambda inside it, on its own before it inlines them.  Where the row pitch was an argument of its own
// the compiler no longer took the index factor for positive (it does where the factor is the variable of the column test `gw < W`) and
// formed seven 64 x 64 bit products per chunk; the output base, passed in, was carried through the K loop in two more SGPRs; the per-call
// f32 path measured 0.3 - 0.9 % slower, outside the spread of its runs, and the segment form of the stride-2 3x3 kernel changed its
// register allocation and waves per SIMD.  Expanded in place, with the per-call kernels naming W / Wo themselves as the pitches, the K
// loops and the register counts are the ones these kernels had when each held its own copy (profiles/conv2d_tile_refactor.txt).
#pragma once
#include "common.h"

namespace sat {

typedef float c2_f32x16 __attribute__((ext_vector_type(16)));

constexpr int C2_TH = 4;     // output rows per block: one per wave
constexpr int C2_TW = 32;    // output columns per block: the N of one 32x32 MFMA tile
constexpr int C2_CI = 8;     // input channels per staged chunk: four k-steps of v_mfma_f32_32x32x2_f32 per tap
constexpr int C2_STEM_CO = 32;

// THE MFMA CONV (conv2d_tile_body.h).  Conv2d (bias=False; KS = 3 with padding 1 or KS = 1 with padding 0; stride S in both axes) as an
// implicit GEMM on the exact f32 MFMA: M = output channels (A = weights), N = 32 output pixels of one row (B = input pixels shifted by the
// tap), K = (tap, input channel).  A block owns one image, 32 MT output channels from co0 and C2_TH x C2_TW output pixels from (ho0, wo0).
// For every chunk of C2_CI input channels it stages the halo tile of xb (zero outside 0 .. H - 1 x 0 .. W - 1: the padding, whatever a
// wider row holds there) and the chunk's weights [tap][ci][co] in LDS (through registers, the next chunk's loads in flight behind this
// chunk's MFMAs); wave w computes output row ho0 + w: per (tap, channel pair) one B fragment and MT A fragments from LDS, MT MFMAs.  The
// sum over K runs in ONE fixed order (chunk, tap, channel pair; no atomics, no split K): the same input gives the same bits, alone, inside
// a batch or as a segment.  Epilogue: v = acc * scale[co] + shift[co] (the BatchNorm in eval, after the sum as the reference applies it),
// optional ReLU; columns 0 .. Wo - 1 of yb [Cout][Ho][ypitch] are written.
//
// THE STEM (conv2d_stem_body.h): Conv2d(1, 32, 3, padding 1, stride 1).  K = 9 does not feed a matrix core; one thread per output pixel
// (ho, wo) of the image xb [H][xpitch] keeps its nine inputs in registers and walks the 32 output channels of yb [32][H][ypitch] (weights
// [tap][co]: wave-uniform reads), an fmaf chain over the taps in order.  The block stages the weights and the affine first, and a thread
// past the image's last column leaves behind that barrier.

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the two passes of MeanStdPooling over one row by one wave: the mean of xr[0 .. T - 1] and the sum of the squared deviations from it,
// in every lane (the caller's lane 0 takes the root of q / (T - 1): the unbiased deviation of torch.std)
__device__ __forceinline__ void row_mean_sqdev_wave(const float* __restrict__ xr, int T, int lane, float* mean_out, float* q_out) {
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += xr[t];
  const float mean = wave_sum(s) / (float)T;
  float q = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float d = xr[t] - mean;
    q = __builtin_fmaf(d, d, q);
  }
  *mean_out = mean;
  *q_out = wave_sum(q);
}

}  // namespace sat
