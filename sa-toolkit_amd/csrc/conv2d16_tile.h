// The tile body of the split-f16 2-D convolution: ONE copy, shared by the per-call kernel (csrc/conv2d16/conv2d_f16x3.hip) and its segment
// form for ragged batches (csrc/ragged2d16/conv2d_f16x3_segments.hip).  Both wrappers only say which image a block works on; every load,
// MFMA and store is issued here, so a segment of a ragged batch has the bits of the single call by construction.
#pragma once
#include "common.h"
#include "../../include/satools_hip_conv2d16.h"

namespace sat {

typedef float c16_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 c16_h8 __attribute__((ext_vector_type(8)));

constexpr int C16_TH = 4;      // output rows per block: one per wave
constexpr int C16_CI = 16;     // input channels per staged chunk: the K of one v_mfma_f32_32x32x16_f16

// Implicit GEMM: M = output channels (A = weights), N = 32 output pixels of one row (B = input pixels shifted by the tap), K = (chunk of
// 16 input channels, tap, channel).  A block owns one image, 32 MT output channels from co0 and C16_TH x 32 NT output pixels from
// (ho0, wo0); wave w computes output row ho0 + w: NT tiles of 32 columns side by side, so that every A fragment serves NT MFMAs and every
// B fragment MT (at MT = NT = 2: eight 16-byte fragment reads per twelve MFMAs; one tile per wave would have the LDS, not the matrix
// core, set the pace).
// The image: xb [Cin][H][xpitch] of which columns 0 .. W - 1 are the image (everything outside 0 .. H - 1 x 0 .. W - 1 is staged as zero:
// the padding, whatever a wider row holds there, and zero raises no flag); yb [Cout][Ho][ypitch] of which columns 0 .. Wo - 1 are written.
// A call of its own has xpitch = W and ypitch = Wo; a segment of a packed time axis has the pitches of the whole rows.
// Per chunk the block stages in LDS
//   X  [hi|lo][channel half][row][column] x 16 B (8 f16): the halo tile, split into hi + lo while it is staged; under stride 2 the even
//      columns of a row come first, then the odd ones, so that the 32 lanes of a tap read consecutive units at either stride
//   W  [tap][hi|lo][channel half][row] x 16 B: a straight copy of the packed weights
// so every A and B fragment is one ds_read_b128 of consecutive units.  The chunk's elements travel through registers: the NEXT chunk's
// loads are issued before this chunk's MFMAs and stored to LDS after them.  The sum over K runs in ONE fixed order (chunk, tap; lo-hi,
// hi-lo, hi-hi): the same input gives the same bits, alone, inside a batch or as a segment.
// Epilogue: v = acc * descale (a power of two), then v * scale[co] + shift[co], optional ReLU.
// Every thread of the block must make the call (two barriers per chunk): a wrapper's early returns are block-uniform and come before it.
template <int KS, int S, int MT, int NT>
__device__ __forceinline__ void conv2d_f16x3_tile(const float* __restrict__ xb, int W, int xpitch, const uint4* __restrict__ w,
                                                  float* __restrict__ yb, int Wo, int ypitch, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, float descale, int relu, int* __restrict__ overflow_flag,
                                                  int Cin, int Cout, int H, int Ho, int ho0, int wo0, int co0) {
  constexpr int P = KS / 2;                                  // padding
  constexpr int TWB = 32 * NT;                               // output columns per block
  constexpr int R = S * (C16_TH - 1) + KS;                   // staged input rows
  constexpr int WC = S * (TWB - 1) + KS;                     // staged input columns
  constexpr int WCH = (WC + 1) / 2;                          // stride 2: where the odd columns of a row begin
  constexpr int WP = S == 2 ? 2 * WCH : WC;                  // row pitch, in 16-byte units
  constexpr int PLN = R * WP;                                // one (part, channel half) plane
  constexpr int COT = 32 * MT;
  constexpr int TAPS = KS * KS;
  __shared__ uint4 xs[4 * PLN];
  __shared__ uint4 wl[TAPS * 4 * COT];
  static_assert(sizeof(uint4) * (4 * PLN + TAPS * 4 * COT) <= 65536, "static LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int gh0 = S * ho0 - P, gw0 = S * wo0 - P;
  const int hw = H * xpitch;                                 // channel pitch

  c16_f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // a staging unit = the eight channels of one channel half at one pixel of the halo tile: eight loads (each coalesced along the row over
  // the lanes; scalar floats, so an image may begin on any column), one 16-byte LDS store per part
  constexpr int NXU = 2 * R * WC, NX = (NXU + 255) / 256;
  constexpr int NWU = TAPS * 4 * COT, NW = (NWU + 255) / 256;
  float xr[NX][8];
  uint4 wr[NW];
  const auto fetch = [&](int ci0) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int u = tid + 256 * k;
      const int half = u / (R * WC), rem = u - half * (R * WC), r = rem / WC, c = rem - r * WC;
      const int gh = gh0 + r, gw = gw0 + c;
      const bool in = u < NXU && gh >= 0 && gh < H && gw >= 0 && gw < W;
      const float* px = xb + (in ? ((ci0 + 8 * half) * H + gh) * xpitch + gw : 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) xr[k][j] = in ? px[j * hw] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int u = tid + 256 * k;
      const int part = u / COT, r = u - part * COT;
      wr[k] = make_uint4(0, 0, 0, 0);
      if (u < NWU) wr[k] = w[((size_t)(ci0 / C16_CI) * (TAPS * 4) + part) * Cout + co0 + r];
    }
  };
  bool bad = false;
  fetch(0);
  for (int ci0 = 0; ci0 < Cin; ci0 += C16_CI) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int u = tid + 256 * k;
      const int half = u / (R * WC), rem = u - half * (R * WC), r = rem / WC, c = rem - r * WC;
      if (u < NXU) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x0 = xr[k][2 * j], x1 = xr[k][2 * j + 1];
          bad |= !(__builtin_fabsf(x0) < SAT_CONV2D16_SPLIT_LIMIT) | !(__builtin_fabsf(x1) < SAT_CONV2D16_SPLIT_LIMIT);
          const auto h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
          const auto l = __builtin_amdgcn_cvt_pkrtz(x0 - (float)h[0], x1 - (float)h[1]);
          hi[j] = __builtin_bit_cast(unsigned, h);
          lo[j] = __builtin_bit_cast(unsigned, l);
        }
        const int cp = S == 2 ? (c & 1) * WCH + (c >> 1) : c;
        xs[(0 + half) * PLN + r * WP + cp] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        xs[(2 + half) * PLN + r * WP + cp] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
      }
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int u = tid + 256 * k;
      if (u < NWU) wl[u] = wr[k];
    }
    __syncthreads();
    if (ci0 + C16_CI < Cin) fetch(ci0 + C16_CI);
    const uint4* xa = xs + lh * PLN + (S * wave) * WP + l31;
    const uint4* wa = wl + lh * COT + l31;
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int tap = kh * KS + kw;
        // column S (32 n + l31) + kw of the tile -> its unit in the row
        const int c0 = S == 2 ? (kw & 1) * WCH + (kw >> 1) : kw;
        c16_h8 a_hi[MT], a_lo[MT], b_hi[NT], b_lo[NT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          a_hi[m] = __builtin_bit_cast(c16_h8, wa[(tap * 4 + 0) * COT + 32 * m]);
          a_lo[m] = __builtin_bit_cast(c16_h8, wa[(tap * 4 + 2) * COT + 32 * m]);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          b_hi[n] = __builtin_bit_cast(c16_h8, xa[kh * WP + c0 + 32 * n]);
          b_lo[n] = __builtin_bit_cast(c16_h8, xa[2 * PLN + kh * WP + c0 + 32 * n]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[m], b_hi[n], acc[m][n], 0, 0, 0);
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[m], b_lo[n], acc[m][n], 0, 0, 0);
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[m], b_hi[n], acc[m][n], 0, 0, 0);
          }
      }
    __syncthreads();
  }

  // a value of this image that could not be split: reported by a plain atomic of a vector lane (never a clear: the caller owns the flag)
  if (bad && overflow_flag) atomicOr(overflow_flag, 1);

  const int ho = ho0 + wave;
  if (ho >= Ho) return;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int wo = wo0 + 32 * n + l31;
    if (wo >= Wo) continue;
    float* yp = yb + (size_t)ho * ypitch + wo;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float v = acc[m][n][r] * descale;
        if (scale) v = v * scale[co] + shift[co];
        if (relu) v = fmaxf(v, 0.f);
        yp[(size_t)co * Ho * ypitch] = v;
      }
  }
}

}  // namespace sat
