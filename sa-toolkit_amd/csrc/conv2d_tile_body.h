// The tile body of conv2d_mfma_kernel (csrc/conv2d.hip) and conv2d_segments_mfma_kernel (csrc/ragged2d/resnet_ragged.hip): statements, not
// declarations, #included INSIDE each kernel (csrc/conv2d_tile.h says what they do, and why they are expanded in place and not called).
// No include guard.  In scope where it is included, as variables or as macros for expressions: the template parameters KS, S, MT and
//   const float* xb; int W, xpitch;      the image [Cin][H][xpitch], columns 0 .. W - 1 its own
//   float* yb; int Wo, ypitch;           the result [Cout][Ho][ypitch], columns 0 .. Wo - 1 written
//   const float *w, *scale, *shift; int relu, Cin, Cout, H, Ho;
//   int ho0, wo0, co0;                   the block's first output row, column and channel
// Every thread of the block reaches it (two barriers per chunk): a kernel's early returns are block-uniform and come before it.
{
  constexpr int P = KS / 2;                                  // padding
  constexpr int R = S * (C2_TH - 1) + KS;                    // staged input rows
  constexpr int WC = S * (C2_TW - 1) + KS;                   // staged input columns
  constexpr int WP = WC | 1;                                 // odd row pitch
  constexpr int PL = R * WP + ((R * WP) % 2 == 0 ? 1 : 0);   // odd plane pitch: the two lane halves read planes ci and ci + 1
  constexpr int COT = 32 * MT;
  constexpr int TAPS = KS * KS;
  __shared__ float xs[C2_CI * PL];
  __shared__ float wl[TAPS * C2_CI * COT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int gh0 = S * ho0 - P, gw0 = S * wo0 - P;

  c2_f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  // the chunk's elements of this thread travel through registers: all loads of a chunk are in flight together, and the NEXT chunk's
  // are issued before this chunk's MFMAs and stored to LDS after them (a load per loop turn behind its LDS store left every block waiting
  // a global round trip per element: 13.3 ms per batch of 32 utterances against 10.3 for the same net in torch)
  constexpr int NXE = C2_CI * R * WC, NX = (NXE + 255) / 256;
  constexpr int NW = TAPS * C2_CI * COT / 256;
  static_assert(TAPS * C2_CI * COT % 256 == 0, "a whole number of weight elements per thread");
  float xr[NX], wr[NW];
  const auto fetch = [&](int ci0) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int i = tid + 256 * k;
      const int ci = i / (R * WC), rem = i - ci * (R * WC), r = rem / WC, c = rem - r * WC;
      const int gh = gh0 + r, gw = gw0 + c;
      float v = 0.f;
      if (i < NXE && gh >= 0 && gh < H && gw >= 0 && gw < W) v = xb[((size_t)(ci0 + ci) * H + gh) * xpitch + gw];
      xr[k] = v;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int i = tid + 256 * k;
      const int tap = i / (C2_CI * COT), rem = i - tap * (C2_CI * COT), ci = rem / COT, co = rem - ci * COT;
      wr[k] = w[((size_t)tap * Cin + ci0 + ci) * Cout + co0 + co];
    }
  };
  fetch(0);
  for (int ci0 = 0; ci0 < Cin; ci0 += C2_CI) {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int i = tid + 256 * k;
      const int ci = i / (R * WC), rem = i - ci * (R * WC), r = rem / WC, c = rem - r * WC;
      if (i < NXE) xs[ci * PL + r * WP + c] = xr[k];
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) wl[tid + 256 * k] = wr[k];
    __syncthreads();
    if (ci0 + C2_CI < Cin) fetch(ci0 + C2_CI);
    const float* xa = xs + lh * PL + (S * wave) * WP + S * l31;
    const float* wa = wl + lh * COT + l31;
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw)
#pragma unroll
        for (int kk = 0; kk < C2_CI / 2; ++kk) {
          const float bv = xa[2 * kk * PL + kh * WP + kw];
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const float av = wa[((kh * KS + kw) * C2_CI + 2 * kk) * COT + 32 * m];
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[m], 0, 0, 0);
          }
        }
    __syncthreads();
  }

  const int ho = ho0 + wave, wo = wo0 + l31;
  if (ho >= Ho || wo >= Wo) return;
  float* yp = yb + (size_t)ho * ypitch + wo;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * lh;
      float v = acc[m][r];
      if (scale) v = v * scale[co] + shift[co];
      if (relu) v = fmaxf(v, 0.f);
      yp[(size_t)co * Ho * ypitch] = v;
    }
}
