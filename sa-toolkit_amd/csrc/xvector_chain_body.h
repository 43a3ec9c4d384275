// The statements of the Res2 chain's block (csrc/xvector_tile.h says what they compute and why they are statements and not a function),
// #included inside res2_chain_kernel<NT> (csrc/xvector.hip) and res2_chain_segments_kernel<NT> (csrc/ragged/xvector_ragged.hip).  The kernel
// provides: NT; yb, zb = row 0 of the utterance's input and output at its first column; T = its columns; t0 = the first column of this
// block's centre tile; R2_PITCH (a macro: the kernel's own variable) = the distance of two rows; w, scale, shift, nums, dil.
  extern __shared__ __attribute__((aligned(16))) float r2_lds[];
  constexpr int W = 64 * NT, WP = W + 2 * R2_MARG, TT = W - 2 * R2_HALO;
  float* bufA = r2_lds;                   // [64][WP] input of the current piece
  float* bufB = bufA + 64 * WP;           // [64][WP] its output (zero outside the utterance)
  float* wl = bufB + 64 * WP;             // [3][64][64] weights of the current piece
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int t_lo = t0 - R2_HALO;
  const int mt = wave >> 1, n0 = (wave & 1) * NT;      // this wave: rows 32 mt .., column tiles n0 .. n0 + NT - 1

  for (int i = tid; i < 64 * 2 * R2_MARG; i += 256) {  // the margins the shifted fragment reads touch: zero, never written again
    const int c = i / (2 * R2_MARG), m = i % (2 * R2_MARG);
    const int col = m < R2_MARG ? m : W + m;
    bufA[c * WP + col] = 0.f;
  }
  {
    float y0[64 * W / 256];
#pragma unroll
    for (int k = 0; k < 64 * W / 256; ++k) {
      const int i = tid + 256 * k, c = i / W, j = i - c * W, t = t_lo + j;
      y0[k] = (t >= 0 && t < T) ? yb[(size_t)c * R2_PITCH + t] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 64 * W / 256; ++k) {
      const int i = tid + 256 * k, c = i / W, j = i - c * W;
      bufA[c * WP + R2_MARG + j] = y0[k];
    }
  }
  constexpr int NIN = 64 * W / 256;                    // input elements per thread
  for (int p = 0; p < nums; ++p) {
    // (every global load of the piece is in flight before anything waits for one: a block is one wave per SIMD, nothing else hides them.
    // Requesting the weights one piece ahead, to wait in registers behind the MFMAs: 135 us against 116, not kept)
    float4 wv[12];
    const float4* w4 = (const float4*)(w + (size_t)p * 3 * 64 * 64);
#pragma unroll
    for (int k = 0; k < 12; ++k) wv[k] = w4[tid + 256 * k];
    float yn[NIN];                                     // piece p + 1 of y, added to this piece's output below
    const bool more = p + 1 < nums;
    {
      const float* yp = yb + (size_t)(p + 1) * 64 * R2_PITCH;
#pragma unroll
      for (int k = 0; k < NIN; ++k) {
        const int i = tid + 256 * k, c = i / W, j = i - c * W, t = t_lo + j;
        yn[k] = (more && t >= 0 && t < T) ? yp[(size_t)c * R2_PITCH + t] : 0.f;
      }
    }
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * lh;
      sc[r] = scale[p * 64 + co], sh[r] = shift[p * 64 + co];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) ((float4*)wl)[tid + 256 * k] = wv[k];
    __syncthreads();
    r2_f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    // 96 steps (tap, channel pair), four at a time: their fragment reads are issued together, so that one LDS round trip stands in front
    // of 4 NT MFMAs instead of NT
    const float* xa = bufA + R2_MARG + 32 * n0 + l31 + lh * WP;
    const float* wa = wl + 32 * mt + l31 + lh * 64;
    for (int tap = 0; tap < 3; ++tap) {
      const float* xt = xa + (tap - 1) * dil;
      const float* wt = wa + tap * 64 * 64;
#pragma unroll 2
      for (int ci = 0; ci < 64; ci += 8) {
        float a4[4], b4[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a4[u] = wt[(ci + 2 * u) * 64];
#pragma unroll
          for (int n = 0; n < NT; ++n) b4[u][n] = xt[(ci + 2 * u) * WP + 32 * n];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], b4[u][n], acc[n], 0, 0, 0);
      }
    }
    // relu, BatchNorm affine; the centre columns to memory, every column (zero outside the utterance) to bufB for the next piece
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int j = 32 * (n0 + n) + l31, t = t_lo + j;
      const bool inside = t >= 0 && t < T, keep = inside && j >= R2_HALO && j < R2_HALO + TT;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float v = fmaxf(acc[n][r], 0.f) * sc[r] + sh[r];
        bufB[co * WP + R2_MARG + j] = inside ? v : 0.f;
        if (keep) zb[(size_t)(p * 64 + co) * R2_PITCH + t] = v;
      }
    }
    __syncthreads();
    if (more) {
#pragma unroll
      for (int k = 0; k < NIN; ++k) {
        const int i = tid + 256 * k, c = i / W, j = i - c * W;
        bufA[c * WP + R2_MARG + j] = yn[k] + bufB[c * WP + R2_MARG + j];
      }
    }
  }
  // the piece the chain leaves untouched
  const float* yl = yb + (size_t)nums * 64 * R2_PITCH;
  float* zl = zb + (size_t)nums * 64 * R2_PITCH;
  for (int i = tid; i < 64 * TT; i += 256) {
    const int c = i / TT, t = t0 + (i - c * TT);
    if (t < T) zl[(size_t)c * R2_PITCH + t] = yl[(size_t)c * R2_PITCH + t];
  }
