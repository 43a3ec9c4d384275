// The body of conv2d_stem_kernel (csrc/conv2d.hip) and conv2d_segments_stem_kernel (csrc/ragged2d/resnet_ragged.hip): statements, not
// declarations, #included INSIDE each kernel (csrc/conv2d_tile.h says what they do, and why they are expanded in place and not called).
// No include guard.  In scope where it is included, as variables or as macros for expressions:
//   const float* xb; int W, xpitch;      the image [H][xpitch], columns 0 .. W - 1 its own
//   float* yb; int ypitch;               the result [32][H][ypitch]
//   const float *w, *scale, *shift; int relu, H;
// The block's output row is blockIdx.y, the thread's column blockIdx.x * 256 + threadIdx.x.
// Every thread of the block reaches it (one barrier): a kernel's early returns are block-uniform and come before it.
{
  __shared__ float ws[9 * C2_STEM_CO], s_sc[C2_STEM_CO], s_sh[C2_STEM_CO];
  for (int i = threadIdx.x; i < 9 * C2_STEM_CO; i += 256) ws[i] = w[i];
  if (threadIdx.x < C2_STEM_CO) {
    s_sc[threadIdx.x] = scale ? scale[threadIdx.x] : 1.f;
    s_sh[threadIdx.x] = scale ? shift[threadIdx.x] : 0.f;
  }
  __syncthreads();
  const int wo = blockIdx.x * 256 + threadIdx.x, ho = blockIdx.y;
  if (wo >= W) return;
  float in[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int gh = ho - 1 + kh, gw = wo - 1 + kw;
      in[kh * 3 + kw] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[(size_t)gh * xpitch + gw] : 0.f;
    }
  float* yp = yb + (size_t)ho * ypitch + wo;
#pragma unroll 4
  for (int co = 0; co < C2_STEM_CO; ++co) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) v = __builtin_fmaf(ws[t * C2_STEM_CO + co], in[t], v);
    if (scale) v = v * s_sc[co] + s_sh[co];
    if (relu) v = fmaxf(v, 0.f);
    yp[(size_t)co * H * ypitch] = v;
  }
}
