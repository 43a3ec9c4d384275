// Kernels of the ResNet x-vector extractor (half-ResNet34 with squeeze-excitation, attentive pooling with global context).
// Reference: egs/asv/voxceleb/local/tuning/resnet.py:17-79, satools/satools/sidekit/archi.py:81-119 (PreHalfResNet34),
// sidekit/nn.py:12-68 (SELayer, ResNetBasicBlock), sidekit/pooling.py:11-37 (MeanStdPooling) and :90-138 (AttentivePooling).
//
// Images are [B][C][H][W] with W contiguous.  The net keeps TIME on W and frequency on H (the reference runs [B, C, T, F]: a 3x3
// conv commutes with transposing both the image and the kernel, so the weights are transposed once when they are packed and the
// [B][256][10][T'] output IS the [B][2560][T'] tensor the pooling reads).  The kernels themselves do not care which axis is which.
#include "common.h"

namespace sat {

typedef float c2_f32x16 __attribute__((ext_vector_type(16)));

constexpr int C2_TH = 4;     // output rows per block: one per wave
constexpr int C2_TW = 32;    // output columns per block: the N of one 32x32 MFMA tile
constexpr int C2_CI = 8;     // input channels per staged chunk: four k-steps of v_mfma_f32_32x32x2_f32 per tap

// Conv2d (bias=False; KS = 3 with padding 1 or KS = 1 with padding 0; stride S in both axes) as an implicit GEMM on the exact f32 MFMA:
// M = output channels (A = weights), N = 32 output pixels of one row (B = input pixels shifted by the tap), K = (tap, input channel).
// A block owns one utterance, 32 MT output channels and C2_TH x C2_TW output pixels.  For every chunk of C2_CI input channels it stages
// the halo tile of x (zero outside the image: the padding) and the chunk's weights [tap][ci][co] in LDS (through registers, the next
// chunk's loads in flight behind this chunk's MFMAs); wave w computes output row w:
// per (tap, channel pair) one B fragment and MT A fragments from LDS, MT MFMAs.  The sum over K runs in ONE fixed order (chunk, tap,
// channel pair; no atomics, no split K): the same input gives the same bits.
// Epilogue: v = acc * scale[co] + shift[co] (the BatchNorm in eval, after the sum as the reference applies it), optional ReLU.
template <int KS, int S, int MT>
__global__ void __launch_bounds__(256) conv2d_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                          const float* __restrict__ scale, const float* __restrict__ shift, int Cin, int Cout,
                                                          int H, int W, int Ho, int Wo, int row_tiles, int relu) {
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
  const int b = blockIdx.z;
  const int rt = blockIdx.y % row_tiles, ct = blockIdx.y / row_tiles;
  const int ho0 = rt * C2_TH, wo0 = blockIdx.x * C2_TW, co0 = ct * COT;
  const int gh0 = S * ho0 - P, gw0 = S * wo0 - P;
  const float* xb = x + (size_t)b * Cin * H * W;

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
      if (i < NXE && gh >= 0 && gh < H && gw >= 0 && gw < W) v = xb[((size_t)(ci0 + ci) * H + gh) * W + gw];
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
  float* yb = y + (size_t)b * Cout * Ho * Wo + (size_t)ho * Wo + wo;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * lh;
      float v = acc[m][r];
      if (scale) v = v * scale[co] + shift[co];
      if (relu) v = fmaxf(v, 0.f);
      yb[(size_t)co * Ho * Wo] = v;
    }
}

// The stem: Conv2d(1, 32, 3, padding 1, stride 1).  K = 9 does not feed a matrix core; one thread per output pixel keeps its nine
// inputs in registers and walks the 32 output channels (weights [tap][co]: wave-uniform reads), an fmaf chain over the taps in order.
constexpr int C2_STEM_CO = 32;
__global__ void __launch_bounds__(256) conv2d_stem_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                          const float* __restrict__ scale, const float* __restrict__ shift, int H, int W,
                                                          int relu) {
  __shared__ float ws[9 * C2_STEM_CO], s_sc[C2_STEM_CO], s_sh[C2_STEM_CO];
  for (int i = threadIdx.x; i < 9 * C2_STEM_CO; i += 256) ws[i] = w[i];
  if (threadIdx.x < C2_STEM_CO) {
    s_sc[threadIdx.x] = scale ? scale[threadIdx.x] : 1.f;
    s_sh[threadIdx.x] = scale ? shift[threadIdx.x] : 0.f;
  }
  __syncthreads();
  const int wo = blockIdx.x * 256 + threadIdx.x, ho = blockIdx.y, b = blockIdx.z;
  if (wo >= W) return;
  const float* xb = x + (size_t)b * H * W;
  float in[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int gh = ho - 1 + kh, gw = wo - 1 + kw;
      in[kh * 3 + kw] = (gh >= 0 && gh < H && gw >= 0 && gw < W) ? xb[(size_t)gh * W + gw] : 0.f;
    }
  float* yb = y + (size_t)b * C2_STEM_CO * H * W + (size_t)ho * W + wo;
#pragma unroll 4
  for (int co = 0; co < C2_STEM_CO; ++co) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) v = __builtin_fmaf(ws[t * C2_STEM_CO + co], in[t], v);
    if (scale) v = v * s_sc[co] + s_sh[co];
    if (relu) v = fmaxf(v, 0.f);
    yb[(size_t)co * H * W] = v;
  }
}

// The tail of ResNetBasicBlock.forward (sidekit/nn.py:63-68): y = relu(z * sigmoid(g[b][c]) + r) on [B][C][N] (N = H W)
__global__ void __launch_bounds__(256) se_scale_add_relu_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                                const float* __restrict__ r, float* __restrict__ y, int C, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int ch = blockIdx.y, bt = blockIdx.z;
  if (n >= N) return;
  const size_t i = ((size_t)bt * C + ch) * N + n;
  const float gate = 1.0f / (1.0f + expf(-g[(size_t)bt * C + ch]));
  const float v = z[i] * gate + r[i];
  y[i] = fmaxf(v, 0.f);
}

__device__ __forceinline__ float c2_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// MeanStdPooling (sidekit/pooling.py:33-37): per (b, c) row of [B][C][T] the mean and the UNBIASED standard deviation over T (torch.std),
// the deviation summed around the mean in a second pass; out [B][2C]: means then deviations.  One wave per row.
__global__ void __launch_bounds__(256) row_mean_std_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int T) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B * C) return;
  const float* xr = x + (size_t)r * T;
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += xr[t];
  const float mean = c2_wave_sum(s) / (float)T;
  float q = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float d = xr[t] - mean;
    q = __builtin_fmaf(d, d, q);
  }
  q = c2_wave_sum(q);
  if (lane == 0) {
    const int b = r / C, c = r - b * C;
    out[(size_t)b * 2 * C + c] = mean;
    out[(size_t)b * 2 * C + C + c] = sqrtf(q / (float)(T - 1));
  }
}

template <int KS, int S, int MT>
static int launch_conv2d(const float* x, const float* w, float* y, const float* scale, const float* shift, int B, int Cin, int Cout, int H,
                         int W, int Ho, int Wo, int relu, hipStream_t stream) {
  const int row_tiles = ceil_div(Ho, C2_TH);
  const dim3 grid(ceil_div(Wo, C2_TW), row_tiles * (Cout / (32 * MT)), B);
  hipLaunchKernelGGL((conv2d_mfma_kernel<KS, S, MT>), grid, dim3(256), 0, stream, x, w, y, scale, shift, Cin, Cout, H, W, Ho, Wo, row_tiles,
                     relu);
  SAT_LAUNCH_CHECK("conv2d_mfma_kernel");
  return SAT_OK;
}

}  // namespace sat

using namespace sat;

extern "C" int sat_conv2d_f32(const float* x, const float* w_packed, float* y, const float* ch_scale, const float* ch_shift, int relu, int B,
                              int Cin, int Cout, int H, int W, int ksize, int stride, void* stream) {
  SAT_REQUIRE(x && w_packed && y && x != y, "conv2d: null pointer, or y aliases x");
  SAT_REQUIRE((ch_scale != nullptr) == (ch_shift != nullptr), "conv2d: ch_scale and ch_shift come together");
  SAT_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "conv2d: B = %d (1 .. 65535), H = %d, W = %d", B, H, W);
  SAT_REQUIRE((ksize == 3 || ksize == 1) && (stride == 1 || stride == 2), "conv2d: ksize %d / stride %d (3x3 with padding 1 or 1x1, stride 1 or 2)",
              ksize, stride);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  SAT_REQUIRE((long long)Cin * H * W < (1ll << 31) && (long long)Cout * Ho * Wo < (1ll << 31), "conv2d: an utterance's image exceeds 2^31 elements");
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 1) {
    SAT_REQUIRE(Cout == C2_STEM_CO && ksize == 3 && stride == 1, "conv2d: Cin = 1 is the stem only (Cout = 32, 3x3, stride 1), got Cout = %d, ksize %d, stride %d",
                Cout, ksize, stride);
    SAT_REQUIRE(H <= 65535, "conv2d: H = %d exceeds the grid", H);
    hipLaunchKernelGGL(conv2d_stem_kernel, dim3(ceil_div(W, 256), H, B), dim3(256), 0, st, x, w_packed, y, ch_scale, ch_shift, H, W, relu);
    SAT_LAUNCH_CHECK("conv2d_stem_kernel");
    return SAT_OK;
  }
  const auto ok = [](int c) { return c == 32 || c == 64 || c == 128 || c == 256; };
  SAT_REQUIRE(ok(Cin) && ok(Cout), "conv2d: Cin = %d / Cout = %d (32, 64, 128 or 256; Cin = 1 for the stem)", Cin, Cout);
  const int mt = Cout == 32 ? 1 : 2;
  SAT_REQUIRE((long long)ceil_div(Ho, C2_TH) * (Cout / (32 * mt)) <= 65535, "conv2d: H = %d exceeds the grid", H);
#define SAT_C2(KS_, S_)                                                                                                        \
  (mt == 1 ? launch_conv2d<KS_, S_, 1>(x, w_packed, y, ch_scale, ch_shift, B, Cin, Cout, H, W, Ho, Wo, relu, st)              \
           : launch_conv2d<KS_, S_, 2>(x, w_packed, y, ch_scale, ch_shift, B, Cin, Cout, H, W, Ho, Wo, relu, st))
  if (ksize == 3) return stride == 1 ? SAT_C2(3, 1) : SAT_C2(3, 2);
  return stride == 1 ? SAT_C2(1, 1) : SAT_C2(1, 2);
#undef SAT_C2
}

extern "C" int sat_se_scale_add_relu_f32(const float* z, const float* gate_logits, const float* r, float* y, int B, int C, int N, void* stream) {
  SAT_REQUIRE(z && gate_logits && r && y && B > 0 && C > 0 && N > 0 && B <= 65535 && C <= 65535, "se_scale_add_relu: bad arguments");
  hipLaunchKernelGGL(se_scale_add_relu_kernel, dim3(ceil_div(N, 256), C, B), dim3(256), 0, (hipStream_t)stream, z, gate_logits, r, y, C, N);
  SAT_LAUNCH_CHECK("se_scale_add_relu_kernel");
  return SAT_OK;
}

extern "C" int sat_row_mean_std_f32(const float* x, float* out, int B, int C, int T, void* stream) {
  SAT_REQUIRE(x && out && B > 0 && C > 0 && (long long)B * C < (1ll << 31) - 4, "row_mean_std: bad arguments");
  SAT_REQUIRE(T >= 2, "row_mean_std: the unbiased deviation of %d value(s) is not a number (T >= 2)", T);
  hipLaunchKernelGGL(row_mean_std_kernel, dim3(ceil_div(B * C, 4)), dim3(256), 0, (hipStream_t)stream, x, out, B, C, T);
  SAT_LAUNCH_CHECK("row_mean_std_kernel");
  return SAT_OK;
}
