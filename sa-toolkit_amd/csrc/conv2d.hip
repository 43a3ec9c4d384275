// Kernels of the ResNet x-vector extractor (half-ResNet34 with squeeze-excitation, attentive pooling with global context).
// Reference: egs/asv/voxceleb/local/tuning/resnet.py:17-79, satools/satools/sidekit/archi.py:81-119 (PreHalfResNet34),
// sidekit/nn.py:12-68 (SELayer, ResNetBasicBlock), sidekit/pooling.py:11-37 (MeanStdPooling) and :90-138 (AttentivePooling).
//
// Images are [B][C][H][W] with W contiguous.  The net keeps TIME on W and frequency on H (the reference runs [B, C, T, F]: a 3x3
// conv commutes with transposing both the image and the kernel, so the weights are transposed once when they are packed and the
// [B][256][10][T'] output IS the [B][2560][T'] tensor the pooling reads).  The kernels themselves do not care which axis is which.
// The bodies of the convs and of the pooling are in csrc/conv2d_tile.h, which the segment forms of csrc/ragged2d/ share.
#include "conv2d_tile.h"

namespace sat {

// The MFMA conv's tile body (csrc/conv2d_tile.h: the tiles, the LDS images and the order of the sum) with a block per (utterance, 32 MT
// output channels, C2_TH x C2_TW output pixels): the image is utterance b, its rows W / Wo apart.
template <int KS, int S, int MT>
__global__ void __launch_bounds__(256) conv2d_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                          const float* __restrict__ scale, const float* __restrict__ shift, int Cin, int Cout,
                                                          int H, int W, int Ho, int Wo, int row_tiles, int relu) {
  const int b = blockIdx.z;
  const int rt = blockIdx.y % row_tiles, ct = blockIdx.y / row_tiles;
  const int ho0 = rt * C2_TH, wo0 = blockIdx.x * C2_TW, co0 = ct * (32 * MT);
  const float* xb = x + (size_t)b * Cin * H * W;
  // the rows are W / Wo apart: the body's pitches are these very variables, not copies of them (the compiler takes the index factor for
  // positive only where it is the variable of the column test `gw < W`), and the output base is formed where the body uses it, behind
  // the K loop, not carried through it (csrc/conv2d_tile.h)
#define xpitch W
#define ypitch Wo
#define yb (y + (size_t)b * Cout * Ho * Wo)
#include "conv2d_tile_body.h"
#undef xpitch
#undef ypitch
#undef yb
}

// The stem, Conv2d(1, 32, 3, padding 1, stride 1): the stem body (csrc/conv2d_tile.h) with a thread per output pixel of utterance b
__global__ void __launch_bounds__(256) conv2d_stem_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                          const float* __restrict__ scale, const float* __restrict__ shift, int H, int W,
                                                          int relu) {
  // (the pitches and the bases as in conv2d_mfma_kernel: the variables themselves, the bases formed where the body uses them)
#define xpitch W
#define ypitch W
#define xb (x + (size_t)(int)blockIdx.z * H * W)
#define yb (y + (size_t)(int)blockIdx.z * C2_STEM_CO * H * W)
#include "conv2d_stem_body.h"
#undef xpitch
#undef ypitch
#undef xb
#undef yb
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

// MeanStdPooling (sidekit/pooling.py:33-37): per (b, c) row of [B][C][T] the mean and the UNBIASED standard deviation over T (torch.std),
// by row_mean_sqdev_wave; out [B][2C]: means then deviations.  One wave per row.
__global__ void __launch_bounds__(256) row_mean_std_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int T) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B * C) return;
  float mean, q;
  row_mean_sqdev_wave(x + (size_t)r * T, T, lane, &mean, &q);
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
