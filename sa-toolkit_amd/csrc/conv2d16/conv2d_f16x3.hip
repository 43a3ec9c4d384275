// Split-f16 form of the 2-D convolutions of the ResNet x-vector extractor (include/satools_hip_conv2d16.h): the semantics of
// sat_conv2d_f32 (csrc/conv2d.hip) with every product computed as w_lo x_hi + w_hi x_lo + w_hi x_hi on v_mfma_f32_32x32x16_f16.
// Images are [B][C][H][W] with W contiguous; the kernel does not care which axis is time.
#include "../conv2d16_tile.h"

namespace sat {

[[maybe_unused]] constexpr int C16_KERNELS = 6;  // instantiations the entry point dispatches to (tests/test_codegen_conv2d16.py counts them)

// conv2d_f16x3_tile (csrc/conv2d16_tile.h: the tiles, the LDS images and the order of the sum) with a block per (utterance, 32 MT output
// channels, C16_TH x 32 NT output pixels): the image is utterance b of [B][C][H][W], its rows W / Wo apart.
template <int KS, int S, int MT, int NT>
__global__ void __launch_bounds__(256) conv2d_f16x3_kernel(const float* __restrict__ x, const uint4* __restrict__ w, float* __restrict__ y,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, float descale,
                                                           int* __restrict__ overflow_flag, int Cin, int Cout, int H, int W, int Ho, int Wo,
                                                           int row_tiles, int relu) {
  const int b = blockIdx.z;
  const int rt = blockIdx.y % row_tiles, ct = blockIdx.y / row_tiles;
  conv2d_f16x3_tile<KS, S, MT, NT>(x + (size_t)b * Cin * (H * W), W, W, w, y + (size_t)b * Cout * Ho * Wo, Wo, Wo, scale, shift, descale, relu,
                                   overflow_flag, Cin, Cout, H, Ho, rt * C16_TH, blockIdx.x * (32 * NT), ct * (32 * MT));
}

template <int KS, int S, int MT, int NT>
static int launch_conv2d16(const float* x, const void* w, float descale, float* y, const float* scale, const float* shift, int B, int Cin,
                           int Cout, int H, int W, int Ho, int Wo, int relu, int* flag, hipStream_t stream) {
  const int row_tiles = ceil_div(Ho, C16_TH);
  const dim3 grid(ceil_div(Wo, 32 * NT), row_tiles * (Cout / (32 * MT)), B);
  hipLaunchKernelGGL((conv2d_f16x3_kernel<KS, S, MT, NT>), grid, dim3(256), 0, stream, x, (const uint4*)w, y, scale, shift, descale, flag, Cin,
                     Cout, H, W, Ho, Wo, row_tiles, relu);
  SAT_LAUNCH_CHECK("conv2d_f16x3_kernel");
  return SAT_OK;
}

}  // namespace sat

using namespace sat;

extern "C" int sat_conv2d_f16x3_f32(const float* x, const void* w_split, float w_descale, float* y, const float* ch_scale,
                                    const float* ch_shift, int relu, int B, int Cin, int Cout, int H, int W, int ksize, int stride,
                                    int32_t* overflow_flag, void* stream) {
  SAT_REQUIRE(x && w_split && y && x != y, "conv2d_f16x3: null pointer, or y aliases x");
  SAT_REQUIRE((ch_scale != nullptr) == (ch_shift != nullptr), "conv2d_f16x3: ch_scale and ch_shift come together");
  SAT_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "conv2d_f16x3: B = %d (1 .. 65535), H = %d, W = %d", B, H, W);
  SAT_REQUIRE((ksize == 3 || ksize == 1) && (stride == 1 || stride == 2),
              "conv2d_f16x3: ksize %d / stride %d (3x3 with padding 1 or 1x1, stride 1 or 2)", ksize, stride);
  SAT_REQUIRE(w_descale > 0.f && w_descale < __builtin_inff(), "conv2d_f16x3: w_descale = %g (the finite, positive 2^-e of the packing)",
              (double)w_descale);
  const auto ok = [](int c) { return c == 32 || c == 64 || c == 128 || c == 256; };
  SAT_REQUIRE(ok(Cin) && ok(Cout), "conv2d_f16x3: Cin = %d / Cout = %d (32, 64, 128 or 256; the Cin = 1 stem stays on sat_conv2d_f32)", Cin,
              Cout);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  SAT_REQUIRE((long long)Cin * H * W < (1ll << 31) && (long long)Cout * Ho * Wo < (1ll << 31),
              "conv2d_f16x3: an utterance's image exceeds 2^31 elements");
  // stride 1: 4 x 64 output pixels per block; stride 2: 4 x 32 and 32 output channels (its halo tile is four times the size per output)
  const int mt = (Cout == 32 || stride == 2) ? 1 : 2;
  SAT_REQUIRE((long long)ceil_div(Ho, C16_TH) * (Cout / (32 * mt)) <= 65535, "conv2d_f16x3: H = %d exceeds the grid", H);
  hipStream_t st = (hipStream_t)stream;
#define SAT_C16(KS_, S_, MT_, NT_) \
  launch_conv2d16<KS_, S_, MT_, NT_>(x, w_split, w_descale, y, ch_scale, ch_shift, B, Cin, Cout, H, W, Ho, Wo, relu, overflow_flag, st)
  if (ksize == 3) {
    if (stride == 2) return SAT_C16(3, 2, 1, 1);
    return mt == 1 ? SAT_C16(3, 1, 1, 2) : SAT_C16(3, 1, 2, 2);
  }
  if (stride == 2) return SAT_C16(1, 2, 1, 1);
  return mt == 1 ? SAT_C16(1, 1, 1, 2) : SAT_C16(1, 1, 2, 2);
#undef SAT_C16
}
