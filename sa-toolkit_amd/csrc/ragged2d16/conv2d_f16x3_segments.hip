// Segment form of the split-f16 2-D convolution (csrc/conv2d16/conv2d_f16x3.hip) for a RAGGED batch on a packed time axis
// (include/satools_hip_ragged2d16.h; the layout is the one of include/satools_hip_ragged2d.h: B utterances of unequal length side by side in
// one image [C][H][T_tot], time innermost, segment i at columns off_i .. off_i + T_i - 1 of every row, gap columns that hold anything).
// The kernel runs the per-call kernel's tile body (csrc/conv2d16_tile.h) on each segment, so that segment i of its result has the bits of
// sat_conv2d_f16x3_f32 on utterance i alone; the body selects on load (a gap column or another segment never reaches an output or an
// overflow flag, NaN included), and the kernel skips what a wrong table names (csrc/segments.h).
#include "../conv2d16_tile.h"
#include "../segments.h"
#include "../../../include/satools_hip_ragged2d16.h"

namespace sat {

[[maybe_unused]] constexpr int R16_KERNELS = 6;  // instantiations the entry point dispatches to (tests/test_codegen_xvector_resnet_ragged16.py counts them)

// conv2d_f16x3_tile with a block per (segment, 32 MT output channels, C16_TH x 32 NT output pixels in the segment's own coordinates): the
// image's width is the segment's W, on the loads (the padding at the utterance's own ends, whatever the gap or the neighbour holds) and on
// the stores alike; rows are T_in / T_out apart; a value of THIS segment that could not be split goes to the segment's own flag (seg < B,
// the grid's z extent).
// The grid's x extent comes from max_len; a block past its segment's last tile leaves before the first barrier (block-uniform).
template <int KS, int S, int MT, int NT>
__global__ void __launch_bounds__(256) conv2d_segments_f16x3_kernel(const float* __restrict__ x, const uint4* __restrict__ w, float* __restrict__ y,
                                                                    const float* __restrict__ scale, const float* __restrict__ shift, float descale,
                                                                    int* __restrict__ overflow_flags, const int* __restrict__ in_off,
                                                                    const int* __restrict__ in_len, const int* __restrict__ out_off, int Cin, int Cout,
                                                                    int H, int T_in, int Ho, int T_out, int max_len, int row_tiles, int relu) {
  const int seg = blockIdx.z;
  int in, W, out, Wo;
  if (!ragged_conv_segment(in_off, in_len, out_off, seg, T_in, T_out, max_len, S, &in, &W, &out, &Wo)) return;
  const int wo0 = blockIdx.x * (32 * NT);
  if (wo0 >= Wo) return;
  const int rt = blockIdx.y % row_tiles, ct = blockIdx.y / row_tiles;
  conv2d_f16x3_tile<KS, S, MT, NT>(x + in, W, T_in, w, y + out, Wo, T_out, scale, shift, descale, relu,
                                   overflow_flags ? overflow_flags + seg : nullptr, Cin, Cout, H, Ho, rt * C16_TH, wo0, ct * (32 * MT));
}

template <int KS, int S, int MT, int NT>
static int launch_conv2d16_segments(const float* x, const void* w, float descale, float* y, const float* scale, const float* shift,
                                    const int32_t* in_off, const int32_t* in_len, const int32_t* out_off, int B, int Cin, int Cout, int H, int T_in,
                                    int Ho, int T_out, int max_len, int relu, int* flags, hipStream_t stream) {
  const int row_tiles = ceil_div(Ho, C16_TH);
  const dim3 grid(ceil_div((max_len - 1) / S + 1, 32 * NT), row_tiles * (Cout / (32 * MT)), B);
  hipLaunchKernelGGL((conv2d_segments_f16x3_kernel<KS, S, MT, NT>), grid, dim3(256), 0, stream, x, (const uint4*)w, y, scale, shift, descale, flags,
                     in_off, in_len, out_off, Cin, Cout, H, T_in, Ho, T_out, max_len, row_tiles, relu);
  SAT_LAUNCH_CHECK("conv2d_segments_f16x3_kernel");
  return SAT_OK;
}

}  // namespace sat

using namespace sat;

extern "C" int sat_conv2d_f16x3_segments_f32(const float* x, const void* w_split, float w_descale, float* y, const float* ch_scale,
                                             const float* ch_shift, int relu, const int32_t* in_off, const int32_t* in_len, const int32_t* out_off,
                                             int B, int max_len, int Cin, int Cout, int H, int T_in, int T_out, int ksize, int stride,
                                             int32_t* overflow_flags, void* stream) {
  SAT_REQUIRE(x && w_split && y && x != y, "conv2d_f16x3_segments: null pointer, or y aliases x");
  SAT_REQUIRE((ch_scale != nullptr) == (ch_shift != nullptr), "conv2d_f16x3_segments: ch_scale and ch_shift come together");
  SAT_REQUIRE(in_off && in_len && out_off && B >= 1 && B <= SAT_RAGGED_MAX_SEGMENTS,
              "conv2d_f16x3_segments: the three segment tables and 1 .. %d segments are needed, got B = %d", SAT_RAGGED_MAX_SEGMENTS, B);
  SAT_REQUIRE(T_in >= 1 && T_out >= 1 && H > 0, "conv2d_f16x3_segments: T_in = %d, T_out = %d, H = %d", T_in, T_out, H);
  SAT_REQUIRE(max_len >= 1 && max_len <= T_in, "conv2d_f16x3_segments: max_len = %d (the longest segment: 1 .. T_in = %d)", max_len, T_in);
  SAT_REQUIRE((ksize == 3 || ksize == 1) && (stride == 1 || stride == 2),
              "conv2d_f16x3_segments: ksize %d / stride %d (3x3 with padding 1 or 1x1, stride 1 or 2)", ksize, stride);
  SAT_REQUIRE(w_descale > 0.f && w_descale < __builtin_inff(), "conv2d_f16x3_segments: w_descale = %g (the finite, positive 2^-e of the packing)",
              (double)w_descale);
  const auto ok = [](int c) { return c == 32 || c == 64 || c == 128 || c == 256; };
  SAT_REQUIRE(ok(Cin) && ok(Cout),
              "conv2d_f16x3_segments: Cin = %d / Cout = %d (32, 64, 128 or 256; the Cin = 1 stem stays on sat_conv2d_segments_f32)", Cin, Cout);
  const int Ho = (H - 1) / stride + 1;
  SAT_REQUIRE((long long)Cin * H * T_in < (1ll << 31) && (long long)Cout * Ho * T_out < (1ll << 31),
              "conv2d_f16x3_segments: an image exceeds 2^31 elements");
  // the per-call kernel's tiles: stride 1: 4 x 64 output pixels per block; stride 2: 4 x 32 and 32 output channels
  const int mt = (Cout == 32 || stride == 2) ? 1 : 2;
  SAT_REQUIRE((long long)ceil_div(Ho, C16_TH) * (Cout / (32 * mt)) <= 65535, "conv2d_f16x3_segments: H = %d exceeds the grid", H);
  hipStream_t st = (hipStream_t)stream;
#define SAT_R16(KS_, S_, MT_, NT_)                                                                                                               \
  launch_conv2d16_segments<KS_, S_, MT_, NT_>(x, w_split, w_descale, y, ch_scale, ch_shift, in_off, in_len, out_off, B, Cin, Cout, H, T_in, Ho, T_out, \
                                              max_len, relu, overflow_flags, st)
  if (ksize == 3) {
    if (stride == 2) return SAT_R16(3, 2, 1, 1);
    return mt == 1 ? SAT_R16(3, 1, 1, 2) : SAT_R16(3, 1, 2, 2);
  }
  if (stride == 2) return SAT_R16(1, 2, 1, 1);
  return mt == 1 ? SAT_R16(1, 1, 1, 2) : SAT_R16(1, 1, 2, 2);
#undef SAT_R16
}
