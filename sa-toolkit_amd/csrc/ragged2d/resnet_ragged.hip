// Segment forms of the ResNet x-vector extractor's kernels (csrc/conv2d.hip) for a RAGGED batch on a packed time axis
// (include/satools_hip_ragged2d.h: B utterances of unequal length side by side in one image [C][H][T_tot], time innermost, segment i at
// columns off_i .. off_i + T_i - 1 of every row, gap columns between them that hold anything; one table per time resolution).  The convs and
// the pooling run the per-call kernels' own bodies (csrc/conv2d_tile.h) on each segment, the other two keep the order of operations of the
// kernel they come from, so that segment i of a result has the bits of the per-call kernel's result on utterance i alone; each selects on
// load (a gap column or another segment never reaches an output, NaN included) and skips what a wrong table names (csrc/segments.h).
#include "../conv2d_tile.h"
#include "../segments.h"
#include "../../../include/satools_hip_ragged2d.h"

namespace sat {

// the MFMA conv's tile body (csrc/conv2d_tile.h) with a block per (segment, 32 MT output channels, C2_TH x C2_TW output pixels of the segment): the image's width is the
// segment's W, on the loads (the padding at the utterance's own ends, whatever the gap or the neighbour holds) and on the stores alike;
// rows are T_in / T_out apart.
// The grid's x extent comes from max_len; a block past its segment's last tile leaves before the first barrier (block-uniform).
template <int KS, int S, int MT>
__global__ void __launch_bounds__(256) conv2d_segments_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   const int* __restrict__ in_off, const int* __restrict__ in_len,
                                                                   const int* __restrict__ out_off, int Cin, int Cout, int H, int T_in, int Ho,
                                                                   int T_out, int max_len, int row_tiles, int relu) {
  int in, W, out, Wo;
  if (!ragged_conv_segment(in_off, in_len, out_off, blockIdx.z, T_in, T_out, max_len, S, &in, &W, &out, &Wo)) return;
  const int wo0 = blockIdx.x * C2_TW;
  if (wo0 >= Wo) return;
  const int rt = blockIdx.y % row_tiles, ct = blockIdx.y / row_tiles;
  const int ho0 = rt * C2_TH, co0 = ct * (32 * MT);
  const int xpitch = T_in, ypitch = T_out;
  const float* xb = x + in;
  float* yb = y + out;
#include "../conv2d_tile_body.h"
}

// the stem body (csrc/conv2d_tile.h) per segment: one thread per output pixel of the segment
__global__ void __launch_bounds__(256) conv2d_segments_stem_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   const int* __restrict__ in_off, const int* __restrict__ in_len,
                                                                   const int* __restrict__ out_off, int H, int T_in, int T_out, int max_len,
                                                                   int relu) {
  int in, W, out, Wo;
  // (block-uniform: nothing below is reached by a part of the block)
  if (!ragged_conv_segment(in_off, in_len, out_off, blockIdx.z, T_in, T_out, max_len, 1, &in, &W, &out, &Wo) || (int)blockIdx.x * 256 >= W) return;
  const int xpitch = T_in, ypitch = T_out;
  const float* xb = x + in;
  float* yb = y + out;
#include "../conv2d_stem_body.h"
}

// row_mean_rows_kernel (csrc/xvector.hip) on the utterance's own contiguous [H][T] plane: element n = h T + t goes to lane n % 64 in turn
// n / 64; one wave per (channel, segment).  (h, t) advance by 64 elements without a division per element: 64 = q T + r.
__global__ void __launch_bounds__(256) plane_mean_segments_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  const int* __restrict__ seg_off, const int* __restrict__ seg_len, int C, int H,
                                                                  int B, int T_tot) {
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= C * B) return;
  const int c = wv / B, i = wv - c * B;
  int off, T;
  if (!ragged_segment(seg_off, seg_len, i, T_tot, &off, &T)) return;
  const float* xc = x + (size_t)c * H * T_tot + off;
  const int q = 64 / T, r = 64 - q * T;
  const long long N = (long long)H * T;
  int h = lane / T, t = lane - h * T;
  float s = 0.f;
  for (long long n = lane; n < N; n += 64) {
    s += xc[(size_t)h * T_tot + t];
    h += q;
    t += r;
    if (t >= T) {
      t -= T;
      ++h;
    }
  }
  s = wave_sum(s);
  if (lane == 0) y[(size_t)i * C + c] = s / (float)N;
}

// se_scale_add_relu_kernel on the columns of segment i: a thread owns one column of the segment and one channel and walks the H rows
__global__ void __launch_bounds__(256) se_scale_add_relu_segments_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                                         const float* __restrict__ r, float* __restrict__ y,
                                                                         const int* __restrict__ seg_off, const int* __restrict__ seg_len, int C,
                                                                         int H, int T_tot, int max_len) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int ch = blockIdx.y, seg = blockIdx.z;
  int off, T;
  if (!ragged_segment(seg_off, seg_len, seg, T_tot, &off, &T) || T > max_len || t >= T) return;
  const float gate = 1.0f / (1.0f + expf(-g[(size_t)seg * C + ch]));
  size_t i = (size_t)ch * H * T_tot + off + t;
  for (int h = 0; h < H; ++h, i += T_tot) {
    const float v = z[i] * gate + r[i];
    y[i] = fmaxf(v, 0.f);
  }
}

// row_mean_std_kernel per (row, segment), on the same row_mean_sqdev_wave: x [R][T_tot] -> out [B][2R], means then unbiased deviations.  One wave each; T < 2 is skipped
__global__ void __launch_bounds__(256) row_mean_std_segments_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                    const int* __restrict__ seg_off, const int* __restrict__ seg_len, int R, int B,
                                                                    int T_tot) {
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= R * B) return;
  const int c = wv / B, b = wv - c * B;
  int off, T;
  if (!ragged_segment(seg_off, seg_len, b, T_tot, &off, &T) || T < 2) return;
  float mean, q;
  row_mean_sqdev_wave(x + (size_t)c * T_tot + off, T, lane, &mean, &q);
  if (lane == 0) {
    out[(size_t)b * 2 * R + c] = mean;
    out[(size_t)b * 2 * R + R + c] = sqrtf(q / (float)(T - 1));
  }
}

template <int KS, int S, int MT>
static int launch_conv2d_segments(const float* x, const float* w, float* y, const float* scale, const float* shift, const int32_t* in_off,
                                  const int32_t* in_len, const int32_t* out_off, int B, int Cin, int Cout, int H, int T_in, int Ho, int T_out,
                                  int max_len, int relu, hipStream_t stream) {
  const int row_tiles = ceil_div(Ho, C2_TH);
  const dim3 grid(ceil_div((max_len - 1) / S + 1, C2_TW), row_tiles * (Cout / (32 * MT)), B);
  hipLaunchKernelGGL((conv2d_segments_mfma_kernel<KS, S, MT>), grid, dim3(256), 0, stream, x, w, y, scale, shift, in_off, in_len, out_off, Cin,
                     Cout, H, T_in, Ho, T_out, max_len, row_tiles, relu);
  SAT_LAUNCH_CHECK("conv2d_segments_mfma_kernel");
  return SAT_OK;
}

}  // namespace sat

using namespace sat;

#define R2_TABLE_OK(what, off, len, T) \
  SAT_REQUIRE((off) && (len) && B >= 1 && B <= SAT_RAGGED_MAX_SEGMENTS && (T) >= 1, what ": a segment table of 1 .. %d segments and T_tot >= 1 are needed", SAT_RAGGED_MAX_SEGMENTS)

extern "C" int sat_conv2d_segments_f32(const float* x, const float* w_packed, float* y, const float* ch_scale, const float* ch_shift, int relu,
                                       const int32_t* in_off, const int32_t* in_len, const int32_t* out_off, int B, int max_len, int Cin, int Cout,
                                       int H, int T_in, int T_out, int ksize, int stride, void* stream) {
  SAT_REQUIRE(x && w_packed && y && x != y, "conv2d_segments: null pointer, or y aliases x");
  SAT_REQUIRE((ch_scale != nullptr) == (ch_shift != nullptr), "conv2d_segments: ch_scale and ch_shift come together");
  R2_TABLE_OK("conv2d_segments", in_off, in_len, T_in);
  SAT_REQUIRE(out_off && T_out >= 1 && H > 0, "conv2d_segments: null output table, T_out = %d, H = %d", T_out, H);
  SAT_REQUIRE(max_len >= 1 && max_len <= T_in, "conv2d_segments: max_len = %d (the longest segment: 1 .. T_in = %d)", max_len, T_in);
  SAT_REQUIRE((ksize == 3 || ksize == 1) && (stride == 1 || stride == 2), "conv2d_segments: ksize %d / stride %d (3x3 with padding 1 or 1x1, stride 1 or 2)",
              ksize, stride);
  const int Ho = (H - 1) / stride + 1;
  SAT_REQUIRE((long long)Cin * H * T_in < (1ll << 31) && (long long)Cout * Ho * T_out < (1ll << 31), "conv2d_segments: an image exceeds 2^31 elements");
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 1) {
    SAT_REQUIRE(Cout == C2_STEM_CO && ksize == 3 && stride == 1,
                "conv2d_segments: Cin = 1 is the stem only (Cout = 32, 3x3, stride 1), got Cout = %d, ksize %d, stride %d", Cout, ksize, stride);
    SAT_REQUIRE(H <= 65535, "conv2d_segments: H = %d exceeds the grid", H);
    hipLaunchKernelGGL(conv2d_segments_stem_kernel, dim3(ceil_div(max_len, 256), H, B), dim3(256), 0, st, x, w_packed, y, ch_scale, ch_shift, in_off,
                       in_len, out_off, H, T_in, T_out, max_len, relu);
    SAT_LAUNCH_CHECK("conv2d_segments_stem_kernel");
    return SAT_OK;
  }
  const auto ok = [](int c) { return c == 32 || c == 64 || c == 128 || c == 256; };
  SAT_REQUIRE(ok(Cin) && ok(Cout), "conv2d_segments: Cin = %d / Cout = %d (32, 64, 128 or 256; Cin = 1 for the stem)", Cin, Cout);
  const int mt = Cout == 32 ? 1 : 2;
  SAT_REQUIRE((long long)ceil_div(Ho, C2_TH) * (Cout / (32 * mt)) <= 65535, "conv2d_segments: H = %d exceeds the grid", H);
#define SAT_R2(KS_, S_)                                                                                                                              \
  (mt == 1 ? launch_conv2d_segments<KS_, S_, 1>(x, w_packed, y, ch_scale, ch_shift, in_off, in_len, out_off, B, Cin, Cout, H, T_in, Ho, T_out, max_len, relu, st) \
           : launch_conv2d_segments<KS_, S_, 2>(x, w_packed, y, ch_scale, ch_shift, in_off, in_len, out_off, B, Cin, Cout, H, T_in, Ho, T_out, max_len, relu, st))
  if (ksize == 3) return stride == 1 ? SAT_R2(3, 1) : SAT_R2(3, 2);
  return stride == 1 ? SAT_R2(1, 1) : SAT_R2(1, 2);
#undef SAT_R2
}

extern "C" int sat_plane_mean_segments_f32(const float* x, float* y, const int32_t* seg_off, const int32_t* seg_len, int C, int H, int B, int T_tot,
                                           void* stream) {
  SAT_REQUIRE(x && y && C > 0 && H > 0, "plane_mean_segments: bad arguments");
  R2_TABLE_OK("plane_mean_segments", seg_off, seg_len, T_tot);
  SAT_REQUIRE((long long)C * B < (1ll << 31) - 4 && (long long)C * H * T_tot < (1ll << 31), "plane_mean_segments: too many (channel, segment) pairs or elements");
  hipLaunchKernelGGL(plane_mean_segments_kernel, dim3(ceil_div(C * B, 4)), dim3(256), 0, (hipStream_t)stream, x, y, seg_off, seg_len, C, H, B, T_tot);
  SAT_LAUNCH_CHECK("plane_mean_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_se_scale_add_relu_segments_f32(const float* z, const float* gate_logits, const float* r, float* y, const int32_t* seg_off,
                                                  const int32_t* seg_len, int B, int max_len, int C, int H, int T_tot, void* stream) {
  SAT_REQUIRE(z && gate_logits && r && y && C > 0 && C <= 65535 && H > 0, "se_scale_add_relu_segments: bad arguments");
  R2_TABLE_OK("se_scale_add_relu_segments", seg_off, seg_len, T_tot);
  SAT_REQUIRE(max_len >= 1 && max_len <= T_tot, "se_scale_add_relu_segments: max_len = %d (the longest segment: 1 .. T_tot = %d)", max_len, T_tot);
  SAT_REQUIRE((long long)C * H * T_tot < (1ll << 31), "se_scale_add_relu_segments: an image exceeds 2^31 elements");
  hipLaunchKernelGGL(se_scale_add_relu_segments_kernel, dim3(ceil_div(max_len, 256), C, B), dim3(256), 0, (hipStream_t)stream, z, gate_logits, r, y,
                     seg_off, seg_len, C, H, T_tot, max_len);
  SAT_LAUNCH_CHECK("se_scale_add_relu_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_row_mean_std_segments_f32(const float* x, float* out, const int32_t* seg_off, const int32_t* seg_len, int R, int B, int T_tot,
                                             void* stream) {
  SAT_REQUIRE(x && out && R > 0, "row_mean_std_segments: bad arguments");
  R2_TABLE_OK("row_mean_std_segments", seg_off, seg_len, T_tot);
  SAT_REQUIRE((long long)R * B < (1ll << 31) - 4, "row_mean_std_segments: too many (row, segment) pairs");
  hipLaunchKernelGGL(row_mean_std_segments_kernel, dim3(ceil_div(R * B, 4)), dim3(256), 0, (hipStream_t)stream, x, out, seg_off, seg_len, R, B, T_tot);
  SAT_LAUNCH_CHECK("row_mean_std_segments_kernel");
  return SAT_OK;
}
