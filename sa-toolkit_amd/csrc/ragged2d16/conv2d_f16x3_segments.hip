// Segment form of the split-f16 2-D convolution (csrc/conv2d16/conv2d_f16x3.hip) for a RAGGED batch on a packed time axis
// (include/satools_hip_ragged2d16.h; the layout is the one of include/satools_hip_ragged2d.h: B utterances of unequal length side by side in
// one image [C][H][T_tot], time innermost, segment i at columns off_i .. off_i + T_i - 1 of every row, gap columns that hold anything).
// The kernel keeps the per-call kernel's tiles, LDS images and order of operations, so that segment i of its result has the bits of
// sat_conv2d_f16x3_f32 on utterance i alone; it selects on load (a gap column or another segment never reaches an output or an overflow
// flag, NaN included) and skips what a wrong table names.  Neither csrc/conv2d16/ nor csrc/ragged2d/ is touched: the K loop is restated
// here, as csrc/ragged2d/resnet_ragged.hip restates the f32 one.
#include "../common.h"
#include "../../../include/satools_hip_ragged2d16.h"

namespace sat {

typedef float r16_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 r16_h8 __attribute__((ext_vector_type(8)));

constexpr int R16_TH = 4;      // output rows per block: one per wave                                       (C16_TH of csrc/conv2d16/)
constexpr int R16_CI = 16;     // input channels per staged chunk: the K of one v_mfma_f32_32x32x16_f16     (C16_CI)
[[maybe_unused]] constexpr int R16_KERNELS = 6;  // instantiations the entry point dispatches to (tests/test_codegen_xvector_resnet_ragged16.py counts them)

// segment i of a conv: W input columns from column `in` of x's rows, Wo = (W - 1) / S + 1 output columns from column `out` of y's rows;
// false unless both lie inside their rows and W <= max_len (the bound the grid was sized by: a longer segment would be computed in part)
__device__ __forceinline__ bool r16_conv_segment(const int* __restrict__ in_off, const int* __restrict__ in_len, const int* __restrict__ out_off, int i,
                                                 int T_in, int T_out, int max_len, int S, int* in, int* W, int* out, int* Wo) {
  const int o = in_off[i], l = in_len[i];
  *in = o;
  *W = l;
  if (!(o >= 0 && l >= 1 && o < T_in && l <= T_in - o) || l > max_len) return false;
  const int oo = out_off[i], wo = (l - 1) / S + 1;
  *out = oo;
  *Wo = wo;
  return oo >= 0 && oo < T_out && wo <= T_out - oo;
}

// conv2d_f16x3_kernel (csrc/conv2d16/conv2d_f16x3.hip) with a block per (segment, 32 MT output channels, R16_TH x 32 NT output pixels in the
// segment's own coordinates): the image's width is the segment's W, on the loads (columns outside 0 .. W - 1 are staged as zero: the padding
// at the utterance's own ends, whatever the gap or the neighbour holds, and zero raises no flag) and on the stores alike; rows are T_in /
// T_out apart.  Per chunk of 16 input channels the block stages in LDS
//   X  [hi|lo][channel half][row][column] x 16 B (8 f16): the halo tile, split into hi + lo while it is staged; under stride 2 the even
//      columns of a row come first, then the odd ones, so that the 32 lanes of a tap read consecutive units at either stride
//   W  [tap][hi|lo][channel half][row] x 16 B: a straight copy of the packed weights
// exactly as that kernel does: every A and B fragment is one ds_read_b128 of consecutive units, the NEXT chunk's loads are issued before this
// chunk's MFMAs and stored after them, and the sum over K runs in the same order (chunk, tap; lo-hi, hi-lo, hi-hi), so every accumulator sees
// the same MFMAs on the same values in the same order.
// The grid's x extent comes from max_len; a block past its segment's last tile leaves before the first barrier (block-uniform).
template <int KS, int S, int MT, int NT>
__global__ void __launch_bounds__(256) conv2d_segments_f16x3_kernel(const float* __restrict__ x, const uint4* __restrict__ w, float* __restrict__ y,
                                                                    const float* __restrict__ scale, const float* __restrict__ shift, float descale,
                                                                    int* __restrict__ overflow_flags, const int* __restrict__ in_off,
                                                                    const int* __restrict__ in_len, const int* __restrict__ out_off, int Cin, int Cout,
                                                                    int H, int T_in, int Ho, int T_out, int max_len, int row_tiles, int relu) {
  constexpr int P = KS / 2;                                  // padding
  constexpr int TWB = 32 * NT;                               // output columns per block
  constexpr int R = S * (R16_TH - 1) + KS;                   // staged input rows
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
  const int seg = blockIdx.z;
  int in, W, out, Wo;
  if (!r16_conv_segment(in_off, in_len, out_off, seg, T_in, T_out, max_len, S, &in, &W, &out, &Wo)) return;
  const int wo0 = blockIdx.x * TWB;
  if (wo0 >= Wo) return;
  const int rt = blockIdx.y % row_tiles, ct = blockIdx.y / row_tiles;
  const int ho0 = rt * R16_TH, co0 = ct * COT;
  const int gh0 = S * ho0 - P, gw0 = S * wo0 - P;
  const int hw = H * T_in;                                   // channel pitch
  const float* xb = x + in;

  r16_f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // a staging unit = the eight channels of one channel half at one pixel of the halo tile: eight loads (each coalesced along the row over
  // the lanes; scalar floats, so a segment may begin on any column), one 16-byte LDS store per part
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
      const bool ok = u < NXU && gh >= 0 && gh < H && gw >= 0 && gw < W;
      const float* px = xb + (ok ? ((ci0 + 8 * half) * H + gh) * T_in + gw : 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) xr[k][j] = ok ? px[j * hw] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int u = tid + 256 * k;
      const int part = u / COT, r = u - part * COT;
      wr[k] = make_uint4(0, 0, 0, 0);
      if (u < NWU) wr[k] = w[((size_t)(ci0 / R16_CI) * (TAPS * 4) + part) * Cout + co0 + r];
    }
  };
  bool bad = false;
  fetch(0);
  for (int ci0 = 0; ci0 < Cin; ci0 += R16_CI) {
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
    if (ci0 + R16_CI < Cin) fetch(ci0 + R16_CI);
    const uint4* xa = xs + lh * PLN + (S * wave) * WP + l31;
    const uint4* wa = wl + lh * COT + l31;
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int tap = kh * KS + kw;
        // column S (32 n + l31) + kw of the tile -> its unit in the row
        const int c0 = S == 2 ? (kw & 1) * WCH + (kw >> 1) : kw;
        r16_h8 a_hi[MT], a_lo[MT], b_hi[NT], b_lo[NT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          a_hi[m] = __builtin_bit_cast(r16_h8, wa[(tap * 4 + 0) * COT + 32 * m]);
          a_lo[m] = __builtin_bit_cast(r16_h8, wa[(tap * 4 + 2) * COT + 32 * m]);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          b_hi[n] = __builtin_bit_cast(r16_h8, xa[kh * WP + c0 + 32 * n]);
          b_lo[n] = __builtin_bit_cast(r16_h8, xa[2 * PLN + kh * WP + c0 + 32 * n]);
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

  // a value of THIS segment that could not be split: reported by a plain atomic of a vector lane into the segment's own flag (never a clear:
  // the caller owns the flags); seg < B, the grid's z extent
  if (bad && overflow_flags) atomicOr(overflow_flags + seg, 1);

  const int ho = ho0 + wave;
  if (ho >= Ho) return;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int wo = wo0 + 32 * n + l31;
    if (wo >= Wo) continue;
    float* yb = y + (size_t)ho * T_out + out + wo;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float v = acc[m][n][r] * descale;
        if (scale) v = v * scale[co] + shift[co];
        if (relu) v = fmaxf(v, 0.f);
        yb[(size_t)co * Ho * T_out] = v;
      }
  }
}

template <int KS, int S, int MT, int NT>
static int launch_conv2d16_segments(const float* x, const void* w, float descale, float* y, const float* scale, const float* shift,
                                    const int32_t* in_off, const int32_t* in_len, const int32_t* out_off, int B, int Cin, int Cout, int H, int T_in,
                                    int Ho, int T_out, int max_len, int relu, int* flags, hipStream_t stream) {
  const int row_tiles = ceil_div(Ho, R16_TH);
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
  SAT_REQUIRE((long long)ceil_div(Ho, R16_TH) * (Cout / (32 * mt)) <= 65535, "conv2d_f16x3_segments: H = %d exceeds the grid", H);
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
