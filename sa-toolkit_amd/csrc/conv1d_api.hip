// The C ABI of the 1-D conv family: descriptor checks, the choice of the kernel, the run-time options.  No kernel lives here;
// every launcher it picks from is declared in conv_common.h.
#include "common.h"
#include "conv_common.h"
#include <cstring>

namespace sat {

// sat_conv_set_option("k1_gemm", v): 1x1 convs on split planes through 0 = the conv tile, 1 = conv1d_f16x3_k1_kernel,
// 2 = gemm_f16x3_ring_kernel where its 256-column tiles fit (else 1), 3 = the 16x16x32-shape ring kernel where its
// epilogue subset covers the call (else 2)
static int g_k1_gemm = 3;
// sat_conv_set_option("lean3" | "lean7" | "lean11", v): 3- / 7- / 11-tap convs on split planes (no folded BatchNorm) through
// the three-blocks-per-CU form of the tile (1, conv_lean.hip) or the two-block form (0)
static int g_lean3 = 1, g_lean7 = 1, g_lean11 = 1;
static int g_trim_halo = 1; // the fused pair kernels load only the columns of their staged window that conv1 reads (window + halo of the dilation)
static int g_half_tile7 = 1;   // conv_pre on 64 x 128 tiles when the 64 x 256 ones are at most one per CU
static int g_pair32s = 1;   // the 3-tap fused step at C = 32 on the streaming kernel (pair32s.hip)

// the ring GEMMs' 256-column tiles pad the time axis (nearly) no more than 128-column ones (249 frames: 256 either way;
// 49 frames: the 128-column kernel)
static bool cols256_pad_no_more(int T_q) {
  return (long long)ceil_div(T_q, 256) * 256 * 8 <= (long long)ceil_div(T_q, 128) * 128 * 9;
}

}  // namespace sat

using namespace sat;

extern "C" int sat_conv1d_packed_dims(int C_in, int C_out, int up, int groups, int* cin_pad,
                                      int* co_pad) {
  SAT_REQUIRE(C_in > 0 && C_out > 0 && up > 0 && groups > 0, "conv1d_packed_dims: bad sizes");
  SAT_REQUIRE(C_in % groups == 0 && C_out % groups == 0, "conv1d_packed_dims: groups must divide channels");
  if (cin_pad) *cin_pad = round_up(C_in / groups, CI_CHUNK);
  if (co_pad) *co_pad = round_up(C_out / groups * up, 64);
  return SAT_OK;
}

extern "C" int sat_upsample_grouped_supported(int C_in, int C_out, int ksize, int stride, int padding) {
  if (stride != 4 || C_in <= 0 || C_out <= 0 || ksize < stride || padding < 0) return 0;
  int lo, hi;
  phase_window(ksize, stride, padding, &lo, &hi);
  const int slots = hi - lo + 1;
  return C_in % 64 == 0 && C_out % 16 == 0 && C_out * 4 > 128 && slots == 3;
}

extern "C" uint32_t sat_convtranspose_zero_taps(int ksize, int stride, int padding) {
  if (stride < 1 || stride > 4 || ksize < 1 || padding < 0) return 0;
  int lo, hi;
  phase_window(ksize, stride, padding, &lo, &hi);
  if (hi - lo + 1 > 8) return 0;
  uint32_t mask = 0;
  for (int slot = 0; slot <= hi - lo; ++slot)
    for (int r = 0; r < stride; ++r) {
      const int j = r + padding - stride * (slot + lo);
      if (j < 0 || j >= ksize) mask |= 1u << (slot * 4 + r);
    }
  return mask;
}

// descriptor -> launch arguments (every check of sat_conv1d_f32 but the choice of the kernel)
static int conv1d_prepare(const sat_conv1d_desc* d, const float* x, const void* w_packed, float* y, ConvArgs& a) {
  SAT_REQUIRE(d && w_packed && (x || d->x_split) && (y || (d->no_y && d->y_split)), "conv1d: null pointer");
  SAT_REQUIRE(d->B > 0 && d->C_in > 0 && d->C_out > 0 && d->T_in > 0 && d->T_q > 0, "conv1d: empty shape");
  SAT_REQUIRE(d->ksize >= 1 && d->dilation >= 1 && d->stride >= 1 && d->up >= 1 && d->groups >= 1,
              "conv1d: bad ksize/dilation/stride/up/groups");
  SAT_REQUIRE(d->C_in % d->groups == 0 && d->C_out % d->groups == 0, "conv1d: groups must divide channels");
  SAT_REQUIRE(d->up == 1 || d->stride == 1, "conv1d: polyphase output requires stride 1");
  SAT_REQUIRE(!d->up_grouped || (d->mode == SAT_CONV_F16X3 && d->up == 4), "conv1d: up_grouped is a SAT_CONV_F16X3 layout of up = 4");
  a = ConvArgs{};
  a.x = x;
  a.w = (const float*)w_packed;
  a.y = y;
  a.bias = d->bias;
  a.res = d->res;
  a.ch_scale = d->ch_scale;
  a.ch_shift = d->ch_shift;
  SAT_REQUIRE((d->ch_scale == nullptr) == (d->ch_shift == nullptr), "conv1d: ch_scale and ch_shift go together");
  a.x_bs = d->x_bstride;
  a.x_cs = d->x_cstride;
  a.y_bs = d->y_bstride;
  a.y_cs = d->y_cstride;
  a.r_bs = d->res_bstride;
  a.r_cs = d->res_cstride;
  a.cin_g = d->C_in / d->groups;
  a.cout_g = d->C_out / d->groups;
  a.rows_g = a.cout_g * d->up;
  a.T_in = d->T_in;
  a.T_q = d->T_q;
  a.ksize = d->ksize;
  a.dil = d->dilation;
  a.stride = d->stride;
  a.pad_left = d->pad_left;
  a.up = d->up;
  a.cin_pad = round_up(a.cin_g, CI_CHUNK);
  a.co_pad = round_up(a.rows_g, 64);
  a.w_gs = (long long)a.cin_pad * a.ksize * a.co_pad;
  a.in_lrelu = d->in_lrelu;
  a.in_slope = d->in_slope;
  a.relu = d->relu;
  a.relu_first = d->relu_first;
  a.gelu = d->gelu;
  a.res_after = d->res_after_act;
  a.accum = d->accum;
  a.accum_div = d->accum_div;
  a.no_store = d->accum_no_store;
  SAT_REQUIRE(!d->accum_no_store || (d->accum && y && d->y_split && !d->no_y && d->up == 1),
              "conv1d: accum_no_store goes with accum (y is read), y_split (the output that is written) and up 1");
  a.res_scale = d->res_scale;
  a.res_toff = d->res_toff;
  a.res_tstride = d->res_tstride > 0 ? d->res_tstride : 1;
  a.w_descale = d->w_descale != 0.f ? d->w_descale : 1.f;
  a.w_descale1 = 1.f;
  SAT_REQUIRE(d->mode != SAT_CONV_F32 || a.w_descale == 1.f, "conv1d: w_descale is a split-f16 option");
  {
    const long long ylim = (long long)a.rows_g * a.y_cs * 4;
    const long long rlim = d->res ? ((long long)a.rows_g * a.r_cs + (long long)a.T_q * a.res_tstride + a.res_toff) * 4 : 0;
    a.fast_epi = d->up == 1 && ylim < (1LL << 31) && rlim < (1LL << 31) && ylim > 0;
  }
  // (res_split among them: the exact-f32 kernels never look at it, and a descriptor that names a residual must not run without one)
  SAT_REQUIRE(d->mode != SAT_CONV_F32 || (!d->x_split && !d->y_split && !d->no_y && !d->res_split), "conv1d: split planes need a split-f16 mode");
  if (d->mode == SAT_CONV_F16X3 || d->mode == SAT_CONV_F16F8 || d->mode == SAT_CONV_F16F8R) {
    a.f8 = d->mode == SAT_CONV_F16F8;
    a.f8r = d->mode == SAT_CONV_F16F8R;
    SAT_REQUIRE(!a.f8 || d->x_split, "conv1d(f16f8): the input must be split planes (SAT_SPLIT_F8)");
    SAT_REQUIRE(!a.f8r || (d->x_split && d->x_split8 && d->y_split_format <= 1 && d->ksize >= 3 && !d->up_grouped && d->up == 1),
                "conv1d(f16f8r): needs x_split (SAT_SPLIT_F16 planes) with its e4m3 sidecar x_split8, SAT_SPLIT_F16 output planes, ksize >= 3 (the ring kernel's taps), up 1");
    SAT_REQUIRE(!d->y_split8 || (d->y_split && d->mode != SAT_CONV_F16F8 && d->y_split_format <= 1), "conv1d: y_split8 is the sidecar of SAT_SPLIT_F16 planes y_split");
    SAT_REQUIRE(!d->y_split_hi_only || d->y_split8, "conv1d: y_split_hi_only goes with y_split8");
    a.x8 = d->x_split8;
    a.y8 = d->y_split8;
    a.y16_hi_only = d->y_split_hi_only;
    SAT_REQUIRE(d->y_split_format >= 0 && d->y_split_format <= 2, "conv1d: unknown y_split_format");
    a.y16_f8 = d->y_split_format == 0 ? a.f8 : d->y_split_format == 2;
    SAT_REQUIRE(d->stride == 1, "conv1d(f16x3): stride 1 only");
    SAT_REQUIRE((long long)a.cin_g * a.x_cs * 4 < (1LL << 31), "conv1d(f16x3): input slab too large for 31-bit offsets");
    a.x16 = d->x_split;
    a.y16 = d->y_split;
    a.y16_slope = d->y_split_slope;
    a.no_y = d->no_y;
    // the split-f16 kernels apply a leaky-relu as max(v, slope v) and undo one as min(r, r / slope) (common.h lrelu_max)
    SAT_REQUIRE((!d->in_lrelu || (d->in_slope >= 0.f && d->in_slope <= 1.f)) && (!d->y_split || (d->y_split_slope >= 0.f && d->y_split_slope <= 1.f)) &&
                    (!d->res_split || d->res_split_slope <= 1.f),
                "conv1d(f16x3): leaky-relu slopes must lie in [0, 1]");
    if (a.x16)
      SAT_REQUIRE(d->groups == 1 && a.cin_g % 16 == 0 && (long long)a.cin_g * a.T_in * 4 < (1LL << 31),
                  "conv1d(f16x3): x_split needs groups 1, C_in %% 16 == 0 and a slab below 2 GiB");
    if (d->x_wrap_channels) {
      SAT_REQUIRE(a.x16 && !a.f8 && d->ksize == 1 && d->groups == 1 && d->x_wrap_channels > 0 && d->x_wrap_channels % 32 == 0 &&
                      d->x_wrap_channels < d->C_in && d->C_in <= 2 * d->x_wrap_channels && d->C_in % 32 == 0 && a.rows_g % 128 == 0,
                  "conv1d: x_wrap_channels needs a 1x1 split-f16 conv on split planes, channel counts multiples of 32 with "
                  "x_wrap < C_in <= 2 x_wrap, C_out %% 128 == 0");
      a.k1_wrap = d->x_wrap_channels / CI_CHUNK;
      a.cin_g = d->x_wrap_channels;            // channels behind x_split (the descriptor range of the planes)
    }
    if (d->res_split) {
      SAT_REQUIRE(!d->res && a.fast_epi && d->groups == 1 && a.rows_g % 16 == 0 && d->res_split_slope > 0.f &&
                  (long long)a.rows_g * a.T_q * 4 < (1LL << 31), "conv1d(f16x3): res_split needs up 1, groups 1, C_out %% 16 == 0, no f32 res");
      a.res16 = d->res_split;
      a.res16_inv = 1.0f / d->res_split_slope;
    }
    if (d->up_grouped) {
      // polyphase upsampler of stride 4 with its rows grouped by phase: the LDS-DMA ring writes the planes itself
      a.up_grouped = 1;
      a.up_zero_taps = d->up_zero_taps;
      a.y = (float*)a.y16;
      SAT_REQUIRE(d->mode == SAT_CONV_F16X3 && d->groups == 1 && !d->res && !d->res_split && !d->accum && !d->relu && !d->gelu && !d->ch_scale &&
                      (long long)a.rows_g * a.T_q * 4 < (1LL << 31) && convring_ups_supports(a),
                  "conv1d(f16x3): up_grouped needs up 4, split planes in and out with no_y, C_in %% 64 == 0, C_out %% 16 == 0, C_out * 4 > 128, "
                  "3 tap slots, a bias and a plain epilogue");
    } else if (d->up > 1 && (a.y16 || a.no_y)) {
      // polyphase upsampler straight to planes (LDS-transposed epilogue)
      const int co_b = a.rows_g > 32 ? 64 : 32;
      SAT_REQUIRE(a.x16 && a.y16 && a.no_y && !a.f8 && !a.y16_f8 && d->groups == 1 && co_b % (8 * d->up) == 0 && a.cout_g % 16 == 0 &&
                      !d->res && !d->res_split && !d->accum && !d->relu && !d->gelu && !d->ch_scale &&
                      (long long)a.rows_g * a.T_q * 4 < (1LL << 31),
                  "conv1d(f16x3): up > 1 with y_split needs split-plane input, no_y, up in {2, 4}, C_out %% 16 == 0, a plain epilogue");
      a.poly_planes = 1;
      a.y = (float*)a.y16;
    } else if (a.y16 || a.no_y) {
      SAT_REQUIRE(a.fast_epi && d->groups == 1 && a.rows_g % 16 == 0 && (long long)a.rows_g * a.T_q * 4 < (1LL << 31),
                  "conv1d(f16x3): y_split / no_y need up 1, groups 1, C_out %% 16 == 0 and a slab below 2 GiB");
      if (a.no_y) a.y = (float*)a.y16, a.accum = 0;   // descriptor base only; nothing is loaded or stored through it
      SAT_REQUIRE(!(d->no_y && d->accum), "conv1d: no_y with accum");
    }
    a.w_gs = (long long)(a.cin_pad / CI_CHUNK) * a.ksize * a.co_pad * 64;   // bytes per group
    // (SAT_CONV_F16F8R packing: [2 ceil(C_in / 32 x k / 2) steps][8 planes][co_pad][16 B])
    if (a.f8r) a.w_gs = (long long)(2 * (((a.cin_pad / (2 * CI_CHUNK)) * a.ksize + 1) / 2)) * 8 * a.co_pad * 16;
    return SAT_OK;
  }
  SAT_REQUIRE(d->mode == SAT_CONV_F32, "conv1d: unknown mode %d", d->mode);
  return SAT_OK;
}

static int conv1d_dispatch(const sat_conv1d_desc* d, ConvArgs& a, hipStream_t s);

extern "C" int sat_conv1d_f32(const sat_conv1d_desc* d, const float* x, const void* w_packed,
                              float* y, void* stream) {
  ConvArgs a;
  int st = conv1d_prepare(d, x, w_packed, y, a);
  if (st != SAT_OK) return st;
  return conv1d_dispatch(d, a, (hipStream_t)stream);
}

// the kernel choice for a prepared conv (sat_conv1d_f32; sat_tdnnf_layer_f32 enters here with the bypass planes' geometry set)
static int conv1d_dispatch(const sat_conv1d_desc* d, ConvArgs& a, hipStream_t s) {
  if (d->mode == SAT_CONV_F16F8R) {
    SAT_REQUIRE(d->groups == 1 && convring_supports(a, d->B),
                "conv1d(f16f8r): served by the LDS-DMA ring kernel only (C_out > 64, C_in %% 32 == 0, ksize >= 3, halo <= 64, bias, plain / "
                "ResBlock epilogue: sat_conv1d_f8r_supported)");
    return launch_f16x3_convring(a, d->B, s);
  }
  if (d->mode == SAT_CONV_F16X3 || d->mode == SAT_CONV_F16F8) {
    // an e4m3 sidecar of the output is written by the epilogues of conv_ring16.hip only
    SAT_REQUIRE(!a.y8 || a.up_grouped || (d->groups == 1 && convring_supports(a, d->B)),
                "conv1d: y_split8 needs a shape the LDS-DMA ring kernel serves (or sat_planes_f8_sidecar after the launch)");
    // 1x1 on split planes with enough rows: the GEMM kernel (activation fragments straight from the planes)
    if (a.x16 && a.ksize == 1 && !a.f8 && !a.poly_planes && a.fast_epi && d->groups == 1 && a.rows_g >= 128 &&
        (a.cin_pad / CI_CHUNK) % 4 == 0 && g_k1_gemm) {
      if (a.k1_wrap) {                         // only the 16x16x32 ring kernel reads wrapped K chunks
        SAT_REQUIRE(ring16_supports(a), "conv1d: x_wrap_channels needs the epilogue of the ring GEMM (up 1, split-f16 planes)");
        return launch_f16x3_ring16(a, d->B, s);
      }
      // ring kernel: whole 128-row weight tiles, and 256-column tiles
      if (g_k1_gemm >= 2 && a.co_pad % 128 == 0 && cols256_pad_no_more(a.T_q)) {
        // more tiles than CUs (the 1024 -> 4096 layer: four per CU): the persistent walk of the same ring (gemm_walk16.hip)
        if (g_k1_gemm >= 3 && gemm_walk_supports(a) && gemm_walk_wanted((long long)ceil_div(a.rows_g, 128) * ceil_div(a.T_q, 256) * d->B))
          return launch_f16x3_gemm_walk(&a, 1, d->B, s);
        return g_k1_gemm >= 3 && ring16_supports(a) ? launch_f16x3_ring16(a, d->B, s) : launch_f16x3_ring(a, d->B, s);
      }
      return launch_f16x3_k1(a, d->B, s);
    }
    SAT_REQUIRE(!a.k1_wrap, "conv1d: x_wrap_channels is only served by the 1x1 GEMM path (C_in %% 64 == 0, up 1, 31-bit slabs)");
    if (a.up_grouped) return launch_f16x3_convring_ups(a, d->B, s);
    // the generator's resblock convs at C >= 128: the LDS-DMA ring on the 16x16x32 shape (conv_ring16.hip)
    if (d->groups == 1 && convring_supports(a, d->B)) return launch_f16x3_convring(a, d->B, s);
    // few blocks (TDNNF linearB: 128 rows x 250 frames x 32 utterances = 64 tiles of 64 x 256 on 256 CUs): half-width
    // tiles double the blocks of these latency-bound launches
    if (a.x16 && a.ksize == 3 && !a.f8 && !a.poly_planes && a.rows_g > 32 && a.T_q > 128 &&
        (long long)ceil_div(a.rows_g, 64) * ceil_div(a.T_q, 256) * d->B * d->groups < 256)
      return launch_f16x3_64x128(a, d->B, d->groups, s);
    // the same for the generator's conv_pre (f32 input, 7 taps, 512 rows x 250 frames x 32 utterances = 256 tiles of 64 x 256)
    if (g_half_tile7 && !a.x16 && a.ksize == 7 && a.rows_g > 32 && a.T_q > 128 &&
        (long long)ceil_div(a.rows_g, 64) * ceil_div(a.T_q, 256) * d->B * d->groups <= 256)
      return launch_f16x3_64x128(a, d->B, d->groups, s);
    // the generator's resblock convs: the three-blocks-per-CU form of the tile (conv_lean.hip)
    if (d->groups == 1 && (a.ksize == 3 ? g_lean3 : a.ksize == 7 ? g_lean7 : g_lean11) && lean_supports(a))
      return launch_f16x3_lean(a, d->B, s);
    if (a.rows_g > 32) return launch_f16x3_64x256(a, d->B, d->groups, s);
    return launch_f16x3_32x512(a, d->B, d->groups, s);
  }
  return launch_conv1d_f32(a, d->B, d->groups, s);
}

// One TDNNF layer per call (chain/nn.py:336-347 TDNNFBatchNorm.forward = TDNNF.forward 267-292 with its bypass -> BatchNorm1d -> ReLU): the
// two launches sat_conv1d_f32 makes for linearB (context_len taps over frames, feat -> bottleneck) and linearA (1x1, bottleneck -> out,
// bias, bypass from the layer input identity_lidx frames in, folded BatchNorm, ReLU) behind ONE descriptor — the host composes nothing
// between them, and the bottleneck never has to exist as f32 when the layer runs on split planes.
extern "C" int sat_tdnnf_layer_f32(const sat_tdnnf_layer_desc* d, void* stream) {
  SAT_REQUIRE(d && d->wB_packed && d->wA_packed, "tdnnf_layer: null pointer");
  SAT_REQUIRE(d->y || (d->y_split && d->mode == SAT_CONV_F16X3), "tdnnf_layer: y, or (split planes) y_split alone");
  SAT_REQUIRE(d->B > 0 && d->feat_dim > 0 && d->bottleneck_dim > 0 && d->out_dim > 0 && d->context_len >= 1 && d->T_in >= d->context_len,
              "tdnnf_layer: unsupported shape");
  SAT_REQUIRE(d->mode == SAT_CONV_F32 || d->mode == SAT_CONV_F16X3, "tdnnf_layer: mode must be SAT_CONV_F32 or SAT_CONV_F16X3");
  SAT_REQUIRE(d->x || d->x_split, "tdnnf_layer: x or x_split");
  const int T_q = d->T_in - (d->context_len - 1);
  const bool planes = d->mode == SAT_CONV_F16X3 && d->z_split && d->bottleneck_dim % 16 == 0;
  SAT_REQUIRE(planes || d->z, "tdnnf_layer: the bottleneck needs z (f32) or, on split planes, z_split");
  const bool bypass_planes = d->bypass_scale != 0.f && !d->x;      // no f32 input: the bypass is rebuilt from the input planes (hi + lo)
  SAT_REQUIRE(d->bypass_scale == 0.f || d->out_dim == d->feat_dim, "tdnnf_layer: the bypass adds the layer input (out_dim == feat_dim)");
  SAT_REQUIRE(!bypass_planes || (d->x_split && d->mode == SAT_CONV_F16X3 && d->feat_dim % 16 == 0),
              "tdnnf_layer: a bypass without the f32 input needs x_split (SAT_CONV_F16X3, feat_dim %% 16 == 0)");
  sat_conv1d_desc b{};
  b.B = d->B, b.C_in = d->feat_dim, b.T_in = d->T_in, b.C_out = d->bottleneck_dim, b.T_q = T_q;
  b.ksize = d->context_len, b.dilation = 1, b.stride = 1, b.pad_left = 0, b.mode = d->mode, b.groups = 1, b.up = 1;
  b.x_cstride = d->T_in, b.x_bstride = (int64_t)d->feat_dim * d->T_in;
  b.y_cstride = T_q, b.y_bstride = (int64_t)d->bottleneck_dim * T_q;
  b.res_tstride = 1;
  b.bias = d->bB;
  b.w_descale = d->wB_descale;
  b.x_split = d->mode == SAT_CONV_F16X3 ? d->x_split : nullptr;
  if (planes) b.y_split = d->z_split, b.y_split_slope = 1.0f, b.no_y = 1;
  int st = sat_conv1d_f32(&b, d->x, d->wB_packed, planes ? (float*)d->z_split : d->z, stream);
  if (st != SAT_OK) return st;
  sat_conv1d_desc a{};
  a.B = d->B, a.C_in = d->bottleneck_dim, a.T_in = T_q, a.C_out = d->out_dim, a.T_q = T_q;
  a.ksize = 1, a.dilation = 1, a.stride = 1, a.pad_left = 0, a.mode = d->mode, a.groups = 1, a.up = 1;
  a.x_cstride = T_q, a.x_bstride = (int64_t)d->bottleneck_dim * T_q;
  a.y_cstride = T_q, a.y_bstride = (int64_t)d->out_dim * T_q;
  a.bias = d->bA, a.ch_scale = d->bn_scale, a.ch_shift = d->bn_shift, a.relu = 1;
  a.w_descale = d->wA_descale;
  a.res_tstride = 1;
  const int lidx = d->context_len == 2 ? 1 : d->context_len / 2;      // identity_lidx, chain/nn.py:233-247
  if (d->bypass_scale != 0.f && !bypass_planes) {
    a.res = d->x, a.res_scale = d->bypass_scale;
    a.res_toff = lidx;
    a.res_cstride = d->T_in, a.res_bstride = (int64_t)d->feat_dim * d->T_in;
  } else if (bypass_planes) {
    a.res_split = d->x_split, a.res_split_slope = 1.0f, a.res_scale = d->bypass_scale;
  }
  if (planes) a.x_split = d->z_split;
  if (d->y_split && d->mode == SAT_CONV_F16X3) a.y_split = d->y_split, a.y_split_slope = 1.0f;
  if (!d->y) a.no_y = 1;
  ConvArgs args;
  st = conv1d_prepare(&a, planes ? (const float*)d->z_split : d->z, d->wA_packed, d->y, args);
  if (st != SAT_OK) return st;
  if (bypass_planes) {
    // the bypass planes are the layer INPUT: rows of T_in positions, output column 0 <-> position identity_lidx (the common epilogues
    // of the 1x1 GEMM kernels take both; conv_common.h res16_T / res16_toff)
    SAT_REQUIRE((long long)d->feat_dim * d->T_in * 4 < (1LL << 31), "tdnnf_layer: input slab too large for 31-bit offsets");
    args.res16_T = d->T_in, args.res16_toff = lidx;
  }
  return conv1d_dispatch(&a, args, (hipStream_t)stream);
}

extern "C" int sat_conv1d_multi_f32(const sat_conv1d_desc* d, const float* const* x, const void* const* w_packed, float* const* y,
                                    int n, void* stream) {
  SAT_REQUIRE(d && x && w_packed && y && n >= 1 && n <= 3, "conv1d_multi: 1..3 convolutions");
  ConvArgs a[3];
  bool ring = true, writes_read = false, partial = false;
  for (int j = 0; j < n; ++j) {
    int st = conv1d_prepare(&d[j], x[j], w_packed[j], y[j], a[j]);
    if (st != SAT_OK) return st;
    ring = ring && (d[j].mode == SAT_CONV_F16X3 || d[j].mode == SAT_CONV_F16F8R) && d[j].groups == 1 && d[j].B == d[0].B && convring_supports(a[j], d[j].B) && convring_same_shape(a[j], a[0]);
  }
  // the order of the jobs may rotate from block to block unless a job reads (accumulates into, takes its residual or
  // input from) what another one writes, or two jobs write the same bytes: compared as BYTE RANGES (views of one buffer at
  // different offsets overlap without being equal; round-4 advisor item)
  struct Span { const char* lo; const char* hi; };
  auto span = [](const void* p, long long bytes) { return Span{(const char*)p, p ? (const char*)p + (bytes > 0 ? bytes : 0) : (const char*)p}; };
  auto overlap = [](const Span& u, const Span& v) { return u.lo && v.lo && u.lo < v.hi && v.lo < u.hi; };
  auto yspan = [&](const ConvArgs& c, int B) {
    return span(c.no_y ? nullptr : (const void*)c.y, ((long long)(B - 1) * c.y_bs + (long long)(c.rows_g - 1) * c.y_cs + (long long)c.T_q * c.up) * 4);
  };
  auto writes = [&](const ConvArgs& c, int B, Span (&w)[3]) {
    w[0] = c.no_store ? Span{nullptr, nullptr} : yspan(c, B);      // (accum_no_store: y is only read)
    w[1] = span(c.y16, (long long)B * c.rows_g * c.T_q * c.up * 4);
    w[2] = span(c.y8, (long long)B * c.rows_g * c.T_q * c.up * 2);
  };
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) {
      if (i == j) continue;
      const int B = d[0].B;
      Span wi[3], wj[3];
      writes(a[i], B, wi);
      writes(a[j], B, wj);
      const Span rd[6] = {a[j].accum ? yspan(a[j], B) : Span{nullptr, nullptr},
                          span(a[j].res, ((long long)(B - 1) * a[j].r_bs + (long long)(a[j].rows_g - 1) * a[j].r_cs + (long long)a[j].T_q * a[j].res_tstride + a[j].res_toff) * 4),
                          span(a[j].res16, (long long)B * a[j].rows_g * a[j].T_q * 4), span(a[j].x16, (long long)B * a[j].cin_g * a[j].T_in * 4),
                          span(a[j].x, ((long long)(B - 1) * a[j].x_bs + (long long)(a[j].cin_g - 1) * a[j].x_cs + a[j].T_in) * 4),
                          span(a[j].x8, (long long)B * a[j].cin_g * a[j].T_in * 2)};
      // the SAME buffer read / written by two jobs: kept in index order inside a block (a tile of job j + 1 touches what its block's
      // tile of job j touched); buffers that overlap at DIFFERENT bases: tiles of different blocks would meet — single launches
      for (const Span& r : rd)
        for (const Span& w : wi)
          if (overlap(r, w)) (r.lo == w.lo ? writes_read : partial) = true;
      for (const Span& u : wi)
        for (const Span& v : wj)
          if (overlap(u, v)) (u.lo == v.lo ? writes_read : partial) = true;
    }
  if (partial) ring = false;
  if (ring && n > 1) return launch_f16x3_convring_multi(a, n, !writes_read, d[0].B, (hipStream_t)stream);
  // 1x1 convs of one shape on split planes (q | k | v of an attention layer): one launch of the persistent ring GEMM
  bool walk = n > 1 && !writes_read && !partial && g_k1_gemm >= 3;
  for (int j = 0; j < n && walk; ++j)
    walk = d[j].mode == SAT_CONV_F16X3 && d[j].groups == 1 && d[j].B == d[0].B && gemm_walk_supports(a[j]) && gemm_walk_same_shape(a[j], a[0]) &&
           cols256_pad_no_more(a[j].T_q);
  if (walk) return launch_f16x3_gemm_walk(a, n, d[0].B, (hipStream_t)stream);
  for (int j = 0; j < n; ++j) {
    int st = sat_conv1d_f32(&d[j], x[j], w_packed[j], y[j], stream);
    if (st != SAT_OK) return st;
  }
  return SAT_OK;
}

extern "C" int sat_resblock_pair_f16x3(const sat_conv1d_desc* d, const float* x, const void* w1_packed,
                                       const float* bias1, const void* w2_packed, float* y, void* stream) {
  return sat_resblock_pair_scaled_f16x3(d, x, w1_packed, bias1, 1.f, w2_packed, y, stream);
}

extern "C" int sat_resblock_pair_scaled_f16x3(const sat_conv1d_desc* d, const float* x, const void* w1_packed,
                                              const float* bias1, float w1_descale, const void* w2_packed, float* y, void* stream) {
  SAT_REQUIRE(d && w1_packed && w2_packed && bias1 && d->bias && (x || d->x_split) && (y || (d->no_y && d->y_split)),
              "resblock_pair: null pointer");
  SAT_REQUIRE(d->C_in == d->C_out && d->C_in % 16 == 0 &&
                  (d->C_in <= 32 || (d->C_in == 64 && d->x_split && d->res_split)),
              "resblock_pair: C must be 16 or 32 (64 with 3 taps and split planes end to end)");
  SAT_REQUIRE(d->groups == 1 && d->up == 1 && d->stride == 1 && d->T_q == d->T_in, "resblock_pair: same-length conv pair only");
  SAT_REQUIRE(d->ksize == 3 || d->ksize == 7 || d->ksize == 11, "resblock_pair: kernel size %d not instantiated", d->ksize);
  SAT_REQUIRE(d->in_lrelu, "resblock_pair: both convs take a leaky-relu input");
  SAT_REQUIRE((d->res && d->res == x && !d->res_split) || (!d->res && d->res_split && d->res_split == d->x_split),
              "resblock_pair: the residual is the block input (res == x, or res_split == x_split)");
  ConvArgs a{};
  a.x = x;
  a.w = (const float*)w1_packed;
  a.w2 = w2_packed;
  a.bias1 = bias1;
  a.y = y;
  a.bias = d->bias;                 // bias of the second conv (the epilogue's)
  a.res = d->res;
  a.x_bs = d->x_bstride; a.x_cs = d->x_cstride;
  a.y_bs = d->y_bstride; a.y_cs = d->y_cstride;
  a.r_bs = d->res_bstride; a.r_cs = d->res_cstride;
  a.cin_g = d->C_in; a.cout_g = d->C_out; a.rows_g = d->C_out;
  a.T_in = d->T_in; a.T_q = d->T_q;
  a.ksize = d->ksize; a.dil = d->dilation; a.stride = 1; a.up = 1;
  a.pad_left = (d->ksize * d->dilation - d->dilation) / 2;   // 'same' padding of the dilated first conv
  a.cin_pad = round_up(a.cin_g, CI_CHUNK);
  a.co_pad = 64;
  a.w_gs = (long long)(a.cin_pad / CI_CHUNK) * a.ksize * a.co_pad * 64;
  a.in_lrelu = 1; a.in_slope = d->in_slope;
  SAT_REQUIRE(d->in_slope >= 0.f && d->in_slope <= 1.f && (!d->y_split || (d->y_split_slope >= 0.f && d->y_split_slope <= 1.f)) &&
                  (!d->res_split || d->res_split_slope <= 1.f),
              "resblock_pair: leaky-relu slopes must lie in [0, 1] (common.h lrelu_max)");
  a.accum = d->accum; a.accum_div = d->accum_div;
  a.no_store = d->accum_no_store;
  SAT_REQUIRE(!d->accum_no_store || (d->accum && y && d->y_split && !d->no_y), "resblock_pair: accum_no_store goes with accum and y_split");
  a.res_scale = 1.f; a.res_toff = 0; a.res_tstride = 1;
  a.w_descale = d->w_descale != 0.f ? d->w_descale : 1.f;        // second conv (the epilogue's)
  a.w_descale1 = w1_descale != 0.f ? w1_descale : 1.f;
  SAT_REQUIRE((long long)a.cin_g * a.x_cs * 4 < (1LL << 31) && (long long)a.rows_g * a.y_cs * 4 < (1LL << 31),
              "resblock_pair: slab too large for 31-bit offsets");
  a.fast_epi = 1;
  a.x16 = d->x_split;
  a.y16 = d->y_split;
  a.y16_slope = d->y_split_slope;
  a.no_y = d->no_y;
  SAT_REQUIRE(!(d->no_y && d->accum), "resblock_pair: no_y with accum");
  if (a.no_y) a.y = (float*)a.y16;
  if (d->res_split) {
    SAT_REQUIRE(d->res_split_slope > 0.f, "resblock_pair: res_split_slope");
    a.res16 = d->res_split;
    a.res16_inv = 1.0f / d->res_split_slope;
  }
  SAT_REQUIRE((long long)a.rows_g * a.T_q * 4 < (1LL << 31), "resblock_pair: slab too large");
  hipStream_t s = (hipStream_t)stream;
  // C = 16 with split planes end to end: the 16-row MFMA shape, everything resident
  if (a.cin_g == 16 && a.x16 && a.res16) return launch_pair16(a, d->B, s);
  if (a.cin_g == 64 && g_pair32s && pair32s_supports(a)) return launch_pair32s(a, d->B, s);
  if (a.cin_g == 64) {
    SAT_REQUIRE(pair64_supports(a), "resblock_pair(C = 64): split planes in, residual from planes, (ksize - 1) * dilation <= 64");
    a.xw = g_trim_halo ? 128 + (a.ksize - 1) * a.dil : 192;      // staged columns conv1 reads (pair64.hip)
    return launch_pair64(a, d->B, s);
  }
  if (a.cin_g == 32 && a.x16 && a.res16) {
    if (g_pair32s && pair32s_supports(a)) return launch_pair32s(a, d->B, s);
    // staged columns conv1 reads (pair.hip): its t1 window, 236 columns at 11 taps and 256 otherwise, plus the halo of the dilation
    a.xw = g_trim_halo ? (a.ksize == 11 ? 236 : 256) + (a.ksize - 1) * a.dil : 320;
    return launch_pair32(a, d->B, s);
  }
  return launch_pair(a, d->B, s);
}

extern "C" int sat_conv1d_f8r_supported(const sat_conv1d_desc* d) {
  if (!d || d->mode != SAT_CONV_F16F8R || !d->x_split || !d->x_split8 || d->groups != 1) return 0;
  ConvArgs a;
  float dummy;
  if (conv1d_prepare(d, nullptr, &dummy, d->no_y ? nullptr : &dummy, a) != SAT_OK) return 0;
  return convring_supports(a, d->B) ? 1 : 0;
}

extern "C" int sat_pair32_debug_stamps(int64_t* buf) { return pair32_debug_stamps((long long*)buf); }
extern "C" int sat_convring_debug_stamps(int64_t* buf) { return convring_debug_stamps((long long*)buf); }

extern "C" int sat_conv_set_option(const char* name, int value) {
  SAT_REQUIRE(name, "conv_set_option: null name");
  // a switch of this file (0 / 1), or a setter of the file that owns the option
  static const struct { const char* name; int* flag; void (*set)(int); } options[] = {
      {"lean3", &g_lean3, nullptr}, {"lean7", &g_lean7, nullptr}, {"lean11", &g_lean11, nullptr}, {"half_tile7", &g_half_tile7, nullptr},
      {"pair32s", &g_pair32s, nullptr}, {"trim_halo", &g_trim_halo, nullptr},
      {"pair32w", nullptr, pair32w_set}, {"pair64w", nullptr, pair64w_set}, {"pair64_rpre", nullptr, pair64_rpre_set},
      {"convpost_quad", nullptr, convpost_set_quad}, {"convring", nullptr, convring_set}, {"convring_blocks", nullptr, convring_set_blocks},
      {"convring_wr", nullptr, convring_set_wr}, {"gemm_walk", nullptr, gemm_walk_set}, {"lean_balance", nullptr, lean_set_balance},
      {"pair32s_waves", nullptr, pair32s_set_waves},
      {"k1_gemm", nullptr, [](int v) { g_k1_gemm = v < 0 ? 0 : v > 3 ? 3 : v; }}};
  for (const auto& o : options) {
    if (strcmp(name, o.name)) continue;
    if (o.flag) *o.flag = value != 0;
    else o.set(value);
    return SAT_OK;
  }
  set_error("conv_set_option: unknown option '%s'", name);
  return SAT_ERR_INVALID;
}
