// Fused ResBlock1 steps of the thin generator stages (C = 16, 32): two convs, their leaky-ReLUs and the residual in one launch.
#include "common.h"
#include "conv_common.h"

namespace sat {

// ------------------------------------------------------------------------------------------------
// Fused ResBlock1 step for the thin generator stages (C <= 32), split-f16 arithmetic:
//     out = conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + x        (hifigan/nn.py:179-186)
// Unfused, a step moves five stage-sized tensors through HBM (x, t1 out, t1 in, residual, out) and the
// thin stages sit on the HBM roofline; fused, the intermediate t1 lives only in LDS (already split into
// hi|lo f16 planes, ready to be the B operand of conv2) and the step reads x once and writes out once.
// A block produces 224 output positions: conv1 is evaluated on the 256-position window that conv2
// needs (t1 positions outside the utterance are zero, they are conv2's zero padding), 8 sub-tiles of
// 32 over 4 waves; conv2 on 7 sub-tiles.  One 32-row weight tile (C = 16 is padded to 32 rows).
// ------------------------------------------------------------------------------------------------
constexpr int FP_TO = 224;    // output positions per block
constexpr int FP_W1 = 256;    // t1 window: [t0 - 16, t0 + 240)
constexpr int FP_OFF = 16;

template <int KS, int XWI, bool X16IN>
__global__ void __launch_bounds__(256, 2) resblock_pair_f16x3_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  constexpr int CO_B = 32;
  constexpr int XWP = 64 * XWI;
  constexpr int NIT = (XWI + 1) / 2;
  constexpr int W_UNITS = KS * 4 * CO_B;
  constexpr int W_IT = (W_UNITS + 255) / 256;
  uint4* ldsx = lds4;                       // [4][XWP]            input chunk, hi|lo x half
  uint4* ldsw = lds4 + 4 * XWP;             // [KS][2][2][32]      weight chunk
  uint4* ldst = ldsw + W_UNITS;             // [nchunk][4][FP_W1]  t1, all channels

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int lh = lane >> 5;
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * FP_TO;
  const int h2 = (KS - 1) / 2;
  const int xi0 = t0 - FP_OFF - p.pad_left;   // first input position of the staged tile (pad_left = conv1 halo)

  const __amdgpu_buffer_rsrc_t xrs = X16IN
      ? __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x16 + (long long)b * p.cin_g * p.T_in * 4), 0,
                                          (unsigned)(p.cin_g * p.T_in * 4), 0x00020000)
      : __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.x + (long long)b * p.x_bs), 0, (unsigned)((long long)p.cin_g * p.x_cs * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t w1rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.w_gs, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, (unsigned)p.w_gs, 0x00020000);
  const int sh = __builtin_amdgcn_readfirstlane(wave & 1);
  const int sp = __builtin_amdgcn_readfirstlane(wave >> 1);
  const int x_row_bytes = (int)p.x_cs * 4;
  const int seg_bytes = p.co_pad * 16;
  const int nchunk = p.cin_pad / CI_CHUNK;

  auto stage_w = [&](const __amdgpu_buffer_rsrc_t& rs, int chunk) {
    uint4 wst[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int u = tid + 256 * i;
      wst[i] = make_uint4(0, 0, 0, 0);
      if (u < W_UNITS)
        wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                               rs, (u % CO_B) * 16 + (u / CO_B) * seg_bytes, chunk * (KS * 4) * seg_bytes, 0));
    }
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int u = tid + 256 * i;
      if (u < W_UNITS) ldsw[u] = wst[i];
    }
  };

  // ================= phase 1: t1 = lrelu(conv1(lrelu(x)) + b1) on the 256-position window =================
  f32x16 acc[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    const int c0 = chunk * CI_CHUNK;
    __syncthreads();
    if constexpr (X16IN) {
      uint4 xst[XWI];
      const int pl = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
      for (int it = 0; it < XWI; ++it) {
        const int xi = xi0 + lane + 64 * it;
        const unsigned voff = (xi >= 0 && xi < p.T_in) ? (unsigned)((pl * p.T_in + xi) * 16) : 0x80000000u;
        xst[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, chunk * 4 * p.T_in * 16, 0));
      }
      stage_w(w1rs, chunk);
#pragma unroll
      for (int it = 0; it < XWI; ++it) ldsx[pl * XWP + lane + 64 * it] = xst[it];
    } else {
      float stg[NIT][8];
#pragma unroll
      for (int ii = 0; ii < NIT; ++ii) {
        const int it = 2 * ii + sp;
        const int xi = xi0 + lane + 64 * it;
        const unsigned voff = (it < XWI && xi >= 0 && xi < p.T_in) ? (unsigned)(xi * 4) : 0x80000000u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ci = c0 + 8 * sh + j;
          float v = 0.f;
          if (ci < p.cin_g) v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, voff, ci * x_row_bytes, 0));
          stg[ii][j] = v;
        }
      }
      stage_w(w1rs, chunk);
#pragma unroll
      for (int ii = 0; ii < NIT; ++ii) {
        const int it = 2 * ii + sp;
        if (it < XWI) {
          const int col = lane + 64 * it;
          split_hilo8(stg[ii], true, p.in_slope, ldsx[(0 * 2 + sh) * XWP + col], ldsx[(1 * 2 + sh) * XWP + col]);
        }
      }
    }
    __syncthreads();
    const uint4* wb = ldsw + lh * CO_B + l31;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const h8 a_hi = __builtin_bit_cast(h8, wb[(t * 4 + 0) * CO_B]);
      const h8 a_lo = __builtin_bit_cast(h8, wb[(t * 4 + 2) * CO_B]);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const uint4* xt = ldsx + lh * XWP + (wave + 4 * n) * 32 + l31 + t * p.dil;
        const h8 b_hi = __builtin_bit_cast(h8, xt[0]);
        const h8 b_lo = __builtin_bit_cast(h8, xt[2 * XWP]);
        mfma_split3(acc[n], a_hi, a_lo, b_hi, b_lo);
      }
    }
  }
  // t1 -> LDS as conv2's B operand.  D layout: lane (col = l31, lh) holds rows 8*rg + 4*lh + (r&3), rg = r>>2:
  // four consecutive channels = 8 bytes of the 16-byte unit (chunk' = rg>>1, half' = rg&1) of its column.
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int col = (wave + 4 * n) * 32 + l31;
    const int pos = t0 - FP_OFF + col;
    const bool inside = pos >= 0 && pos < p.T_in;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      if ((rg >> 1) >= nchunk) continue;   // C = 16: rows 16..31 are padding, no t1 plane for them
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 8 * rg + 4 * lh + k;
        float t = __builtin_fmaf(acc[n][4 * rg + k], p.w_descale1, row < p.rows_g ? p.bias1[row] : 0.f);
        t = lrelu_max(t, p.in_slope);
        v[k] = inside ? t : 0.f;
      }
      const auto h01 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
      const auto h23 = __builtin_amdgcn_cvt_pkrtz(v[2], v[3]);
      const auto l01 = split_lo2(h01, v[0], v[1]);
      const auto l23 = split_lo2(h23, v[2], v[3]);
      uint2* dh = (uint2*)(ldst + (((rg >> 1) * 4 + 0 * 2 + (rg & 1)) * FP_W1 + col)) + lh;
      uint2* dl = (uint2*)(ldst + (((rg >> 1) * 4 + 1 * 2 + (rg & 1)) * FP_W1 + col)) + lh;
      *dh = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
      *dl = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
    }
  }

  // ================= phase 2: out = conv2(t1) + b2 + x =================
  f32x16 acc2[1][2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[0][n][r] = 0.f;
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    __syncthreads();
    stage_w(w2rs, chunk);
    __syncthreads();
    const uint4* wb = ldsw + lh * CO_B + l31;
    const uint4* tb = ldst + (chunk * 4 + lh) * FP_W1 + FP_OFF - h2 + l31;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const h8 a_hi = __builtin_bit_cast(h8, wb[(t * 4 + 0) * CO_B]);
      const h8 a_lo = __builtin_bit_cast(h8, wb[(t * 4 + 2) * CO_B]);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (wave + 4 * n < FP_TO / 32) {   // wave-uniform: 7 output sub-tiles over 4 waves
          const uint4* xt = tb + (wave + 4 * n) * 32 + t;
          const h8 b_hi = __builtin_bit_cast(h8, xt[0]);
          const h8 b_lo = __builtin_bit_cast(h8, xt[2 * FP_W1]);
          mfma_split3(acc2[0][n], a_hi, a_lo, b_hi, b_lo);
        }
      }
    }
  }
  conv_epilogue<1, 2>(p, acc2, b, 0, 0, t0 + wave * 32, l31, lh, 128, t0 + FP_TO);
}

// (one exported launcher per kernel: its instance for the 3, 7 or 11 taps of a.ksize; the entry point has checked the count)
template <int KS>
static int launch_pair_ks(const ConvArgs& a, int B, hipStream_t s) {
  constexpr int XWI = (FP_W1 + (KS - 1) * 5 + 63) / 64;
  ConvArgs p = a;
  if (FP_W1 + (p.ksize - 1) * p.dil > 64 * XWI) {
    set_error("resblock_pair: dilation %d too large", p.dil);
    return SAT_ERR_INVALID;
  }
  p.co_tiles_g = 1;
  const size_t lds_bytes = ((size_t)4 * 64 * XWI + (size_t)KS * 4 * 32 + (size_t)(p.cin_pad / CI_CHUNK) * 4 * FP_W1) * 16;
  auto kern = p.x16 ? resblock_pair_f16x3_kernel<KS, XWI, true> : resblock_pair_f16x3_kernel<KS, XWI, false>;
  dim3 grid(ceil_div(p.T_q, FP_TO), 1, B);
  if (int st = launch_lds(kern, grid, lds_bytes, s, p)) return st;
  SAT_LAUNCH_CHECK("resblock_pair_f16x3_kernel");
  return SAT_OK;
}
int launch_pair(const ConvArgs& a, int B, hipStream_t s) { return a.ksize == 3 ? launch_pair_ks<3>(a, B, s) : a.ksize == 7 ? launch_pair_ks<7>(a, B, s) : launch_pair_ks<11>(a, B, s); }

// ------------------------------------------------------------------------------------------------
// ResBlock1 step for the C = 16 stage on the 16x16x32 MFMA shape: 16 rows = the 16 channels exactly
// (the 32x32 tile pads them to 32 and wastes half the matrix work), K = 32 = a PAIR of taps x 16
// channels.  Split planes in, split planes out.  Persistent blocks: both convs' A fragments stay in
// registers (every wave holds all 16 rows), the input tile and the intermediate t1 live in LDS (36 KB,
// 3-4 blocks per CU), the next tile's input is prefetched into registers under this tile's matrix
// work, and the residual comes from the input tile the block already holds.
//   lanes: A[row l&15][k = 8(l>>4)..], B[k = 8(l>>4)..][col l&15], D col = l&15, rows 4(l>>4) + r
//   k-group g = l>>4: tap (g>>1) of the pair, channel half (g&1) -> the same 16-byte units as before
// ------------------------------------------------------------------------------------------------
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int KS>
__global__ void __launch_bounds__(256, KS == 11 ? 2 : 3) resblock_pair16_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  constexpr int XWI = 5, XWP = 64 * XWI;
  constexpr int NTP = (KS + 1) / 2;         // tap pairs; an odd tap count gets a zero phantom tap
  uint4* ldsx = lds4;                       // [4][XWP]
  uint4* ldst = ldsx + 4 * XWP;             // [4][FP_W1]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int j16 = lane & 15;
  const int g = lane >> 4;
  const int gh = g & 1, gt = g >> 1;        // channel half / tap of the pair
  const int h2 = (KS - 1) / 2;
  const unsigned OOB = 0x80000000u;

  const __amdgpu_buffer_rsrc_t w1rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.w_gs, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, (unsigned)p.w_gs, 0x00020000);
  const int seg_bytes = p.co_pad * 16;
  const int pl = __builtin_amdgcn_readfirstlane(wave);

  // persistent walk: workgroups go round-robin to the 8 XCDs, so XCD x (= blockIdx.x & 7) owns the contiguous tile
  // range [x, x+1) * pp_per_xcd and its pp_nslots blocks take consecutive tiles of it at the same time — neighbouring
  // tiles share their 96-column halo through that XCD's L2.  Weights are staged once per block; the input tile of
  // the next step is loaded into registers while this one computes.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int tile_end = min((xcd + 1) * p.pp_per_xcd, p.pp_total);
  int tile = xcd * p.pp_per_xcd + slot;
  if (tile >= tile_end) return;

  uint4 xst[XWI];
  auto issue_x = [&](int tl) {
    const int ub = __builtin_amdgcn_readfirstlane(tl / p.pp_tiles_t);
    const int xi_0 = (tl - ub * p.pp_tiles_t) * FP_TO - FP_OFF - p.pad_left;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)p.x16 + (long long)ub * 16 * p.T_in * 4), 0, (unsigned)(16 * p.T_in * 4), 0x00020000);
#pragma unroll
    for (int it = 0; it < XWI; ++it) {
      const int xi = xi_0 + lane + 64 * it;
      const unsigned voff = (xi >= 0 && xi < p.T_in) ? (unsigned)((pl * p.T_in + xi) * 16) : OOB;
      xst[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, 0, 0));
    }
  };
  issue_x(tile);
  // both convs' A fragments live in registers for the block's whole walk (the 16 rows are all the channels, so every
  // wave holds the same ones): packed units [tap][hi|lo][half][16 rows], the phantom tap of an odd count reads zeros
  h8 w1h[NTP], w1l[NTP], w2h[NTP], w2l[NTP];
#pragma unroll
  for (int tp = 0; tp < NTP; ++tp) {
    const int tap = 2 * tp + gt;
    const unsigned vh = tap < KS ? (unsigned)(j16 * 16 + (tap * 4 + 0 + gh) * seg_bytes) : OOB;
    const unsigned vl = tap < KS ? (unsigned)(j16 * 16 + (tap * 4 + 2 + gh) * seg_bytes) : OOB;
    w1h[tp] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(w1rs, vh, 0, 0));
    w1l[tp] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(w1rs, vl, 0, 0));
    w2h[tp] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(w2rs, vh, 0, 0));
    w2l[tp] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(w2rs, vl, 0, 0));
  }
  float bias1[4], bias2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bias1[k] = p.bias1[4 * g + k];
    bias2[k] = p.bias[4 * g + k];
  }
  for (;;) {
  const int b = __builtin_amdgcn_readfirstlane(tile / p.pp_tiles_t);     // (division runs on the vector ALU: keep it scalar)
  const int t0 = (tile - b * p.pp_tiles_t) * FP_TO;
  __syncthreads();            // the previous step's readers of the input tile and of t1 are done
#pragma unroll
  for (int it = 0; it < XWI; ++it) ldsx[pl * XWP + lane + 64 * it] = xst[it];
  __syncthreads();
  const int next = tile + p.pp_nslots;
  const bool more = next < tile_end;
  if (more) issue_x(next);
  __builtin_amdgcn_sched_barrier(0);

  // ================= phase 1: t1 = lrelu(conv1(x planes) + b1) on the 256-column window =================
  f32x4v acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = f32x4v{0.f, 0.f, 0.f, 0.f};
  {
    const uint4* xl = ldsx + gh * XWP + wave * 64 + j16;
#pragma unroll
    for (int tp = 0; tp < NTP; ++tp) {
      const int tap = 2 * tp + gt;
      const h8 a_hi = w1h[tp], a_lo = w1l[tp];
      const uint4* xt = xl + tap * p.dil;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const h8 b_hi = __builtin_bit_cast(h8, xt[16 * s]);
        const h8 b_lo = __builtin_bit_cast(h8, xt[2 * XWP + 16 * s]);
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, b_hi, acc[s], 0, 0, 0);
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_lo, acc[s], 0, 0, 0);
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, acc[s], 0, 0, 0);
      }
    }
  }
  // t1 -> LDS planes: this lane's four consecutive channels 4g .. 4g+3 = 8 bytes of the unit (half g>>1)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int col = wave * 64 + 16 * s + j16;
    const int pos = t0 - FP_OFF + col;
    const bool inside = pos >= 0 && pos < p.T_in;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float t = __builtin_fmaf(acc[s][k], p.w_descale1, bias1[k]);
      t = lrelu_max(t, p.in_slope);
      v[k] = inside ? t : 0.f;      // t1 outside the utterance is conv2's zero padding
    }
    const auto h01 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
    const auto h23 = __builtin_amdgcn_cvt_pkrtz(v[2], v[3]);
    const auto l01 = split_lo2(h01, v[0], v[1]);
    const auto l23 = split_lo2(h23, v[2], v[3]);
    ((uint2*)(ldst + (0 + gt) * FP_W1 + col))[gh] = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
    ((uint2*)(ldst + (2 + gt) * FP_W1 + col))[gh] = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
  }
  __syncthreads();

  // ================= phase 2: out = conv2(t1) + b2 + x on 224 columns (14 sub-tiles: 4, 4, 4, 2) =================
  const int ns = wave < 3 ? 4 : 2;
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = f32x4v{0.f, 0.f, 0.f, 0.f};
  {
    const uint4* tl = ldst + gh * FP_W1 + wave * 64 + j16 + FP_OFF - h2;
#pragma unroll
    for (int tp = 0; tp < NTP; ++tp) {
      const int tap = 2 * tp + gt;
      const h8 a_hi = w2h[tp], a_lo = w2l[tp];
      const uint4* xt = tl + tap;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < ns) {     // wave-uniform
          const h8 b_hi = __builtin_bit_cast(h8, xt[16 * s]);
          const h8 b_lo = __builtin_bit_cast(h8, xt[2 * FP_W1 + 16 * s]);
          acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, b_hi, acc[s], 0, 0, 0);
          acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_lo, acc[s], 0, 0, 0);
          acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, acc[s], 0, 0, 0);
        }
      }
    }
  }

  // ================= epilogue: + b2 + x (from the input tile in LDS), MRF sum, stores =================
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.y + (long long)b * p.y_bs), 0, (unsigned)(16 * p.y_cs * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t y16rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.y16 ? (char*)p.y16 + (long long)b * 16 * p.T_q * 4 : (char*)p.y), 0, p.y16 ? (unsigned)(16 * p.T_q * 4) : 0u, 0x00020000);
  const int y_rb = (int)p.y_cs * 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= ns) continue;
    const int o = wave * 64 + 16 * s + j16;
    const int q = t0 + o;
    const bool ok = q < p.T_q;
    // residual: the block input at this position, still in the LDS tile (planes of lrelu(x): undo it)
    const int xcol = o + FP_OFF + p.pad_left;
    const uint2 rh = ((const uint2*)(ldsx + (0 + gt) * XWP + xcol))[gh];
    const uint2 rl = ((const uint2*)(ldsx + (2 + gt) * XWP + xcol))[gh];
    float r[4];
    decode_res16(__builtin_bit_cast(float, rh.x), __builtin_bit_cast(float, rh.y), __builtin_bit_cast(float, rl.x),
                 __builtin_bit_cast(float, rl.y), p.res16_inv, r);
    const unsigned yoff = ok ? (unsigned)((4 * g) * y_rb + q * 4) : OOB;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __builtin_fmaf(acc[s][k], p.w_descale, bias2[k]) + r[k];
    if (p.accum) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yrs, yoff + k * y_rb, 0, 0)) + v[k];
    }
    if (p.accum_div != 0.f) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] / p.accum_div;
    }
    if (!p.no_y && !p.no_store) {
#pragma unroll
      for (int k = 0; k < 4; ++k) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[k]), yrs, yoff + k * y_rb, 0, 0);
    }
    if (p.y16) {
      float u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = lrelu_max(v[k], p.y16_slope);
      const auto h01 = __builtin_amdgcn_cvt_pkrtz(u[0], u[1]);
      const auto h23 = __builtin_amdgcn_cvt_pkrtz(u[2], u[3]);
      const auto l01 = split_lo2(h01, u[0], u[1]);
      const auto l23 = split_lo2(h23, u[2], u[3]);
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      u32x2 hv, lv;
      hv[0] = __builtin_bit_cast(unsigned, h01); hv[1] = __builtin_bit_cast(unsigned, h23);
      lv[0] = __builtin_bit_cast(unsigned, l01); lv[1] = __builtin_bit_cast(unsigned, l23);
      const unsigned off = ok ? (unsigned)(((0 + gt) * p.T_q + q) * 16 + 8 * gh) : OOB;
      __builtin_amdgcn_raw_buffer_store_b64(hv, y16rs, off, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b64(lv, y16rs, off, 2 * p.T_q * 16, 0);
    }
  }
  if (!more) break;
  tile = next;
  }
}

template <int KS>
static int launch_pair16_ks(const ConvArgs& a, int B, hipStream_t s) {
  ConvArgs p = a;
  if (FP_W1 + (p.ksize - 1) * p.dil > 320) {
    set_error("resblock_pair: dilation %d too large", p.dil);
    return SAT_ERR_INVALID;
  }
  const size_t lds_bytes = ((size_t)4 * 320 + 4 * FP_W1) * 16;
  auto kern = resblock_pair16_kernel<KS>;
  // persistent: as many blocks as fit the chip at once (LDS-limited), a multiple of the 8 XCDs
  const int per_cu = KS == 11 ? 2 : KS == 7 ? 3 : 4;    // register-limited: 16 B x 4 x ceil(KS/2) weight fragments per lane
  p.pp_tiles_t = ceil_div(p.T_q, FP_TO);
  p.pp_total = p.pp_tiles_t * B;
  p.pp_per_xcd = ceil_div(p.pp_total, 8);
  p.pp_nslots = std::max(1, std::min(32 * per_cu, p.pp_per_xcd));
  dim3 grid(8 * p.pp_nslots, 1, 1);
  if (int st = launch_lds(kern, grid, lds_bytes, s, p)) return st;
  SAT_LAUNCH_CHECK("resblock_pair16_kernel");
  return SAT_OK;
}
int launch_pair16(const ConvArgs& a, int B, hipStream_t s) { return a.ksize == 3 ? launch_pair16_ks<3>(a, B, s) : a.ksize == 7 ? launch_pair16_ks<7>(a, B, s) : launch_pair16_ks<11>(a, B, s); }

// ------------------------------------------------------------------------------------------------
// ResBlock1 step for C = 32 with split planes end to end: the fused pair kernel above with its four
// global-load round trips (x + W1 chunk 0, x + W1 chunk 1, W2 chunk 0, W2 chunk 1) pipelined through
// registers — each is issued before the previous step's MFMA phase — and the residual (the input
// planes again, L2-resident) prefetched under the last one.
// ------------------------------------------------------------------------------------------------
template <int KS>
__global__ void __launch_bounds__(256, 3) resblock_pair32_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  constexpr int CO_B = 32;
  constexpr int XWI = 5, XWP = 64 * XWI;
  constexpr int W_UNITS = KS * 4 * CO_B;
  constexpr int W_IT = (W_UNITS + 255) / 256;
  // Three blocks per CU (168 VGPRs allow it; the kernel waits on memory 45 % of its cycles at two): the t1 image lies
  // OVER the input chunk, which is dead once conv1's last MFMA phase has read it (one barrier in between), and for 11
  // taps the t1 window is trimmed to the 234 columns conv2 reads — 22.5 KB of weights + 29.5 KB = 52 KB per block.
  constexpr int W1 = KS == 11 ? 236 : FP_W1;      // t1 window [t0 - OFF, t0 - OFF + W1)
  constexpr int OFF = KS == 11 ? 6 : FP_OFF;
  static_assert(OFF >= (KS - 1) / 2 && OFF - (KS - 1) / 2 + FP_TO + KS - 1 <= W1, "conv2 reads t1 columns OFF - h2 .. OFF - h2 + 224 + 2 h2");
  uint4* ldsw = lds4;                       // [KS][4][32]    weight chunk
  uint4* ldsx = lds4 + W_UNITS;             // [4][XWP]       input chunk
  uint4* ldst = ldsx;                       // [2][4][W1]     t1, both chunks (over the input chunk)
  static_assert(2 * 4 * W1 >= 4 * XWP, "the LDS size of the launcher is that of the t1 image");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int lh = lane >> 5;
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * FP_TO;
  const int h2 = (KS - 1) / 2;
  const int xi0 = t0 - OFF - p.pad_left;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const char*)p.x16 + (long long)b * 32 * p.T_in * 4), 0, (unsigned)(32 * p.T_in * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t w1rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.w_gs, 0x00020000);
  const __amdgpu_buffer_rsrc_t w2rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, (unsigned)p.w_gs, 0x00020000);
  const int seg_bytes = p.co_pad * 16;
  const int pl = __builtin_amdgcn_readfirstlane(wave);

  uint4 xst[XWI], wst[W_IT];
  auto issue_x = [&](int chunk) {
#pragma unroll
    for (int it = 0; it < XWI; ++it) {
      const int xi = xi0 + lane + 64 * it;
      // (p.xw: the columns conv1 reads — its W1-column window plus the halo of the dilated taps; the rest of the 320 is never multiplied)
      const unsigned voff = (xi >= 0 && xi < p.T_in && lane + 64 * it < p.xw) ? (unsigned)((pl * p.T_in + xi) * 16) : 0x80000000u;
      xst[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, chunk * 4 * p.T_in * 16, 0));
    }
  };
  auto issue_w = [&](const __amdgpu_buffer_rsrc_t& rs, int chunk) {
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int u = tid + 256 * i;
      const unsigned voff = u < W_UNITS ? (unsigned)((u % CO_B) * 16 + (u / CO_B) * seg_bytes) : 0x80000000u;
      wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, chunk * (KS * 4) * seg_bytes, 0));
    }
  };
  auto publish_x = [&]() {
#pragma unroll
    for (int it = 0; it < XWI; ++it) ldsx[pl * XWP + lane + 64 * it] = xst[it];
  };
  auto publish_w = [&]() {
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int u = tid + 256 * i;
      if (u < W_UNITS) ldsw[u] = wst[i];
    }
  };
  f32x16 acc[1][2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][n][r] = 0.f;
  };
  // one chunk of MFMAs: B fragments at `base + n*128 + tap*step` in an image of plane pitch `pitch`
  auto mfma_chunk = [&](const uint4* base, int pitch, int step, bool seven) {
    const uint4* wb = ldsw + lh * CO_B + l31;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const h8 a_hi = __builtin_bit_cast(h8, wb[(t * 4 + 0) * CO_B]);
      const h8 a_lo = __builtin_bit_cast(h8, wb[(t * 4 + 2) * CO_B]);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (!seven || wave + 4 * n < FP_TO / 32) {   // wave-uniform: conv2 has 7 output sub-tiles over 4 waves
          const uint4* xt = base + n * 128 + t * step;
          const h8 b_hi = __builtin_bit_cast(h8, xt[0]);
          const h8 b_lo = __builtin_bit_cast(h8, xt[2 * pitch]);
          mfma_split3(acc[0][n], a_hi, a_lo, b_hi, b_lo);
        }
      }
    }
  };
  const uint4* xbase = ldsx + lh * XWP + wave * 32 + l31;

  // ---- conv1, chunk 0 and 1 ----
  issue_x(0);
  issue_w(w1rs, 0);
  zero_acc();
  publish_x();
  publish_w();
  __syncthreads();
  issue_x(1);
  issue_w(w1rs, 1);
  __builtin_amdgcn_sched_barrier(0);
  mfma_chunk(xbase, XWP, p.dil, false);
  __syncthreads();
  publish_x();
  publish_w();
  __syncthreads();
  issue_w(w2rs, 0);
  __builtin_amdgcn_sched_barrier(0);
  mfma_chunk(xbase, XWP, p.dil, false);
  __syncthreads();                          // every wave is done reading the input chunk: t1 goes over it
  // t1 -> LDS as conv2's B operand (hi|lo planes of both chunks)
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int col = (wave + 4 * n) * 32 + l31;
    const int pos = t0 - OFF + col;
    const bool inside = pos >= 0 && pos < p.T_in;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float t = __builtin_fmaf(acc[0][n][4 * rg + k], p.w_descale1, p.bias1[8 * rg + 4 * lh + k]);
        t = lrelu_max(t, p.in_slope);
        v[k] = inside ? t : 0.f;
      }
      const auto h01 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
      const auto h23 = __builtin_amdgcn_cvt_pkrtz(v[2], v[3]);
      const auto l01 = split_lo2(h01, v[0], v[1]);
      const auto l23 = split_lo2(h23, v[2], v[3]);
      if (col < W1) {
        ((uint2*)(ldst + (((rg >> 1) * 4 + 0 + (rg & 1)) * W1 + col)))[lh] =
            make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
        ((uint2*)(ldst + (((rg >> 1) * 4 + 2 + (rg & 1)) * W1 + col)))[lh] =
            make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
      }
    }
  }
  // ---- conv2, chunk 0 and 1 ----
  zero_acc();
  __syncthreads();
  publish_w();
  __syncthreads();
  issue_w(w2rs, 1);
  __builtin_amdgcn_sched_barrier(0);
  const uint4* tbase = ldst + lh * W1 + OFF - h2 + wave * 32 + l31;
  mfma_chunk(tbase, W1, 1, true);
  __syncthreads();
  publish_w();
  __syncthreads();
  float rpre[1][2][16];
  epilogue_prefetch_res<1, 2>(p, rpre, b, 0, 0, t0 + wave * 32, l31, lh, 128, t0 + FP_TO);
  __builtin_amdgcn_sched_barrier(0);
  mfma_chunk(tbase + 4 * W1, W1, 1, true);
  conv_epilogue<1, 2, true>(p, acc, b, 0, 0, t0 + wave * 32, l31, lh, 128, t0 + FP_TO, rpre);
}

template <int KS>
static int launch_pair32_ks(const ConvArgs& a, int B, hipStream_t s) {
  ConvArgs p = a;
  if (FP_W1 + (p.ksize - 1) * p.dil > 320) {
    set_error("resblock_pair: dilation %d too large", p.dil);
    return SAT_ERR_INVALID;
  }
  const size_t lds_bytes = ((size_t)KS * 4 * 32 + (size_t)2 * 4 * (KS == 11 ? 236 : FP_W1)) * 16;   // weights + t1 (over the input chunk)
  auto kern = resblock_pair32_kernel<KS>;
  dim3 grid(ceil_div(p.T_q, FP_TO), 1, B);
  if (int st = launch_lds(kern, grid, lds_bytes, s, p)) return st;
  SAT_LAUNCH_CHECK("resblock_pair32_kernel");
  return SAT_OK;
}
int launch_pair32(const ConvArgs& a, int B, hipStream_t s) { return a.ksize == 3 ? launch_pair32_ks<3>(a, B, s) : a.ksize == 7 ? launch_pair32_ks<7>(a, B, s) : launch_pair32_ks<11>(a, B, s); }

}  // namespace sat
