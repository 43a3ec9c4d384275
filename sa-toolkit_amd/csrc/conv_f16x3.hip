// The split-f16 form of the fused conv1d on 32x32x16 MFMA tiles: from f32 input, from split planes (software-pipelined),
// and the 1x1 GEMM form.  GEMM view and epilogue as in conv1d_mfma.hip; the epilogue itself is conv_common.h's.
#include "common.h"
#include "conv_common.h"

namespace sat {

// ------------------------------------------------------------------------------------------------
// Every f32 operand is carried as hi + lo f16 (hi = x rounded to f16, lo = x - hi,
// together 22 significand bits) and a product is hi*hi + hi*lo + lo*hi on the f16 matrix cores with
// f32 accumulation (v_mfma_f32_32x32x16_f16: 16 input channels per instruction in 32 cycles, i.e.
// 16x the f32-MFMA rate, x3 instructions).  The dropped lo*lo term and the lo rounding are ~2^-21
// relative per product, two orders of magnitude below the path's 1e-4 RMS parity bar and at the
// level of the f32 re-association noise measured against the CPU oracle.  Used for the generator
// (activations O(1), inside f16 range); the TDNNF/VQ path stays on the exact-f32 kernel because its
// arg-min decisions are sensitive to 1e-6 perturbations.
//
// At these MFMA rates the weight fragments can no longer be streamed from L2 per wave (that alone
// would need ~43 B/clk/CU): a block = 4 waves side by side in time over ONE 32*MT-row weight tile, and
// per 16-channel chunk both operands are staged in LDS:
//   W  [tap][hi|lo][channel half][row]      x 16 B (8 f16)  — a straight copy of the packed weights
//   X  [hi|lo][channel half][column]        x 16 B          — lrelu + hi/lo split while staging
// so every A and B fragment is one conflict-free ds_read_b128 and the main loop issues no global
// loads.  Weights arrive packed as w16[g][chunk][tap][hi|lo][half][co_pad][8] f16.
// ------------------------------------------------------------------------------------------------

template <int MT, int NT, int KS, int XWI>
__global__ void __launch_bounds__(256, 2) conv1d_f16x3_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  constexpr int CO_B = 32 * MT;
  constexpr int T_B = 128 * NT;          // 4 waves x NT x 32 positions
  constexpr int XWP = 64 * XWI;
  constexpr int NIT = (XWI + 1) / 2;
  constexpr int W_UNITS = KS * 4 * CO_B;  // 16-byte units of one weight chunk
  constexpr int W_IT = (W_UNITS + 255) / 256;
  uint4* ldsx = lds4;                     // [4][XWP]
  uint4* ldsw = lds4 + 4 * XWP;           // [KS][2][2][CO_B]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int lh = lane >> 5;

  const int b = blockIdx.z;
  const int g = blockIdx.y / p.co_tiles_g;
  const int cot = blockIdx.y - g * p.co_tiles_g;
  const int co_w = cot * CO_B;            // every wave of the block works on the same rows
  const int q_b = blockIdx.x * T_B;
  const int q_w = q_b + wave * (32 * NT);
  const int xi0 = q_b - p.pad_left;

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.x + (long long)b * p.x_bs + (long long)(g * p.cin_g) * p.x_cs), 0,
      (unsigned)((long long)p.cin_g * p.x_cs * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const char*)p.w + (long long)g * p.w_gs), 0, (unsigned)p.w_gs, 0x00020000);
  const int sh = __builtin_amdgcn_readfirstlane(wave & 1);   // channel half staged by this wave
  const int sp = __builtin_amdgcn_readfirstlane(wave >> 1);  // parity of the 64-column slices it stages
  const int x_row_bytes = (int)p.x_cs * 4;
  const int seg_bytes = p.co_pad * 16;                        // one (tap, part, half) segment of all rows

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  int chunk = 0;
  for (int c0 = 0; c0 < p.cin_pad; c0 += CI_CHUNK, ++chunk) {
    __syncthreads();
    {
      // ---- issue every load of the chunk first: weights (copy) then the input tile ----
      uint4 wst[W_IT];
#pragma unroll
      for (int i = 0; i < W_IT; ++i) {
        const int u = tid + 256 * i;
        const int seg = u / CO_B, r = u % CO_B;
        wst[i] = make_uint4(0, 0, 0, 0);
        if (u < W_UNITS)
          wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 wrs, (co_w + r) * 16 + seg * seg_bytes, chunk * (KS * 4) * seg_bytes, 0));
      }
      {
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
#pragma unroll
        for (int i = 0; i < W_IT; ++i) {
          const int u = tid + 256 * i;
          if (u < W_UNITS) ldsw[u] = wst[i];
        }
#pragma unroll
        for (int ii = 0; ii < NIT; ++ii) {
          const int it = 2 * ii + sp;
          if (it < XWI) {
            unsigned hi[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float x0 = stg[ii][2 * j], x1 = stg[ii][2 * j + 1];
              if (p.in_lrelu) {
                x0 = lrelu_max(x0, p.in_slope);
                x1 = lrelu_max(x1, p.in_slope);
              }
              split_hilo2(x0, x1, hi[j], lo[j]);
            }
            const int col = lane + 64 * it;
            ldsx[(0 * 2 + sh) * XWP + col] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            ldsx[(1 * 2 + sh) * XWP + col] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
          }
        }
      }
    }
    __syncthreads();

    const uint4* xb = ldsx + lh * XWP + wave * (32 * NT) + l31;
    const uint4* wb = ldsw + lh * CO_B + l31;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      h8 a_hi[MT], a_lo[MT], b_hi[NT], b_lo[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        a_hi[m] = __builtin_bit_cast(h8, wb[(t * 4 + 0) * CO_B + m * 32]);
        a_lo[m] = __builtin_bit_cast(h8, wb[(t * 4 + 2) * CO_B + m * 32]);
      }
      const uint4* xt = xb + t * p.dil;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        b_hi[n] = __builtin_bit_cast(h8, xt[n * 32]);
        b_lo[n] = __builtin_bit_cast(h8, xt[2 * XWP + n * 32]);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) mfma_split3(acc[m][n], a_hi[m], a_lo[m], b_hi[n], b_lo[n]);
    }
  }
  conv_epilogue<MT, NT>(p, acc, b, g, co_w, q_w, l31, lh);
}

// ------------------------------------------------------------------------------------------------
// Split-plane input (x16): the B operand arrives as ready hi|lo f16 planes, staging is a 16-byte copy.
// Software-pipelined over K-chunks through registers: chunk c+1's global loads (weights + planes,
// W_IT + XWI 16-byte loads per lane) are issued right after chunk c's tile is published in LDS and
// stay in flight during its MFMA phase; during the LAST chunk's MFMA phase the same registers
// prefetch the residual the epilogue adds.  Measured with s_memtime stamps (tools/stamp_conv.hip) the
// un-pipelined form spent 1.7-2.7k cycles per chunk waiting on loads and 22-32k cycles in the epilogue
// against a 4.2k-cycle MFMA phase (k = 11).
// ------------------------------------------------------------------------------------------------
// ---- polyphase (transposed-conv) output straight to split planes.  The accumulator rows are (channel, phase)
// pairs and a lane holds a column q of them, but a plane unit is 8 CHANNELS at one output time t = q*up + phase:
// the tile goes through LDS once (f32, pitch +1 against bank conflicts between phases) and is read back in
// plane order — 16-byte stores, consecutive lanes on consecutive times.  Replaces the f32 store of the
// upsampled tensor and the separate split pass (12 bytes per element of HBM traffic).
// Needs 32*MT % (8*up) == 0 (a block's rows are whole 8-channel groups).
template <int MT, int NT>
__device__ __forceinline__ void polyphase_planes_epilogue(const ConvArgs& p, f32x16 (&acc)[MT][NT], float* tile, int b,
                                                          int co_w, int q_b, int wave, int l31, int lh) {
  constexpr int CO_B = 32 * MT, T_B = 128 * NT, PITCH = T_B + 1;
  const int up = p.up;
  __syncthreads();                                   // every wave is done with the operand tiles
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int grow = co_w + row;
        const float bias = (p.bias && grow < p.rows_g) ? p.bias[grow / up] : 0.f;
        tile[row * PITCH + wave * (32 * NT) + n * 32 + l31] = __builtin_fmaf(acc[m][n][r], p.w_descale, bias);
      }
  __syncthreads();
  const int T_out = p.T_q * up;
  uint4* yb = (uint4*)p.y16 + (long long)b * (p.cout_g / 4) * T_out;     // cout_g * T_out * 4 bytes per utterance
  const int n_tt = T_B * up;                            // output times of the block
  const int n_cg = CO_B / (8 * up);                     // 8-channel groups of the block
  for (int it = threadIdx.x; it < n_cg * n_tt; it += 256) {
    const int cg = it / n_tt, tt = it - cg * n_tt;
    const int ql = tt / up, ph = tt - ql * up;
    const int t = q_b * up + tt;
    const int c0 = co_w / up + cg * 8;                  // first channel of the group
    if (t >= T_out || c0 >= p.cout_g) continue;
    unsigned hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x0 = tile[((cg * 8 + 2 * j) * up + ph) * PITCH + ql];
      float x1 = tile[((cg * 8 + 2 * j + 1) * up + ph) * PITCH + ql];
      x0 = lrelu_max(x0, p.y16_slope);
      x1 = lrelu_max(x1, p.y16_slope);
      split_hilo2(x0, x1, hi[j], lo[j]);
    }
    const long long u = ((long long)((c0 >> 4) * 4 + ((c0 >> 3) & 1))) * T_out + t;
    yb[u] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    yb[u + 2LL * T_out] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

// S: 16-channel sub-chunks per pipeline stage.  With few taps the matrix work of a 16-channel chunk (1152
// cycles at 3 taps) is dwarfed by the ~2800 cycles of barriers, LDS stores and load issue around it: S = 2
// halves the number of stages.
template <int MT, int NT, int KS, int XWI, bool F8, int S>
__global__ void __launch_bounds__(256, 2) conv1d_f16x3_planes_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  constexpr int CO_B = 32 * MT;
  constexpr int T_B = 128 * NT;
  constexpr int XWP = 64 * XWI;
  constexpr int W_UNITS = KS * 4 * CO_B;
  constexpr int W_IT = (W_UNITS + 255) / 256;
  uint4* ldsx = lds4;                     // [S][4][XWP]
  uint4* ldsw = lds4 + S * 4 * XWP;       // [S][KS][2][2][CO_B]
  static_assert(!F8 || S == 1, "e4m3 cross terms: one sub-chunk per stage");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int lh = lane >> 5;
  const int b = blockIdx.z;
  const int co_w = blockIdx.y * CO_B;
  const int q_b = blockIdx.x * T_B;
  const int q_w = q_b + wave * (32 * NT);
  const int xi0 = q_b - p.pad_left;
  const int nch = p.cin_pad / CI_CHUNK / S;   // pipeline stages

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const char*)p.x16 + (long long)b * p.cin_g * p.T_in * 4), 0, (unsigned)(p.cin_g * p.T_in * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.w_gs, 0x00020000);
  const int seg_bytes = p.co_pad * 16;
  const int pl = __builtin_amdgcn_readfirstlane(wave);    // plane (part*2 + half) this wave copies
  const int x_chunk_bytes = 4 * p.T_in * 16;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  uint4 wst[S][W_IT], xst[S][XWI];
  auto issue_loads = [&](int stage) {
#pragma unroll
    for (int sc = 0; sc < S; ++sc) {
      const int chunk = stage * S + sc;
#pragma unroll
      for (int i = 0; i < W_IT; ++i) {
        const int u = tid + 256 * i;
        const int seg = u / CO_B, r = u % CO_B;
        wst[sc][i] = make_uint4(0, 0, 0, 0);
        if (u < W_UNITS)
          wst[sc][i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                      wrs, (co_w + r) * 16 + seg * seg_bytes, chunk * (KS * 4) * seg_bytes, 0));
      }
#pragma unroll
      for (int it = 0; it < XWI; ++it) {
        const int xi = xi0 + lane + 64 * it;
        const unsigned voff = (xi >= 0 && xi < p.T_in) ? (unsigned)((pl * p.T_in + xi) * 16) : 0x80000000u;
        xst[sc][it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, chunk * x_chunk_bytes, 0));
      }
    }
  };
  auto publish = [&]() {
#pragma unroll
    for (int sc = 0; sc < S; ++sc) {
#pragma unroll
      for (int i = 0; i < W_IT; ++i) {
        const int u = tid + 256 * i;
        if (u < W_UNITS) ldsw[sc * W_UNITS + u] = wst[sc][i];
      }
#pragma unroll
      for (int it = 0; it < XWI; ++it) ldsx[(sc * 4 + pl) * XWP + lane + 64 * it] = xst[sc][it];
    }
  };
  const uint4* xb0 = ldsx + lh * XWP + wave * (32 * NT) + l31;
  const uint4* wb0 = ldsw + lh * CO_B + l31;
  // F8: per-lane E8M0 scale bytes of the cross-term MFMA (lanes 0-31: W_lo8 . x_hi8, lanes 32-63: W_hi8 . x_lo8)
  const int sc_a = lh ? F8_E_WHI : F8_E_WLO;
  const int sc_b = lh ? F8_E_XLO : F8_E_XHI;
  auto mfma_phase = [&]() {
   if constexpr (!F8) {
    // fragments of tap idx + 1 are read from LDS ahead of tap idx's MFMAs (double-buffered registers; the
    // scheduler would otherwise sink the reads to their first use and every tap would start on an LDS round trip)
    h8 fa[2][MT][2], fb[2][NT][2];
    auto ld = [&](int buf, int sc, int t) {
      const uint4* wb = wb0 + sc * W_UNITS;
      const uint4* xt = xb0 + sc * 4 * XWP + t * p.dil;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        fa[buf][m][0] = __builtin_bit_cast(h8, wb[(t * 4 + 0) * CO_B + m * 32]);
        fa[buf][m][1] = __builtin_bit_cast(h8, wb[(t * 4 + 2) * CO_B + m * 32]);
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        fb[buf][n][0] = __builtin_bit_cast(h8, xt[n * 32]);
        fb[buf][n][1] = __builtin_bit_cast(h8, xt[2 * XWP + n * 32]);
      }
    };
    ld(0, 0, 0);
#pragma unroll
    for (int idx = 0; idx < S * KS; ++idx) {
      if (idx + 1 < S * KS) ld((idx + 1) & 1, (idx + 1) / KS, (idx + 1) % KS);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) mfma_split3(acc[m][n], fa[idx & 1][m][0], fa[idx & 1][m][1], fb[idx & 1][n][0], fb[idx & 1][n][1]);
      __builtin_amdgcn_sched_barrier(0);
    }
   } else {
      // (S == 1) hi*hi on the f16 MFMA per tap; both cross terms of a PAIR of taps in one block-scaled e4m3
      // MFMA (K = 64 = 2 terms x 2 taps x 16 channels) at twice the f16 rate per K
      const uint4 *xb = xb0, *wb = wb0;
#pragma unroll
      for (int tp = 0; tp < (KS + 1) / 2; ++tp) {
        const int t0 = 2 * tp, t1 = 2 * tp + 1;
        const bool two = t1 < KS;
        h8 a_h0[MT], a_h1[MT], b_h0[NT], b_h1[NT];
        uint4 a8_0[MT], a8_1[MT], b8_0[NT], b8_1[NT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          a_h0[m] = __builtin_bit_cast(h8, wb[(t0 * 4 + 0) * CO_B + m * 32]);
          a8_0[m] = wb[(t0 * 4 + 2) * CO_B + m * 32];
          if (two) {
            a_h1[m] = __builtin_bit_cast(h8, wb[(t1 * 4 + 0) * CO_B + m * 32]);
            a8_1[m] = wb[(t1 * 4 + 2) * CO_B + m * 32];
          } else {
            a8_1[m] = make_uint4(0, 0, 0, 0);   // phantom tap: zero weights
          }
        }
        const uint4* x0 = xb + t0 * p.dil;
        const uint4* x1 = xb + t1 * p.dil;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          b_h0[n] = __builtin_bit_cast(h8, x0[n * 32]);
          b8_0[n] = x0[2 * XWP + n * 32];
          if (two) {
            b_h1[n] = __builtin_bit_cast(h8, x1[n * 32]);
            b8_1[n] = x1[2 * XWP + n * 32];
          } else {
            b8_1[n] = b8_0[n];                  // finite bytes against the zero weights
          }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h0[m], b_h0[n], acc[m][n], 0, 0, 0);
            if (two) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h1[m], b_h1[n], acc[m][n], 0, 0, 0);
            const i32x8 a8 = {(int)a8_0[m].x, (int)a8_0[m].y, (int)a8_0[m].z, (int)a8_0[m].w,
                              (int)a8_1[m].x, (int)a8_1[m].y, (int)a8_1[m].z, (int)a8_1[m].w};
            const i32x8 b8 = {(int)b8_0[n].x, (int)b8_0[n].y, (int)b8_0[n].z, (int)b8_0[n].w,
                              (int)b8_1[n].x, (int)b8_1[n].y, (int)b8_1[n].z, (int)b8_1[n].w};
            acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc[m][n], 0, 0, 0, sc_a, 0, sc_b);
          }
      }
   }
  };

  int chunk = 0;
  SAT_STAMP_BLOCK(6, __builtin_amdgcn_s_memrealtime());
  SAT_STAMP_BLOCK(7, ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | __builtin_amdgcn_s_getreg(63492));
  issue_loads(0);
  for (; chunk < nch - 1; ++chunk) {
    __syncthreads();   // every wave is done reading the previous tile
    SAT_STAMP(0);
    publish();
    SAT_STAMP(2);
    __syncthreads();
    SAT_STAMP(3);
    issue_loads(chunk + 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_phase();
    SAT_STAMP(4);
  }
  __syncthreads();
  SAT_STAMP(0);
  publish();
  SAT_STAMP(2);
  __syncthreads();
  SAT_STAMP(3);
  float rpre[MT][NT][16];
  if (p.res || p.res16) epilogue_prefetch_res<MT, NT>(p, rpre, b, 0, co_w, q_w, l31, lh);
  __builtin_amdgcn_sched_barrier(0);
  mfma_phase();
  SAT_STAMP(4);
  if (p.poly_planes) {                                  // wave-uniform: polyphase upsampler writing planes only
    polyphase_planes_epilogue<MT, NT>(p, acc, (float*)lds4, b, co_w, q_b, wave, l31, lh);
    return;
  }
  conv_epilogue<MT, NT, true>(p, acc, b, 0, co_w, q_w, l31, lh, 32, 0x7fffffff, rpre);
  SAT_STAMP(5);
  SAT_STAMP_BLOCK(14, __builtin_amdgcn_s_memrealtime());
}

template <int MT, int NT, int KS>
static int launch_f16x3(const ConvArgs& a, int B, int groups, hipStream_t s) {
  constexpr int CO_B = 32 * MT;
  constexpr int T_B = 128 * NT;
  constexpr int XWI = (T_B + (KS - 1) * 5 + 63) / 64;
  ConvArgs p = a;
#ifdef SAT_STAMPS
  p.dbg = g_stamp_buffer;
  if (g_stamp_variant & 1) p.y16 = nullptr;
  if (g_stamp_variant & 2) p.res16 = nullptr, p.res = nullptr;
#endif
  p.xw = T_B + (p.ksize - 1) * p.dil;
  if (p.xw > 64 * XWI) {
    set_error("conv1d(f16x3): dilation %d too large for the %d-tap kernel", p.dil, p.ksize);
    return SAT_ERR_INVALID;
  }
  p.co_tiles_g = ceil_div(p.rows_g, CO_B);
  size_t lds_bytes = ((size_t)4 * 64 * XWI + (size_t)KS * 4 * CO_B) * 16;
  void (*kern)(const ConvArgs) = conv1d_f16x3_kernel<MT, NT, KS, XWI>;
  if (p.x16) {
    kern = nullptr;
    // split-plane input: the tap counts of the generator (3, 7, 11), of the TDNNF stack (1, 3) and of the wav2vec2
    // feature extractor's polyphase stride-2 convs (2, 1)
    if constexpr (KS == 3 || KS == 7 || KS == 11)
      kern = p.f8 ? conv1d_f16x3_planes_kernel<MT, NT, KS, XWI, true, 1> : conv1d_f16x3_planes_kernel<MT, NT, KS, XWI, false, 1>;
    if constexpr ((KS == 1 || KS == 2 || KS == 3) && MT == 2) {
      // few taps: two 16-channel sub-chunks per pipeline stage
      if (!p.f8 && (p.cin_pad / CI_CHUNK) % 2 == 0) {
        kern = conv1d_f16x3_planes_kernel<MT, NT, KS, XWI, false, 2>;
        lds_bytes *= 2;
      }
    }
    if constexpr (KS == 1 || KS == 2) {
      if (!kern && !p.f8) kern = conv1d_f16x3_planes_kernel<MT, NT, KS, XWI, false, 1>;
    }
    if (!kern) {
      set_error("conv1d(split planes): %d taps not instantiated", KS);
      return SAT_ERR_INVALID;
    }
    if (p.poly_planes) lds_bytes = std::max(lds_bytes, (size_t)CO_B * (T_B + 1) * 4);   // the f32 tile of the transposed epilogue
  }
  dim3 grid(ceil_div(p.T_q, T_B), p.co_tiles_g * groups, B);
  if (int st = launch_lds(kern, grid, lds_bytes, s, p)) return st;
  SAT_LAUNCH_CHECK("conv1d_f16x3_kernel");
  return SAT_OK;
}

// ------------------------------------------------------------------------------------------------
// 1x1 convolution on split planes = a GEMM (TDNNF linearA/B, wav2vec2 Linear layers, ASR output affines).  With
// one tap nothing is shared between columns, so the B operand (activations) never goes through LDS: a lane loads
// its own two 16-byte fragments per 16-channel chunk straight from the planes (coalesced, 512 B per half wave).
// Only the weight tile is shared (4 waves side by side in time): 128 rows x 64 channels per stage, double-buffered
// in LDS (2 x 32 KB), ONE barrier per stage; the next stage's fragments and weights fly in registers during this
// stage's 48 MFMAs per wave.  Block tile = 128 rows x 128 positions (wave: 128 x 32, 64 accumulator registers):
// half the activation traffic per MFMA of the 64-row conv tile.  Blocks are numbered so that the co tiles of one
// (utterance, time tile) land on the same XCD and share the activations through its L2.
// ------------------------------------------------------------------------------------------------
template <int SC>
__global__ void __launch_bounds__(256, 2) conv1d_f16x3_k1_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  constexpr int CO_B = 128, T_B = 128, MT = 4;
  constexpr int WST = SC * 4 * CO_B;        // 16-byte units of one stage's weight tile: [chunk][part*2 + half][row]
  constexpr int W_IT = WST / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  // block -> (co tile, time tile, utterance): id = xcd + 8 * (co + n_co * (g >> 3)), g = 8 * (g >> 3) + xcd
  const int n_co = p.co_tiles_g, n_tt = p.pp_tiles_t;
  const int xcd = blockIdx.x & 7, rest = blockIdx.x >> 3;
  const int co_t = __builtin_amdgcn_readfirstlane(rest % n_co);
  const int g = __builtin_amdgcn_readfirstlane((rest / n_co) * 8 + xcd);
  if (g >= p.pp_total) return;
  const int b = __builtin_amdgcn_readfirstlane(g / n_tt);     // (division runs on the vector ALU: keep the results scalar)
  const int co_w = co_t * CO_B;
  const int q_w = (g - b * n_tt) * T_B + wave * 32;
  const int nst = p.cin_pad / CI_CHUNK / SC;

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const char*)p.x16 + (long long)b * p.cin_g * p.T_in * 4), 0, (unsigned)(p.cin_g * p.T_in * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (unsigned)p.w_gs, 0x00020000);
  const int seg_bytes = p.co_pad * 16;
  const int x_chunk_bytes = 4 * p.T_in * 16;
  const int xi = q_w + l31 - p.pad_left;
  const bool xok = xi >= 0 && xi < p.T_in;
  const unsigned xo_hi = xok ? (unsigned)(((0 + lh) * p.T_in + xi) * 16) : 0x80000000u;
  const unsigned xo_lo = xok ? (unsigned)(((2 + lh) * p.T_in + xi) * 16) : 0x80000000u;

  f32x16 acc[MT][1];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][0][r] = 0.f;

  uint4 wst[W_IT], bst[SC][2], bcur[SC][2];
  auto issue = [&](int st) {
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      // unit u = tid + 256 i of the stage tile [chunk][seg][128 rows]: chunk = i / 2 for every thread (a scalar offset)
      const int cl = i >> 1, seg = (tid >> 7) + 2 * (i & 1), r = tid & 127;
      wst[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, (co_w + r) * 16 + seg * seg_bytes,
                                                                                (st * SC + cl) * 4 * seg_bytes, 0));
    }
#pragma unroll
    for (int cl = 0; cl < SC; ++cl) {
      bst[cl][0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xo_hi, (st * SC + cl) * x_chunk_bytes, 0));
      bst[cl][1] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xo_lo, (st * SC + cl) * x_chunk_bytes, 0));
    }
  };
  issue(0);
  for (int st = 0; st < nst; ++st) {
    uint4* wl = lds4 + (st & 1) * WST;
#pragma unroll
    for (int i = 0; i < W_IT; ++i) wl[tid + 256 * i] = wst[i];
#pragma unroll
    for (int cl = 0; cl < SC; ++cl) {
      bcur[cl][0] = bst[cl][0];
      bcur[cl][1] = bst[cl][1];
    }
    __syncthreads();       // this stage's weights are visible; every wave has left the stage before, whose buffer the next one overwrites
    if (st + 1 < nst) issue(st + 1);
    __builtin_amdgcn_sched_barrier(0);
    const uint4* wb = wl + lh * CO_B + l31;
    // A fragments of chunk cl + 1 are read from LDS ahead of chunk cl's MFMAs (double-buffered registers): no
    // MFMA waits on a read issued just before it
    h8 af[2][MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      af[0][m][0] = __builtin_bit_cast(h8, wb[(0 * 4 + 0) * CO_B + m * 32]);
      af[0][m][1] = __builtin_bit_cast(h8, wb[(0 * 4 + 2) * CO_B + m * 32]);
    }
#pragma unroll
    for (int cl = 0; cl < SC; ++cl) {
      const h8 b_hi = __builtin_bit_cast(h8, bcur[cl][0]);
      const h8 b_lo = __builtin_bit_cast(h8, bcur[cl][1]);
      if (cl + 1 < SC) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          af[(cl + 1) & 1][m][0] = __builtin_bit_cast(h8, wb[((cl + 1) * 4 + 0) * CO_B + m * 32]);
          af[(cl + 1) & 1][m][1] = __builtin_bit_cast(h8, wb[((cl + 1) * 4 + 2) * CO_B + m * 32]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);     // the scheduler would sink those reads to their first use
#pragma unroll
      for (int m = 0; m < MT; ++m) mfma_split3(acc[m][0], af[cl & 1][m][0], af[cl & 1][m][1], b_hi, b_lo);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  conv_epilogue<MT, 1>(p, acc, b, 0, co_w, q_w, l31, lh);
}

int launch_f16x3_k1(const ConvArgs& a, int B, hipStream_t s) {
  constexpr int SC = 4;
  ConvArgs p = a;
  p.xw = 128;
  p.co_tiles_g = ceil_div(p.rows_g, 128);
  p.pp_tiles_t = ceil_div(p.T_q, 128);
  p.pp_total = p.pp_tiles_t * B;
  const size_t lds_bytes = (size_t)2 * SC * 4 * 128 * 16;
  auto kern = conv1d_f16x3_k1_kernel<SC>;
  static std::atomic<uint64_t> attr_done{0};      // per device (one static per SC instantiation)
  int dev;
  if (attr_needed_on_current_device(attr_done, &dev)) {
    SAT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    attr_done_on_device(attr_done, dev);
  }
  dim3 grid(8 * p.co_tiles_g * ceil_div(p.pp_total, 8), 1, 1);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, s, p);
  SAT_LAUNCH_CHECK("conv1d_f16x3_k1_kernel");
  return SAT_OK;
}

template <int MT, int NT>
static int launch_f16x3_ks(const ConvArgs& a, int B, int groups, hipStream_t s) {
  switch (a.ksize) {
    case 1: return launch_f16x3<MT, NT, 1>(a, B, groups, s);
    case 2: return launch_f16x3<MT, NT, 2>(a, B, groups, s);
    case 3: return launch_f16x3<MT, NT, 3>(a, B, groups, s);
    case 7: return launch_f16x3<MT, NT, 7>(a, B, groups, s);
    case 11: return launch_f16x3<MT, NT, 11>(a, B, groups, s);
    default:
      set_error("conv1d(f16x3): kernel size %d not instantiated (1, 2, 3, 7, 11)", a.ksize);
      return SAT_ERR_INVALID;
  }
}

int launch_f16x3_64x128(const ConvArgs& a, int B, int groups, hipStream_t s) {
  SAT_REQUIRE(a.ksize == 3 || a.ksize == 7, "conv1d(f16x3): kernel size %d not instantiated on 64 x 128 tiles (3, 7)", a.ksize);
  return a.ksize == 3 ? launch_f16x3<2, 1, 3>(a, B, groups, s) : launch_f16x3<2, 1, 7>(a, B, groups, s);
}
int launch_f16x3_64x256(const ConvArgs& a, int B, int groups, hipStream_t s) { return launch_f16x3_ks<2, 2>(a, B, groups, s); }
int launch_f16x3_32x512(const ConvArgs& a, int B, int groups, hipStream_t s) { return launch_f16x3_ks<1, 4>(a, B, groups, s); }

}  // namespace sat
