// Fused conv1d as an implicit GEMM on the gfx950 f32 matrix cores.
//
//   GEMM view:  M = output rows (C_out*up, per group), N = time positions, K = C_in/g * ksize
//   MFMA:       v_mfma_f32_32x32x2_f32 — A[i][k] from lane (i = l&31, k = l>>5),
//               B[k][j] from lane (k = l>>5, j = l&31), D: col = l&31, row = (r&3)+8(r>>2)+4(l>>5)
//               (cdna_hip_programming.md §3).  k = a PAIR of input channels at one tap.
//   B operand:  the input tile [16 channels][tile width + halo] staged in LDS; a fragment read is
//               32 consecutive floats of one channel row per half-wave -> conflict-free ds_read_b32.
//   A operand:  packed weights w[g][ci][tap][co] (co fastest) read straight from L2: one coalesced
//               128-B row per half-wave; all blocks share the same few MB of weights.
//   Epilogue:   bias, residual / bypass, folded BatchNorm, ReLU, MRF accumulation, polyphase store.
//
// Replaces (reference): torch Conv1d/ConvTranspose1d calls of hifigan/archi.py:77-91 and
// hifigan/nn.py:179-186; unfold+matmul/addmm of chain/nn.py:267-292 + BatchNorm/ReLU :338-347.
#include "common.h"
#include "conv_common.h"

namespace sat {

template <int MT, int NT, int WM, int WN, int KS, bool STRIDE1, int XWI>
__global__ void __launch_bounds__(256, 2) conv1d_mfma_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int CO_B = 32 * MT * WM;
  constexpr int T_B = 32 * NT * WN;
  static_assert(WM * WN == 4, "4 waves per block");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave % WM;
  const int wn = wave / WM;
  const int l31 = lane & 31;
  const int lh = lane >> 5;

  const int b = blockIdx.z;
  const int g = blockIdx.y / p.co_tiles_g;
  const int cot = blockIdx.y - g * p.co_tiles_g;
  const int co_w = cot * CO_B + wm * (32 * MT);  // first row of this wave inside the group
  const int q_b = blockIdx.x * T_B;              // first output position of the block
  const int q_w = q_b + wn * (32 * NT);
  const bool wave_active = co_w < p.rows_g;  // co_pad is a multiple of 64 >= rows_g, so the wave's rows stay inside the packed weights

  const int ks = KS > 0 ? KS : p.ksize;
  const int st = STRIDE1 ? 1 : p.stride;
  const int XW = XWI > 0 ? 64 * XWI : p.xw;  // LDS row pitch (columns past the tile are never read)
  const int xi0 = q_b * st - p.pad_left;

  const float* __restrict__ xg = p.x + (long long)b * p.x_bs + (long long)(g * p.cin_g) * p.x_cs;
  // weights of this group behind one buffer descriptor; per-lane part of the A-fragment address in
  // ONE 32-bit VGPR (channel half lh, row l31), everything else (chunk, pair, tap, m) scalar/immediate
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.w + (long long)g * p.w_gs), 0, (unsigned)(p.w_gs * 4), 0x00020000);
  const int w_ci_bytes = ks * p.co_pad * 4;            // bytes between input channels
  const int a_voff = lh * w_ci_bytes + (co_w + l31) * 4;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // XWI > 0 (compile-time trip counts): the input rows of chunk c + 1 are requested into registers BEFORE the MFMA phase of chunk c and
  // stored to LDS behind it (round 6): a launch with few blocks per CU — one or two utterances on the exact-f32 kernels, what the
  // near-tie guard of the VQ runs — no longer pays one exposed global round trip per 16-channel chunk.  Same chunks in the same order:
  // the same bits.
  constexpr int XWR = XWI > 0 ? XWI : 1;
  float stg[CI_CHUNK / 4][XWR];
  auto request_rows = [&](int c0) __attribute__((always_inline)) {
    // every global load of the chunk is issued before the first LDS store, so the loads overlap each other
    const int voff = (xi0 + lane) * 4;  // byte offset inside the row; negative / past-the-end -> 0 by the range check
#pragma unroll
    for (int rr = 0; rr < CI_CHUNK / 4; ++rr) {
      const int ci = c0 + wave + rr * 4;
      // one buffer descriptor per (utterance, channel) row: the hardware range check supplies the
      // conv's zero padding on both sides; descriptor inputs are wave-uniform (readfirstlane, T20)
      const unsigned long long a = (unsigned long long)(xg + (long long)ci * p.x_cs);
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
      const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
      const unsigned nbytes = __builtin_amdgcn_readfirstlane(ci < p.cin_g ? (unsigned)p.T_in * 4u : 0u);
      const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(((unsigned long long)hi << 32) | lo), 0, nbytes, 0x00020000);
#pragma unroll
      for (int it = 0; it < XWR; ++it)
        stg[rr][it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff + 256 * it, 0, 0));
    }
  };
  if constexpr (XWI > 0) request_rows(0);

  for (int c0 = 0; c0 < p.cin_pad; c0 += CI_CHUNK) {
    __syncthreads();
    // ---- stage the input tile: 16 channels x XW columns, pre-activation fused ----
    if constexpr (XWI > 0) {
#pragma unroll
      for (int rr = 0; rr < CI_CHUNK / 4; ++rr) {
        float* dst = lds + (wave + rr * 4) * XW;
#pragma unroll
        for (int it = 0; it < XWI; ++it) {
          const int col = lane + 64 * it;
          float v = stg[rr][it];
          if (p.in_lrelu) v = v > 0.f ? v : v * p.in_slope;
          dst[col] = v;
        }
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < CI_CHUNK / 4; ++rr) {
        const int r = wave + rr * 4;
        const int ci = c0 + r;
        const bool cok = ci < p.cin_g;
        const float* __restrict__ src = xg + (long long)ci * p.x_cs;
        float* dst = lds + r * XW;
        for (int col = lane; col < XW; col += 64) {
          const int xi = xi0 + col;
          float v = 0.f;
          if (cok && xi >= 0 && xi < p.T_in) {
            v = src[xi];
            if (p.in_lrelu) v = v > 0.f ? v : v * p.in_slope;
          }
          dst[col] = v;
        }
      }
    }
    __syncthreads();
    // (the next chunk's rows are requested BEHIND this chunk's first weight loads: vmcnt retires in issue order, so a wait for a
    // weight fragment also waits for every older load)
    auto request_next = [&]() __attribute__((always_inline)) {
      if constexpr (XWI > 0) {
        if (c0 + CI_CHUNK < p.cin_pad) request_rows(c0 + CI_CHUNK);      // in flight during this chunk's MFMA phase
      }
    };
    if (!wave_active) {
      request_next();
      continue;
    }

    const int wc_soff = c0 * w_ci_bytes;   // scalar byte offset of this chunk's first channel
    const float* xrow = lds + lh * XW + (wn * (32 * NT) + l31) * st;
#define SAT_LOAD_A(pair, tap, m) \
  __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32( \
      wrsrc, a_voff + (m) * 128, wc_soff + (2 * (pair)) * w_ci_bytes + (tap) * p.co_pad * 4, 0))

    if constexpr (KS > 0 && KS * MT <= 4) {
      // few taps and row tiles (the 1x1 GEMM shapes of the encoders, TDNNF linearA / linearB): ALL weight fragments of the chunk are
      // requested up front (8 channel pairs x KS x MT <= 32 registers) — one round trip per chunk instead of one per channel pair,
      // which is what a launch of a few blocks per CU waits for (round 6; the same products in the same order)
      float a_all[CI_CHUNK / 2][KS][MT];
#pragma unroll
      for (int pr = 0; pr < CI_CHUNK / 2; ++pr)
#pragma unroll
        for (int t = 0; t < KS; ++t)
#pragma unroll
          for (int m = 0; m < MT; ++m) a_all[pr][t][m] = SAT_LOAD_A(pr, t, m);
      request_next();
#pragma unroll
      for (int pr = 0; pr < CI_CHUNK / 2; ++pr) {
        const float* xp = xrow + (2 * pr) * XW;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
          float bf[NT];
          const float* xt = xp + t * p.dil;
#pragma unroll
          for (int n = 0; n < NT; ++n) bf[n] = xt[n * 32 * st];
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
              acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_all[pr][t][m], bf[n], acc[m][n], 0, 0, 0);
        }
      }
    } else if constexpr (KS > 0) {
      float a_cur[KS][MT];
#pragma unroll
      for (int t = 0; t < KS; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) a_cur[t][m] = SAT_LOAD_A(0, t, m);
      request_next();
#pragma unroll
      for (int pr = 0; pr < CI_CHUNK / 2; ++pr) {
        float a_nxt[KS][MT];
        if (pr + 1 < CI_CHUNK / 2) {
#pragma unroll
          for (int t = 0; t < KS; ++t)
#pragma unroll
            for (int m = 0; m < MT; ++m) a_nxt[t][m] = SAT_LOAD_A(pr + 1, t, m);
        }
        const float* xp = xrow + (2 * pr) * XW;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
          float bf[NT];
          const float* xt = xp + t * p.dil;
#pragma unroll
          for (int n = 0; n < NT; ++n) bf[n] = xt[n * 32 * st];
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
              acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[t][m], bf[n], acc[m][n], 0, 0, 0);
        }
        if (pr + 1 < CI_CHUNK / 2) {
#pragma unroll
          for (int t = 0; t < KS; ++t)
#pragma unroll
            for (int m = 0; m < MT; ++m) a_cur[t][m] = a_nxt[t][m];
        }
        // keep the software pipeline one channel pair deep: without this fence the scheduler hoists
        // the weight loads of all 8 unrolled pairs to the top of the chunk and spills
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // runtime tap count (k = 2, 10, 128 ...): taps looped, one k-pair of channels at a time
      request_next();
#pragma unroll 1
      for (int pr = 0; pr < CI_CHUNK / 2; ++pr) {
        const float* xp = xrow + (2 * pr) * XW;
        float a_nx[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) a_nx[m] = SAT_LOAD_A(pr, 0, m);
#pragma unroll 2
        for (int t = 0; t < ks; ++t) {
          float a[MT];
#pragma unroll
          for (int m = 0; m < MT; ++m) a[m] = a_nx[m];
          if (t + 1 < ks) {
#pragma unroll
            for (int m = 0; m < MT; ++m) a_nx[m] = SAT_LOAD_A(pr, t + 1, m);
          }
          float bf[NT];
          const float* xt = xp + t * p.dil;
#pragma unroll
          for (int n = 0; n < NT; ++n) bf[n] = xt[n * 32 * st];
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
              acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bf[n], acc[m][n], 0, 0, 0);
        }
      }
    }
  }

#undef SAT_LOAD_A
  if (!wave_active) return;

  conv_epilogue<MT, NT>(p, acc, b, g, co_w, q_w, l31, lh);
}

template <int MT, int NT, int WM, int WN, int KS, bool S1, int XWI>
static int launch_cfg(const ConvArgs& a, int B, int groups, hipStream_t s) {
  constexpr int CO_B = 32 * MT * WM;
  constexpr int T_B = 32 * NT * WN;
  ConvArgs p = a;
  p.xw = (T_B - 1) * p.stride + (p.ksize - 1) * p.dil + 1;
  p.co_tiles_g = ceil_div(p.rows_g, CO_B);
  const size_t lds_bytes = (size_t)CI_CHUNK * (XWI > 0 ? 64 * XWI : p.xw) * sizeof(float);
  auto kern = conv1d_mfma_kernel<MT, NT, WM, WN, KS, S1, XWI>;
  if (lds_bytes > 160 * 1024) {
    set_error("conv1d: input tile of %zu bytes does not fit LDS (stride %d, ksize %d, dilation %d)",
              lds_bytes, p.stride, p.ksize, p.dil);
    return SAT_ERR_INVALID;
  }
  dim3 grid(ceil_div(p.T_q, T_B), p.co_tiles_g * groups, B);
  if (int st = launch_lds(kern, grid, lds_bytes, s, p)) return st;
  SAT_LAUNCH_CHECK("conv1d_mfma_kernel");
  return SAT_OK;
}

// batched staging needs a compile-time bound on the tile width: tile + (KS-1)*dilation columns,
// instantiated for dilation <= 5 (every dilated layer of the generator); wider halos fall back to
// the dynamic staging loop
template <int MT, int NT, int WM, int WN, int KS>
static int launch_xwi(const ConvArgs& a, int B, int groups, hipStream_t s) {
  constexpr int T_B = 32 * NT * WN;
  constexpr int XWI = (T_B + (KS - 1) * 5 + 63) / 64;
  const int xw = T_B + (a.ksize - 1) * a.dil;
  if (xw <= 64 * XWI) return launch_cfg<MT, NT, WM, WN, KS, true, XWI>(a, B, groups, s);
  return launch_cfg<MT, NT, WM, WN, KS, true, 0>(a, B, groups, s);
}

template <int MT, int NT, int WM, int WN>
static int launch_ks(const ConvArgs& a, int B, int groups, hipStream_t s) {
  if (a.stride == 1) {
    switch (a.ksize) {
      case 1: return launch_xwi<MT, NT, WM, WN, 1>(a, B, groups, s);
      case 2: return launch_xwi<MT, NT, WM, WN, 2>(a, B, groups, s);
      case 3: return launch_xwi<MT, NT, WM, WN, 3>(a, B, groups, s);
      case 7: return launch_xwi<MT, NT, WM, WN, 7>(a, B, groups, s);
      case 11: return launch_xwi<MT, NT, WM, WN, 11>(a, B, groups, s);
      default: return launch_cfg<MT, NT, WM, WN, 0, true, 0>(a, B, groups, s);
    }
  }
  return launch_cfg<MT, NT, WM, WN, 0, false, 0>(a, B, groups, s);
}

// tile shape by output rows per group: wide-in-time tiles for thin layers
int launch_conv1d_f32(const ConvArgs& a, int B, int groups, hipStream_t s) {
  if (a.rows_g > 64) {
    // few, long GEMM-like layers (TDNNF: 128 rows x ~530 frames per utterance, K = 3072) would
    // launch fewer 128x128 blocks than there are CUs: cut the time tile to 32 positions instead
    const long long blocks128 = (long long)ceil_div(a.T_q, 128) * ceil_div(a.rows_g, 128) * groups * B;
    if (blocks128 < 2 * 256) return launch_ks<1, 1, 4, 1>(a, B, groups, s);   // 128 rows x 32 positions
    return launch_ks<2, 2, 2, 2>(a, B, groups, s);                              // 128 rows x 128 positions
  }
  if (a.rows_g > 32) return launch_ks<2, 2, 1, 4>(a, B, groups, s);   //  64 rows x 256 positions
  return launch_ks<1, 4, 1, 4>(a, B, groups, s);                       //  32 rows x 512 positions
}

}  // namespace sat
