// YAAPT pitch tracking on gfx950, batched over (utterance, frame).
//
// Reference: satools/satools/hifigan/yaapt.py:795-951 (`_yaapt`/`yaapt`: a serial Python loop over
// the batch, forced onto the CPU) with the options of egs/vc/libritts/local/tuning/hifigan.py:31-36.
// Kernel by kernel:
//   prefilter     SignalObj.filtered_version :42-51 (torchaudio biquads; third-party)
//   nlfer_frames  nlfer :148-176                    one 8192-point real FFT in LDS per frame (4096 packed points)
//   energy_norm   PitchObj.set_energy :125-128
//   spec_frames   spec_track :209-238 + peaks :383-497   FFT -> |X| -> SHC -> candidate peaks
//   spec_post     spec_track :241-312, dynamic5 :506-523, path1 :530-570, medfilt :54-69
//   frame_means   the in-place mean subtraction on overlapping frame views, time_track :711-714 + :589
//   nccf_frames   crs_corr :577-602 + cmp_rate :609-673 + merit weighting :724-727
//   refine_dp     refine :732-784, dynamic :321-370, path1
// Decision rules (strict/non-strict comparisons, first/last extremum on ties, stable ordering) are
// kept exactly; f32 operation order is kept wherever the reference's order is defined by its source.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "yaapt_dev.h"     // the constants and the per-utterance device helpers, shared with csrc/yaapt_long/

namespace sat {

// ------------------------------------------------------------------------------------------------
// prefilter: zero-pad, (square), low-pass biquad -> clamp -> high-pass biquad -> clamp   (yaapt.py:42-51).
// torchaudio's lfilter order (third party, restated in oracle/biquad.py, order "torchaudio"):
//   FIR   f[t] = fma(b0', x[t], fma(b1', x[t-1], b2' * x[t-2]))      b' = b / a0  (conv1d's FMA chain in tap order)
//   IIR   v = f[t] - c2 * y[t-2];  v = v - c1 * y[t-1];  y[t] = v    c = a / a0   (multiply, subtract; no fma)
//   out   clamp(y[t], -1, 1); the recursion itself runs on unclamped values
// The recursion is sequential in t and its f32 rounding order is part of the result, so the only parallelism is
// ACROSS chains: a chain = (utterance, signal in {x, x^2}), and a lane of the IIR waves owns one chain (one
// wave-instruction advances 64 chains by one sample).  A block takes 32 utterances = 64 chains through a six-stage
// software pipeline over tiles of 64 samples, one role per wave, one barrier per tile, the tile's LDS buffer
// (row = chain, 68 floats: 16-byte rows, ds_read_b128 of 64 rows conflict-free) handed down the stages and
// transformed IN PLACE:
//   L  load 32 utterances (coalesced, registers one tile ahead), write rows x | x^2        lane = 4 samples of a row
//   F1 low-pass FIR    (3 VALU per sample)                                                  lane = chain
//   I1 low-pass IIR + clamp (sub, sub, 2 mul, clamp: the critical wave, ~18 cycles/sample)  lane = chain
//   F2 high-pass FIR, I2 high-pass IIR + clamp                                              lane = chain
//   S  store rows (zero past the chain's own padded length: the zero extension spec_track reads)
// A workgroup's waves are dealt to the CU's four SIMDs cyclically (k and k + 4 share one), so the roles are
// numbered to leave each IIR wave alone on its SIMD: waves 0 / 1 = I1 / I2, 2 / 3 = F1 / F2, 4 / 5 idle,
// 6 = L (beside F1), 7 = S (beside F2; placement checked with s_getreg HW_ID).  Measured (s_memtime stamps per role,
// 32 x 5 s): 2.2k cycles per tile in the IIR waves (34 cycles per sample: sub, sub, pk_mul — 8 issue cycles, no
// gain over two v_mul —, clamp, plus the row's LDS traffic; a lone wave issues one VALU per ~4.2 cycles,
// tools/valu_lat.hip), 2.0-2.5k in the others; 1 260 tiles = 1.25 ms at the 2.4 GHz the chip holds under this
// one-CU kernel, for any batch up to 32 (round 1: one block of two waves per chain with wave-uniform recursions,
// 1.7-2.5 ms, 64 blocks).
// ------------------------------------------------------------------------------------------------
constexpr int PF_T = 64;
constexpr int PF_PITCH = 68;
constexpr int PF_RING = 6;
constexpr int PF_THREADS = 512;

__device__ __forceinline__ void pf_fir_tile(float* __restrict__ row, float b0, float b1, float b2, float& x1, float& x2) {
  float4 xq[PF_T / 4];
#pragma unroll
  for (int q = 0; q < PF_T / 4; ++q) xq[q] = *reinterpret_cast<const float4*>(row + 4 * q);
#pragma unroll
  for (int q = 0; q < PF_T / 4; ++q) {
    const float4 x = xq[q];
    float4 f;
    f.x = __builtin_fmaf(b0, x.x, __builtin_fmaf(b1, x1, b2 * x2));
    f.y = __builtin_fmaf(b0, x.y, __builtin_fmaf(b1, x.x, b2 * x1));
    f.z = __builtin_fmaf(b0, x.z, __builtin_fmaf(b1, x.y, b2 * x.x));
    f.w = __builtin_fmaf(b0, x.w, __builtin_fmaf(b1, x.z, b2 * x.y));
    x2 = x.z;
    x1 = x.w;
    *reinterpret_cast<float4*>(row + 4 * q) = f;
  }
}

// One step of the recursion.  State: p1 = c1*y[t-1], p2n = c2*y[t-1], d = f[t] - c2*y[t-2] (the first subtraction, taken
// one step ahead: it does not depend on y[t-1], and in program order right behind `v = d - p1` it fills that
// instruction's result latency instead of standing in front of it).  Dependent chain per sample: sub -> pk_mul.
// The operations and their order per sample are exactly  v = f - c2*y2;  v = v - c1*y1.
__device__ __forceinline__ float pf_iir_step(float f_next, float c1, float c2, float& p1, float& p2n, float& d) {
  const float v = d - p1;
  d = f_next - p2n;
  typedef float v2f __attribute__((ext_vector_type(2)));
  const v2f q = (v2f){c1, c2} * (v2f){v, v};      // one v_pk_mul_f32: the same two IEEE products
  p1 = q.x;
  p2n = q.y;
  return fminf(fmaxf(v, -1.f), 1.f);
}
// `d` enters holding f[first sample of this tile] - c2*y[t-2] ... which needs this tile's first f: the caller passes
// `dp2` = c2*y[t-2] pending from the previous tile instead, and the tile finishes the subtraction itself.
__device__ __forceinline__ void pf_iir_tile(float* __restrict__ row, float c1, float c2, float& p1, float& p2n, float& dp2) {
  // the whole row up front (64 registers): one LDS round trip per tile instead of one per group of reads
  float4 fq[PF_T / 4];
#pragma unroll
  for (int q = 0; q < PF_T / 4; ++q) fq[q] = *reinterpret_cast<const float4*>(row + 4 * q);
  float d = fq[0].x - dp2;
#pragma unroll
  for (int q = 0; q < PF_T / 4; ++q) {
    const float4 f = fq[q];
    float4 u;
    u.x = pf_iir_step(f.y, c1, c2, p1, p2n, d);
    u.y = pf_iir_step(f.z, c1, c2, p1, p2n, d);
    u.z = pf_iir_step(f.w, c1, c2, p1, p2n, d);
    if (q + 1 < PF_T / 4) {
      u.w = pf_iir_step(fq[q + 1 < PF_T / 4 ? q + 1 : q].x, c1, c2, p1, p2n, d);
    } else {                                    // last sample of the tile: the next f is not here yet
      const float v = d - p1;
      dp2 = p2n;                                // c2*y[t-1] of this sample = c2*y[t-2] of the next tile's first
      typedef float v2f __attribute__((ext_vector_type(2)));
      const v2f qq = (v2f){c1, c2} * (v2f){v, v};
      p1 = qq.x;
      p2n = qq.y;
      u.w = fminf(fmaxf(v, -1.f), 1.f);
    }
    *reinterpret_cast<float4*>(row + 4 * q) = u;
  }
}

// VEC: rows of wav / filt are 16-byte aligned (n, pad, Lz multiples of 4): 16-byte global accesses.
// Loads and stores go through buffer descriptors over the block's rows: a lane outside its row's valid range gets
// an out-of-range offset (loads return 0, stores are dropped), so both roles are branch-free and the compiler
// batches a tile's LDS reads and memory operations instead of one round trip per row.
template <bool VEC>
__global__ void __launch_bounds__(PF_THREADS) yaapt_prefilter_kernel(const float* __restrict__ wav, float* __restrict__ filt,
                                                                     const int* __restrict__ U, const Plan P, int B) {
  __shared__ __attribute__((aligned(16))) float ring[PF_RING][64 * PF_PITCH];
  __shared__ int s_n[32], s_L[32];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int ub = blockIdx.x * 32;                       // first utterance of the block
  const int rows = min(32, B - ub);
  if (threadIdx.x < 32) {
    const int b = ub + threadIdx.x;
    s_n[threadIdx.x] = b < B ? ulen(U, b, 0, P.n) : 0;
    s_L[threadIdx.x] = b < B ? ulen(U, b, 1, P.L) : 0;
  }
  __syncthreads();
  // role -> pipeline stage
  const int stage = wave == 6 ? 0 : wave == 2 ? 1 : wave == 0 ? 2 : wave == 3 ? 3 : wave == 1 ? 4 : wave == 7 ? 5 : -1;
  const int ntiles = (P.Lz + PF_T - 1) / PF_T;
  const float* kc = (wave == 0 || wave == 2) ? P.lp : P.hp;
  const float kb0 = kc[0], kb1 = kc[1], kb2 = kc[2], c1 = kc[4], c2 = kc[5];
  float x1 = 0.f, x2 = 0.f;                 // FIR history
  float p1 = 0.f, p2n = 0.f, dp2 = 0.f;     // IIR history (products of zeros)
  constexpr unsigned OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(wav + (size_t)ub * P.n), 0, (unsigned)((size_t)rows * P.n * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t frs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(filt + (size_t)ub * 2 * P.Lz), 0, (unsigned)((size_t)rows * 2 * P.Lz * 4), 0x00020000);
  const int rsub = lane >> 4, jq = lane & 15;
  // per-lane row constants of the loader (NL rows per tile and lane) and of the storer (NS)
  constexpr int NL = VEC ? 8 : 32, NS = VEC ? 16 : 64;
  int l_n[NL], s_len[NS];
  unsigned l_off[NL], s_off[NS];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int r = VEC ? i * 4 + rsub : i;
    l_n[i] = stage == 0 ? s_n[r] : 0;
    l_off[i] = r < rows ? (unsigned)r * (unsigned)P.n * 4u : OOB;            // OOB + a row offset stays out of range
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int c = VEC ? i * 4 + rsub : i;
    s_len[i] = stage == 5 ? s_L[c >> 1] : 0;
    s_off[i] = (c >> 1) < rows ? (unsigned)c * (unsigned)P.Lz * 4u : OOB;     // no such chain: nothing stored
  }
  int n_min = P.n, L_min = P.L;          // over the block's utterances: tiles inside them need no per-lane masks
  for (int r = 0; r < rows; ++r) {
    n_min = min(n_min, s_n[r]);
    L_min = min(L_min, s_L[r]);
  }
  constexpr int NPRE = VEC ? 8 : 32;
  typedef typename std::conditional<VEC, float4, float>::type pre_t;
  constexpr int PD = 2;                  // tiles in flight in the loader's registers (two tile periods of latency)
  pre_t pre[PD][NPRE];
  auto load_tile = [&](int tile, pre_t* pre) {
    const int src = tile * PF_T + (VEC ? 4 * jq : lane) - P.pad;   // VEC: a multiple of 4, a quad starts inside [0, n) or outside
    const bool interior = tile * PF_T - P.pad >= 0 && tile * PF_T + PF_T - P.pad <= n_min;     // wave-uniform
    if (interior) {
#pragma unroll
      for (int i = 0; i < NPRE; ++i) {
        const unsigned off = l_off[i] + (unsigned)src * 4u;
        if constexpr (VEC) pre[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 0));
        else pre[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrs, off, 0, 0));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NPRE; ++i) {
        const unsigned off = (tile < ntiles && src >= 0 && src < l_n[i]) ? l_off[i] + (unsigned)src * 4u : OOB;
        if constexpr (VEC) {
          float4 v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 0));
          if (src + 1 >= l_n[i]) v.y = 0.f;      // ragged tail inside the row pitch
          if (src + 2 >= l_n[i]) v.z = 0.f;
          if (src + 3 >= l_n[i]) v.w = 0.f;
          pre[i] = v;
        } else {
          pre[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrs, off, 0, 0));
        }
      }
    }
  };
  if (stage == 0) {
#pragma unroll
    for (int k = 0; k < PD; ++k) load_tile(k, pre[k]);
  }
  auto loader = [&](int tile, float* buf, pre_t* pk) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      if constexpr (VEC) {
        const int r = i * 4 + rsub;
        const float4 v = pk[i];
        *reinterpret_cast<float4*>(buf + (2 * r) * PF_PITCH + 4 * jq) = v;
        *reinterpret_cast<float4*>(buf + (2 * r + 1) * PF_PITCH + 4 * jq) = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
      } else {
        buf[(2 * i) * PF_PITCH + lane] = pk[i];
        buf[(2 * i + 1) * PF_PITCH + lane] = pk[i] * pk[i];
      }
    }
    load_tile(tile + PD, pk);              // the same registers: lands during the next PD tile periods
  };
  for (int it = 0; it < ntiles + PF_RING - 1; ++it) {
    const int tile = it - stage;
    if (stage >= 0 && tile >= 0 && tile < ntiles) {
      float* buf = ring[tile % PF_RING];
      if (stage == 0) {
        switch (tile & (PD - 1)) {          // compile-time register set per case
          case 0: loader(tile, buf, pre[0]); break;
          default: loader(tile, buf, pre[1]); break;
        }
      } else if (stage == 1 || stage == 3) {
        pf_fir_tile(buf + lane * PF_PITCH, kb0, kb1, kb2, x1, x2);
      } else if (stage == 2 || stage == 4) {
        pf_iir_tile(buf + lane * PF_PITCH, c1, c2, p1, p2n, dp2);
      } else {
        typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4;
        const int t = tile * PF_T + (VEC ? 4 * jq : lane);   // VEC: Lz % 4 == 0, a quad is inside or outside as a whole
        const bool interior = tile * PF_T + PF_T <= L_min;   // wave-uniform (L_min <= L <= Lz)
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const unsigned off = (interior || t < P.Lz) ? s_off[i] + (unsigned)t * 4u : OOB;
          if constexpr (VEC) {
            float4 v = *reinterpret_cast<const float4*>(buf + (i * 4 + rsub) * PF_PITCH + 4 * jq);
            if (!interior) {
              if (t + 0 >= s_len[i]) v.x = 0.f;         // zero extension past the chain's own padded length
              if (t + 1 >= s_len[i]) v.y = 0.f;
              if (t + 2 >= s_len[i]) v.z = 0.f;
              if (t + 3 >= s_len[i]) v.w = 0.f;
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), frs, off, 0, 0);
          } else {
            float v = buf[i * PF_PITCH + lane];
            if (!interior && t >= s_len[i]) v = 0.f;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), frs, off, 0, 0);
          }
        }
      }
    }
    // LDS-only barrier: __syncthreads() also drains vmcnt, i.e. it would wait every tile for the loader's prefetch
    // and for the storer's write acknowledgements
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
}

// ------------------------------------------------------------------------------------------------
// 8192-point transform of a REAL frame in LDS.  The frame is packed two samples to a complex point,
// z[m] = x[2m] + i x[2m+1], one 4096-point complex FFT (radix-2 decimation in time, input stored in bit-reversed
// order) gives Z, and a wanted bin follows from Z[k] and Z[4096 - k] (fft_packed_mag below): half the points, half
// the LDS (32 KB) and no imaginary half full of zeros carried through every pass.
// tw = the staged table of yaapt_stage_twiddles_kernel over the host's tw[k] = exp(-2*pi*i*k/8192), k < 4096 (f64 -> f32).
// ------------------------------------------------------------------------------------------------
// 512 threads = 8 waves: a block's 32 KB let four of them share a CU, which is the CU's 32 waves (the waves are what hides
// the LDS round trips of a pass); one radix-8 group per thread and pass.  What follows the FFT keeps its 256-thread shape.
// (Measured: YAAPT on 32 x 5 s 2.08 ms; with 256 threads, two groups per thread, 83 VGPRs and 16 waves per CU, 2.12 ms.)
constexpr int FFT_THREADS = 512;
template <int LOG>
__device__ __forceinline__ int brev(int j) { return (int)(__brev((unsigned)j) >> (32 - LOG)); }

// One pass = NST consecutive radix-2 stages (s .. s+NST-1) of the 2^LOG-point FFT done in registers on groups of 2^NST
// elements spaced 2^(s-1) apart: the butterflies, their twiddles and their order of operations are exactly those of the
// stage-by-stage loop, so the result is bit-identical to it — only the LDS round trips and barriers between
// the stages of a pass are gone (12 -> 3-4 passes).  T = threads of the block.
template <int LOG, int T, int NST>
__device__ __forceinline__ void fft_pass(float* re, float* im, const float2* __restrict__ tw, int s) {
  constexpr int N = 1 << LOG;
  constexpr int R = 1 << NST;
  const int h = 1 << (s - 1);
#pragma unroll 2
  for (int k = 0; k < (N / R + T - 1) / T; ++k) {
    const int i = threadIdx.x + T * k;
    if (N / R < T && i >= N / R) break;
    const int pos = i & (h - 1);
    const int base = ((i >> (s - 1)) << (s - 1 + NST)) + pos;
    float xr[R], xi[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      xr[j] = re[base + j * h];
      xi[j] = im[base + j * h];
    }
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int d = 1 << st;                              // partner distance in group slots at stage s + st
      // staged table (yaapt_stage_twiddles_kernel): stage s + st's 2^(s + st - 1) twiddles are contiguous from entry
      // 2^(s + st - 1) - 1 on, whatever the size of the transform (entry (h - 1) + p = exp(-2 pi i p / 2h)), so consecutive
      // lanes (consecutive pos) read consecutive entries instead of a gather at the stage's stride
      const float2* __restrict__ ts = tw + ((h << st) - 1);
#pragma unroll
      for (int j = 0; j < R; ++j) {
        if (j & d) continue;                              // j = the "a" element, j + d = the "c" element
        const int p = pos + (j & (d - 1)) * h;            // index of a inside its half-block of stage s + st
        const float2 w = ts[p];
        const float tr = xr[j + d] * w.x - xi[j + d] * w.y;
        const float ti = xr[j + d] * w.y + xi[j + d] * w.x;
        const float ur = xr[j], ui = xi[j];
        xr[j] = ur + tr;
        xi[j] = ui + ti;
        xr[j + d] = ur - tr;
        xi[j + d] = ui - ti;
      }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      re[base + j * h] = xr[j];
      im[base + j * h] = xi[j];
    }
  }
  __syncthreads();
}

// stages first .. LOG of the 2^LOG-point radix-2 DIT FFT (input in bit-reversed order).
// (Round 3, on the 8192-point complex form, measured and not kept: the twiddles of a radix-8 pass in registers, requested one pass
// ahead — nlfer 268 -> 418 us; the last pass computing only the wanted output bins, 7 of 24 butterfly results and 1 of 8 LDS writes —
// 229 -> 238 us at the same occupancy.  What did pay: the per-stage contiguous twiddle table below, 268 -> 229 and 304 -> 222 us.)
template <int LOG, int T>
__device__ void fft_from(float* re, float* im, const float2* __restrict__ tw, int first) {
  int s = first;
  const int lead = (LOG - first + 1) % 3;
  if (lead == 1) { fft_pass<LOG, T, 1>(re, im, tw, s); s += 1; }
  if (lead == 2) { fft_pass<LOG, T, 2>(re, im, tw, s); s += 2; }
  for (; s <= LOG; s += 3) fft_pass<LOG, T, 3>(re, im, tw, s);
}

// Packed, zero-padded real input of L samples, Lp = ceil(L / 2) <= 2^LOG >> z points (an odd L leaves the last imaginary part 0):
// in bit-reversed order the points sit at multiples of 2^z and the first z stages only copy each one over its block of 2^z
// (z + w*0 and z - w*0).  Fills re/im with that state, every element of both, and returns the first stage left to do.
// get(j) = sample j.
template <int LOG, int T, typename Get>
__device__ __forceinline__ int fft_load_packed(float* re, float* im, int L, Get get) {
  constexpr int N = 1 << LOG;
  const int Lp = (L + 1) >> 1;
  const int z = Lp <= N / 8 ? 3 : (Lp <= N / 4 ? 2 : (Lp <= N / 2 ? 1 : 0));
  // Element (m, r) = re/im[brev(m) + r], m < N >> z, r < 2^z.  The low six address bits, the LDS bank, are r and, above it, the
  // TOP 6 - z bits of m reversed (bits 6 .. 11 - z), so a wave that walks 64 consecutive m writes all its lanes to ONE bank
  // (64-way conflict on every store; in the 8192-point form with 8000 blocks per launch such a fill was a third of the FFT kernels'
  // time).  Here a lane is (r, q): r = its low z bits, q = the top 6 - z bits of m; the 6 low bits of m come from (wave, round).  A
  // 4-byte store is banked modulo 32 within each half of the wave, which drops address bit 5 = bit 0 of q: that bit is the lane's
  // half, the others come from the lane's bits z .. 4 — 32 distinct banks per half.
  constexpr int WAVES = T / 64, ROUNDS = 64 / WAVES;
  static_assert(LOG == 12 && T % 64 == 0 && WAVES * ROUNDS == 64, "waves x rounds = the 64 low-bit values of m");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & ((1 << z) - 1), q = (((lane & 31) >> z) << 1) | (lane >> 5);
#pragma unroll
  for (int round = 0; round < ROUNDS; ++round) {
    const int m = (q << 6) | (wave * ROUNDS + round);
    const int j = 2 * m;
    const float a = j < L ? get(j) : 0.f;
    const float b = j + 1 < L ? get(j + 1) : 0.f;
    const int at = brev<LOG>(m) + r;
    re[at] = a;
    im[at] = b;
  }
  __syncthreads();
  return z + 1;
}

// |X[k]|, k < 4096, of the 8192-point transform X of the real frame whose packed transform Z lies in re/im ("untangle"):
//   E[k] = (Z[k] + conj Z[4096 - k]) / 2    the transform of the even samples
//   O[k] = (Z[k] - conj Z[4096 - k]) / 2i   the transform of the odd ones
//   X[k] = E[k] + w^k O[k], w = exp(-2 pi i / 8192): the last stage's butterfly of the 8192-point form with its twiddle, entry
//   (4096 - 1) + k of the staged table;  X[0] = Re Z[0] + Im Z[0].
// The halving is an exact multiply; one rounding each in E and O, then the four-multiply product and the two additions of a butterfly.
__device__ __forceinline__ float fft_packed_mag(const float* re, const float* im, const float2* __restrict__ tw, int k) {
  if (k == 0) return hypotf(re[0] + im[0], 0.f);
  const float ar = re[k], ai = im[k], br = re[FFT_NP - k], bi = im[FFT_NP - k];
  const float er = (ar + br) * 0.5f, ei = (ai - bi) * 0.5f;
  const float pr = (ai + bi) * 0.5f, pi = (br - ar) * 0.5f;
  const float2 w = tw[(FFT_NP - 1) + k];
  const float tr = pr * w.x - pi * w.y;
  const float ti = pr * w.y + pi * w.x;
  return hypotf(er + tr, ei + ti);
}

// staged twiddles: out[(h - 1) + p] = tw[p * (4096 / h)] for every stage half-size h = 1, 2, ... 4096 and p < h (8191 entries):
// the same table values, laid out so that a stage's twiddles are contiguous
__global__ void __launch_bounds__(256) yaapt_stage_twiddles_kernel(const float2* __restrict__ tw, float2* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // 0 .. 8190
  if (i >= FFT_N - 1) return;
  const int h = 1 << (31 - __clz(i + 1));                // largest power of two <= i + 1
  const int p = i + 1 - h;
  out[i] = tw[p * ((FFT_N / 2) / h)];
}

// nlfer: frame (560 samples) x hann -> FFT -> sum |X[nl_lo:nl_hi]|
__global__ void __launch_bounds__(FFT_THREADS) yaapt_nlfer_kernel(const float* __restrict__ filt, const float* __restrict__ hann,
                                                         const float2* __restrict__ tw, float* __restrict__ e_raw,
                                                         const int* __restrict__ U, const Plan P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* re = lds;
  float* im = lds + FFT_NP;
  __shared__ float red[8];
  const int f = blockIdx.x, b = blockIdx.y;
  if (f >= ulen(U, b, 2, P.nframes)) return;
  const float* x = filt + ((size_t)b * 2 + 0) * P.Lz + (size_t)f * P.frame_jump;
  const int first = fft_load_packed<FFT_LOG, FFT_THREADS>(re, im, P.frame_size, [&](int j) { return x[j] * hann[j]; });
  fft_from<FFT_LOG, FFT_THREADS>(re, im, tw, first);
  if (threadIdx.x >= 256) return;          // whole waves: the reduction keeps its 256-thread order
  float part = 0.f;
  for (int k = P.nl_lo + threadIdx.x; k < P.nl_hi; k += 256) part += fft_packed_mag(re, im, tw, k);
  const float tot = block_sum256(part, red);
  if (threadIdx.x == 0) e_raw[(size_t)b * P.nframes + f] = tot;
}

// energy / mean(energy), vuv = energy > nlfer_thresh1   (one block per utterance)
__global__ void __launch_bounds__(256) yaapt_energy_norm_kernel(const float* __restrict__ e_raw, float* __restrict__ energy,
                                                               int* __restrict__ vuv, const int* __restrict__ U, const Plan P) {
  __shared__ float red[8];
  const int b = blockIdx.x;
  const int nf = ulen(U, b, 2, P.nframes);
  const float* e = e_raw + (size_t)b * P.nframes;
  float part = 0.f;
  for (int f = threadIdx.x; f < nf; f += 256) part += e[f];
  const float mean = block_sum256(part, red) / (float)nf;
  for (int f = threadIdx.x; f < P.nframes; f += 256) {
    const float v = f < nf ? e[f] / mean : 0.f;
    energy[(size_t)b * P.nframes + f] = v;
    vuv[(size_t)b * P.nframes + f] = (f < nf && v > P.nlfer_thresh1) ? 1 : 0;
  }
}

// spectral track, per voiced frame: 1120 samples x kaiser, minus mean -> FFT -> |X| -> SHC -> peaks
// cand layout: [b][8][nframes] = pitch[0..3], merit[0..3]
// Two kernels (round 3): the FFT block held 64 KB of LDS and 16 waves (32 KB and 8 since the packed form), the SHC / peak search
// after it is a 256-thread, then one-thread, latency-bound tail of about the same duration — kept in one kernel it pinned that LDS
// for twice as long, and the FFT blocks leave little room on a CU for the generator's conv blocks of the other job streams.  The FFT
// kernel ends at the magnitude window (n_mag <= 1280 floats per frame, through the workspace); the tail runs with 6 KB of LDS.
// Same arithmetic in the same order: the F0 track was unchanged bit for bit by the split.
__global__ void __launch_bounds__(FFT_THREADS) yaapt_spec_kernel(const float* __restrict__ filt, const float* __restrict__ kaiser,
                                                        const float2* __restrict__ tw, const int* __restrict__ vuv,
                                                        float* __restrict__ magbuf, const int* __restrict__ U, const Plan P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* re = lds;
  float* im = lds + FFT_NP;
  __shared__ float red[8];
  const int tid = threadIdx.x;
  const int f = blockIdx.x, b = blockIdx.y;
  const int nf = P.nframes;                       // row stride
  if (f >= ulen(U, b, 2, nf)) return;
  if (!vuv[(size_t)b * nf + f]) return;           // unvoiced: the tail kernel writes the defaults
  const float* x = filt + ((size_t)b * 2 + 1) * P.Lz + (size_t)f * P.frame_jump;
  // windowed slice and its mean (nframe_size <= 5*256)
  float part = 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int j = tid + 256 * k;
    if (tid < 256 && j < P.nframe_size) part += x[j] * kaiser[j];
  }
  const float mean = block_sum256(part, red) / (float)P.nframe_size;
  const int first = fft_load_packed<FFT_LOG, FFT_THREADS>(re, im, P.nframe_size, [&](int j) { return x[j] * kaiser[j] - mean; });
  const int n_mag = P.min_shc * (P.nharm + 1) + (P.max_shc - P.min_shc) * (P.nharm + 1) + P.wl;  // exclusive bound
  fft_from<FFT_LOG, FFT_THREADS>(re, im, tw, first);
  // magnitude[i] = i < half_wl ? 0 : |X[i - half_wl]|
  float* mo = magbuf + ((size_t)b * nf + f) * SPEC_MAGP;
  for (int i = tid; i < n_mag; i += FFT_THREADS) mo[i] = i >= P.half_wl ? fft_packed_mag(re, im, tw, i - P.half_wl) : 0.f;
}

__global__ void __launch_bounds__(256) yaapt_spec_peaks_kernel(const float* __restrict__ magbuf, const int* __restrict__ vuv,
                                                               float* __restrict__ cand, const int* __restrict__ U, const Plan P) {
  __shared__ float mag[SPEC_MAGP];
  __shared__ float red[8];
  __shared__ float s_shc[256];
  __shared__ unsigned char s_flag[256];
  const int tid = threadIdx.x;
  const int f = blockIdx.x, b = blockIdx.y;
  const int nf = P.nframes;                       // row stride
  if (f >= ulen(U, b, 2, nf)) return;
  float* cp = cand + (size_t)b * 8 * nf;
  float* cm = cp + 4 * (size_t)nf;
  if (!vuv[(size_t)b * nf + f]) {
    if (tid < MAXP) { cp[(size_t)tid * nf + f] = 0.f; cm[(size_t)tid * nf + f] = 1.f; }
    return;
  }
  const int n_mag = P.min_shc * (P.nharm + 1) + (P.max_shc - P.min_shc) * (P.nharm + 1) + P.wl;  // exclusive bound
  const float* mi = magbuf + ((size_t)b * nf + f) * SPEC_MAGP;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int i = tid + 256 * k;
    if (i < n_mag) mag[i] = mi[i];
  }
  __syncthreads();
  // SHC[min_shc-1 + r] = sum_w prod_h mag[min_shc*(h+1) + r*(h+1) + w]
  const int rows = P.max_shc - P.min_shc + 1;
  float shc = 0.f;
  if (tid >= P.min_shc - 1 && tid < P.min_shc - 1 + rows) {
    const int r = tid - (P.min_shc - 1);
    float s = 0.f;
    for (int w = 0; w < P.wl; ++w) {
      float pr = mag[P.min_shc + r + w];
      for (int h = 1; h <= P.nharm; ++h) pr = pr * mag[(P.min_shc + r) * (h + 1) + w];
      s += pr;
    }
    shc = s;
  }
  // ---- peaks() on the 256-vector (yaapt.py:383-497) ----
  const int lo = P.pk_min_lag, hi = P.pk_max_lag, c = P.pk_center;
  const bool in_rng = tid >= lo && tid <= hi;
  const float mx = block_max256(in_rng ? shc : -INFINITY, red);
  if (mx > 1e-14f) shc = shc / mx;
  s_shc[tid] = shc;
  const float avg = block_sum256(in_rng ? shc : 0.f, red) / (float)(hi - lo + 1);
  bool ispk = false;
  if (tid >= lo + c + 1 && tid <= hi - c) {
    const float v = s_shc[tid];
    if (v > s_shc[tid - 1] && v > s_shc[tid + 1] && v > P.shc_thresh2 * avg) {
      ispk = true;  // argmax(data[n-c : n+c+1]) == c  <=>  strictly above everything before, >= everything after
      for (int i = tid - c; i < tid; ++i) ispk = ispk && (s_shc[i] < v);
      for (int i = tid + 1; i <= tid + c; ++i) ispk = ispk && (s_shc[i] <= v);
    }
  }
  s_flag[tid] = ispk ? 1 : 0;
  __syncthreads();
  if (tid != 0) return;
  float pit[MAXP], mer[MAXP];
  for (int i = 0; i < MAXP; ++i) { pit[i] = 0.f; mer[i] = 1.f; }
  bool done = avg > P.inv_shc_thresh1;
  if (!done) {
    // collect peaks in ascending lag; keep the MAXP largest merits, earlier index first on ties
    float sp[MAXP], sm[MAXP];
    int np = 0, total = 0;
    float maxm = 0.f;
    for (int n = lo + c + 1; n <= hi - c; ++n) {
      if (!s_flag[n]) continue;
      const float m = s_shc[n];
      const float pv = (float)n * P.delta;
      ++total;
      maxm = total == 1 ? m : fmaxf(maxm, m);
      int pos = np;
      while (pos > 0 && sm[pos - 1] < m) --pos;   // stable descending insertion
      if (pos < MAXP) {
        const int last = np < MAXP ? np : MAXP - 1;
        for (int i = last; i > pos; --i) { sp[i] = sp[i - 1]; sm[i] = sm[i - 1]; }
        sp[pos] = pv;
        sm[pos] = m;
        if (np < MAXP) ++np;
      }
    }
    if (total == 0) maxm = 0.f;
    if (maxm / avg < P.shc_thresh1) {
      done = true;
    } else if (np > 0) {
      for (int i = 0; i < MAXP; ++i) { pit[i] = i < np ? sp[i] : 0.f; mer[i] = i < np ? sm[i] : 0.f; }
      int k = np;
      if (pit[0] > P.f0_double) { k = k + 1 < MAXP ? k + 1 : MAXP; pit[k - 1] = pit[0] / 2.0f; mer[k - 1] = P.merit_extra; }
      if (pit[0] < P.f0_half) { k = k + 1 < MAXP ? k + 1 : MAXP; pit[k - 1] = pit[0] * 2.0f; mer[k - 1] = P.merit_extra; }
      for (int i = k; i < MAXP; ++i) { pit[i] = pit[0]; mer[i] = mer[0]; }
    }
  }
  for (int i = 0; i < MAXP; ++i) { cp[(size_t)i * nf + f] = pit[i]; cm[(size_t)i * nf + f] = mer[i]; }
}

// (the per-utterance helpers, median_small .. compact_frames, are in yaapt_dev.h)

// spec_track after the per-frame candidates: selection, smoothing, Viterbi, interpolation.
// LDS (floats): vcp[4*nf] vcm[4*nf] a[nf] b[nf] spec[nf]; shorts: vidx[nf], index[nf]; bytes pred[4*nf] path[nf]
// The statements are those of yaapt_spec_select_body.h, which the long form (csrc/yaapt_long/) includes too.
__global__ void __launch_bounds__(64) yaapt_spec_post_kernel(const float* __restrict__ cand, float* __restrict__ spec_out,
                                                            float* __restrict__ scal, int* __restrict__ status,
                                                            const int* __restrict__ U, const Plan P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
#define YAAPT_ARENA lds
#define YAAPT_SPEC_PATH1()                                                          \
  auto tr = [&](int i, int j, int t) {                                              \
    const float d = fabsf(vcp[j * nf + t] - vcp[i * nf + (t - 1)]) / f0min;         \
    return k1 * (0.05f * d + d * d);                                                \
  };                                                                                \
  path1_wave<4>(vcm, nf, nv, tr, pred, path)
#include "yaapt_spec_select_body.h"
#undef YAAPT_SPEC_PATH1
#undef YAAPT_ARENA
}

// frame means of time_track's in-place subtraction on overlapping views: frame k's first `ov`
// samples already carry frame k-1's mean, so  mean_k = (sum_{j<ov} (x_j - mean_{k-1}) + sum_{j>=ov} x_j) / n.
// One block per (utterance, signal): all four waves first reduce the recurrence-free tails of every
// frame (LDS), then wave 0 walks the frames with only the `ov`-sample head on the critical path
// (next frame's head prefetched).
__global__ void __launch_bounds__(256) yaapt_frame_means_kernel(const float* __restrict__ filt, float* __restrict__ fmean,
                                                               const int* __restrict__ U, const Plan P) {
  __shared__ float s_tail[2048];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, sig = blockIdx.y;
  const float* x = filt + ((size_t)b * 2 + sig) * P.Lz;
  float* m = fmean + ((size_t)b * 2 + sig) * P.nframes;
  const int ov = P.tda_len - P.frame_jump;
  const int T = ulen(U, b, 3, P.tda_nframes);
  for (int k = wave; k < T; k += 4) {
    float part = 0.f;
    for (int j = ov + lane; j < P.tda_len; j += 64) part += x[(size_t)k * P.frame_jump + j];
    part = wsum(part);
    if (lane == 0) s_tail[k] = part;
  }
  __syncthreads();
  if (wave != 0) return;
  auto head = [&](int k, int j) { return (k < T && j < ov) ? x[(size_t)k * P.frame_jump + j] : 0.f; };
  float h0 = head(0, lane), h1 = head(0, lane + 64);
  float prev = 0.f;
  for (int k = 0; k < T; ++k) {
    const float n0 = head(k + 1, lane), n1 = head(k + 1, lane + 64);   // prefetch
    float v0 = h0, v1 = h1;
    if (k > 0) {
      if (lane < ov) v0 = v0 - prev;
      if (lane + 64 < ov) v1 = v1 - prev;
    }
    const float mean = (wsum(v0 + v1) + s_tail[k]) / (float)P.tda_len;
    if (lane == 0) m[k] = mean;
    prev = mean;
    h0 = n0;
    h1 = n1;
  }
}

// NCCF candidate of one (utterance, signal, frame)
__global__ void __launch_bounds__(256) yaapt_nccf_kernel(const float* __restrict__ filt, const float* __restrict__ fmean,
                                                        const float* __restrict__ spec, float* __restrict__ scal,
                                                        float* __restrict__ tp, float* __restrict__ tm,
                                                        int* __restrict__ status, const int* __restrict__ U, const Plan P) {
  // the first `ov` samples carry the previous frame's mean and no older one (an overlap of at most 128 samples: yaapt_check_plan; the
  // wide form of csrc/yaapt_long/ subtracts every earlier mean).  The statements: yaapt_nccf_body.h, which the wide form includes too.
#define YAAPT_NCCF_PREVIOUS_MEANS()             \
  const float mprev = k > 0 ? fm[k - 1] : 0.f;  \
  const int ov = P.tda_len - P.frame_jump
#define YAAPT_NCCF_HEAD(v, j) \
  if (k > 0 && j < ov) v = v - mprev
#include "yaapt_nccf_body.h"
#undef YAAPT_NCCF_HEAD
#undef YAAPT_NCCF_PREVIOUS_MEANS
}

// refine + dynamic + path1 -> final pitch.  One wave per utterance; frames spread over lanes.
// LDS floats: rp[6*nf] rm[6*nf] ta[nf] tb[nf]; bytes pred[6*nf] path[nf]
// The statements are those of yaapt_refine_body.h, which the long form (csrc/yaapt_long/) includes too.
__global__ void __launch_bounds__(64) yaapt_refine_dp_kernel(const float* __restrict__ tp, const float* __restrict__ tm,
                                                            const float* __restrict__ spec, const float* __restrict__ energy,
                                                            const int* __restrict__ vuv, float* __restrict__ f0,
                                                            const float* __restrict__ scal, int* __restrict__ status,
                                                            float* __restrict__ refined, const int* __restrict__ U, const Plan P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
#define YAAPT_ARENA lds
#define YAAPT_REFINE_PATH1()                                                                                                      \
  auto tr = [&](int i, int j, int t) {                                                                                            \
    const float p1 = rp[j * nf + t], p2 = rp[i * nf + (t - 1)];                                                                   \
    float v = 1.f;                                                                                                                \
    if (p1 > 0.f && p2 > 0.f) v = w1 * (fabsf(p1 - p2) / mean_pitch);                                                             \
    else if ((p1 == 0.f && p2 > 0.f) || (p1 > 0.f && p2 == 0.f)) v = w2 * (1.f - tmin(1.f, fabsf(en[t - 1] - en[t])));            \
    else if (p1 == 0.f && p2 == 0.f) v = w3;                                                                                      \
    return v / w4;                                                                                                                \
  };                                                                                                                              \
  path1_wave<NC>(rm, nf, nf, tr, pred, path)
#include "yaapt_refine_body.h"
#undef YAAPT_REFINE_PATH1
#undef YAAPT_ARENA
}

// ---- host side.  The pieces below are what sat_yaapt_long_f32 (csrc/yaapt_long/) calls too: declared in yaapt_dev.h ----
size_t yaapt_ws_floats(const Plan& P, int B) {
  const size_t nf = P.nframes;
  return (size_t)B * (2 * (size_t)P.Lz + 3 * nf /*e_raw, energy, vuv*/ + 8 * nf /*cand*/ + nf /*spec*/ + 4 /*scal*/ +
                      2 * nf /*fmean*/ + 4 * nf /*tp, tm*/ + 2 * NC * nf /*refined*/ + (size_t)SPEC_MAGP * nf /*magnitude windows*/) + 2 * FFT_N /*staged twiddles*/ + 8 + 64;
}

YaaptBuffers yaapt_carve(const Plan& P, int B, void* workspace) {
  YaaptBuffers W;
  const size_t nf = P.nframes;
  float* w = (float*)workspace;
  W.filt = w;            w += (size_t)B * 2 * P.Lz;
  W.e_raw = w;           w += (size_t)B * nf;
  W.energy = w;          w += (size_t)B * nf;
  W.vuv = (int*)w;       w += (size_t)B * nf;
  W.cand = w;            w += (size_t)B * 8 * nf;
  W.spec = w;            w += (size_t)B * nf;
  W.scal = w;            w += (size_t)B * 4;
  W.fmean = w;           w += (size_t)B * 2 * nf;
  W.tp = w;              w += (size_t)B * 2 * nf;
  W.tm = w;              w += (size_t)B * 2 * nf;
  W.refined = w;         w += (size_t)B * 2 * NC * nf;
  W.magbuf = w;          w += (size_t)B * nf * SPEC_MAGP;
  w += (4 - ((uintptr_t)w / 4) % 4) % 4;                     // 16-byte alignment of the float2 table
  W.stw = (float2*)w;
  return W;
}

int yaapt_check_plan(const Plan& P, int B, bool resident) {
  SAT_REQUIRE(B > 0 && P.n > 0, "yaapt: empty batch");
  SAT_REQUIRE(P.nfft == FFT_N, "yaapt: fft_length %d not supported (8192 only)", P.nfft);
  SAT_REQUIRE(P.maxpeaks == MAXP && P.maxcands * 2 == NC, "yaapt: shc_maxpeaks/nccf_maxcands must be 4/3");
  SAT_REQUIRE(P.nharm >= 1 && P.nharm <= 7, "yaapt: shc_numharms out of range");
  // reference asserts 15 < frame_size < 2048 (yaapt.py:885-886)
  SAT_REQUIRE(P.frame_size > 15, "Frame length value %d is too short.", P.frame_size);
  SAT_REQUIRE(P.frame_size < 2048, "Frame length value %d exceeds the limit.", P.frame_size);
  SAT_REQUIRE(P.nframe_size <= 5 * 256 && P.frame_size <= FFT_N, "yaapt: frame_length too long for the spectral kernel");
  // the bins read off the packed transform: Z[k] and Z[4096 - k], 0 <= k < 4096 (the SHC's are below 5 * 256, next requirement but one)
  SAT_REQUIRE(P.nl_lo >= 0 && P.nl_hi <= FFT_NP, "yaapt: NLFER bins %d..%d outside the half spectrum", P.nl_lo, P.nl_hi);
  SAT_REQUIRE(P.max_shc <= 256 && P.pk_max_lag + 1 < 256 && P.pk_min_lag + P.pk_center + 1 >= 1 &&
                  P.pk_min_lag - 0 >= 0, "yaapt: SHC range out of the 256-bin kernel window");
  SAT_REQUIRE(P.min_shc * (P.nharm + 1) + (P.max_shc - P.min_shc) * (P.nharm + 1) + P.wl <= 5 * 256,
              "yaapt: SHC harmonics exceed the spectral kernel's magnitude window");
  // the overlap of at most 128 samples is the resident kernels' (two head loads per lane, the previous mean only); the long form has
  // kernels for a frame that overlaps several earlier ones and its own limit on their number
  SAT_REQUIRE(P.tda_len <= 1024 && P.tda_len > P.frame_jump && (!resident || P.tda_len - P.frame_jump <= 128),
              "yaapt: tda_frame_length / frame_space combination not supported");
  SAT_REQUIRE(P.median_value >= 1 && P.median_value <= 7 && (P.median_value & 1), "yaapt: median_value must be odd <= 7");
  if (resident)
    SAT_REQUIRE(P.nframes >= 4 && P.nframes <= YAAPT_MAX_RESIDENT_FRAMES, "yaapt: %d frames not supported (4..2048, i.e. up to ~40 s)", P.nframes);
  SAT_REQUIRE(P.tda_nframes == P.nframes, "yaapt: tda frame count differs from the analysis frame count");
  // frame_space > frame_length: the reference fails on a negative zero extension of spec_track (yaapt.py:206-210)
  SAT_REQUIRE(P.nframe_size + (P.nframes - 1) * P.frame_jump >= P.L,
              "yaapt: frame_space too long for frame_length: the last spectral frame ends at sample %d of the %d padded ones "
              "(the reference fails on the negative zero extension of spec_track)", P.nframe_size + (P.nframes - 1) * P.frame_jump, P.L);
  SAT_REQUIRE(P.L == P.n + 2 * P.pad && P.Lz >= P.L && P.Lz >= P.nframe_size + (P.nframes - 1) * P.frame_jump,
              "yaapt: plan lengths inconsistent (L = n + 2 pad, Lz covers the padded signal and the last spectral frame)");
  return SAT_OK;
}

int yaapt_launch_front(const Plan& P, const float* wav, const int32_t* U, int32_t* status, const float* hann, const float* kaiser,
                       const float* twiddle, const YaaptBuffers& W, int B, hipStream_t s) {
  float* filt = W.filt;
  const float2* tw = (const float2*)twiddle;
  SAT_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * B, s));

  const bool pf_vec = (P.n % 4 == 0) && (P.pad % 4 == 0) && (P.Lz % 4 == 0) && (((uintptr_t)wav & 15) == 0) && (((uintptr_t)filt & 15) == 0);
  SAT_REQUIRE((size_t)32 * P.n * 4 < ((size_t)1 << 31) && (size_t)64 * P.Lz * 4 < ((size_t)1 << 31), "yaapt: utterance too long for the prefilter's 31-bit row offsets");
  if (pf_vec) hipLaunchKernelGGL(yaapt_prefilter_kernel<true>, dim3((B + 31) / 32), dim3(PF_THREADS), 0, s, wav, filt, U, P, B);
  else hipLaunchKernelGGL(yaapt_prefilter_kernel<false>, dim3((B + 31) / 32), dim3(PF_THREADS), 0, s, wav, filt, U, P, B);
  SAT_LAUNCH_CHECK("yaapt_prefilter_kernel");
  const size_t fft_lds = 2 * FFT_NP * sizeof(float);
  static std::atomic<uint64_t> attr_done{0};      // per device
  int dev;
  if (attr_needed_on_current_device(attr_done, &dev)) {
    SAT_HIP(hipFuncSetAttribute((const void*)yaapt_nlfer_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    SAT_HIP(hipFuncSetAttribute((const void*)yaapt_spec_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
    SAT_HIP(hipFuncSetAttribute((const void*)yaapt_spec_post_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    SAT_HIP(hipFuncSetAttribute((const void*)yaapt_refine_dp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done_on_device(attr_done, dev);
  }
  hipLaunchKernelGGL(yaapt_stage_twiddles_kernel, dim3(FFT_N / 256), dim3(256), 0, s, tw, W.stw);
  SAT_LAUNCH_CHECK("yaapt_stage_twiddles_kernel");
  hipLaunchKernelGGL(yaapt_nlfer_kernel, dim3(P.nframes, B), dim3(FFT_THREADS), fft_lds, s, filt, hann, W.stw, W.e_raw, U, P);
  SAT_LAUNCH_CHECK("yaapt_nlfer_kernel");
  hipLaunchKernelGGL(yaapt_energy_norm_kernel, dim3(B), dim3(256), 0, s, W.e_raw, W.energy, W.vuv, U, P);
  SAT_LAUNCH_CHECK("yaapt_energy_norm_kernel");
  hipLaunchKernelGGL(yaapt_spec_kernel, dim3(P.nframes, B), dim3(FFT_THREADS), fft_lds, s, filt, kaiser, W.stw, W.vuv, W.magbuf, U, P);
  SAT_LAUNCH_CHECK("yaapt_spec_kernel");
  hipLaunchKernelGGL(yaapt_spec_peaks_kernel, dim3(P.nframes, B), dim3(256), 0, s, W.magbuf, W.vuv, W.cand, U, P);
  SAT_LAUNCH_CHECK("yaapt_spec_peaks_kernel");
  return SAT_OK;
}

int yaapt_launch_nccf(const Plan& P, const int32_t* U, int32_t* status, const YaaptBuffers& W, int B, hipStream_t s) {
  hipLaunchKernelGGL(yaapt_nccf_kernel, dim3(P.nframes, 2, B), dim3(256), 0, s, W.filt, W.fmean, W.spec, W.scal, W.tp, W.tm, status, U, P);
  SAT_LAUNCH_CHECK("yaapt_nccf_kernel");
  return SAT_OK;
}

}  // namespace sat

using namespace sat;

extern "C" size_t sat_yaapt_workspace_bytes(const sat_yaapt_plan* plan, int B) {
  if (!plan || B <= 0) return 0;
  return align_up(yaapt_ws_floats(*plan, B) * sizeof(float), 256);
}

static int yaapt_run(const sat_yaapt_plan* plan, const float* wav, const int32_t* U, float* f0, int32_t* status,
                     const float* hann, const float* kaiser, const float* twiddle, void* workspace,
                     size_t workspace_bytes, int B, void* stream) {
  SAT_REQUIRE(plan && wav && f0 && status && hann && kaiser && twiddle && workspace, "yaapt: null pointer");
  const Plan& P = *plan;
  const int ok = yaapt_check_plan(P, B, true);
  if (ok != SAT_OK) return ok;
  SAT_REQUIRE_WORKSPACE(workspace_bytes >= sat_yaapt_workspace_bytes(plan, B), "yaapt: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t nf = P.nframes;
  const YaaptBuffers W = yaapt_carve(P, B, workspace);
  const int front = yaapt_launch_front(P, wav, U, status, hann, kaiser, twiddle, W, B, s);
  if (front != SAT_OK) return front;
  const size_t post_lds = (size_t)nf * (4 + 4 + 3) * sizeof(float) + nf * 2 * sizeof(short) + nf * 5;
  hipLaunchKernelGGL(yaapt_spec_post_kernel, dim3(B), dim3(64), post_lds, s, W.cand, W.spec, W.scal, status, U, P);
  SAT_LAUNCH_CHECK("yaapt_spec_post_kernel");
  hipLaunchKernelGGL(yaapt_frame_means_kernel, dim3(B, 2), dim3(256), 0, s, W.filt, W.fmean, U, P);
  SAT_LAUNCH_CHECK("yaapt_frame_means_kernel");
  const int nccf = yaapt_launch_nccf(P, U, status, W, B, s);
  if (nccf != SAT_OK) return nccf;
  const size_t dp_lds = (size_t)nf * (2 * NC + 2) * sizeof(float) + nf * (NC + 1);
  hipLaunchKernelGGL(yaapt_refine_dp_kernel, dim3(B), dim3(64), dp_lds, s, W.tp, W.tm, W.spec, W.energy, W.vuv, f0, W.scal, status, W.refined, U, P);
  SAT_LAUNCH_CHECK("yaapt_refine_dp_kernel");
  return SAT_OK;
}

extern "C" int sat_yaapt_f32(const sat_yaapt_plan* plan, const float* wav, float* f0, int32_t* status,
                             const float* hann, const float* kaiser, const float* twiddle, void* workspace,
                             size_t workspace_bytes, int B, void* stream) {
  return yaapt_run(plan, wav, nullptr, f0, status, hann, kaiser, twiddle, workspace, workspace_bytes, B, stream);
}

extern "C" int sat_yaapt_ragged_f32(const sat_yaapt_plan* plan, const float* wav, const int32_t* utt_dims, float* f0,
                                    int32_t* status, const float* hann, const float* kaiser, const float* twiddle,
                                    void* workspace, size_t workspace_bytes, int B, void* stream) {
  SAT_REQUIRE(utt_dims, "yaapt_ragged: null utt_dims");
  return yaapt_run(plan, wav, utt_dims, f0, status, hann, kaiser, twiddle, workspace, workspace_bytes, B, stream);
}
