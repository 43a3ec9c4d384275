// What the kernels of the x-vector extractor (ECAPA-TDNN) share between their row form (csrc/xvector.hip: one utterance per row of a
// [B][C][T] tensor) and their segment form (csrc/ragged/xvector_ragged.hip: B utterances of unequal length side by side on a packed time
// axis): ONE copy of each body.  The kernels only say which utterance, row or tile a block or wave works on, where its rows lie and how
// far apart they are; every load, operation and store of a result is issued by the text below, so a segment of a ragged batch has the
// bits of the single call by construction.  The bodies are __forceinline__ functions, except the Res2 chain's, which is expanded in place
// (below, at R2_MARG; profiles/xvector_tile_refactor.txt).
// Reference: satools/satools/sidekit/preprocessor.py:164-236 (MelSpecFrontEnd: PreEmphasis -> torchaudio
// MelSpectrogram(n_fft 1024, win 400, hop 160, 90-7600 Hz, 80 mel, power 2) + 1e-6 -> log -> InstanceNorm1d),
// satools/satools/augmentation.py:219-244 (PreEmphasis), sidekit/nn.py:75-154 (Res2Net sums, SE gate),
// sidekit/pooling.py:141-155 (AttentiveStatsPool).
#pragma once
#include "common.h"

namespace sat {

constexpr int XV_NFFT = 1024;
constexpr int XV_WIN = 400;
constexpr int XV_HOP = 160;
constexpr int XV_FPB = 4;   // frames per block, one wave each

__device__ __forceinline__ float xv_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float xv_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// pre-emphasised sample i of the utterance: x[i] - coef * x[i-1], x[-1] := x[1] (reflect pad of one sample)
__device__ __forceinline__ float preemph(const float* __restrict__ x, int n, int i, float coef) {
  const float prev = i > 0 ? x[i - 1] : x[n > 1 ? 1 : 0];
  return x[i] - coef * prev;
}

// One wave per frame, XV_FPB frames per block (every wave of the block comes here, `live` or not: the twiddles and the barriers are the
// block's): 400 windowed samples of the pre-emphasised, centre-reflect-padded utterance x[0 .. n - 1] in the middle of a 1024-point frame
// -> radix-2 FFT in LDS -> power -> sparse mel dot products -> log(. + 1e-6).  Frame f = 0 .. n / hop (torch.stft, center=True); mel m of
// it goes to col[m * pitch].
__device__ __forceinline__ void melspec_logmel_frame(const float* __restrict__ x, int n, int f, bool live, float* __restrict__ col, int pitch,
                                                     const float* __restrict__ window, const float* __restrict__ fb,
                                                     const int* __restrict__ fb_lo, const int* __restrict__ fb_hi, int n_mel, float coef) {
  __shared__ float s_re[XV_FPB][XV_NFFT];
  __shared__ float s_im[XV_FPB][XV_NFFT];
  __shared__ float s_twr[XV_NFFT / 2], s_twi[XV_NFFT / 2];
  __shared__ float s_pw[XV_FPB][XV_NFFT / 2 + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < XV_NFFT / 2; k += blockDim.x) {
    float s, c;
    sincospif(-(float)k / (float)(XV_NFFT / 2), &s, &c);
    s_twr[k] = c;
    s_twi[k] = s;
  }
  float* re = s_re[wv];
  float* im = s_im[wv];
  constexpr int off = (XV_NFFT - XV_WIN) / 2;   // the window sits in the middle of the n_fft frame (torch.stft)
#pragma unroll
  for (int k = 0; k < XV_NFFT / 64; ++k) {
    const int j = lane + 64 * k;
    float v = 0.f;
    if (live && j >= off && j < off + XV_WIN) {
      int s = f * XV_HOP + j - XV_NFFT / 2;       // index into the signal, reflect-padded by n_fft/2 on both sides
      if (s < 0) s = -s;
      if (s >= n) s = 2 * (n - 1) - s;
      s = s < 0 ? 0 : (s >= n ? n - 1 : s);
      v = preemph(x, n, s, coef) * window[j - off];
    }
    re[(int)(__brev((unsigned)j) >> 22)] = v;   // bit-reversed scatter (10 bits)
    im[j] = 0.f;
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 1; s <= 10; ++s) {
    const int half = 1 << (s - 1);
    const int tstep = XV_NFFT >> s;
#pragma unroll
    for (int k = 0; k < XV_NFFT / 2 / 64; ++k) {
      const int i = lane + 64 * k;
      const int pos = i & (half - 1);
      const int a = ((i >> (s - 1)) << s) + pos;
      const int c = a + half;
      const float wr = s_twr[pos * tstep], wi = s_twi[pos * tstep];
      const float xr = re[c], xi = im[c];
      const float tr = xr * wr - xi * wi;
      const float ti = xr * wi + xi * wr;
      const float ur = re[a], ui = im[a];
      re[a] = ur + tr;
      im[a] = ui + ti;
      re[c] = ur - tr;
      im[c] = ui - ti;
    }
    __syncthreads();
  }
  for (int k = lane; k <= XV_NFFT / 2; k += 64) s_pw[wv][k] = re[k] * re[k] + im[k] * im[k];   // |X|^2 (power = 2)
  __syncthreads();
  if (!live) return;
  for (int m = lane; m < n_mel; m += 64) {
    const float* row = fb + (size_t)m * (XV_NFFT / 2 + 1);
    float acc = 0.f;
    for (int k = fb_lo[m]; k < fb_hi[m]; ++k) acc = fmaf(s_pw[wv][k], row[k], acc);
    col[(size_t)m * pitch] = logf(acc + 1e-6f);
  }
}

// InstanceNorm1d(affine=False, eps) of one row by one wave: yr[t] = (xr[t] - mean) / sqrt(biased var + eps), t = 0 .. T - 1
__device__ __forceinline__ void instnorm_row_wave(const float* __restrict__ xr, float* __restrict__ yr, int T, int lane, float eps) {
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += xr[t];
  const float mean = xv_wave_sum(s) / (float)T;
  float q = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float d = xr[t] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(xv_wave_sum(q) / (float)T + eps);
  for (int t = lane; t < T; t += 64) yr[t] = (xr[t] - mean) * rstd;
}

// mean over time of one row by one wave, stored by lane 0 (SE_Connect's x.mean(dim=2), sidekit/nn.py:132)
__device__ __forceinline__ void row_mean_wave(const float* __restrict__ xr, int T, int lane, float* __restrict__ dst) {
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += xr[t];
  s = xv_wave_sum(s);
  if (lane == 0) *dst = s / (float)T;
}

// SE gate and the block's skip connections at element i: z * sigmoid(g) + s1 (+ s2 (+ s3)), added left to right like
// `layer(x) + out1 + out2 + out3` (sidekit/archi.py:183-185)
__device__ __forceinline__ float se_gate_value(const float* __restrict__ z, float g, const float* __restrict__ s1, const float* __restrict__ s2,
                                               const float* __restrict__ s3, size_t i) {
  const float gate = 1.0f / (1.0f + expf(-g));
  float v = z[i] * gate;
  if (s1) v = v + s1[i];
  if (s2) v = v + s2[i];
  if (s3) v = v + s3[i];
  return v;
}

// AttentiveStatsPool tail of one (utterance, channel) row by one wave: w = softmax_t(lr), m1 = sum w xr, m2 = sum w xr^2, in every lane
__device__ __forceinline__ void attentive_stats_wave(const float* __restrict__ xr, const float* __restrict__ lr, int T, int lane, float* m1_out,
                                                     float* m2_out) {
  float mx = -INFINITY;
  for (int t = lane; t < T; t += 64) mx = fmaxf(mx, lr[t]);
  mx = xv_wave_max(mx);
  float se = 0.f;
  for (int t = lane; t < T; t += 64) se += expf(lr[t] - mx);
  se = xv_wave_sum(se);
  float m1 = 0.f, m2 = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float w = expf(lr[t] - mx) / se;
    const float v = xr[t];
    m1 += w * v;
    m2 += w * (v * v);
  }
  *m1_out = xv_wave_sum(m1);
  *m2_out = xv_wave_sum(m2);
}
// ... and what the row's lane 0 stores in out [B][2C] (means then stds), dst = &out[b][c]: mean = m1, std = sqrt(max(m2 - m1^2, 1e-9))
__device__ __forceinline__ void attentive_stats_store(float* __restrict__ dst, int C, float m1, float m2) {
  const float var = m2 - m1 * m1;
  dst[0] = m1;
  dst[C] = sqrtf(var > 1e-9f ? var : 1e-9f);
}

// ---- Res2Conv1dReluBn (sidekit/nn.py:74-110) of 64-channel pieces as ONE launch: sp_i = bn_i(relu(conv_i(sp_{i-1} + x_i))), i = 0 .. nums - 1,
// the last piece copied.  Launched conv by conv the chain is 7 x (add3 + a 64 -> 64 three-tap conv of 31 us, latency-bound) per block of the
// net.  Here a block keeps a window of W = 64 NT columns of ONE utterance in LDS — the piece's input (x_i + previous output) and its output,
// 32 columns of halo on either side (the receptive field of the chain grows by one dilation per piece: 7 x 4 <= 32) — and walks the pieces:
// exact f32 on v_mfma_f32_32x32x2_f32 (A = the piece's weights [tap][ci][co] staged in LDS, B = input columns shifted by the tap), four waves =
// two 32-row tiles x two halves of the window.  Only the W - 64 centre columns are stored; fringe columns compute on zeros and are dropped.
constexpr int R2_MARG = 4, R2_HALO = 32;
typedef float r2_f32x16 __attribute__((ext_vector_type(16)));

constexpr size_t res2_chain_lds_bytes(int NT) { return ((size_t)2 * 64 * (64 * NT + 2 * R2_MARG) + 3 * 64 * 64) * sizeof(float); }

// The block's work on one (utterance or segment, centre tile) is csrc/xvector_chain_body.h: STATEMENTS #included inside the two kernel
// templates, not a function.  Columns 0 .. T - 1 of the rows of yb / zb are the utterance, the tile's centre starts at column t0, and the
// kernel names the distance of two rows by the macro R2_PITCH (a call of its own: T itself; a segment of a packed axis: T_tot).  As a
// __forceinline__ function template res2_chain_tile<NT>(yb, zb, pitch, T, t0, ...) the same statements compiled to other code (hipcc
// optimises a callee on its own before it inlines it): 16 ds_write_b32 fewer in all four instantiations, 1887 -> 1873 and 3776 -> 3756
// instructions per call, 4074 -> 3712 per segment at NT = 3.  Expanded in place the four kernels have the instruction counts and registers
// they had when each held its own copy (profiles/xvector_tile_refactor.txt).

// the chain kernels need more dynamic LDS than the default limit: the attribute is set once per device, then the launch.  `kernel` is
// the source's own chain kernel <NT>: one `attr_done` per NT and source, so a source passes ONE kernel per NT
template <int NT, typename... P, typename... A>
static int launch_res2_chain(void (*kernel)(P...), dim3 grid, hipStream_t stream, A... args) {
  constexpr size_t lds = res2_chain_lds_bytes(NT);
  static std::atomic<uint64_t> attr_done{0};      // per device
  int dev;
  if (attr_needed_on_current_device(attr_done, &dev)) {
    SAT_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_done_on_device(attr_done, dev);
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, args...);
  return SAT_OK;
}

}  // namespace sat
