// Device helpers of the YAAPT kernels that csrc/yaapt.hip (one block holds a whole utterance, up to 2048 frames) and
// csrc/yaapt_long/yaapt_long.hip (any length, the per-utterance arrays in the workspace) share, and the host-side pieces of
// yaapt_run that the long entry point calls: the plan checks, the workspace layout and the launches of the per-frame kernels,
// which live in yaapt.hip (the library is not linked with relocatable device code: a kernel is launched from its own file).
#pragma once
#include <cmath>

#include "common.h"

namespace sat {

typedef sat_yaapt_plan Plan;

constexpr int FFT_N = 8192;          // fft_length: the real transform whose bins the stages read
constexpr int FFT_LOG = 12;          // the frames are real: two samples per complex point, FFT_N / 2 points (see the FFT in yaapt.hip)
constexpr int FFT_NP = 1 << FFT_LOG;
constexpr int MAXP = 4;   // shc_maxpeaks
constexpr int NC = 6;     // refine candidates: 2 tracks x nccf_maxcands
constexpr int SPEC_MAGP = 5 * 256;      // floats per frame of the magnitude hand-over (the kernels' 5 x 256 window)
constexpr int YAAPT_MAX_RESIDENT_FRAMES = 2048;   // sat_yaapt_f32 / sat_yaapt_ragged_f32: one block's LDS holds the utterance

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wmin_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
// block-wide sum of one float per thread (256 threads), result broadcast; `red` = 8 floats of LDS
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wsum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) red[threadIdx.x >> 6] = v;   // waves past the fourth (FFT helpers) only read
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max256(float v, float* red) {
  v = wmax(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// torch.maximum / torch.minimum propagate NaN
__device__ __forceinline__ float tmax(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }
__device__ __forceinline__ float tmin(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }

// ragged batches: U[b] = {samples, padded length L, frames, tda frames} of utterance b (host-computed with the
// plan's formulas); null = every utterance has the plan's length.  Row strides stay the plan's (the longest).
__device__ __forceinline__ int ulen(const int* __restrict__ U, int b, int k, int dflt) { return U ? U[b * 4 + k] : dflt; }

// ------------------------------------------------------------------------------------------------
// per-utterance helpers: ONE wave per utterance, all 64 lanes work (frames are spread
// over lanes; only the Viterbi recursion itself is sequential in time, and it runs its C x C
// transitions on C*C lanes).  Callers separate phases with __syncthreads() (a one-wave block).
// The arrays are in LDS (yaapt.hip) or in the workspace (yaapt_long.hip): the loops are lane-strided, no load depends on another.
// ------------------------------------------------------------------------------------------------
__device__ float median_small(float* v, int k) {  // k odd, <= 7: middle order statistic
  for (int i = 1; i < k; ++i) {
    const float x = v[i];
    int j = i - 1;
    while (j >= 0 && v[j] > x) { v[j + 1] = v[j]; --j; }
    v[j + 1] = x;
  }
  return v[k / 2];
}
__device__ void medfilt_par(const float* in, float* out, int n, int k) {  // zero-padded sliding median
  const int pad = k / 2;
  for (int i = threadIdx.x; i < n; i += 64) {
    float w[7];
    for (int j = 0; j < 7; ++j) {
      const int s = i + j - pad;
      w[j] = (j < k && s >= 0 && s < n) ? in[s] : 0.f;
    }
    out[i] = median_small(w, k);
  }
}
__device__ double wsum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ float mean_par(const float* v, int n) {   // f64 accumulation, rounded once
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += (double)v[i];
  return (float)(wsum_d(s) / (double)n);   // n == 0 -> NaN like torch.mean of an empty tensor
}
__device__ float std_unbiased_par(const float* v, int n) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += (double)v[i];
  const double m = wsum_d(s) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) { const double d = (double)v[i] - m; q += d * d; }
  return (float)sqrt(wsum_d(q) / (double)(n - 1));  // n == 1 -> NaN
}

// path1 (yaapt.py:530-570) on one wave.  local [C][T] (row stride ls), trans(i, j, t) supplied by
// a functor.  aux[i][j] = PCOST[j] + trans[i][j][t]; K[i] = LAST argmin_j; CCOST[i] = PCOST[K[i]] +
// trans[K[i]][i][t] + local[i][t]; p_small = LAST argmin_i CCOST.  Back-trace P[t] = PRED[P[t+1]][t+1].
// Lane (i*C + j) evaluates transition (i, j); lane l < C carries PCOST[l].
// torch.argmin treats NaN as the smallest value and returns the FIRST one; the reference takes it on the flipped row
// ("last minimum"), so a NaN cost beats every number and the LAST NaN of a row wins.  NaN costs are real: an utterance
// whose median-filtered best track is all zero (noise: `rand` inputs) has mean_pitch = mean(empty) = NaN in
// dynamic() (yaapt.py:326), and every voiced-to-voiced transition cost is NaN.
__device__ __forceinline__ bool path1_takes(float cand, float best) {
  return (cand != cand) || (!(best != best) && cand <= best);
}
template <int C, class TransFn>
__device__ void path1_wave(const float* local, int ls, int T, TransFn trans, unsigned char* pred,
                           unsigned char* path_out) {
  const int lane = threadIdx.x;
  const bool act = lane < C * C;
  const int i = act ? lane / C : 0;
  const int j = act ? lane % C : 0;
  float pc = lane < C ? local[lane * ls] : 0.f;
  for (int t = 1; t < T; ++t) {
    const float pcj = __shfl(pc, j, 64);
    const float v = pcj + trans(i, j, t);
    int K = 0;
    float bv = __shfl(v, i * C, 64);
#pragma unroll
    for (int jj = 1; jj < C; ++jj) {
      const float vv = __shfl(v, i * C + jj, 64);
      if (path1_takes(vv, bv)) { bv = vv; K = jj; }   // last minimum wins
    }
    const float pcK = __shfl(pc, K, 64);
    const float cc = (pcK + trans(K, i, t)) + local[i * ls + t];
    if (act && j == 0) pred[(size_t)i * T + t] = (unsigned char)K;
    pc = __shfl(cc, (lane * C) & 63, 64);   // lane l < C <- CCOST[l] (held by lane l*C)
  }
  __syncthreads();
  // p_small[T-1] = last argmin_i PCOST (0 when T == 1); every lane computes it from the shuffles
  int p = 0;
  {
    float jv = __shfl(pc, 0, 64);
#pragma unroll
    for (int ii = 1; ii < C; ++ii) {
      const float cv = __shfl(pc, ii, 64);
      if (path1_takes(cv, jv)) { jv = cv; p = ii; }
    }
    if (T <= 1) p = 0;
  }
  if (lane == 0) {
    path_out[T - 1] = (unsigned char)p;
    for (int t = T - 2; t >= 0; --t) {
      p = pred[(size_t)p * T + (t + 1)];
      path_out[t] = (unsigned char)p;
    }
  }
  __syncthreads();
}

// stable compaction of the frames selected by `flag(f)` (ascending frame order): returns the count,
// writes the selected frame indices to idx[]
template <class Pred>
__device__ int compact_frames(int nf, Pred flag, short* idx) {
  int base = 0;
  for (int f0 = 0; f0 < nf; f0 += 64) {
    const int f = f0 + threadIdx.x;
    const bool on = f < nf && flag(f);
    const unsigned long long mask = __ballot(on);
    if (on) idx[base + __popcll(mask & ((1ull << threadIdx.x) - 1ull))] = (short)f;
    base += __popcll(mask);
  }
  return base;
}

// ---- host side, defined in yaapt.hip -----------------------------------------------------------------------------
// the workspace of sat_yaapt_f32, carved: the long form keeps this layout at the head of its own workspace
struct YaaptBuffers {
  float *filt, *e_raw, *energy;
  int* vuv;
  float *cand, *spec, *scal, *fmean, *tp, *tm, *refined, *magbuf;
  float2* stw;
};
size_t yaapt_ws_floats(const Plan& P, int B);
YaaptBuffers yaapt_carve(const Plan& P, int B, void* workspace);
// every requirement of yaapt_run on a plan but the workspace's size; `resident` = with the 4..2048 frame range of the
// one-block kernels and their overlap of at most 128 samples (the long form has its own ranges)
int yaapt_check_plan(const Plan& P, int B, bool resident);
// status memset, prefilter, staged twiddles, NLFER, energy norm, spectrum, peaks  /  NCCF: the per-frame kernels, any frame count
int yaapt_launch_front(const Plan& P, const float* wav, const int32_t* U, int32_t* status, const float* hann, const float* kaiser,
                       const float* twiddle, const YaaptBuffers& W, int B, hipStream_t s);
int yaapt_launch_nccf(const Plan& P, const int32_t* U, int32_t* status, const YaaptBuffers& W, int B, hipStream_t s);

}  // namespace sat
