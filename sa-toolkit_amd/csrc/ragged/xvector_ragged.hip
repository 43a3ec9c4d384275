// Segment forms of the x-vector extractor's row kernels (csrc/xvector.hip) for a RAGGED batch on a packed time axis
// (include/satools_hip_ragged.h: B utterances of unequal length side by side in one [C][T_tot] tensor, segment i at columns
// off_i .. off_i + T_i - 1, gap columns between them that hold anything).  Each kernel keeps the per-row order of operations of the row
// kernel it comes from, so that segment i of its result has the bits of that kernel's result on utterance i alone; each selects on load
// (a gap column or another segment never reaches an output, NaN included) and clamps or skips what a wrong table names.
#include "../common.h"
#include "../../../include/satools_hip_ragged.h"

namespace sat {

constexpr int RG_NFFT = 1024;
constexpr int RG_WIN = 400;
constexpr int RG_HOP = 160;
constexpr int RG_FPB = 4;    // frames per block, one wave each
constexpr int RG_CPB = 8;    // channels per block of the gate kernel: one segment search per thread serves them all

__device__ __forceinline__ float rg_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float rg_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// segment i of the table -> (first column, columns); false for an entry that does not lie inside 0 .. T_tot - 1
__device__ __forceinline__ bool rg_segment(const int* __restrict__ seg_off, const int* __restrict__ seg_len, int i, int T_tot, int* off,
                                           int* len) {
  const int o = seg_off[i], l = seg_len[i];
  *off = o;
  *len = l;
  return o >= 0 && l >= 1 && o < T_tot && l <= T_tot - o;
}

// the segment that holds column t, or -1 for a gap column: the last i with seg_off[i] <= t (ascending offsets), then its length
__device__ __forceinline__ int rg_find(const int* __restrict__ seg_off, const int* __restrict__ seg_len, int B, int T_tot, int t, int* off) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= t) lo = mid;
    else hi = mid;
  }
  int len;
  if (!rg_segment(seg_off, seg_len, lo, T_tot, off, &len)) return -1;
  return (t >= *off && t - *off < len) ? lo : -1;
}

__device__ __forceinline__ float rg_preemph(const float* __restrict__ x, int n, int i, float coef) {
  const float prev = i > 0 ? x[i - 1] : x[n > 1 ? 1 : 0];
  return x[i] - coef * prev;
}

// melspec_logmel_kernel with the utterance's own length: one wave per frame, frame f of utterance b at column off_b + f of out [n_mel][T_tot]
__global__ void __launch_bounds__(64 * RG_FPB)
melspec_logmel_segments_kernel(const float* __restrict__ wav, const int* __restrict__ n_samples, const int* __restrict__ seg_off,
                               const int* __restrict__ seg_len, float* __restrict__ out, const float* __restrict__ window,
                               const float* __restrict__ fb, const int* __restrict__ fb_lo, const int* __restrict__ fb_hi, int n_max,
                               int T_tot, int n_mel, float coef) {
  __shared__ float s_re[RG_FPB][RG_NFFT];
  __shared__ float s_im[RG_FPB][RG_NFFT];
  __shared__ float s_twr[RG_NFFT / 2], s_twi[RG_NFFT / 2];
  __shared__ float s_pw[RG_FPB][RG_NFFT / 2 + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int n = n_samples[b];
  int col0, frames;
  // (the whole block leaves together: nothing below is reached by a part of it)
  if (!rg_segment(seg_off, seg_len, b, T_tot, &col0, &frames) || n < 1 || n > n_max || (int)blockIdx.x * RG_FPB >= frames) return;
  const int f = blockIdx.x * RG_FPB + wv;
  const bool live = f < frames;
  const float* x = wav + (size_t)b * n_max;
  for (int k = threadIdx.x; k < RG_NFFT / 2; k += blockDim.x) {
    float s, c;
    sincospif(-(float)k / (float)(RG_NFFT / 2), &s, &c);
    s_twr[k] = c;
    s_twi[k] = s;
  }
  float* re = s_re[wv];
  float* im = s_im[wv];
  constexpr int off = (RG_NFFT - RG_WIN) / 2;
#pragma unroll
  for (int k = 0; k < RG_NFFT / 64; ++k) {
    const int j = lane + 64 * k;
    float v = 0.f;
    if (live && j >= off && j < off + RG_WIN) {
      int s = f * RG_HOP + j - RG_NFFT / 2;       // reflect at the utterance's own ends
      if (s < 0) s = -s;
      if (s >= n) s = 2 * (n - 1) - s;
      s = s < 0 ? 0 : (s >= n ? n - 1 : s);
      v = rg_preemph(x, n, s, coef) * window[j - off];
    }
    re[(int)(__brev((unsigned)j) >> 22)] = v;
    im[j] = 0.f;
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 1; s <= 10; ++s) {
    const int half = 1 << (s - 1);
    const int tstep = RG_NFFT >> s;
#pragma unroll
    for (int k = 0; k < RG_NFFT / 2 / 64; ++k) {
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
  for (int k = lane; k <= RG_NFFT / 2; k += 64) s_pw[wv][k] = re[k] * re[k] + im[k] * im[k];
  __syncthreads();
  if (!live) return;
  for (int m = lane; m < n_mel; m += 64) {
    const float* row = fb + (size_t)m * (RG_NFFT / 2 + 1);
    float acc = 0.f;
    for (int k = fb_lo[m]; k < fb_hi[m]; ++k) acc = fmaf(s_pw[wv][k], row[k], acc);
    out[(size_t)m * T_tot + col0 + f] = logf(acc + 1e-6f);
  }
}

// instnorm_rows_kernel per (row, segment), one wave each; the wave also writes the zeros that follow its segment up to the next one
// (the first segment's wave: those in front of it too), so that every column of y is written exactly once
__global__ void __launch_bounds__(256) instnorm_segments_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                const int* __restrict__ seg_off, const int* __restrict__ seg_len, int R, int B,
                                                                int T_tot, float eps) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= R * B) return;
  const int r = w / B, i = w - r * B;
  // a wrong table is clamped into the row: 0 <= off <= off + T <= nxt <= T_tot
  int off = seg_off[i], T = seg_len[i], nxt = i + 1 < B ? seg_off[i + 1] : T_tot;
  off = min(max(off, 0), T_tot);
  T = min(max(T, 0), T_tot - off);
  nxt = min(max(nxt, off + T), T_tot);
  const float* xr = x + (size_t)r * T_tot + off;
  float* yr = y + (size_t)r * T_tot;
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += xr[t];
  const float mean = rg_wave_sum(s) / (float)T;
  float q = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float d = xr[t] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(rg_wave_sum(q) / (float)T + eps);
  for (int t = lane; t < T; t += 64) yr[off + t] = (xr[t] - mean) * rstd;
  for (int t = off + T + lane; t < nxt; t += 64) yr[t] = 0.f;
  if (i == 0)
    for (int t = lane; t < off; t += 64) yr[t] = 0.f;
}

// row_mean_rows_kernel per (channel, segment): x [C][T_tot] -> y [B][C]
__global__ void __launch_bounds__(256) row_mean_segments_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                const int* __restrict__ seg_off, const int* __restrict__ seg_len, int C, int B,
                                                                int T_tot) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= C * B) return;
  const int c = w / B, i = w - c * B;
  int off, T;
  if (!rg_segment(seg_off, seg_len, i, T_tot, &off, &T)) return;
  const float* xr = x + (size_t)c * T_tot + off;
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += xr[t];
  s = rg_wave_sum(s);
  if (lane == 0) y[(size_t)i * C + c] = s / (float)T;
}

// se_gate_add_kernel on the packed axis: a thread owns one column, finds its segment once and walks RG_CPB channels; gap columns leave
__global__ void __launch_bounds__(256) se_gate_add_segments_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                                   const float* __restrict__ s1, const float* __restrict__ s2,
                                                                   const float* __restrict__ s3, float* __restrict__ y,
                                                                   const int* __restrict__ seg_off, const int* __restrict__ seg_len, int C, int B,
                                                                   int T_tot, long long y_cs) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T_tot) return;
  int off;
  const int seg = rg_find(seg_off, seg_len, B, T_tot, t, &off);
  if (seg < 0) return;
  const int c0 = blockIdx.y * RG_CPB, c1 = min(c0 + RG_CPB, C);
  for (int ch = c0; ch < c1; ++ch) {
    const size_t i = (size_t)ch * T_tot + t;
    const float gate = 1.0f / (1.0f + expf(-g[(size_t)seg * C + ch]));
    float v = z[i] * gate;
    if (s1) v = v + s1[i];
    if (s2) v = v + s2[i];
    if (s3) v = v + s3[i];
    y[ch * y_cs + t] = v;
  }
}

// attentive_stats_kernel per (channel, segment): x, logits [C][T_tot] -> out [B][2C]
__global__ void __launch_bounds__(256) attentive_stats_segments_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                                       float* __restrict__ out, const int* __restrict__ seg_off,
                                                                       const int* __restrict__ seg_len, int C, int B, int T_tot) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= C * B) return;
  const int c = w / B, b = w - c * B;
  int off, T;
  if (!rg_segment(seg_off, seg_len, b, T_tot, &off, &T)) return;
  const float* xr = x + (size_t)c * T_tot + off;
  const float* lr = logits + (size_t)c * T_tot + off;
  float mx = -INFINITY;
  for (int t = lane; t < T; t += 64) mx = fmaxf(mx, lr[t]);
  mx = rg_wave_max(mx);
  float se = 0.f;
  for (int t = lane; t < T; t += 64) se += expf(lr[t] - mx);
  se = rg_wave_sum(se);
  float m1 = 0.f, m2 = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float wgt = expf(lr[t] - mx) / se;
    const float v = xr[t];
    m1 += wgt * v;
    m2 += wgt * (v * v);
  }
  m1 = rg_wave_sum(m1);
  m2 = rg_wave_sum(m2);
  if (lane == 0) {
    const float var = m2 - m1 * m1;
    out[(size_t)b * 2 * C + c] = m1;
    out[(size_t)b * 2 * C + C + c] = sqrtf(var > 1e-9f ? var : 1e-9f);
  }
}

// ---- res2_chain_kernel<NT> (csrc/xvector.hip) with a block per (segment, centre tile): the utterance's bounds 0 <= t < T are the segment's,
// on the loads and on the inside / keep tests alike; rows are T_tot apart and the segment starts at column `off` of each.  The window, the
// halo, the wave layout and the (tap, channel) order of the 96 MFMA steps are that kernel's.
constexpr int RG_MARG = 4, RG_HALO = 32;
typedef float rg_f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
__global__ void __launch_bounds__(256) res2_chain_segments_kernel(const float* __restrict__ y, float* __restrict__ z, const float* __restrict__ w,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const int* __restrict__ seg_off, const int* __restrict__ seg_len,
                                                                  const int* __restrict__ tiles, int B, int T_tot, int nums, int dil) {
  extern __shared__ __attribute__((aligned(16))) float rg_lds[];
  constexpr int W = 64 * NT, WP = W + 2 * RG_MARG, TT = W - 2 * RG_HALO;
  float* bufA = rg_lds;                   // [64][WP] input of the current piece
  float* bufB = bufA + 64 * WP;           // [64][WP] its output (zero outside the segment)
  float* wl = bufB + 64 * WP;             // [3][64][64] weights of the current piece
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int seg = tiles[2 * blockIdx.x], t0 = tiles[2 * blockIdx.x + 1];
  if (seg < 0 || seg >= B) return;        // (block-uniform, like the two tests below)
  int off, T;
  if (!rg_segment(seg_off, seg_len, seg, T_tot, &off, &T)) return;
  if (t0 < 0 || t0 >= T) return;
  const int t_lo = t0 - RG_HALO;
  const float* yb = y + off;
  float* zb = z + off;
  const int mt = wave >> 1, n0 = (wave & 1) * NT;

  for (int i = tid; i < 64 * 2 * RG_MARG; i += 256) {
    const int c = i / (2 * RG_MARG), m = i % (2 * RG_MARG);
    const int col = m < RG_MARG ? m : W + m;
    bufA[c * WP + col] = 0.f;
  }
  {
    float y0[64 * W / 256];
#pragma unroll
    for (int k = 0; k < 64 * W / 256; ++k) {
      const int i = tid + 256 * k, c = i / W, j = i - c * W, t = t_lo + j;
      y0[k] = (t >= 0 && t < T) ? yb[(size_t)c * T_tot + t] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 64 * W / 256; ++k) {
      const int i = tid + 256 * k, c = i / W, j = i - c * W;
      bufA[c * WP + RG_MARG + j] = y0[k];
    }
  }
  constexpr int NIN = 64 * W / 256;
  for (int p = 0; p < nums; ++p) {
    float4 wv[12];
    const float4* w4 = (const float4*)(w + (size_t)p * 3 * 64 * 64);
#pragma unroll
    for (int k = 0; k < 12; ++k) wv[k] = w4[tid + 256 * k];
    float yn[NIN];
    const bool more = p + 1 < nums;
    {
      const float* yp = yb + (size_t)(p + 1) * 64 * T_tot;
#pragma unroll
      for (int k = 0; k < NIN; ++k) {
        const int i = tid + 256 * k, c = i / W, j = i - c * W, t = t_lo + j;
        yn[k] = (more && t >= 0 && t < T) ? yp[(size_t)c * T_tot + t] : 0.f;
      }
    }
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * lh;
      sc[r] = scale[p * 64 + co], sh[r] = shift[p * 64 + co];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) ((float4*)wl)[tid + 256 * k] = wv[k];
    __syncthreads();
    rg_f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const float* xa = bufA + RG_MARG + 32 * n0 + l31 + lh * WP;
    const float* wa = wl + 32 * mt + l31 + lh * 64;
    for (int tap = 0; tap < 3; ++tap) {
      const float* xt = xa + (tap - 1) * dil;
      const float* wt = wa + tap * 64 * 64;
#pragma unroll 2
      for (int ci = 0; ci < 64; ci += 8) {
        float a4[4], b4[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a4[u] = wt[(ci + 2 * u) * 64];
#pragma unroll
          for (int n = 0; n < NT; ++n) b4[u][n] = xt[(ci + 2 * u) * WP + 32 * n];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], b4[u][n], acc[n], 0, 0, 0);
      }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int j = 32 * (n0 + n) + l31, t = t_lo + j;
      const bool inside = t >= 0 && t < T, keep = inside && j >= RG_HALO && j < RG_HALO + TT;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float v = fmaxf(acc[n][r], 0.f) * sc[r] + sh[r];
        bufB[co * WP + RG_MARG + j] = inside ? v : 0.f;
        if (keep) zb[(size_t)(p * 64 + co) * T_tot + t] = v;
      }
    }
    __syncthreads();
    if (more) {
#pragma unroll
      for (int k = 0; k < NIN; ++k) {
        const int i = tid + 256 * k, c = i / W, j = i - c * W;
        bufA[c * WP + RG_MARG + j] = yn[k] + bufB[c * WP + RG_MARG + j];
      }
    }
  }
  // the piece the chain leaves untouched
  const float* yl = yb + (size_t)nums * 64 * T_tot;
  float* zl = zb + (size_t)nums * 64 * T_tot;
  for (int i = tid; i < 64 * TT; i += 256) {
    const int c = i / TT, t = t0 + (i - c * TT);
    if (t < T) zl[(size_t)c * T_tot + t] = yl[(size_t)c * T_tot + t];
  }
}

template <int NT>
static int launch_res2_chain_segments(const float* y, float* z, const float* w, const float* scale, const float* shift, const int32_t* seg_off,
                                      const int32_t* seg_len, const int32_t* tiles, int n_tiles, int B, int T_tot, int nums, int dilation,
                                      hipStream_t stream) {
  const size_t lds = ((size_t)2 * 64 * (64 * NT + 2 * RG_MARG) + 3 * 64 * 64) * sizeof(float);
  static std::atomic<uint64_t> attr_done{0};      // per device (one per instantiation)
  int dev;
  if (attr_needed_on_current_device(attr_done, &dev)) {
    SAT_HIP(hipFuncSetAttribute((const void*)res2_chain_segments_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_done_on_device(attr_done, dev);
  }
  hipLaunchKernelGGL(res2_chain_segments_kernel<NT>, dim3(n_tiles), dim3(256), lds, stream, y, z, w, scale, shift, seg_off, seg_len, tiles, B,
                     T_tot, nums, dilation);
  return SAT_OK;
}

}  // namespace sat

using namespace sat;

#define RG_TABLE_OK(what) \
  SAT_REQUIRE(seg_off && seg_len && B >= 1 && B <= SAT_RAGGED_MAX_SEGMENTS && T_tot >= 1, what ": a segment table of 1 .. %d segments and T_tot >= 1 are needed", SAT_RAGGED_MAX_SEGMENTS)

extern "C" int sat_melspec_logmel_segments_f32(const float* wav, const int32_t* n_samples, const int32_t* n_samples_host, const int32_t* seg_off,
                                               const int32_t* seg_len, float* out, const float* window, const float* fb, const int32_t* fb_lo,
                                               const int32_t* fb_hi, int B, int n_max, int T_tot, int n_mel, float coef, void* stream) {
  SAT_REQUIRE(wav && n_samples && out && window && fb && fb_lo && fb_hi, "melspec_logmel_segments: null pointer");
  RG_TABLE_OK("melspec_logmel_segments");
  SAT_REQUIRE(n_max > RG_NFFT / 2 && n_mel > 0, "melspec_logmel_segments: rows of %d samples are shorter than the reflect padding", n_max);
  SAT_REQUIRE((long long)n_mel * T_tot < (1ll << 31), "melspec_logmel_segments: output of 2^31 elements or more");
  if (n_samples_host)
    for (int i = 0; i < B; ++i)
      SAT_REQUIRE(n_samples_host[i] > RG_NFFT / 2 && n_samples_host[i] <= n_max,
                  "melspec_logmel_segments: utterance %d of %d samples is shorter than the reflect padding (513 samples) or longer than the row (%d)", i,
                  n_samples_host[i], n_max);
  dim3 grid(ceil_div(1 + n_max / RG_HOP, RG_FPB), B);
  hipLaunchKernelGGL(melspec_logmel_segments_kernel, grid, dim3(64 * RG_FPB), 0, (hipStream_t)stream, wav, n_samples, seg_off, seg_len, out,
                     window, fb, fb_lo, fb_hi, n_max, T_tot, n_mel, coef);
  SAT_LAUNCH_CHECK("melspec_logmel_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_instnorm_segments_f32(const float* x, float* y, const int32_t* seg_off, const int32_t* seg_len, int R, int B, int T_tot,
                                         float eps, void* stream) {
  SAT_REQUIRE(x && y && R > 0, "instnorm_segments: bad arguments");
  RG_TABLE_OK("instnorm_segments");
  SAT_REQUIRE((long long)R * B < (1ll << 31), "instnorm_segments: too many (row, segment) pairs");
  hipLaunchKernelGGL(instnorm_segments_kernel, dim3(ceil_div(R * B, 4)), dim3(256), 0, (hipStream_t)stream, x, y, seg_off, seg_len, R, B, T_tot,
                     eps);
  SAT_LAUNCH_CHECK("instnorm_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_row_mean_segments_f32(const float* x, float* y, const int32_t* seg_off, const int32_t* seg_len, int C, int B, int T_tot,
                                         void* stream) {
  SAT_REQUIRE(x && y && C > 0, "row_mean_segments: bad arguments");
  RG_TABLE_OK("row_mean_segments");
  SAT_REQUIRE((long long)C * B < (1ll << 31), "row_mean_segments: too many (channel, segment) pairs");
  hipLaunchKernelGGL(row_mean_segments_kernel, dim3(ceil_div(C * B, 4)), dim3(256), 0, (hipStream_t)stream, x, y, seg_off, seg_len, C, B, T_tot);
  SAT_LAUNCH_CHECK("row_mean_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_se_gate_add_segments_f32(const float* z, const float* gate_logits, const float* s1, const float* s2, const float* s3, float* y,
                                            const int32_t* seg_off, const int32_t* seg_len, int C, int B, int T_tot, int64_t y_cs, void* stream) {
  SAT_REQUIRE(z && gate_logits && y && C > 0 && C < 65536 * RG_CPB, "se_gate_add_segments: bad arguments");
  SAT_REQUIRE((s1 || !s2) && (s2 || !s3), "se_gate_add_segments: the skips are given from the left");
  RG_TABLE_OK("se_gate_add_segments");
  hipLaunchKernelGGL(se_gate_add_segments_kernel, dim3(ceil_div(T_tot, 256), ceil_div(C, RG_CPB)), dim3(256), 0, (hipStream_t)stream, z,
                     gate_logits, s1, s2, s3, y, seg_off, seg_len, C, B, T_tot, (long long)y_cs);
  SAT_LAUNCH_CHECK("se_gate_add_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_attentive_stats_segments_f32(const float* x, const float* logits, float* out, const int32_t* seg_off, const int32_t* seg_len,
                                                int C, int B, int T_tot, void* stream) {
  SAT_REQUIRE(x && logits && out && C > 0, "attentive_stats_segments: bad arguments");
  RG_TABLE_OK("attentive_stats_segments");
  SAT_REQUIRE((long long)C * B < (1ll << 31), "attentive_stats_segments: too many (channel, segment) pairs");
  hipLaunchKernelGGL(attentive_stats_segments_kernel, dim3(ceil_div(C * B, 4)), dim3(256), 0, (hipStream_t)stream, x, logits, out, seg_off,
                     seg_len, C, B, T_tot);
  SAT_LAUNCH_CHECK("attentive_stats_segments_kernel");
  return SAT_OK;
}

extern "C" int sat_res2_chain_segments_f32(const float* y, float* z, const float* w, const float* scale, const float* shift,
                                           const int32_t* seg_off, const int32_t* seg_len, const int32_t* tiles, int n_tiles64, int n_tiles128,
                                           int B, int C, int T_tot, int nums, int dilation, int centre, void* stream) {
  SAT_REQUIRE(y && z && y != z && w && scale && shift && tiles, "res2_chain_segments: bad arguments");
  RG_TABLE_OK("res2_chain_segments");
  SAT_REQUIRE(nums >= 1 && C == (nums + 1) * 64, "res2_chain_segments: pieces of 64 channels, C = (nums + 1) * 64");
  SAT_REQUIRE(dilation >= 1 && dilation <= RG_MARG && dilation * nums <= RG_HALO, "res2_chain_segments: dilation x pieces exceeds the staged halo");
  SAT_REQUIRE(centre == 0 || centre == 64 || centre == 128, "res2_chain_segments: centre is 0 (automatic), 64 or 128, not %d", centre);
  SAT_REQUIRE(n_tiles64 >= 0 && n_tiles128 >= 0, "res2_chain_segments: negative tile count");
  // 128-column centres when that fills the CUs, else 64 (sat_res2_chain_f32's rule)
  const bool wide = centre == 128 || (centre == 0 && n_tiles128 >= 256);
  SAT_REQUIRE((wide ? n_tiles128 : n_tiles64) >= 1, "res2_chain_segments: no tile of %d-column centres in the table", wide ? 128 : 64);
  int st;
  if (wide) st = launch_res2_chain_segments<3>(y, z, w, scale, shift, seg_off, seg_len, tiles + 2 * (size_t)n_tiles64, n_tiles128, B, T_tot, nums, dilation, (hipStream_t)stream);
  else st = launch_res2_chain_segments<2>(y, z, w, scale, shift, seg_off, seg_len, tiles, n_tiles64, B, T_tot, nums, dilation, (hipStream_t)stream);
  if (st != SAT_OK) return st;
  SAT_LAUNCH_CHECK("res2_chain_segments_kernel");
  return SAT_OK;
}
