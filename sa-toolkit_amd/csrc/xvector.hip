// Kernels of the x-vector extractor (ECAPA-TDNN) that are not convolutions, in their row form: one utterance per row of [B][C][T].
// The bodies they share with the segment forms of csrc/ragged/xvector_ragged.hip are in csrc/xvector_tile.h, with the reference lines;
// here: egs/asv/voxceleb/local/tuning/ecapa_tdnn.py:74-76 (L2 norm).
#include "xvector_tile.h"

namespace sat {

// melspec_logmel_frame per (utterance b, frame f): out [B][n_mel][frames], frames = 1 + n / hop
__global__ void __launch_bounds__(64 * XV_FPB)
melspec_logmel_kernel(const float* __restrict__ wav, float* __restrict__ out, const float* __restrict__ window,
                      const float* __restrict__ fb, const int* __restrict__ fb_lo, const int* __restrict__ fb_hi, int n,
                      int frames, int n_mel, float coef) {
  const int b = blockIdx.y;
  const int f = blockIdx.x * XV_FPB + (threadIdx.x >> 6);
  melspec_logmel_frame(wav + (size_t)b * n, n, f, f < frames, out + (size_t)b * n_mel * frames + f, frames, window, fb, fb_lo, fb_hi, n_mel,
                       coef);
}

// instnorm_row_wave per row of [R][T]
__global__ void __launch_bounds__(256) instnorm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int T,
                                                            float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  instnorm_row_wave(x + (size_t)r * T, y + (size_t)r * T, T, lane, eps);
}

// row_mean_wave per row of [R][T] -> y [R]
__global__ void __launch_bounds__(256) row_mean_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int T) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  row_mean_wave(x + (size_t)r * T, T, lane, y + r);
}

// y = a + b (+ c): channel slices of [B][C][T] tensors (batch / channel strides, T contiguous)
__global__ void __launch_bounds__(256) add3_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                   const float* __restrict__ c, float* __restrict__ y, int C, int T,
                                                   long long a_bs, long long a_cs, long long b_bs, long long b_cs,
                                                   long long c_bs, long long c_cs, long long y_bs, long long y_cs) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int ch = blockIdx.y, bt = blockIdx.z;
  if (t >= T) return;
  float v = a[bt * a_bs + ch * a_cs + t] + b[bt * b_bs + ch * b_cs + t];
  if (c) v = v + c[bt * c_bs + ch * c_cs + t];
  y[bt * y_bs + ch * y_cs + t] = v;
}

// se_gate_value per element of [B][C][T]; y with batch / channel strides
__global__ void __launch_bounds__(256) se_gate_add_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                          const float* __restrict__ s1, const float* __restrict__ s2,
                                                          const float* __restrict__ s3, float* __restrict__ y, int C, int T,
                                                          long long y_bs, long long y_cs) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int ch = blockIdx.y, bt = blockIdx.z;
  if (t >= T) return;
  y[bt * y_bs + ch * y_cs + t] = se_gate_value(z, g[(size_t)bt * C + ch], s1, s2, s3, ((size_t)bt * C + ch) * T + t);
}

__global__ void __launch_bounds__(256) tanh_kernel(float* __restrict__ x, size_t n) {
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i < n) x[i] = tanhf(x[i]);
}

// attentive_stats_wave per (b, c) row of x, logits [B][C][T] -> out [B][2C]
__global__ void __launch_bounds__(256) attentive_stats_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                              float* __restrict__ out, int B, int C, int T) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B * C) return;
  float m1, m2;
  attentive_stats_wave(x + (size_t)r * T, logits + (size_t)r * T, T, lane, &m1, &m2);
  if (lane == 0) {
    const int b = r / C, c = r - b * C;
    attentive_stats_store(out + (size_t)b * 2 * C + c, C, m1, m2);
  }
}

// F.normalize(x, dim=1): rows of [R][D] divided by max(||row||, 1e-12); one wave per row
__global__ void __launch_bounds__(256) l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int D) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s = fmaf(x[(size_t)r * D + d], x[(size_t)r * D + d], s);
  const float nrm = fmaxf(sqrtf(xv_wave_sum(s)), 1e-12f);
  for (int d = lane; d < D; d += 64) y[(size_t)r * D + d] = x[(size_t)r * D + d] / nrm;
}

// ---- Linear layers on pooled vectors (the squeeze-excitation MLP, the embedding layer): y[b][o] = epi(w[o] . x[b]).
// One wave per output row and group of NB batch rows (the weight row is read once for the group); the conv tile at T = 1 spent
// 141 us per layer on a K loop of 32 dependent chunk round trips for one useful column.
template <int NB, bool VEC>
__global__ void __launch_bounds__(256) linear_rows_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ y,
                                                          int B, int Cin, int Cout, int relu) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = blockIdx.x * 4 + wave, b0 = blockIdx.y * NB;
  if (o >= Cout) return;
  const int nb = min(NB, B - b0);
  float acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.f;
  const float* wr = w + (size_t)o * Cin;
  if (VEC) {
    for (int i = 4 * lane; i < Cin; i += 256) {
      const float4 wv = *(const float4*)(wr + i);
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const float4 xv = *(const float4*)(x + (size_t)(b0 + (k < nb ? k : 0)) * Cin + i);
        acc[k] = __builtin_fmaf(wv.x, xv.x, acc[k]);
        acc[k] = __builtin_fmaf(wv.y, xv.y, acc[k]);
        acc[k] = __builtin_fmaf(wv.z, xv.z, acc[k]);
        acc[k] = __builtin_fmaf(wv.w, xv.w, acc[k]);
      }
    }
  } else {
    for (int i = lane; i < Cin; i += 64) {
      const float wv = wr[i];
#pragma unroll
      for (int k = 0; k < NB; ++k) acc[k] = __builtin_fmaf(wv, x[(size_t)(b0 + (k < nb ? k : 0)) * Cin + i], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
  if (lane == 0) {
    const float bi = bias ? bias[o] : 0.f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (k >= nb) break;
      float v = acc[k] + bi;
      if (relu) v = fmaxf(v, 0.f);
      if (scale) v = v * scale[o] + (shift ? shift[o] : 0.f);
      y[(size_t)(b0 + k) * Cout + o] = v;
    }
  }
}

// the Res2 chain (csrc/xvector_tile.h) per (utterance b, centre tile) of y, z [B][C][T]: the rows are the utterance's own, T apart
template <int NT>
__global__ void __launch_bounds__(256) res2_chain_kernel(const float* __restrict__ y, float* __restrict__ z, const float* __restrict__ w,
                                                         const float* __restrict__ scale, const float* __restrict__ shift, int C, int T, int nums,
                                                         int dil) {
  const int b = blockIdx.y, t0 = blockIdx.x * (64 * NT - 2 * R2_HALO);
  const float* yb = y + (size_t)b * C * T;
  float* zb = z + (size_t)b * C * T;
#define R2_PITCH T
#include "xvector_chain_body.h"
#undef R2_PITCH
}

}  // namespace sat

using namespace sat;

extern "C" int sat_melspec_logmel_f32(const float* wav, float* out, const float* window, const float* fb,
                                      const int32_t* fb_lo, const int32_t* fb_hi, int B, int n, int n_mel, float coef,
                                      void* stream) {
  SAT_REQUIRE(wav && out && window && fb && fb_lo && fb_hi, "melspec_logmel: null pointer");
  SAT_REQUIRE(B > 0 && n > XV_NFFT / 2 && n_mel > 0, "melspec_logmel: utterance of %d samples is shorter than the reflect padding", n);
  const int frames = 1 + n / XV_HOP;
  dim3 grid(ceil_div(frames, XV_FPB), B);
  hipLaunchKernelGGL(melspec_logmel_kernel, grid, dim3(64 * XV_FPB), 0, (hipStream_t)stream, wav, out, window, fb, fb_lo, fb_hi,
                     n, frames, n_mel, coef);
  SAT_LAUNCH_CHECK("melspec_logmel_kernel");
  return SAT_OK;
}

extern "C" int sat_instnorm_rows_f32(const float* x, float* y, int R, int T, float eps, void* stream) {
  SAT_REQUIRE(x && y && R > 0 && T > 0, "instnorm_rows: bad arguments");
  hipLaunchKernelGGL(instnorm_rows_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, x, y, R, T, eps);
  SAT_LAUNCH_CHECK("instnorm_rows_kernel");
  return SAT_OK;
}

extern "C" int sat_row_mean_f32(const float* x, float* y, int R, int T, void* stream) {
  SAT_REQUIRE(x && y && R > 0 && T > 0, "row_mean: bad arguments");
  hipLaunchKernelGGL(row_mean_rows_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, x, y, R, T);
  SAT_LAUNCH_CHECK("row_mean_rows_kernel");
  return SAT_OK;
}

extern "C" int sat_add3_f32(const float* a, const float* b, const float* c, float* y, int B, int C, int T, int64_t a_bs,
                            int64_t a_cs, int64_t b_bs, int64_t b_cs, int64_t c_bs, int64_t c_cs, int64_t y_bs, int64_t y_cs,
                            void* stream) {
  SAT_REQUIRE(a && b && y && B > 0 && C > 0 && T > 0 && B < 65536 && C < 65536, "add3: bad arguments");
  hipLaunchKernelGGL(add3_kernel, dim3(ceil_div(T, 256), C, B), dim3(256), 0, (hipStream_t)stream, a, b, c, y, C, T,
                     (long long)a_bs, (long long)a_cs, (long long)b_bs, (long long)b_cs, (long long)c_bs, (long long)c_cs,
                     (long long)y_bs, (long long)y_cs);
  SAT_LAUNCH_CHECK("add3_kernel");
  return SAT_OK;
}

extern "C" int sat_se_gate_add_f32(const float* z, const float* gate_logits, const float* s1, const float* s2,
                                   const float* s3, float* y, int B, int C, int T, int64_t y_bs, int64_t y_cs, void* stream) {
  SAT_REQUIRE(z && gate_logits && y && B > 0 && C > 0 && T > 0 && B < 65536 && C < 65536, "se_gate_add: bad arguments");
  hipLaunchKernelGGL(se_gate_add_kernel, dim3(ceil_div(T, 256), C, B), dim3(256), 0, (hipStream_t)stream, z, gate_logits, s1, s2,
                     s3, y, C, T, (long long)y_bs, (long long)y_cs);
  SAT_LAUNCH_CHECK("se_gate_add_kernel");
  return SAT_OK;
}

extern "C" int sat_tanh_inplace_f32(float* x, size_t n, void* stream) {
  SAT_REQUIRE(x && n > 0, "tanh: bad arguments");
  hipLaunchKernelGGL(tanh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n);
  SAT_LAUNCH_CHECK("tanh_kernel");
  return SAT_OK;
}

extern "C" int sat_attentive_stats_f32(const float* x, const float* logits, float* out, int B, int C, int T, void* stream) {
  SAT_REQUIRE(x && logits && out && B > 0 && C > 0 && T > 0, "attentive_stats: bad arguments");
  hipLaunchKernelGGL(attentive_stats_kernel, dim3(ceil_div(B * C, 4)), dim3(256), 0, (hipStream_t)stream, x, logits, out, B, C, T);
  SAT_LAUNCH_CHECK("attentive_stats_kernel");
  return SAT_OK;
}

extern "C" int sat_l2norm_rows_f32(const float* x, float* y, int R, int D, void* stream) {
  SAT_REQUIRE(x && y && R > 0 && D > 0, "l2norm_rows: bad arguments");
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, x, y, R, D);
  SAT_LAUNCH_CHECK("l2norm_rows_kernel");
  return SAT_OK;
}

extern "C" int sat_linear_rows_f32(const float* x, const float* w, const float* bias, const float* ch_scale, const float* ch_shift,
                                   int relu, float* y, int B, int Cin, int Cout, void* stream) {
  SAT_REQUIRE(x && w && y && x != y && B > 0 && Cin > 0 && Cout > 0 && B < 65536 * 8, "linear_rows: bad arguments");
  SAT_REQUIRE(ch_scale || !ch_shift, "linear_rows: ch_shift without ch_scale");
  constexpr int NB = 8;
  const bool vec = Cin % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0;
  const dim3 grid(ceil_div(Cout, 4), ceil_div(B, NB));
  if (vec) hipLaunchKernelGGL((linear_rows_kernel<NB, true>), grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, ch_scale, ch_shift, y, B, Cin, Cout, relu);
  else hipLaunchKernelGGL((linear_rows_kernel<NB, false>), grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, ch_scale, ch_shift, y, B, Cin, Cout, relu);
  SAT_LAUNCH_CHECK("linear_rows_kernel");
  return SAT_OK;
}

extern "C" int sat_res2_chain_f32(const float* y, float* z, const float* w, const float* scale, const float* shift, int B, int C, int T,
                                  int nums, int dilation, void* stream) {
  SAT_REQUIRE(y && z && y != z && w && scale && shift && B > 0 && T > 0 && B < 65536, "res2_chain: bad arguments");
  SAT_REQUIRE(nums >= 1 && C == (nums + 1) * 64, "res2_chain: pieces of 64 channels, C = (nums + 1) * 64");
  SAT_REQUIRE(dilation >= 1 && dilation <= R2_MARG && dilation * nums <= R2_HALO, "res2_chain: dilation x pieces exceeds the staged halo");
  // 128-column centres when that fills the CUs, else 64
  const bool wide = (long long)B * ceil_div(T, 128) >= 256;
  const int st = wide ? launch_res2_chain<3>(res2_chain_kernel<3>, dim3(ceil_div(T, 128), B), (hipStream_t)stream, y, z, w, scale, shift, C, T, nums, dilation)
                      : launch_res2_chain<2>(res2_chain_kernel<2>, dim3(ceil_div(T, 64), B), (hipStream_t)stream, y, z, w, scale, shift, C, T, nums, dilation);
  if (st != SAT_OK) return st;
  SAT_LAUNCH_CHECK("res2_chain_kernel");
  return SAT_OK;
}
