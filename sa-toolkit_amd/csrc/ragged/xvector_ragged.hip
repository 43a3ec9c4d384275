// Segment forms of the x-vector extractor's row kernels (csrc/xvector.hip) for a RAGGED batch on a packed time axis
// (include/satools_hip_ragged.h: B utterances of unequal length side by side in one [C][T_tot] tensor, segment i at columns
// off_i .. off_i + T_i - 1, gap columns between them that hold anything).  Each kernel keeps the per-row order of operations of the row
// kernel it comes from, so that segment i of its result has the bits of that kernel's result on utterance i alone; each selects on load
// (a gap column or another segment never reaches an output, NaN included) and clamps or skips what a wrong table names.
//
// The bodies are the row kernels' own, once, in csrc/xvector_tile.h; the table lookup with its range check is csrc/segments.h.  A kernel here
// holds what its row kernel does not have: the lookup, the block-uniform exits, the segment's base pointers and the pitch of the whole rows.
#include "../xvector_tile.h"
#include "../segments.h"
#include "../../../include/satools_hip_ragged.h"

namespace sat {

constexpr int RG_CPB = 8;    // channels per block of the gate kernel: one segment search per thread serves them all

// the segment that holds column t, or -1 for a gap column: the last i with seg_off[i] <= t (ascending offsets), then its length
__device__ __forceinline__ int rg_find(const int* __restrict__ seg_off, const int* __restrict__ seg_len, int B, int T_tot, int t, int* off) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= t) lo = mid;
    else hi = mid;
  }
  int len;
  if (!ragged_segment(seg_off, seg_len, lo, T_tot, off, &len)) return -1;
  return (t >= *off && t - *off < len) ? lo : -1;
}

// melspec_logmel_frame with the utterance's own length: frame f of utterance b at column off_b + f of out [n_mel][T_tot]
__global__ void __launch_bounds__(64 * XV_FPB)
melspec_logmel_segments_kernel(const float* __restrict__ wav, const int* __restrict__ n_samples, const int* __restrict__ seg_off,
                               const int* __restrict__ seg_len, float* __restrict__ out, const float* __restrict__ window,
                               const float* __restrict__ fb, const int* __restrict__ fb_lo, const int* __restrict__ fb_hi, int n_max,
                               int T_tot, int n_mel, float coef) {
  const int b = blockIdx.y;
  const int n = n_samples[b];
  int col0, frames;
  // (the whole block leaves together: nothing below is reached by a part of it)
  if (!ragged_segment(seg_off, seg_len, b, T_tot, &col0, &frames) || n < 1 || n > n_max || (int)blockIdx.x * XV_FPB >= frames) return;
  const int f = blockIdx.x * XV_FPB + (threadIdx.x >> 6);
  melspec_logmel_frame(wav + (size_t)b * n_max, n, f, f < frames, out + col0 + f, T_tot, window, fb, fb_lo, fb_hi, n_mel, coef);
}

// instnorm_row_wave per (row, segment), one wave each; the wave also writes the zeros that follow its segment up to the next one
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
  float* yr = y + (size_t)r * T_tot;
  instnorm_row_wave(x + (size_t)r * T_tot + off, yr + off, T, lane, eps);
  for (int t = off + T + lane; t < nxt; t += 64) yr[t] = 0.f;
  if (i == 0)
    for (int t = lane; t < off; t += 64) yr[t] = 0.f;
}

// row_mean_wave per (channel, segment): x [C][T_tot] -> y [B][C]
__global__ void __launch_bounds__(256) row_mean_segments_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                const int* __restrict__ seg_off, const int* __restrict__ seg_len, int C, int B,
                                                                int T_tot) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= C * B) return;
  const int c = w / B, i = w - c * B;
  int off, T;
  if (!ragged_segment(seg_off, seg_len, i, T_tot, &off, &T)) return;
  row_mean_wave(x + (size_t)c * T_tot + off, T, lane, y + (size_t)i * C + c);
}

// se_gate_value on the packed axis: a thread owns one column, finds its segment once and walks RG_CPB channels; gap columns leave
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
  for (int ch = c0; ch < c1; ++ch) y[ch * y_cs + t] = se_gate_value(z, g[(size_t)seg * C + ch], s1, s2, s3, (size_t)ch * T_tot + t);
}

// attentive_stats_wave per (channel, segment): x, logits [C][T_tot] -> out [B][2C]
__global__ void __launch_bounds__(256) attentive_stats_segments_kernel(const float* __restrict__ x, const float* __restrict__ logits,
                                                                       float* __restrict__ out, const int* __restrict__ seg_off,
                                                                       const int* __restrict__ seg_len, int C, int B, int T_tot) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= C * B) return;
  const int c = w / B, b = w - c * B;
  int off, T;
  if (!ragged_segment(seg_off, seg_len, b, T_tot, &off, &T)) return;
  float m1, m2;
  attentive_stats_wave(x + (size_t)c * T_tot + off, logits + (size_t)c * T_tot + off, T, lane, &m1, &m2);
  if (lane == 0) attentive_stats_store(out + (size_t)b * 2 * C + c, C, m1, m2);
}

// the Res2 chain (csrc/xvector_tile.h) with a block per (segment, centre tile) of the table `tiles`: the utterance's bounds 0 <= t < T are the segment's, rows
// are T_tot apart and the segment starts at column `off` of each
template <int NT>
__global__ void __launch_bounds__(256) res2_chain_segments_kernel(const float* __restrict__ y, float* __restrict__ z, const float* __restrict__ w,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const int* __restrict__ seg_off, const int* __restrict__ seg_len,
                                                                  const int* __restrict__ tiles, int B, int T_tot, int nums, int dil) {
  const int seg = tiles[2 * blockIdx.x], t0 = tiles[2 * blockIdx.x + 1];
  if (seg < 0 || seg >= B) return;        // (block-uniform, like the two tests below)
  int off, T;
  if (!ragged_segment(seg_off, seg_len, seg, T_tot, &off, &T)) return;
  if (t0 < 0 || t0 >= T) return;
  const float* yb = y + off;
  float* zb = z + off;
#define R2_PITCH T_tot
#include "../xvector_chain_body.h"
#undef R2_PITCH
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
  SAT_REQUIRE(n_max > XV_NFFT / 2 && n_mel > 0, "melspec_logmel_segments: rows of %d samples are shorter than the reflect padding", n_max);
  SAT_REQUIRE((long long)n_mel * T_tot < (1ll << 31), "melspec_logmel_segments: output of 2^31 elements or more");
  if (n_samples_host)
    for (int i = 0; i < B; ++i)
      SAT_REQUIRE(n_samples_host[i] > XV_NFFT / 2 && n_samples_host[i] <= n_max,
                  "melspec_logmel_segments: utterance %d of %d samples is shorter than the reflect padding (513 samples) or longer than the row (%d)", i,
                  n_samples_host[i], n_max);
  dim3 grid(ceil_div(1 + n_max / XV_HOP, XV_FPB), B);
  hipLaunchKernelGGL(melspec_logmel_segments_kernel, grid, dim3(64 * XV_FPB), 0, (hipStream_t)stream, wav, n_samples, seg_off, seg_len, out,
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
  SAT_REQUIRE(dilation >= 1 && dilation <= R2_MARG && dilation * nums <= R2_HALO, "res2_chain_segments: dilation x pieces exceeds the staged halo");
  SAT_REQUIRE(centre == 0 || centre == 64 || centre == 128, "res2_chain_segments: centre is 0 (automatic), 64 or 128, not %d", centre);
  SAT_REQUIRE(n_tiles64 >= 0 && n_tiles128 >= 0, "res2_chain_segments: negative tile count");
  // 128-column centres when that fills the CUs, else 64 (sat_res2_chain_f32's rule)
  const bool wide = centre == 128 || (centre == 0 && n_tiles128 >= 256);
  SAT_REQUIRE((wide ? n_tiles128 : n_tiles64) >= 1, "res2_chain_segments: no tile of %d-column centres in the table", wide ? 128 : 64);
  const int st = wide ? launch_res2_chain<3>(res2_chain_segments_kernel<3>, dim3(n_tiles128), (hipStream_t)stream, y, z, w, scale, shift, seg_off, seg_len,
                                             tiles + 2 * (size_t)n_tiles64, B, T_tot, nums, dilation)
                      : launch_res2_chain<2>(res2_chain_segments_kernel<2>, dim3(n_tiles64), (hipStream_t)stream, y, z, w, scale, shift, seg_off, seg_len,
                                             tiles, B, T_tot, nums, dilation);
  if (st != SAT_OK) return st;
  SAT_LAUNCH_CHECK("res2_chain_segments_kernel");
  return SAT_OK;
}
