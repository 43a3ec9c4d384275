// The generator's input in one launch (include/satools_hip_geninput.h): the bottleneck features through their own strides, the F0 row
// normalised with its slice's statistics, transformed and resampled, the speaker rows broadcast — what sat_f0_apply_f32,
// sat_assemble_input_f32 and two .contiguous() copies do for the batch-coupled config (csrc/bottleneck.hip), for the configs that need
// per-slice statistics or no speaker rows.
//
// The normalisation, the quantiser, the re-zeroing after noise and the interpolation index are RESTATED from f0_apply_kernel and
// assemble_kernel, statement for statement (both sources stay as they are; tests/test_hip_geninput.py holds the two paths together bit
// for bit).  They are pointwise, so they commute with the gather: the F0 row of x is the transform of the raw element the index selects.
#include "../common.h"
#include "../../../include/satools_hip_geninput.h"

namespace sat {

constexpr int GI_TILE = SAT_GENINPUT_TILE;   // columns and channels of a block's tile
constexpr int GI_PITCH = GI_TILE + 1;        // 65 floats = 1 mod 64 banks: the transposed read (lane -> row) touches 64 different banks
constexpr int GI_ROWS = 256 / GI_TILE;       // rows of the tile the 4 waves take per step

struct GiArgs {
  const float* bn;
  const float* f0;
  const float* stats;
  const int* slice_stat;
  const float* noise;
  const float* spk;
  float* x;
  float* f0_norm;
  long long sb, sc, st;
  int C_bn, T, T_f0, R, n_stats, n_spk, quant_bins;
};

// the statistics row of batch row b, or -1 for a slice to skip (the convention of csrc/segments.h: a table entry is checked, never trusted)
__device__ __forceinline__ int gi_stat_row(const GiArgs& a, int b) {
  if (!a.slice_stat) return 0;
  const int k = a.slice_stat[b / a.R];
  return k >= 0 && k < a.n_stats ? k : -1;
}

// raw element i of flat row-major f0 -> (normalised, transformed): f0_apply_kernel's statements
__device__ __forceinline__ float gi_transform(const GiArgs& a, float v, float mean, float std, size_t i, float* norm) {
  if (v != 0.f) {
    v = v - mean;
    v = v / std;
  }
  *norm = v;
  if (a.quant_bins > 0) {
    if (v != 0.f) v = rintf(v * (float)a.quant_bins) / (float)a.quant_bins;  // torch.round: half to even
  }
  if (a.noise) {
    if (v != 0.f) v = v + a.noise[i];  // positions that are 0 after quantisation stay 0
  }
  return v;
}

// grid (ceil(T / 64), ceil(C_bn / 64) + 1, B): rows y < gridDim.y - 1 move a 64 x 64 tile of bn, the last row of blocks writes the F0
// row and the speaker rows of its 64 columns and its share of f0_norm
template <bool VIA_LDS>
__global__ void __launch_bounds__(256) generator_input_kernel(const GiArgs a) {
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * GI_TILE;
  const int lane = threadIdx.x & (GI_TILE - 1), w = threadIdx.x / GI_TILE;
  const int C = a.C_bn + 1 + a.n_spk;
  float* __restrict__ xb = a.x + (size_t)b * C * a.T;
  if (blockIdx.y + 1 < gridDim.y) {
    const int c0 = blockIdx.y * GI_TILE;
    const float* __restrict__ src = a.bn + (long long)b * a.sb;
    if constexpr (VIA_LDS) {
      __shared__ float tile[GI_TILE * GI_PITCH];
      const int c = c0 + lane;
      for (int r = w; r < GI_TILE; r += GI_ROWS) {      // loads along c
        const int t = t0 + r;
        if (c < a.C_bn && t < a.T) tile[r * GI_PITCH + lane] = src[(long long)c * a.sc + (long long)t * a.st];
      }
      __syncthreads();
      const int t = t0 + lane;
      for (int r = w; r < GI_TILE; r += GI_ROWS) {      // stores along t
        const int cc = c0 + r;
        if (cc < a.C_bn && t < a.T) xb[(size_t)cc * a.T + t] = tile[lane * GI_PITCH + r];
      }
    } else {
      const int t = t0 + lane;
      if (t >= a.T) return;
      for (int r = w; r < GI_TILE; r += GI_ROWS) {
        const int c = c0 + r;
        if (c < a.C_bn) xb[(size_t)c * a.T + t] = src[(long long)c * a.sc + t];
      }
    }
    return;
  }
  const int k = gi_stat_row(a, b);
  const float mean = k >= 0 ? a.stats[2 * k] : 0.f, std = k >= 0 ? a.stats[2 * k + 1] : 1.f;
  const size_t row = (size_t)b * a.T_f0;
  const int t = t0 + lane;
  if (t < a.T) {
    if (w == 0 && k >= 0) {
      // F.interpolate(mode='nearest'): src = min(floor(dst * (in/out)), in-1), scale in f32
      const float scale = (float)a.T_f0 / (float)a.T;
      int s = (int)floorf((float)t * scale);
      s = s < a.T_f0 - 1 ? s : a.T_f0 - 1;
      float norm;
      xb[(size_t)a.C_bn * a.T + t] = gi_transform(a, a.f0[row + s], mean, std, row + s, &norm);
    }
    for (int j = w; j < a.n_spk; j += GI_ROWS)
      xb[(size_t)(a.C_bn + 1 + j) * a.T + t] = a.spk[(size_t)b * a.n_spk + j];  // nearest interpolation of a length-1 axis = broadcast
  }
  if (a.f0_norm && k >= 0) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.T_f0; i += gridDim.x * 256) {
      float norm;
      gi_transform(a, a.f0[row + i], mean, std, row + i, &norm);
      a.f0_norm[row + i] = norm;
    }
  }
}

// true when no two elements (b, c, t) of the view share an address: every stride positive and, in the order of the strides, each one
// at least the extent the smaller ones span (axes of length 1 carry no stride)
static bool gi_strides_distinct(long long sb, int B, long long sc, int C, long long st, int T) {
  long long s[3] = {sb, sc, st};
  int n[3] = {B, C, T};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (s[j] < s[i]) {
        const long long ts = s[i];
        s[i] = s[j], s[j] = ts;
        const int tn = n[i];
        n[i] = n[j], n[j] = tn;
      }
  long long span = 1;      // one past the largest offset the axes so far reach
  for (int i = 0; i < 3; ++i) {
    if (n[i] == 1) continue;
    if (s[i] < span) return false;
    span = s[i] * (n[i] - 1) + span;
  }
  return true;
}

}  // namespace sat

using namespace sat;

extern "C" int sat_generator_input_f32(const sat_geninput_desc* d, void* stream) {
  SAT_REQUIRE(d, "generator_input: null descriptor");
  SAT_REQUIRE(d->bn && d->f0 && d->stats && d->x, "generator_input: null pointer (bn, f0, stats and x are required)");
  SAT_REQUIRE(d->n_spk >= 0 && (d->spk != nullptr) == (d->n_spk > 0), "generator_input: spk and n_spk = %d disagree", d->n_spk);
  SAT_REQUIRE(d->B > 0 && d->C_bn > 0 && d->T > 0 && d->T_f0 > 0 && d->S > 0 && d->R > 0 && d->n_stats > 0 && d->quant_bins >= 0,
              "generator_input: bad sizes");
  SAT_REQUIRE((long long)d->S * d->R == d->B, "generator_input: S * R = %d * %d is not B = %d", d->S, d->R, d->B);
  // B and the channel tiles are grid dimensions z / y (at most 65535 blocks each)
  SAT_REQUIRE(d->B < 65536, "generator_input: batch of %d utterances exceeds the 65535 one launch takes", d->B);
  SAT_REQUIRE((long long)d->C_bn + 1 + d->n_spk < 65536, "generator_input: %lld channels exceed the 65535 one launch takes",
              (long long)d->C_bn + 1 + d->n_spk);
  SAT_REQUIRE((d->B == 1 || d->bn_bstride > 0) && (d->C_bn == 1 || d->bn_cstride > 0) && (d->T == 1 || d->bn_tstride > 0) &&
                  gi_strides_distinct(d->bn_bstride, d->B, d->bn_cstride, d->C_bn, d->bn_tstride, d->T),
              "generator_input: bn strides (b %lld, c %lld, t %lld) let elements alias", (long long)d->bn_bstride,
              (long long)d->bn_cstride, (long long)d->bn_tstride);
  GiArgs a;
  a.bn = d->bn, a.f0 = d->f0, a.stats = d->stats, a.slice_stat = d->slice_stat, a.noise = d->noise, a.spk = d->spk;
  a.x = d->x, a.f0_norm = d->f0_norm;
  // an axis of length 1 is never stepped along: its stride is normalised so that the kernel's choice below does not depend on it
  a.sb = d->B == 1 ? 0 : d->bn_bstride, a.sc = d->C_bn == 1 ? 0 : d->bn_cstride, a.st = d->T == 1 ? 1 : d->bn_tstride;
  a.C_bn = d->C_bn, a.T = d->T, a.T_f0 = d->T_f0, a.R = d->R, a.n_stats = d->n_stats, a.n_spk = d->n_spk, a.quant_bins = d->quant_bins;
  dim3 grid(ceil_div(d->T, GI_TILE), ceil_div(d->C_bn, GI_TILE) + 1, d->B);
  if (a.st == 1) {
    hipLaunchKernelGGL(generator_input_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(generator_input_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  }
  SAT_LAUNCH_CHECK("generator_input_kernel");
  return SAT_OK;
}
