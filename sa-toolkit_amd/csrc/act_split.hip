// Streaming passes around the split-f16 conv family: f32 -> split planes, and the 8-bit sidecar of split planes.
#include "common.h"
#include "conv_common.h"

namespace sat {

// f32 [B][C][T] -> split planes of lrelu(x, slope): thread = (utterance, 8-channel group, position);
// 8 coalesced dword loads, two coalesced 16-byte stores (HBM-streaming)
__global__ void __launch_bounds__(256) act_split_kernel(const float* __restrict__ x, uint4* __restrict__ y,
                                                        int C, int T, float slope, int f8) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int cg = blockIdx.y;            // 8-channel group: chunk = cg >> 1, half = cg & 1
  const int b = blockIdx.z;
  if (t >= T) return;
  const float* xr = x + ((long long)b * C + cg * 8) * T + t;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = xr[(long long)j * T];
  uint4 hi4, lo4;
  split_hilo8(v, true, slope, hi4, lo4);
  const unsigned hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
  uint4* yb = y + (long long)b * (C / 4) * T;                     // C*T*4 bytes per utterance
  const long long u = ((long long)((cg >> 1) * 4 + (cg & 1))) * T + t;
  yb[u] = hi4;
  if (!f8) {
    yb[u + 2LL * T] = lo4;
    return;
  }
  // planes 2 / 3: e4m3(hi) and e4m3(lo * 2^10), one byte per channel; this thread owns 8 of the 16 bytes
  float hf[8], lf[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float xv = v[j];
    xv = lrelu_max(xv, slope);
    const auto hh = __builtin_bit_cast(decltype(__builtin_amdgcn_cvt_pkrtz(0.f, 0.f)), hi[j >> 1]);
    hf[j] = (float)hh[j & 1];
    lf[j] = (xv - hf[j]) * F8_XLO_SCALE;
  }
  uint2* y8 = (uint2*)(yb + ((long long)((cg >> 1) * 4 + 2)) * T + t) + (cg & 1);
  *y8 = make_uint2(pack_e4m3x4(hf[0], hf[1], hf[2], hf[3]), pack_e4m3x4(hf[4], hf[5], hf[6], hf[7]));
  y8[2LL * T] = make_uint2(pack_e4m3x4(lf[0], lf[1], lf[2], lf[3]), pack_e4m3x4(lf[4], lf[5], lf[6], lf[7]));
}

}  // namespace sat

using namespace sat;

// 8-bit sidecar of SAT_SPLIT_F16 planes: thread = (utterance, chunk, position); reads the chunk's four 16-byte units at t, writes
// e5m2(hi) and e5m2(lo * 2^10) of its 16 channels as two 16-byte units (HBM-streaming)
__global__ void __launch_bounds__(256) planes_f8_sidecar_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int C, int T) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int chunk = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const uint4* xb = x + ((long long)b * (C / 16) + chunk) * 4 * T + t;
  typedef _Float16 h8v __attribute__((ext_vector_type(8)));
  const h8v h0 = __builtin_bit_cast(h8v, xb[0]), h1 = __builtin_bit_cast(h8v, xb[T]);
  const h8v l0 = __builtin_bit_cast(h8v, xb[2LL * T]), l1 = __builtin_bit_cast(h8v, xb[3LL * T]);
  uint4 oh, ol;
  oh.x = pack_e5m2x4((float)h0[0], (float)h0[1], (float)h0[2], (float)h0[3]);
  oh.y = pack_e5m2x4((float)h0[4], (float)h0[5], (float)h0[6], (float)h0[7]);
  oh.z = pack_e5m2x4((float)h1[0], (float)h1[1], (float)h1[2], (float)h1[3]);
  oh.w = pack_e5m2x4((float)h1[4], (float)h1[5], (float)h1[6], (float)h1[7]);
  const float k = F8_XLO_SCALE;
  ol.x = pack_e5m2x4((float)l0[0] * k, (float)l0[1] * k, (float)l0[2] * k, (float)l0[3] * k);
  ol.y = pack_e5m2x4((float)l0[4] * k, (float)l0[5] * k, (float)l0[6] * k, (float)l0[7] * k);
  ol.z = pack_e5m2x4((float)l1[0] * k, (float)l1[1] * k, (float)l1[2] * k, (float)l1[3] * k);
  ol.w = pack_e5m2x4((float)l1[4] * k, (float)l1[5] * k, (float)l1[6] * k, (float)l1[7] * k);
  uint4* yb = y + ((long long)b * (C / 16) + chunk) * 2 * T + t;
  yb[0] = oh;
  yb[T] = ol;
}

extern "C" int sat_planes_f8_sidecar(const void* x_split, void* x_split8, int B, int C, int T, void* stream) {
  SAT_REQUIRE(x_split && x_split8, "planes_f8_sidecar: null pointer");
  SAT_REQUIRE(B > 0 && C > 0 && T > 0 && C % 16 == 0 && B < 65536 && C / 16 < 65536, "planes_f8_sidecar: unsupported shape B=%d C=%d T=%d", B, C, T);
  dim3 grid(ceil_div(T, 256), C / 16, B);
  hipLaunchKernelGGL(planes_f8_sidecar_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)x_split, (uint4*)x_split8, C, T);
  SAT_LAUNCH_CHECK("planes_f8_sidecar_kernel");
  return SAT_OK;
}

extern "C" int sat_act_split_f32(const float* x, void* x_split, int B, int C, int T, float slope, int format, void* stream) {
  SAT_REQUIRE(x && x_split, "act_split: null pointer");
  SAT_REQUIRE(format == SAT_SPLIT_F16 || format == SAT_SPLIT_F8, "act_split: unknown format");
  SAT_REQUIRE(B > 0 && C > 0 && T > 0 && C % 16 == 0 && B < 65536, "act_split: unsupported shape B=%d C=%d T=%d", B, C, T);
  SAT_REQUIRE(slope >= 0.f && slope <= 1.f, "act_split: slope must lie in [0, 1]");
  dim3 grid(ceil_div(T, 256), C / 8, B);
  hipLaunchKernelGGL(act_split_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, (uint4*)x_split, C, T, slope, format == SAT_SPLIT_F8);
  SAT_LAUNCH_CHECK("act_split_kernel");
  return SAT_OK;
}

