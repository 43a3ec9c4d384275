// Bottleneck vector quantiser for codebooks that do not fit LDS whole (the 256-code tag: 256 x 256 f32 = 256 KB).
//
// Reference: VectorQuantizerEMA.forward (eval), satools/satools/chain/nn.py:402-476.
// Same contract as vq_kernel (bottleneck.hip): all f32, dist[e] = (sum_d x_d^2 + sum_d e_d^2) - 2 * (x . e) with the dot product
// as one d-ordered fma chain per (frame, code), the first minimum in code order wins, q = x + (e - x); the TIE form keeps best and
// runner-up and counts the near-ties.  For n_codes <= 64 every number that leaves this kernel has the bits vq_kernel gives it.
#include "common.h"

namespace sat {

constexpr int VQT_TILE = 64;          // codes per LDS tile: 64 KB at D = 256, two blocks per CU
constexpr int VQT_MAX_CODES = 1024;
constexpr int VQT_PF = 64;            // prefetch registers per thread: a tile of up to 256 * 64 values

// (distance, code) pairs are ordered by distance, then by code: "first minimum" for the best AND for the runner-up
__device__ __forceinline__ bool vqt_before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// put candidate (d, i) into the running two best of a frame
template <bool TIE>
__device__ __forceinline__ void vqt_insert(float d, int i, float& bestd, int& best, float& secondd, int& second) {
  if (best < 0 || vqt_before(d, i, bestd, best)) {
    if (TIE) second = best, secondd = bestd;
    bestd = d, best = i;
  } else if (TIE && (second < 0 || vqt_before(d, i, secondd, second))) {
    secondd = d, second = i;
  }
}

// LDS tile [D][64] = codebook rows of the tile, transposed; the sixteen 4-code groups of a row are permuted by the row number
// (group g of row d lies at g ^ (d & 15)): the transposing stores of a wave — one code, consecutive d — then spread over
// sixteen bank groups instead of hitting one, and the 16-byte broadcast reads of the FMA loop stay aligned.
__device__ __forceinline__ int vqt_at(int d, int e) { return d * VQT_TILE + ((((e >> 2) ^ (d & 15)) << 2) | (e & 3)); }

// Block = 64 frames x 4 waves; wave g owns codes 16 g .. 16 g + 15 of every tile and carries its best / runner-up over the tiles
// in registers (its codes come in ascending order: a strict '<' keeps the first minimum); the four waves' pairs meet once, at the
// end, ordered by (distance, code).  z is read again per tile (it stays in L2).  PF: the next tile's global loads are issued
// before the current tile's FMA loop and land in registers; they go to LDS once every wave has left the tile.
template <bool TIE, bool PF>
__global__ void __launch_bounds__(256) vq_tiled_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                       float* __restrict__ q, int* __restrict__ idx_out,
                                                       float* __restrict__ dist_out, int D, int T, int n_codes,
                                                       const float* __restrict__ pair_dist, float tie_scale, int* __restrict__ tie_count) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [D][64] tile^T, then [64] norms, then [4][64] (d, idx, d2, idx2)
  constexpr int G = 4, CPG = VQT_TILE / G;
  float* et = lds;
  float* ee = lds + (size_t)D * VQT_TILE;
  float* bd = ee + VQT_TILE;
  int* bi = (int*)(bd + G * 64);
  float* bd2 = (float*)(bi + G * 64);
  int* bi2 = (int*)(bd2 + G * 64);
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  const bool live = t < T;
  const float* zb = z + (size_t)b * D * T + (live ? t : 0);
  const int n_tiles = (n_codes + VQT_TILE - 1) / VQT_TILE;
  const int slots = D * VQT_TILE;      // values of a whole tile, padding codes (zeros) included

  float pf[PF ? VQT_PF : 1];
  auto fetch = [&](int tile) {         // PF: the tile's rows as they lie in memory, consecutive threads consecutive words
    const float* src = cb + (size_t)tile * VQT_TILE * D;
    const int total = min(VQT_TILE, n_codes - tile * VQT_TILE) * D;
#pragma unroll
    for (int j = 0; j < VQT_PF; ++j) {
      const int i = threadIdx.x + 256 * j;
      pf[PF ? j : 0] = i < total ? src[i] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < VQT_PF; ++j) {
      const int i = threadIdx.x + 256 * j;
      if (i < slots) {
        const int e = i / D, d = i - e * D;
        et[vqt_at(d, e)] = pf[PF ? j : 0];
      }
    }
  };
  if (PF) fetch(0);

  int best = -1, second = -1;
  float bestd = 0.f, secondd = 0.f, xx = 0.f;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int c0 = tile * VQT_TILE;
    if (tile) __syncthreads();         // every wave has left the previous tile
    if (PF) {
      store();
    } else {
      const float* src = cb + (size_t)c0 * D;
      const int total = min(VQT_TILE, n_codes - c0) * D;
      for (int base = threadIdx.x; base < slots; base += 256 * 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = base + 256 * k;
          v[k] = i < total ? src[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = base + 256 * k;
          if (i < slots) {
            const int e = i / D, d = i - e * D;
            et[vqt_at(d, e)] = v[k];
          }
        }
      }
    }
    __syncthreads();
    if (PF && tile + 1 < n_tiles) fetch(tile + 1);
    if (threadIdx.x < VQT_TILE) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) {
        const float v = et[vqt_at(d, threadIdx.x)];
        s += v * v;
      }
      ee[threadIdx.x] = s;
    }
    __syncthreads();
    float dot[CPG];
#pragma unroll
    for (int e = 0; e < CPG; ++e) dot[e] = 0.f;
    const int e0 = grp * CPG;
    // per accumulator one d-ordered chain; the frame's values eight rows ahead, the codes of the wave four at a time
    int d0 = 0;
    for (; d0 + 8 <= D; d0 += 8) {
      float xv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) xv[k] = zb[(size_t)(d0 + k) * T];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x = xv[k];
        if (tile == 0) xx += x * x;
        const int d = d0 + k;
#pragma unroll
        for (int e4 = 0; e4 < CPG / 4; ++e4) {
          const float4 c = *(const float4*)(et + d * VQT_TILE + (((grp * (CPG / 4) + e4) ^ (d & 15)) << 2));
          dot[4 * e4 + 0] = fmaf(x, c.x, dot[4 * e4 + 0]);
          dot[4 * e4 + 1] = fmaf(x, c.y, dot[4 * e4 + 1]);
          dot[4 * e4 + 2] = fmaf(x, c.z, dot[4 * e4 + 2]);
          dot[4 * e4 + 3] = fmaf(x, c.w, dot[4 * e4 + 3]);
        }
      }
    }
    for (int d = d0; d < D; ++d) {
      const float x = zb[(size_t)d * T];
      if (tile == 0) xx += x * x;
#pragma unroll
      for (int e4 = 0; e4 < CPG / 4; ++e4) {
        const float4 c = *(const float4*)(et + d * VQT_TILE + (((grp * (CPG / 4) + e4) ^ (d & 15)) << 2));
        dot[4 * e4 + 0] = fmaf(x, c.x, dot[4 * e4 + 0]);
        dot[4 * e4 + 1] = fmaf(x, c.y, dot[4 * e4 + 1]);
        dot[4 * e4 + 2] = fmaf(x, c.z, dot[4 * e4 + 2]);
        dot[4 * e4 + 3] = fmaf(x, c.w, dot[4 * e4 + 3]);
      }
    }
#pragma unroll
    for (int e = 0; e < CPG; ++e) {
      const int code = c0 + e0 + e;
      if (code < n_codes) {
        const float dd = (xx + ee[e0 + e]) - 2.f * dot[e];
        if (dist_out && live) dist_out[((size_t)b * T + t) * n_codes + code] = dd;
        if (best < 0 || dd < bestd) {
          if (TIE) second = best, secondd = bestd;
          bestd = dd;
          best = code;
        } else if (TIE && (second < 0 || dd < secondd)) {
          second = code, secondd = dd;
        }
      }
    }
  }
  bd[grp * 64 + lane] = bestd;
  bi[grp * 64 + lane] = best;
  if (TIE) bd2[grp * 64 + lane] = secondd, bi2[grp * 64 + lane] = second;
  __syncthreads();
  best = bi[lane];
  bestd = bd[lane];
  if (TIE) second = bi2[lane], secondd = bd2[lane];
#pragma unroll
  for (int g = 1; g < G; ++g) {
    const int cand = bi[g * 64 + lane];
    if (cand >= 0) vqt_insert<TIE>(bd[g * 64 + lane], cand, bestd, best, secondd, second);
    if (TIE) {
      const int c2 = bi2[g * 64 + lane];
      if (c2 >= 0) vqt_insert<TIE>(bd2[g * 64 + lane], c2, bestd, best, secondd, second);
    }
  }
  if (TIE && live && grp == 0 && second >= 0) {
    // the near-tie rule of vq_kernel<NC, true>
    const float gap = secondd - bestd;
    if (!(gap > tie_scale * sqrtf(xx) * pair_dist[(size_t)best * n_codes + second])) {
      const int B = (int)gridDim.y;
      atomicAdd(tie_count + b, 1);
      atomicMin(tie_count + B + b, t);
      atomicMax(tie_count + 2 * B + b, t);
    }
  }
  if (!live) return;
  if (grp == 0) idx_out[(size_t)b * T + t] = best;
  float* qb = q + (size_t)b * D * T + t;
  const float* er = cb + (size_t)best * D;       // the chosen row from memory: its tile may have left LDS
  for (int d = grp; d < D; d += G) {
    const float x = zb[(size_t)d * T];
    const float e = er[d];
    qb[(size_t)d * T] = x + (e - x);  // `inputs + (quantized - inputs)` (chain/nn.py:459)
  }
}

}  // namespace sat

using namespace sat;

static int vq_tiled_launch(const float* z, const float* codebook, float* q, int32_t* idx, float* dist, const float* pair_dist,
                           float tie_scale, int32_t* tie_count, int B, int D, int T, int n_codes, void* stream) {
  SAT_REQUIRE(z && codebook && q && idx, "vq_tiled: null pointer");
  SAT_REQUIRE(B > 0 && B < 65536 && D > 0 && T > 0 && n_codes > 0 && n_codes <= VQT_MAX_CODES, "vq_tiled: unsupported sizes (n_codes <= %d)",
              VQT_MAX_CODES);
  const size_t lds = ((size_t)D * VQT_TILE + VQT_TILE + 1024) * sizeof(float);
  SAT_REQUIRE(lds <= 160 * 1024, "vq_tiled: a tile of %d codes does not fit LDS at D = %d", VQT_TILE, D);
  dim3 grid(ceil_div(T, 64), B);
  const bool tie = tie_count != nullptr;
  const bool pf = D * VQT_TILE <= 256 * VQT_PF;
  auto kern = pf ? (tie ? vq_tiled_kernel<true, true> : vq_tiled_kernel<false, true>)
                 : (tie ? vq_tiled_kernel<true, false> : vq_tiled_kernel<false, false>);
  if (lds > 64 * 1024) SAT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, z, codebook, q, idx, dist, D, T, n_codes, pair_dist, tie_scale, tie_count);
  SAT_LAUNCH_CHECK("vq_tiled_kernel");
  return SAT_OK;
}

extern "C" int sat_vq_argmin_gather_tiled_f32(const float* z, const float* codebook, float* q, int32_t* idx, float* dist,
                                              int B, int D, int T, int n_codes, void* stream) {
  return vq_tiled_launch(z, codebook, q, idx, dist, nullptr, 0.f, nullptr, B, D, T, n_codes, stream);
}

extern "C" int sat_vq_argmin_gather_tiled_tie_f32(const float* z, const float* codebook, float* q, int32_t* idx, float* dist,
                                                  const float* pair_dist, float tie_scale, int32_t* tie_count,
                                                  int B, int D, int T, int n_codes, void* stream) {
  SAT_REQUIRE(pair_dist && tie_count && tie_scale >= 0.f, "vq_tiled(tie): pair_dist [n_codes][n_codes], tie_count [3][B] and a tie_scale >= 0");
  return vq_tiled_launch(z, codebook, q, idx, dist, pair_dist, tie_scale, tie_count, B, D, T, n_codes, stream);
}
