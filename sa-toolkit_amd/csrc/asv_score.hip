// ASV privacy evaluation on the device: per-speaker enrolment vectors, cosine trial scores and the cohort statistics of
// adaptive s-norm (include/satools_hip.h, "ASV evaluation").  gfx950; plain HIP, no inline assembly.
//
// cohort_topk_stats_kernel: a block owns AS_ROWS = 4 rows of x and keeps their C cohort scores in LDS — as the order-preserving
// unsigned image of the floats — so the N x C score matrix never reaches memory.
//   scores   a cohort row is shared by 4 neighbouring lanes (coalesced 64-byte pieces); a lane owns every fourth float4 of the row and
//            spreads its products over 16 accumulators per x row (4 components x 4 float4 phases), so an accumulator takes
//            ceil(D / 64) FMAs; a 4-level tree and 2 shuffle levels finish the dot: ceil(D / 64) + 6 roundings, inside the
//            k(D) = ceil(D / 64) + 8 that tests/ref64.py allows a wave-wide sum.  The accumulators are indexed statically (no scratch).
//   select   one wave per row finds the k-th largest key by bisection on the 32 key bits: 32 counting sweeps of conflict-free
//            128-bit LDS reads.  (The score STORES of the phase before are not conflict-free: the four lanes that share a cohort row write
//            the four x rows' keys Cp words apart, Cp a multiple of 256, into one bank — one 4-way store per 64 cohort rows.)  A histogram radix select would need 4 sweeps, but top-k cohort scores of unit vectors share their
//            leading key bytes, so all 64 lanes would add to ONE histogram word and serialise; counting compares has no such case.
//   moments  sum of the values above the threshold + (k - count_above) copies of the threshold value (ties at the k-th place cannot
//            change the result), then, with the mean known, the sum of squared deviations the same way: two passes, because
//            m2 - m1^2 cancels for scores in a narrow band.
#include "common.h"

namespace sat {

constexpr int AS_ROWS = 4;
constexpr int AS_THREADS = 256;
constexpr int AS_MAX_C = 8192;
constexpr int AS_MAX_D = 512;

__device__ __forceinline__ unsigned as_key(float v) {
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float as_value(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

__device__ __forceinline__ float as_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int as_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Cp = C rounded up to 256: the padding holds key 0, below the key of every float, so no sweep needs a tail
__global__ void __launch_bounds__(AS_THREADS) cohort_topk_stats_kernel(const float* __restrict__ x, const float* __restrict__ cohort, int N,
                                                                       int C, int D, int k, int Cp, float* __restrict__ mean,
                                                                       float* __restrict__ sd) {
  extern __shared__ uint4 as_lds[];
  unsigned* keys = reinterpret_cast<unsigned*>(as_lds);                 // [AS_ROWS][Cp]
  float4* xs = reinterpret_cast<float4*>(keys + AS_ROWS * Cp);          // [AS_ROWS][D / 4]
  const int tid = threadIdx.x, D4 = D >> 2;
  const int row0 = blockIdx.x * AS_ROWS;
  for (int i = tid; i < AS_ROWS * D4; i += AS_THREADS) {
    const int r = i / D4, j = i - r * D4;
    const int row = min(row0 + r, N - 1);                               // a row past the end repeats the last one; its result is dropped
    xs[i] = reinterpret_cast<const float4*>(x + (size_t)row * D)[j];
  }
  __syncthreads();

  const int g = tid & 3, q = tid >> 2;
  for (int c0 = 0; c0 < Cp; c0 += AS_THREADS / 4) {
    const int c = c0 + q;
    const float4* crow = reinterpret_cast<const float4*>(cohort + (size_t)min(c, C - 1) * D);
    float acc[AS_ROWS][4][4];
#pragma unroll
    for (int r = 0; r < AS_ROWS; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][u][e] = 0.f;
    for (int j0 = g; j0 < D4; j0 += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + 4 * u;
        if (j < D4) {
          const float4 cv = crow[j];
#pragma unroll
          for (int r = 0; r < AS_ROWS; ++r) {
            const float4 xv = xs[r * D4 + j];
            acc[r][u][0] = fmaf(xv.x, cv.x, acc[r][u][0]);
            acc[r][u][1] = fmaf(xv.y, cv.y, acc[r][u][1]);
            acc[r][u][2] = fmaf(xv.z, cv.z, acc[r][u][2]);
            acc[r][u][3] = fmaf(xv.w, cv.w, acc[r][u][3]);
          }
        }
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int r = 0; r < AS_ROWS; ++r) {
      float s[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = (acc[r][u][0] + acc[r][u][1]) + (acc[r][u][2] + acc[r][u][3]);
      float t = (s[0] + s[1]) + (s[2] + s[3]);
      t += __shfl_xor(t, 1);
      t += __shfl_xor(t, 2);
      mine = g == r ? t : mine;                                         // lane g of the four stores the score of x row g
    }
    keys[g * Cp + c] = c < C ? as_key(mine) : 0u;
  }
  __syncthreads();

  // ---- one wave per row from here on (no further block barrier)
  const int w = tid >> 6, lane = tid & 63;
  const int row = row0 + w;
  if (row >= N) return;
  const uint4* kr = reinterpret_cast<const uint4*>(keys + w * Cp);
  const int n4 = Cp >> 2;                                               // a multiple of 64
  unsigned T = 0;
  for (int b = 31; b >= 0; --b) {
    const unsigned cand = T | (1u << b);
    int cnt = 0;
    for (int i = lane; i < n4; i += 64) {
      const uint4 v = kr[i];
      cnt += (int)(v.x >= cand) + (int)(v.y >= cand) + (int)(v.z >= cand) + (int)(v.w >= cand);
    }
    if (as_wave_sum(cnt) >= k) T = cand;                                // at least k keys reach cand: the k-th largest does too
  }
  // T = the k-th largest key (k <= C, and every real key is >= 1 > the padding)
  const float vT = as_value(T);
  int above = 0;
  float s1 = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const uint4 v = kr[i];
    const unsigned kk[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (kk[e] > T) {
        ++above;
        s1 += as_value(kk[e]);
      }
  }
  above = as_wave_sum(above);
  s1 = as_wave_sum(s1);
  const float rep = (float)(k - above);                                 // copies of the threshold value inside the top k
  const float m = (s1 + rep * vT) / (float)k;
  float s2 = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const uint4 v = kr[i];
    const unsigned kk[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (kk[e] > T) {
        const float d = as_value(kk[e]) - m;
        s2 += d * d;
      }
  }
  s2 = as_wave_sum(s2);
  const float dT = vT - m;
  s2 = s2 + rep * (dT * dT);
  if (lane == 0) {
    mean[row] = m;
    sd[row] = sqrtf(s2 / (float)(k - 1));                               // k = 1: 0 / 0 = NaN, as torch.std
  }
}

// one wave per trial; idx = [M enrolment indices][M test indices]
__global__ void __launch_bounds__(AS_THREADS) trial_scores_kernel(const float* __restrict__ enroll, const float* __restrict__ test,
                                                                  const int32_t* __restrict__ idx, int M, int D, const float* __restrict__ mu_e,
                                                                  const float* __restrict__ sd_e, const float* __restrict__ mu_t,
                                                                  const float* __restrict__ sd_t, float* __restrict__ score,
                                                                  float* __restrict__ score_asnorm) {
  const int m = blockIdx.x * (AS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;
  const int ie = idx[m], it = idx[M + m];
  const float* a = enroll + (size_t)ie * D;
  const float* b = test + (size_t)it * D;
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float av = a[d], bv = b[d];
    ab = fmaf(av, bv, ab);
    aa = fmaf(av, av, aa);
    bb = fmaf(bv, bv, bb);
  }
  ab = as_wave_sum(ab);
  aa = as_wave_sum(aa);
  bb = as_wave_sum(bb);
  if (lane == 0) {
    const float s = ab / (sqrtf(aa) * sqrtf(bb));
    score[m] = s;
    if (score_asnorm) score_asnorm[m] = 0.5f * ((s - mu_e[ie]) / sd_e[ie] + (s - mu_t[it]) / sd_t[it]);
  }
}

// one wave per speaker; seg = [U row numbers in speaker order][S + 1 offsets into them]
__global__ void __launch_bounds__(AS_THREADS) segment_mean_l2norm_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg, int U,
                                                                         int S, int D, float* __restrict__ out) {
  const int s = blockIdx.x * (AS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;
  const int32_t* order = seg;
  const int lo = seg[U + s], hi = seg[U + s + 1];
  float* o = out + (size_t)s * D;
  if (hi - lo == 1) {                                                   // already normalised by the extractor: the same bits
    const float* r = x + (size_t)order[lo] * D;
    for (int d = lane; d < D; d += 64) o[d] = r[d];
    return;
  }
  const float n = (float)(hi - lo);
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    float t = 0.f;
    for (int u = lo; u < hi; ++u) t += x[(size_t)order[u] * D + d];
    t = t / n;
    o[d] = t;
    ss = fmaf(t, t, ss);
  }
  const float nrm = sqrtf(as_wave_sum(ss));
  for (int d = lane; d < D; d += 64) o[d] = o[d] / nrm;                 // (each lane re-reads what it wrote itself)
}

}  // namespace sat

using namespace sat;

extern "C" int sat_cohort_topk_stats_f32(const float* x, const float* cohort, int N, int C, int D, int k, float* mean, float* std,
                                         void* stream) {
  SAT_REQUIRE(x && cohort && mean && std && N > 0, "cohort_topk_stats: bad arguments");
  SAT_REQUIRE(C >= 1 && C <= AS_MAX_C, "cohort_topk_stats: C = %d outside 1 .. %d (the scores of a row live in LDS)", C, AS_MAX_C);
  SAT_REQUIRE(D >= 4 && D <= AS_MAX_D && D % 4 == 0, "cohort_topk_stats: D = %d must be a multiple of 4 in 4 .. %d", D, AS_MAX_D);
  SAT_REQUIRE(k >= 1 && k <= C, "cohort_topk_stats: k = %d outside 1 .. C = %d", k, C);
  SAT_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)cohort % 16 == 0, "cohort_topk_stats: x and cohort must be 16-byte aligned");
  const int Cp = round_up(C, AS_THREADS);
  const size_t lds_bytes = (size_t)AS_ROWS * Cp * 4 + (size_t)AS_ROWS * D * 4;        // <= 128 KiB + 8 KiB of the 160 KiB
  static std::atomic<uint64_t> attr_done{0};      // per device
  int dev;
  if (attr_needed_on_current_device(attr_done, &dev)) {
    SAT_HIP(hipFuncSetAttribute((const void*)cohort_topk_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                AS_ROWS * AS_MAX_C * 4 + AS_ROWS * AS_MAX_D * 4));
    attr_done_on_device(attr_done, dev);
  }
  hipLaunchKernelGGL(cohort_topk_stats_kernel, dim3(ceil_div(N, AS_ROWS)), dim3(AS_THREADS), lds_bytes, (hipStream_t)stream, x, cohort, N, C,
                     D, k, Cp, mean, std);
  SAT_LAUNCH_CHECK("cohort_topk_stats_kernel");
  return SAT_OK;
}

extern "C" int sat_trial_scores_f32(const float* enroll, const float* test, const int32_t* idx_e, const int32_t* idx_t, int32_t* idx_dev,
                                    int E, int T, int M, int D, const float* mu_e, const float* sd_e, const float* mu_t, const float* sd_t,
                                    float* score, float* score_asnorm, void* stream) {
  SAT_REQUIRE(enroll && test && idx_e && idx_t && idx_dev && score && E > 0 && T > 0 && M > 0 && D > 0, "trial_scores: bad arguments");
  const int n_stats = (mu_e != nullptr) + (sd_e != nullptr) + (mu_t != nullptr) + (sd_t != nullptr);
  SAT_REQUIRE(n_stats == 0 || n_stats == 4, "trial_scores: pass all four statistics or none");
  SAT_REQUIRE((n_stats == 4) == (score_asnorm != nullptr), "trial_scores: score_asnorm goes with the four statistics");
  for (int m = 0; m < M; ++m) {                   // the index lists are host arrays: checked here, never in the kernel
    SAT_REQUIRE(idx_e[m] >= 0 && idx_e[m] < E, "trial_scores: trial %d names enrolment row %d of %d", m, (int)idx_e[m], E);
    SAT_REQUIRE(idx_t[m] >= 0 && idx_t[m] < T, "trial_scores: trial %d names test row %d of %d", m, (int)idx_t[m], T);
  }
  SAT_HIP(hipMemcpyAsync(idx_dev, idx_e, (size_t)M * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
  SAT_HIP(hipMemcpyAsync(idx_dev + M, idx_t, (size_t)M * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
  hipLaunchKernelGGL(trial_scores_kernel, dim3(ceil_div(M, AS_THREADS / 64)), dim3(AS_THREADS), 0, (hipStream_t)stream, enroll, test, idx_dev,
                     M, D, mu_e, sd_e, mu_t, sd_t, score, score_asnorm);
  SAT_LAUNCH_CHECK("trial_scores_kernel");
  return SAT_OK;
}

extern "C" int sat_segment_mean_l2norm_f32(const float* x, const int32_t* order, const int32_t* offsets, int32_t* seg_dev, int U, int S, int D,
                                           float* out, void* stream) {
  SAT_REQUIRE(x && order && offsets && seg_dev && out && U > 0 && S > 0 && D > 0, "segment_mean_l2norm: bad arguments");
  SAT_REQUIRE(offsets[0] == 0 && offsets[S] == U, "segment_mean_l2norm: offsets must run from 0 to U = %d", U);
  for (int s = 0; s < S; ++s)
    SAT_REQUIRE(offsets[s + 1] > offsets[s], "segment_mean_l2norm: speaker %d has no utterance (offsets must increase)", s);
  for (int u = 0; u < U; ++u) SAT_REQUIRE(order[u] >= 0 && order[u] < U, "segment_mean_l2norm: order[%d] = %d outside 0 .. %d", u, (int)order[u], U - 1);
  SAT_HIP(hipMemcpyAsync(seg_dev, order, (size_t)U * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
  SAT_HIP(hipMemcpyAsync(seg_dev + U, offsets, (size_t)(S + 1) * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
  hipLaunchKernelGGL(segment_mean_l2norm_kernel, dim3(ceil_div(S, AS_THREADS / 64)), dim3(AS_THREADS), 0, (hipStream_t)stream, x, seg_dev, U, S,
                     D, out);
  SAT_LAUNCH_CHECK("segment_mean_l2norm_kernel");
  return SAT_OK;
}
