// Bootstrap replicates of the empirical EER (include/satools_hip_stats.h).  gfx950; plain HIP, no inline assembly; integers only.
//
// eer_bootstrap_kernel: a replicate is a bisection on the threshold index k over 1 .. K; every step is one counting sweep over the
// replicate's n_tar + n_non draws against the two scalar cuts cut_tar[mid] and cut_non[mid] — ceil(log2 K) sweeps and one more for the
// two counts of the result.  The draws are regenerated from Philox4x32-10 in every sweep: a replicate owns no memory at all, neither
// LDS nor scratch, at any size (a Philox call gives four draws for 40 integer multiplies; at 2^20 draws per side nothing else would
// hold them on the chip).  One loop covers both streams: Philox call q of the replicate belongs to the targets below
// ceil(n_tar / 4) and to the non-targets from there on, so the lanes stay busy when one side is tiny.
//   WAVE form   (n_tar + n_non <= EB_WAVE_MAX)  one wave per replicate, four replicates per block, shuffle reductions, no barrier:
//               at 100 + 100 trials the 50 Philox calls of a sweep fill one pass of a wave where a block would idle three quarters
//   BLOCK form  (above)                         one block of 256 threads per replicate; a sweep ends in the shuffle reduction of each
//               wave and ONE barrier (the four partial sums alternate between two LDS slots)
// The cut tables are compared with draws and never index anything: whatever they hold, the kernel touches cut_*[0 .. K] and its two
// outputs only.
#include "../common.h"
#include "../../../include/satools_hip_stats.h"
#include "philox.h"

namespace sat {

constexpr int EB_THREADS = 256;
constexpr int EB_WAVES = EB_THREADS / 64;
constexpr int EB_WAVE_MAX = 4096;               // n_tar + n_non up to which a wave owns a replicate (16 Philox calls per lane and sweep)

__device__ __forceinline__ int eb_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool BLOCK>
__global__ void __launch_bounds__(EB_THREADS) eer_bootstrap_kernel(const int32_t* __restrict__ cut_tar, const int32_t* __restrict__ cut_non, int K,
                                                                   int n_tar, int n_non, int first_replicate, int m, uint32_t key0, uint32_t key1,
                                                                   int32_t* __restrict__ miss_at, int32_t* __restrict__ fa_before) {
  __shared__ int red[2][EB_WAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = BLOCK ? (int)blockIdx.x : (int)blockIdx.x * EB_WAVES + wave;
  if (i >= m) return;                           // (WAVE form: the waves past the last replicate; no barrier follows there)
  const uint32_t r = (uint32_t)first_replicate + (uint32_t)i;
  const int Qt = (n_tar + 3) >> 2, Q = Qt + ((n_non + 3) >> 2);
  const int start = BLOCK ? tid : lane, step = BLOCK ? EB_THREADS : 64;
  int slot = 0;

  // -> #{d_t < ct}, #{d_n < cn}, the same values in every thread of the replicate
  auto count = [&](int ct, int cn, int& below_t, int& below_n) {
    int a = 0, b = 0;
    for (int q = start; q < Q; q += step) {
      const bool non = q >= Qt;
      const int qq = non ? q - Qt : q;
      const uint32_t n = (uint32_t)(non ? n_non : n_tar);
      const int c = non ? cn : ct;
      uint32_t w[4];
      philox4x32_10((uint32_t)qq, r, non ? 1u : 0u, 0u, key0, key1, w);
      int hit = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)               // (the last call of a stream holds n & 3 draws)
        hit += (int)(((uint32_t)(4 * qq + e) < n) & ((int)index_of_word(w[e], n) < c));
      a += non ? 0 : hit;
      b += non ? hit : 0;
    }
    a = eb_wave_sum(a);
    b = eb_wave_sum(b);
    if constexpr (BLOCK) {
      if (lane == 0) red[slot][wave][0] = a, red[slot][wave][1] = b;
      __syncthreads();
      a = b = 0;
#pragma unroll
      for (int v = 0; v < EB_WAVES; ++v) a += red[slot][v][0], b += red[slot][v][1];
      slot ^= 1;                                // the next sweep writes the other slot: its writers have passed this barrier, and whoever
    }                                           // writes THIS slot again has passed the next one, behind every read of it here
    below_t = a, below_n = b;
  };

  int lo = 1, hi = K;                           // the predicate holds at K (miss = n_tar, fa = 0 for tables that end in n_tar, n_non)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    int bt, bn;
    count(cut_tar[mid], cut_non[mid], bt, bn);
    if ((long long)bt * n_non >= (long long)(n_non - bn) * n_tar) hi = mid;
    else lo = mid + 1;
  }
  int bt, bn;
  count(cut_tar[lo], cut_non[lo - 1], bt, bn);
  if ((BLOCK ? tid : lane) == 0) {
    miss_at[i] = bt;
    fa_before[i] = n_non - bn;
  }
}

}  // namespace sat

using namespace sat;

extern "C" int sat_eer_bootstrap_i32(const int32_t* cut_tar, const int32_t* cut_non, int K, int n_tar, int n_non, int first_replicate, int m,
                                     uint64_t seed, int32_t* miss_at, int32_t* fa_before, void* stream) {
  SAT_REQUIRE(cut_tar && cut_non && miss_at && fa_before, "eer_bootstrap: null pointer");
  SAT_REQUIRE(n_tar >= 1 && n_non >= 1 && m >= 1, "eer_bootstrap: n_tar = %d, n_non = %d, m = %d must all be at least 1", n_tar, n_non, m);
  SAT_REQUIRE(n_tar <= SAT_EER_BOOTSTRAP_MAX_SIDE && n_non <= SAT_EER_BOOTSTRAP_MAX_SIDE,
              "eer_bootstrap: n_tar = %d, n_non = %d: a side holds at most %d trials", n_tar, n_non, SAT_EER_BOOTSTRAP_MAX_SIDE);
  SAT_REQUIRE(K >= 1 && K <= n_tar + n_non, "eer_bootstrap: K = %d outside 1 .. n_tar + n_non = %d", K, n_tar + n_non);
  SAT_REQUIRE(first_replicate >= 0 && (long long)first_replicate + m <= INT32_MAX,
              "eer_bootstrap: replicates %d .. %lld do not fit 0 .. 2^31 - 1", first_replicate, (long long)first_replicate + m - 1);
  const uint32_t key0 = (uint32_t)(seed & 0xffffffffu), key1 = (uint32_t)(seed >> 32);
  if (n_tar + n_non <= EB_WAVE_MAX)
    hipLaunchKernelGGL(eer_bootstrap_kernel<false>, dim3(ceil_div(m, EB_WAVES)), dim3(EB_THREADS), 0, (hipStream_t)stream, cut_tar, cut_non, K, n_tar,
                       n_non, first_replicate, m, key0, key1, miss_at, fa_before);
  else
    hipLaunchKernelGGL(eer_bootstrap_kernel<true>, dim3(m), dim3(EB_THREADS), 0, (hipStream_t)stream, cut_tar, cut_non, K, n_tar, n_non,
                       first_replicate, m, key0, key1, miss_at, fa_before);
  SAT_LAUNCH_CHECK("eer_bootstrap_kernel");
  return SAT_OK;
}
