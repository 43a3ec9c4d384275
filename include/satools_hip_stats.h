/*
 * satools_hip_stats.h — the statistics entry points of libsatools_hip.so (gfx950 / MI355X): resampling statistics of the ASV
 * evaluation, compiled from sa-toolkit_amd/csrc/stats/ into the same library as include/satools_hip.h.
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every
 * launch asynchronous on it) are those of satools_hip.h; the ABI number is the one of that header.
 */
#ifndef SATOOLS_HIP_STATS_H
#define SATOOLS_HIP_STATS_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest n_tar and the largest n_non sat_eer_bootstrap_i32 takes (VoxCeleb1-E / -H: about 580 000 trials) */
#define SAT_EER_BOOTSTRAP_MAX_SIDE 1048576

/*
 * Bootstrap replicates of the empirical equal error rate of two score sets, in integers.
 *
 * The two sets enter as their cut tables over the K distinct values v_0 < ... < v_{K-1} of both sets together (and +inf as
 * index K):   cut_tar[k] = #{targets < v_k},  cut_non[k] = #{non-targets < v_k},  cut_tar[K] = n_tar,  cut_non[K] = n_non,
 * K + 1 non-decreasing int32 values each, on the device.
 *
 * Replicate r draws n_tar indices into the sorted targets (stream 0) and n_non into the sorted non-targets (stream 1), with
 * replacement: draw j of stream s is (u * n) >> 32 with u = word j & 3 of Philox4x32-10 (Salmon et al., SC'11) at the counter
 * (j >> 2, r, s, 0) under the key (seed & 0xffffffff, seed >> 32).  With d_t / d_n the draws,
 *     miss_r(k) = #{d_t < cut_tar[k]},     fa_r(k) = n_non - #{d_n < cut_non[k]},
 *     k* = the smallest k of 1 .. K with miss_r(k) * n_non >= fa_r(k) * n_tar     (64-bit integer products),
 * and replicate first_replicate + i writes  miss_at[i] = miss_r(k*),  fa_before[i] = fa_r(k* - 1);  its equal error rate is
 * min(miss_at / n_tar, fa_before / n_non), two float64 divisions the caller makes.  A replicate depends on (seed, r) alone: not on
 * the launch, the split of the replicates over calls, or the device.
 *
 * The cut tables are only ever compared with draws, never used as addresses.  Nothing is written to the device besides the m + m
 * results.  SAT_ERR_INVALID with a message, before anything is launched: a null pointer; n_tar < 1, n_non < 1 or m < 1; n_tar or
 * n_non above SAT_EER_BOOTSTRAP_MAX_SIDE; K < 1 or K > n_tar + n_non; first_replicate < 0 or first_replicate + m above INT32_MAX.
 */
int sat_eer_bootstrap_i32(const int32_t* cut_tar, const int32_t* cut_non, int K, int n_tar, int n_non,
                          int first_replicate, int m, uint64_t seed,
                          int32_t* miss_at, int32_t* fa_before, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_STATS_H */
