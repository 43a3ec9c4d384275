/*
 * satools_hip_geninput.h — the generator-input entry point of libsatools_hip.so (gfx950 / MI355X): everything between the feature
 * extractors and the generator of an anonymizer in ONE launch, compiled from sa-toolkit_amd/csrc/geninput/ into the same library as
 * include/satools_hip.h.
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every
 * launch asynchronous on it) are those of satools_hip.h; the ABI number is the one of that header.
 */
#ifndef SATOOLS_HIP_GENINPUT_H
#define SATOOLS_HIP_GENINPUT_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the tile of the launch: SAT_GENINPUT_TILE columns of SAT_GENINPUT_TILE channels per block, staged in LDS at a pitch of
 * SAT_GENINPUT_TILE + 1 floats when bn's time axis is not its contiguous one */
#define SAT_GENINPUT_TILE 64

/*
 * x[b] = [ bn[b] (C_bn x T) ; transformed F0 of row b at the nearest-interpolation index (1 x T_f0 -> T) ; spk[b] broadcast over T ]
 *
 *   bn         element (b, c, t) at bn[b * bn_bstride + c * bn_cstride + t * bn_tstride]: the [B][T][C_bn] tensor an extractor writes is
 *              read through its permuted view (bstride T * C_bn, cstride 1, tstride C_bn) without a copy.  With bn_tstride == 1 the
 *              rows are copied straight through; otherwise a tile goes through LDS so that loads run along c and stores along t.
 *   f0         raw track, [S][R][T_f0] with S * R = B; row b = s * R + r belongs to slice s.  Never written.
 *   stats      [n_stats][2] = {mean, std}.
 *   slice_stat int32 [S] or NULL: the row of `stats` slice s is normalised with; NULL = row 0 for every slice (the pair
 *              sat_f0_stats_f32 wrote).  A slice whose entry lies outside 0 .. n_stats - 1 is SKIPPED: neither its F0 rows of x nor
 *              its rows of f0_norm are written (its bn and speaker rows are); the caller that owns the table checks it beforehand.
 *   quant_bins, noise ([B][T_f0] or NULL): as in sat_f0_apply_f32.
 *   spk        [B][n_spk] f32, or NULL with n_spk = 0.
 *   x          [B][C_bn + 1 + n_spk][T].
 *   f0_norm    [S][R][T_f0] or NULL: the NORMALISED values — voiced (v - mean) / std, zeros kept — before quantisation and noise.
 *
 * The F0 value is  v != 0 ? (v - mean) / std : 0,  then  v != 0 ? rint(v * bins) / bins : v  when quant_bins > 0,  then
 * v != 0 ? v + noise : v  when noise is given: the statements of sat_f0_apply_f32, applied to the element the index of
 * sat_assemble_input_f32 selects (src = min(floor(t * ((float)T_f0 / (float)T)), T_f0 - 1) in f32).  With S = 1, slice_stat = NULL and a
 * contiguous bn the launch writes the bits of sat_f0_apply_f32 followed by sat_assemble_input_f32.
 *
 * No atomics; nothing is written besides x and f0_norm.  SAT_ERR_INVALID with a message, before anything is launched: a null
 * descriptor or a null bn / f0 / stats / x; spk and n_spk disagreeing; a size below 1 (n_spk, quant_bins below 0); S * R != B; B or
 * C_bn + 1 + n_spk above 65535; bn strides that are not positive or that let two elements of bn share an address.
 */
typedef struct sat_geninput_desc {
  int32_t B, C_bn, T, T_f0;
  int32_t S, R, n_stats, n_spk;
  int32_t quant_bins, reserved;
  int64_t bn_bstride, bn_cstride, bn_tstride;
  const float* bn;
  const float* f0;
  const float* stats;
  const int32_t* slice_stat;
  const float* noise;
  const float* spk;
  float* x;
  float* f0_norm;
} sat_geninput_desc;

int sat_generator_input_f32(const sat_geninput_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_GENINPUT_H */
