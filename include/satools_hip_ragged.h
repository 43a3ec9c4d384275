/*
 * satools_hip_ragged.h — the segment forms of the ECAPA-TDNN x-vector extractor's row kernels in libsatools_hip.so (gfx950 / MI355X),
 * compiled from sa-toolkit_amd/csrc/ragged/ into the same library as include/satools_hip.h.  With them a RAGGED batch — B utterances
 * of unequal length — goes through the extractor in one launch sequence (satools_amd.xvector Net.extract_batch).
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every
 * launch asynchronous on it) are those of satools_hip.h; the ABI number is the one of that header.
 *
 * THE PACKED TIME AXIS.  The B utterances, T_i = 1 + n_i / 160 frames each, live in ONE tensor [C][T_tot] (a batch of one): segment i
 * occupies columns off_i .. off_i + T_i - 1, in the order of the batch, and at least 2 gap columns follow every segment, the last one
 * included.  The rule of satools_amd.ops.ragged_layout:
 *     off_0 = 0,    off_{i+1} = round_up(off_i + T_i + 2, 4),    T_tot = off_B
 * (2 columns: the only convolution with more than one tap outside the Res2Net chain is the first layer's, 5 taps with 2 columns of
 * padding, and it reads the feature tensor, whose gap columns sat_instnorm_segments_f32 writes as zeros; multiples of 4: every segment
 * starts on a 16-byte boundary of its row).  Every 1x1 convolution and every pointwise kernel of satools_hip.h runs on [1][C][T_tot]
 * unchanged.  The kernels here need no more of the table than
 *     0 <= off_i,   1 <= T_i,   off_i + T_i <= T_tot,   off_i + T_i <= off_{i+1}:
 * seg_off[B] and seg_len[B], two int32 arrays ON THE DEVICE.  An entry that breaks the first three is skipped by every kernel (its
 * outputs stay unwritten); nothing is read or written outside the buffers whatever the table holds.
 *
 * GAP COLUMNS of every tensor but the feature tensor hold anything, uninitialised memory included.  The kernels here select on load
 * and never multiply by a mask: no output depends on a gap column or on another segment, NaN and infinity included.  They reduce over
 * segment columns only and write segment columns only (sat_instnorm_segments_f32 aside, which owns its gaps).
 *
 * ARITHMETIC.  Exact f32, wave64, no atomics.  Each kernel is the segment form of a row kernel of sa-toolkit_amd/csrc/xvector.hip and
 * runs that kernel's own body (csrc/xvector_tile.h, csrc/xvector_chain_body.h: one copy, shared by both), so it
 * keeps that kernel's order of operations per row — for the reductions the lane-strided loop t = lane, lane + 64, ... < T_i and the same
 * butterfly; for the chain the same (tap, input channel) order of its 96 MFMA steps — so that its result on segment i has the bits of the
 * row kernel's on utterance i alone.
 */
#ifndef SATOOLS_HIP_RAGGED_H
#define SATOOLS_HIP_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most utterances of one ragged batch */
#define SAT_RAGGED_MAX_SEGMENTS 1024

/*
 * sat_melspec_logmel_f32 per utterance at its own length: wav [B][n_max] (samples past n_i hold anything), n_samples[B] int32 on the
 * device, out [n_mel][T_tot].  Frame f of utterance i reflects at n_i, not at n_max, and is written at column off_i + f, f < T_i; no
 * other column is written.  window [400], fb [n_mel][513], fb_lo / fb_hi [n_mel] as for sat_melspec_logmel_f32.
 * n_samples_host: the same B lengths in host memory, or NULL.  When given, SAT_ERR_INVALID before anything is launched for the first
 * n_i <= 512 (the reflect padding: sat_melspec_logmel_f32's limit) or n_i > n_max, the message naming i.  On the device an n_i outside
 * 1 .. n_max skips the utterance.
 */
int sat_melspec_logmel_segments_f32(const float* wav, const int32_t* n_samples, const int32_t* n_samples_host, const int32_t* seg_off,
                                    const int32_t* seg_len, float* out, const float* window, const float* fb, const int32_t* fb_lo,
                                    const int32_t* fb_hi, int B, int n_max, int T_tot, int n_mel, float coef, void* stream);

/*
 * InstanceNorm1d(affine = False) per (row, segment) of x [R][T_tot] -> y [R][T_tot]: (x - mean) / sqrt(biased variance + eps) over the
 * T_i columns of the segment.  y's gap columns are OWNED output: every column of 0 .. T_tot - 1 outside the segments is written as 0
 * (the columns before off_0, between two segments and from the last segment's end to T_tot).  Needs the segments in ascending order.
 * y == x is allowed.
 */
int sat_instnorm_segments_f32(const float* x, float* y, const int32_t* seg_off, const int32_t* seg_len, int R, int B, int T_tot, float eps,
                              void* stream);

/* mean over the segment's columns: x [C][T_tot] -> y [B][C] */
int sat_row_mean_segments_f32(const float* x, float* y, const int32_t* seg_off, const int32_t* seg_len, int C, int B, int T_tot,
                              void* stream);

/*
 * y = z * sigmoid(gate_logits[i][c]) + s1 (+ s2 (+ s3)) on the columns of segment i, added left to right as sat_se_gate_add_f32 adds
 * them.  z, s1, s2, s3 [C][T_tot] (s1 .. s3 may be NULL from the right); gate_logits [B][C]; y: row c at y + c * y_cs (a channel slice
 * of a wider tensor), its gap columns untouched.
 */
int sat_se_gate_add_segments_f32(const float* z, const float* gate_logits, const float* s1, const float* s2, const float* s3, float* y,
                                 const int32_t* seg_off, const int32_t* seg_len, int C, int B, int T_tot, int64_t y_cs, void* stream);

/*
 * AttentiveStatsPool's tail per (channel, segment): w = softmax over the segment's columns of logits, mean = sum w x,
 * std = sqrt(max(sum w x^2 - mean^2, 1e-9)).  x, logits [C][T_tot] -> out [B][2 C]: means then stds.
 */
int sat_attentive_stats_segments_f32(const float* x, const float* logits, float* out, const int32_t* seg_off, const int32_t* seg_len,
                                     int C, int B, int T_tot, void* stream);

/*
 * sat_res2_chain_f32 with every segment an utterance of its own: y, z [C][T_tot], C = (nums + 1) * 64, w [nums][3][64][64],
 * scale / shift [nums][64].  Columns outside the segment read as zeros (the convolutions' padding), whatever the gaps hold; only
 * segment columns of z are written.  One block per (segment, centre tile of 64 or 128 columns), found in `tiles`: int32 pairs
 * (segment, first column of the tile inside the segment), the n_tiles64 tiles of 64-column centres — every segment's columns 0, 64,
 * 128, ... < T_i, in any order — followed by the n_tiles128 tiles of 128-column centres (satools_amd.ops.ragged_tiles).  A pair that
 * names no segment or no column of it is skipped.
 * centre: 64 or 128 forces the tile; 0 picks 128 when n_tiles128 >= 256 (sat_res2_chain_f32's rule), else 64.  Both give the same bits.
 * SAT_ERR_INVALID as sat_res2_chain_f32 refuses (null pointers, z == y, C != (nums + 1) * 64, dilation outside 1 .. 4,
 * dilation * nums > 32), and for a null table, B outside 1 .. SAT_RAGGED_MAX_SEGMENTS, T_tot < 1, a centre other than 0 / 64 / 128 or
 * no tile of the chosen centre.
 */
int sat_res2_chain_segments_f32(const float* y, float* z, const float* w, const float* scale, const float* shift, const int32_t* seg_off,
                                const int32_t* seg_len, const int32_t* tiles, int n_tiles64, int n_tiles128, int B, int C, int T_tot,
                                int nums, int dilation, int centre, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_RAGGED_H */
