/*
 * satools_hip_ragged2d.h — the segment forms of the ResNet x-vector extractor's kernels in libsatools_hip.so (gfx950 / MI355X),
 * compiled from sa-toolkit_amd/csrc/ragged2d/ into the same library as include/satools_hip.h.  With them a RAGGED batch — B utterances
 * of unequal length — goes through the half-ResNet34 extractor in one launch sequence (satools_amd.xvector_resnet Net.extract_batch).
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every launch
 * asynchronous on it, no allocation) are those of satools_hip.h and satools_hip_ragged.h; the ABI number is the one of satools_hip.h.
 *
 * ONE PACKED TIME AXIS PER RESOLUTION.  The net halves the time resolution three times (layer2, layer3, layer4; stride 2 each):
 *     T_i^{l+1} = (T_i^l - 1) / 2 + 1,    l = 0 .. 2,    T_i^0 = 1 + n_i / 160 frames.
 * At level l the B utterances live in ONE image [C][H][T_tot_l], time innermost: segment i occupies columns off_i .. off_i + T_i - 1 of
 * every row.  Each level has its own table (seg_off, seg_len, T_tot) by the rule of satools_hip_ragged.h (ops.ragged_layout applied to
 * the level's frame counts; ops.ragged_levels gives the four).  No alignment between the levels is needed: the convolution takes the
 * input's table and the output's offsets separately and works in each segment's own columns.  The tables are int32 arrays ON THE DEVICE.
 *
 * A table entry that breaks  0 <= off,  1 <= len,  off + len <= T  (on the input or on the output side) is skipped by every kernel (its
 * outputs stay unwritten); nothing is read or written outside the buffers whatever the tables hold.  Two entries whose OUTPUT columns
 * overlap leave those columns with either one's values.
 *
 * max_len (sat_conv2d_segments_f32, sat_se_scale_add_relu_segments_f32): the longest segment of the input table, known to the host that
 * built it; the grid is sized by it, nothing waits for the device.  A segment LONGER than max_len is skipped like a broken entry.
 *
 * GAP COLUMNS of every input hold anything, uninitialised memory included.  The kernels select on load and never multiply by a mask: no
 * output depends on a gap column or on another segment, NaN and infinity included.  Only segment columns of an output are written.
 *
 * ARITHMETIC.  Exact f32, wave64, no atomics, one fixed summation order.  Each kernel is the segment form of a kernel of
 * sa-toolkit_amd/csrc/conv2d.hip (the SE squeeze: of row_mean_rows_kernel, csrc/xvector.hip, on row_mean_wave of csrc/xvector_tile.h)
 * and keeps its order of operations, so that its result on segment i has the bits of that kernel's on utterance i alone.
 *
 * The split-f16 form of the block convolutions on the same tables (the segment form of satools_hip_conv2d16.h's kernel, with one
 * overflow flag per segment) is declared in satools_hip_ragged2d16.h.
 */
#ifndef SATOOLS_HIP_RAGGED2D_H
#define SATOOLS_HIP_RAGGED2D_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"
#include "satools_hip_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * sat_conv2d_f32 with every segment an image of its own: x [Cin][H][T_in], y [Cout][Ho][T_out], Ho = (H - 1) / stride + 1; w_packed,
 * ch_scale / ch_shift (both or neither), relu, ksize (3 with padding 1, or 1) and stride (1 or 2) as for sat_conv2d_f32.  Segment i is an
 * image of width W_i = in_len[i] at column in_off[i] of x's rows; columns outside 0 .. W_i - 1 read as zero (the padding at the
 * utterance's own ends).  Its Wo_i = (W_i - 1) / stride + 1 output columns go to columns out_off[i] .. of y's rows; no other column of y
 * is written.  in_off / in_len / out_off [B]; the two sides need not follow one layout rule or one order.
 * Cin, Cout in {32, 64, 128, 256} on v_mfma_f32_32x32x2_f32, or Cin = 1 with Cout = 32, 3x3, stride 1 (the stem, on the vector unit).
 * A block owns (segment, 32 or 64 output channels, 4 x 32 output pixels in the segment's own coordinates) and sums over K in the order
 * of conv2d_mfma_kernel (chunk of 8 input channels, tap, channel pair): the bits of sat_conv2d_f32 on utterance i alone.
 * SAT_ERR_INVALID as sat_conv2d_f32 refuses, and for a null table, B outside 1 .. SAT_RAGGED_MAX_SEGMENTS, T_in or T_out < 1, max_len
 * outside 1 .. T_in, an image of 2^31 elements or more.
 */
int sat_conv2d_segments_f32(const float* x, const float* w_packed, float* y, const float* ch_scale, const float* ch_shift, int relu,
                            const int32_t* in_off, const int32_t* in_len, const int32_t* out_off, int B, int max_len, int Cin, int Cout,
                            int H, int T_in, int T_out, int ksize, int stride, void* stream);

/*
 * The squeeze of the SE layer: x [C][H][T_tot] -> y [B][C], the mean over the H T_i elements of segment i, summed in the order
 * sat_row_mean_f32 sums the utterance's own contiguous [H][T_i] plane (element n = h T_i + t on lane n % 64 in turn n / 64, the same
 * butterfly, one divide).
 */
int sat_plane_mean_segments_f32(const float* x, float* y, const int32_t* seg_off, const int32_t* seg_len, int C, int H, int B, int T_tot,
                                void* stream);

/*
 * y = relu(z * sigmoid(gate_logits[i][c]) + r) on the columns of segment i (sat_se_scale_add_relu_f32's expression): z, r, y
 * [C][H][T_tot], gate_logits [B][C]; y's gap columns untouched.
 */
int sat_se_scale_add_relu_segments_f32(const float* z, const float* gate_logits, const float* r, float* y, const int32_t* seg_off,
                                       const int32_t* seg_len, int B, int max_len, int C, int H, int T_tot, void* stream);

/*
 * sat_row_mean_std_f32 per (row, segment): x [R][T_tot] -> out [B][2 R], the means then the UNBIASED deviations (second pass around the
 * mean) over the segment's columns.  A segment of fewer than 2 columns has no unbiased deviation: it is skipped (the caller refuses it).
 */
int sat_row_mean_std_segments_f32(const float* x, float* out, const int32_t* seg_off, const int32_t* seg_len, int R, int B, int T_tot,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_RAGGED2D_H */
