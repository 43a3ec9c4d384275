/*
 * satools_hip_ragged2d16.h — the segment form of the split-f16 2-D convolution of the ResNet x-vector extractor in libsatools_hip.so
 * (gfx950 / MI355X), compiled from sa-toolkit_amd/csrc/ragged2d16/ into the same library as include/satools_hip.h.  With it a RAGGED batch
 * (include/satools_hip_ragged2d.h: B utterances of unequal length on one packed time axis per time resolution) runs its 36 block
 * convolutions in the arithmetic of include/satools_hip_conv2d16.h (satools_amd.xvector_resnet Net.ragged_conv2d_precision = "f16x3").
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every launch
 * asynchronous on it, no allocation) are those of satools_hip.h; the ABI number is the one of that header.  The packed time axis, the
 * segment tables (int32 arrays ON THE DEVICE), max_len and the rule for broken table entries are those of satools_hip_ragged2d.h; the
 * arithmetic, the weight format, w_descale and SAT_CONV2D16_SPLIT_LIMIT are those of satools_hip_conv2d16.h.
 */
#ifndef SATOOLS_HIP_RAGGED2D16_H
#define SATOOLS_HIP_RAGGED2D16_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"
#include "satools_hip_conv2d16.h"
#include "satools_hip_ragged.h"
#include "satools_hip_ragged2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * sat_conv2d_f16x3_f32 with every segment an image of its own, in the layout of sat_conv2d_segments_f32: x [Cin][H][T_in],
 * y [Cout][Ho][T_out], Ho = (H - 1) / stride + 1; w_split and w_descale from the packing of satools_hip_conv2d16.h; ch_scale / ch_shift
 * (both or neither), relu, ksize (3 with padding 1, or 1) and stride (1 or 2) as there.  Segment i is an image of width W_i = in_len[i]
 * at column in_off[i] of x's rows; columns outside 0 .. W_i - 1 are staged as zero (the padding at the utterance's own ends).  Its
 * Wo_i = (W_i - 1) / stride + 1 output columns go to columns out_off[i] .. of y's rows; no other column of y is written.
 * in_off / in_len / out_off [B]; the two sides need not follow one layout rule or one order; a segment may begin on any column.
 * Cin, Cout in {32, 64, 128, 256}.  Cin = 1 (the stem) is refused: it stays on sat_conv2d_segments_f32.
 *
 * A table entry that breaks  0 <= off,  1 <= len,  off + len <= T  (on the input or on the output side), or a segment longer than max_len,
 * is skipped: its outputs stay unwritten and its flag untouched.  Nothing is read or written outside the buffers whatever the tables hold.
 *
 * ARITHMETIC.  Every product is w_lo x_hi + w_hi x_lo + w_hi x_hi on v_mfma_f32_32x32x16_f16, accumulated in f32; the activations are
 * split (v_cvt_pkrtz_f16_f32) while the halo tile of 16 input channels is staged in LDS.  A block owns (segment, 32 or 64 output channels,
 * 4 x 32 or 4 x 64 output pixels in the segment's own coordinates) with the tile choice of sat_conv2d_f16x3_f32, and sums over K in its
 * order (chunk of 16 input channels, tap; lo-hi, hi-lo, hi-hi): the result on segment i has the BITS of sat_conv2d_f16x3_f32 on
 * utterance i alone (B = 1, W = W_i).  No atomics and no split K take part in the sum.
 *
 * RANGE.  overflow_flags: int32 [B] on the device, or NULL (don't report).  A staged value OF SEGMENT i with
 * |x| >= SAT_CONV2D16_SPLIT_LIMIT, or a non-finite one, ORs 1 into overflow_flags[i] with an atomic from a vector lane; flag i is nonzero
 * after the call iff it was nonzero before or such a value was staged.  The kernel never clears a flag.  Outputs of segment i that depend
 * on such a value are unspecified; every other segment's outputs and flags are unaffected.  GAP COLUMNS hold anything, NaN, infinity and
 * 1e30 included: they are selected away on load, raise no flag and reach no result.
 *
 * SAT_ERR_INVALID with a message, before anything is launched: a null x, w_split, y or table; y == x; only one of ch_scale / ch_shift;
 * B outside 1 .. SAT_RAGGED_MAX_SEGMENTS; H < 1; T_in or T_out < 1; max_len outside 1 .. T_in; a ksize other than 3 or 1; a stride other
 * than 1 or 2; Cin or Cout outside the set; a w_descale that is not finite and positive; an image (Cin H T_in or Cout Ho T_out) of 2^31
 * elements or more; more row tiles x channel tiles than the grid takes.
 */
int sat_conv2d_f16x3_segments_f32(const float* x, const void* w_split, float w_descale, float* y, const float* ch_scale,
                                  const float* ch_shift, int relu, const int32_t* in_off, const int32_t* in_len, const int32_t* out_off,
                                  int B, int max_len, int Cin, int Cout, int H, int T_in, int T_out, int ksize, int stride,
                                  int32_t* overflow_flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_RAGGED2D16_H */
