/*
 * satools_hip_conv2d16.h — the split-f16 form of the 2-D convolutions of the ResNet x-vector extractor in libsatools_hip.so
 * (gfx950 / MI355X), compiled from sa-toolkit_amd/csrc/conv2d16/ into the same library as include/satools_hip.h.
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every
 * launch asynchronous on it) are those of satools_hip.h; the ABI number is the one of that header.
 */
#ifndef SATOOLS_HIP_CONV2D16_H
#define SATOOLS_HIP_CONV2D16_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a staged activation with |x| >= this, or a non-finite one, has no hi + lo f16 split (65 520 rounds to the f16 infinity) */
#define SAT_CONV2D16_SPLIT_LIMIT 65520.0f

/*
 * torch.nn.Conv2d(bias=False) + per-channel affine + optional ReLU with the semantics of sat_conv2d_f32 (satools_hip.h):
 *     y[b][co][ho][wo] = act(ch_scale[co] * w_descale * sum_{ci,kh,kw} w'[co][ci][kh][kw] x[b][ci][s ho - p + kh][s wo - p + kw]
 *                            + ch_shift[co]),    x = 0 outside the image,    w' = w * 2^e,  w_descale = 2^-e
 * ksize 3 (p = 1) or 1 (p = 0); stride s = 1 or 2 in both axes; Ho = (H - 1) / s + 1, Wo likewise.  x [B][Cin][H][W] f32 and
 * y [B][Cout][Ho][Wo] f32, W contiguous, y != x.  ch_scale / ch_shift: both or neither, applied AFTER the sum; relu != 0 clamps last.
 * Cin, Cout in {32, 64, 128, 256}.  Cin = 1 (the stem) is refused: it stays on sat_conv2d_f32.
 *
 * ARITHMETIC.  Every f32 operand is carried as hi + lo, two f16 values (22 significand bits together), and every product is
 *     w_lo x_hi + w_hi x_lo + w_hi x_hi        on v_mfma_f32_32x32x16_f16, accumulated in f32
 * (the dropped w_lo x_lo and the rounding of the lo halves: about 2^-21 of the product).  Activations are split inside the kernel while
 * the halo tile of 16 input channels is staged in LDS: hi = f16(x) and lo = f16(x - hi), both rounded toward zero (v_cvt_pkrtz_f16_f32,
 * f16 subnormals kept: below |x| = 2^-3 the split carries x to an absolute 2^-24 only).  There is no plane tensor in memory.
 * The accumulator is multiplied by w_descale (a power of two: exact) before the affine.  The sum over K = (16-channel chunk, tap,
 * channel) runs in one fixed order inside one block per output; no atomics and no split K take part in it: the same input gives the same
 * bits, and an image gives the same bits alone or inside a batch.
 *
 * WEIGHTS arrive split, w_split = f16 [Cin / 16][ksize * ksize taps, kh major][2: hi | lo][2: channel half][Cout][8]:
 * element (chunk c, tap t, part, half h, co, j) is the part of w'[co][16 c + 8 h + j][t / ksize][t % ksize], hi = f16(w'),
 * lo = f16(w' - hi) (round to nearest), with the per-layer scale 2^e that moves the largest |w'| into [2^9, 2^10)
 * (packing.f16x3_scale_exponent; e = 0 for an all-zero weight).  w_descale must be finite and positive.
 *
 * RANGE.  A staged value with |x| >= SAT_CONV2D16_SPLIT_LIMIT, or a non-finite one, cannot be split: the kernel then ORs 1 into
 * *overflow_flag (an int32 on the device) with an atomic from a vector lane.  The flag is nonzero after the call iff it was nonzero
 * before or some staged value could not be split; the kernel never clears it.  overflow_flag = NULL: don't report.  Outputs that
 * depend on such a value are unspecified; nothing outside y is written either way.
 *
 * SAT_ERR_INVALID with a message, before anything is launched: a null x, w_split or y; y == x; only one of ch_scale / ch_shift;
 * B outside 1 .. 65535; H < 1 or W < 1; a ksize other than 3 or 1; a stride other than 1 or 2; Cin or Cout outside the set; a
 * w_descale that is not finite and positive; an image (Cin H W or Cout Ho Wo) of 2^31 elements or more; more row tiles x channel
 * tiles than the grid takes.
 */
int sat_conv2d_f16x3_f32(const float* x, const void* w_split, float w_descale, float* y, const float* ch_scale, const float* ch_shift,
                         int relu, int B, int Cin, int Cout, int H, int W, int ksize, int stride, int32_t* overflow_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_CONV2D16_H */
