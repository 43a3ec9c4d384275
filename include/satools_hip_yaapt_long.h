/*
 * satools_hip_yaapt_long.h — YAAPT F0 tracking of utterances beyond the 2048 frames of sat_yaapt_f32, in libsatools_hip.so (gfx950 / MI355X),
 * compiled from sa-toolkit_amd/csrc/yaapt_long/ into the same library as include/satools_hip.h.
 *
 * Status codes, `sat_last_error()` and the conventions (plain C ABI, device pointers, `stream` = a hipStream_t or NULL, every launch
 * asynchronous on it, no allocation) are those of satools_hip.h; the ABI number is the one of that header.  sat_yaapt_plan, the tables
 * (hann, kaiser, twiddle), the status words (0 ok; 1 .. 4 as sat_yaapt_f32 reports them) and the rows of utt_dims are those of
 * sat_yaapt_f32 / sat_yaapt_ragged_f32.
 *
 * sat_yaapt_f32 holds a whole utterance in one block's LDS in three of its kernels (spectral selection, frame means, refine + dynamic
 * programming) and so ends at 2048 frames.  The long form keeps those per-utterance arrays in the workspace; the two Viterbi recursions and
 * their back-traces, and the frame-mean recurrence, walk the frames in chunks of `chunk_frames` staged in LDS, carrying the path costs, the
 * previous frame mean and the back-trace state from chunk to chunk.  Every other launch is the kernel sat_yaapt_f32 launches.  The
 * arithmetic and its order are those of sat_yaapt_f32: on a plan of 4 .. 2048 frames the track, the status words and every view of the
 * workspace's head have the bits of sat_yaapt_f32 (utt_dims == NULL) or sat_yaapt_ragged_f32, whatever chunk_frames is.
 *
 * OVERLAP.  sat_yaapt_f32 serves frames of the time-domain stage that overlap their predecessor by at most 128 samples
 * (plan->tda_len - plan->frame_jump <= 128).  The long form also accepts a larger overlap, at any frame count, as long as a frame overlaps at
 * most 7 earlier frames:  plan->frame_jump < plan->tda_len <= 8 * plan->frame_jump  (and tda_len <= 1024 as before).  The reference's default
 * options are such a plan: 560-sample frames at a hop of 160, three frames deep.  The reference subtracts each frame's mean in place on
 * overlapping views of one buffer, so a sample loses the mean of every earlier frame that covers it, oldest first; for these plans the frame
 * means and the NCCF run as a wide pair of kernels that does the same, sample by sample, every subtraction rounded.  A plan of a smaller
 * overlap runs exactly the launches it ran before (the previous frame's mean only, also where tda_len > 2 * frame_jump).  A deeper plan is
 * refused by name, with its depth, before anything is launched.
 *
 * FRAMES.  4 frames up to the limit of the prefilter kernel, whose row offsets are 31-bit:  64 * plan->Lz * 4 < 2^31  and
 * 32 * plan->n * 4 < 2^31,  about 26 200 frames (8.7 minutes at a 20 ms hop).  A longer plan is refused by name before anything is launched.
 *
 * chunk_frames: 0 (the default, SAT_YAAPT_LONG_DEFAULT_CHUNK), or a multiple of 64 in 64 .. SAT_YAAPT_LONG_MAX_CHUNK.
 *
 * WORKSPACE.  sat_yaapt_long_workspace_bytes(plan, B, chunk_frames) bytes, 0 for a null plan, B <= 0 or a chunk_frames outside its set.  Its
 * head has the layout of sat_yaapt_f32's workspace (filt, e_raw, energy, vuv, cand, spec_pitch, scal, fmean, tp, tm, refined, then the
 * magnitude windows and the staged twiddles); SAT_YAAPT_LONG_SCRATCH_FLOATS floats per (utterance, frame) follow: the candidate rows and
 * costs of the stage that runs, its median buffers, the compaction indices, the Viterbi's `pred` and `path` bytes.
 *
 * SAT_ERR_INVALID with a message, before anything is launched: a null pointer; every plan that sat_yaapt_f32 refuses for a reason other than
 * its frame count or its overlap of more than 128 samples; a frame that overlaps more than 7 earlier ones; fewer than 4 frames; a plan beyond
 * the prefilter's limit; a chunk_frames outside its set.  SAT_ERR_WORKSPACE: a workspace
 * smaller than sat_yaapt_long_workspace_bytes.
 */
#ifndef SATOOLS_HIP_YAAPT_LONG_H
#define SATOOLS_HIP_YAAPT_LONG_H

#include <stddef.h>
#include <stdint.h>

#include "satools_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAT_YAAPT_LONG_DEFAULT_CHUNK 1024
#define SAT_YAAPT_LONG_MAX_CHUNK 2048
#define SAT_YAAPT_LONG_SCRATCH_FLOATS 17

size_t sat_yaapt_long_workspace_bytes(const sat_yaapt_plan* plan, int B, int chunk_frames);

/* utt_dims: NULL (every utterance has the plan's length), or int32 [B][4] on the device as in sat_yaapt_ragged_f32 */
int sat_yaapt_long_f32(const sat_yaapt_plan* plan, const float* wav, const int32_t* utt_dims, float* f0, int32_t* status,
                       const float* hann, const float* kaiser, const float* twiddle, void* workspace, size_t workspace_bytes, int B,
                       int chunk_frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATOOLS_HIP_YAAPT_LONG_H */
