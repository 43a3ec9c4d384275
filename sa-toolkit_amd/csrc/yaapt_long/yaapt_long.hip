// YAAPT beyond 2048 frames (include/satools_hip_yaapt_long.h): the long form of the three per-utterance kernels of csrc/yaapt.hip.
//
// yaapt_spec_post_kernel, yaapt_frame_means_kernel and yaapt_refine_dp_kernel hold a whole utterance in one block's LDS (53 and 63 bytes
// per frame, s_tail[2048]).  Here the per-utterance arrays live in the workspace (the "arena": SAT_YAAPT_LONG_SCRATCH_FLOATS floats per
// frame) and the statements are the SAME TEXT as the resident kernels' (yaapt_spec_select_body.h, yaapt_refine_body.h, the helpers of
// yaapt_dev.h): every loop over frames is lane-strided, no load depends on another one, and a one-wave block's __syncthreads() orders its
// global stores before the loads of the next phase exactly as it orders the LDS ones.  What IS sequential in time walks the frames in
// chunks of CH frames staged in LDS:
//   path1_long   the Viterbi recursion reads `local` and the transition's operands at t and t - 1: a chunk of all C local rows, all C
//                operand rows (and the energy row of dynamic()) is staged with the one frame before it (slot 0), the path costs `pc` stay in
//                registers from chunk to chunk, `pred` collects in LDS and goes out per chunk.  The back-trace walks the chunks in reverse:
//                the whole wave loads a chunk's `pred` rows into LDS, lane 0 walks them and carries the state p across the edge
//                (path[u - 1] = pred[p][u]: the step out of a chunk's first frame writes the previous chunk's last path byte).
//   frame means  all four waves reduce the recurrence-free tails of a chunk's frames into LDS, wave 0 walks the chunk and carries the
//                previous mean and the prefetched head of the next frame in registers.
// The arithmetic and its order are the resident kernels': float64 sums are lane-strided by 64 from frame 0 whatever CH is, the per-step
// expressions of path1_long are those of path1_wave, so a plan of up to 2048 frames gives the resident form's bits.
// Everything else (prefilter .. peaks, NCCF) is launched by csrc/yaapt.hip's own launchers: the same kernels.
// A plan whose frames overlap by more than 128 samples (the reference's default options: 560-sample frames at a hop of 160) is served
// here alone, at any length: the frame means and the NCCF then run as the wide pair further down.
#include "../common.h"
#include "../yaapt_dev.h"
#include "../../../include/satools_hip_yaapt_long.h"

namespace sat {

constexpr int YL_CHUNK_STEP = 64;                              // chunk_frames is a multiple of the wave
constexpr int YL_CHUNK_DEFAULT = SAT_YAAPT_LONG_DEFAULT_CHUNK;
constexpr int YL_CHUNK_MAX = SAT_YAAPT_LONG_MAX_CHUNK;         // 13 staged rows x 2049 floats + 6 x 2048 pred bytes = 116 KB of LDS
constexpr int YL_ARENA = SAT_YAAPT_LONG_SCRATCH_FLOATS;        // floats per (utterance, frame): 68 bytes >= 63 (refine) >= 53 (spec select)
constexpr int YL_HALO = 1;                                     // frames staged before a chunk: the recursion reads t - 1

// path1_wave (yaapt_dev.h) with local [C][ls], oper [C][ls] (and extra [ls] when NX) in global memory.  sl / so / se: LDS rows of
// SP = CH + YL_HALO floats; slot q of a chunk that starts at frame c0 holds frame c0 - YL_HALO + q.  trans(i, j, q) reads so / se at
// slots q and q - 1.  pred [C][ls] in global memory (frame 0 of every row is never written and never read), s_pred [C][CH] in LDS.
template <int C, int NX, class TransFn>
__device__ void path1_long(const float* local, const float* oper, const float* extra, int ls, int T, int CH, float* sl, float* so,
                           float* se, int SP, unsigned char* s_pred, TransFn trans, unsigned char* pred, unsigned char* path_out) {
  const int lane = threadIdx.x;
  const bool act = lane < C * C;
  const int i = act ? lane / C : 0;
  const int j = act ? lane % C : 0;
  float pc = lane < C ? local[lane * ls] : 0.f;
  for (int c0 = 0; c0 < T; c0 += CH) {
    const int n = min(CH, T - c0);                     // frames c0 .. c0 + n - 1
    __syncthreads();                                   // the previous chunk's pred rows have left s_pred
    for (int q = lane; q < n + YL_HALO; q += 64) {
      const int t = c0 - YL_HALO + q;
      if (t >= 0) {
#pragma unroll
        for (int r = 0; r < C; ++r) {
          sl[r * SP + q] = local[(size_t)r * ls + t];
          so[r * SP + q] = oper[(size_t)r * ls + t];
        }
        if (NX) se[q] = extra[t];
      }
    }
    __syncthreads();
    for (int t = c0 > 1 ? c0 : 1; t < c0 + n; ++t) {
      const int q = t - c0 + YL_HALO;
      const float pcj = __shfl(pc, j, 64);
      const float v = pcj + trans(i, j, q);
      int K = 0;
      float bv = __shfl(v, i * C, 64);
#pragma unroll
      for (int jj = 1; jj < C; ++jj) {
        const float vv = __shfl(v, i * C + jj, 64);
        if (path1_takes(vv, bv)) { bv = vv; K = jj; }   // last minimum wins
      }
      const float pcK = __shfl(pc, K, 64);
      const float cc = (pcK + trans(K, i, q)) + sl[i * SP + q];
      if (act && j == 0) s_pred[i * CH + (t - c0)] = (unsigned char)K;
      pc = __shfl(cc, (lane * C) & 63, 64);   // lane l < C <- CCOST[l] (held by lane l*C)
    }
    __syncthreads();
    for (int e = lane; e < C * n; e += 64) {
      const int r = e / n, tt = e - r * n;
      if (c0 + tt >= 1) pred[(size_t)r * ls + c0 + tt] = s_pred[r * CH + tt];
    }
  }
  __syncthreads();
  // p_small[T-1] = last argmin_i PCOST (0 when T == 1); every lane computes it from the shuffles
  int p = 0;
  {
    float jv = __shfl(pc, 0, 64);
#pragma unroll
    for (int ii = 1; ii < C; ++ii) {
      const float cv = __shfl(pc, ii, 64);
      if (path1_takes(cv, jv)) { jv = cv; p = ii; }
    }
    if (T <= 1) p = 0;
  }
  if (lane == 0) path_out[T - 1] = (unsigned char)p;
  for (int c0 = ((T - 1) / CH) * CH; c0 >= 0; c0 -= CH) {
    const int n = min(CH, T - c0);
    __syncthreads();
    for (int e = lane; e < C * n; e += 64) {
      const int r = e / n, tt = e - r * n;
      s_pred[r * CH + tt] = pred[(size_t)r * ls + c0 + tt];
    }
    __syncthreads();
    if (lane == 0) {
      for (int u = c0 + n - 1; u >= (c0 > 1 ? c0 : 1); --u) {     // P[u - 1] = PRED[P[u]][u]
        p = s_pred[p * CH + (u - c0)];
        path_out[u - 1] = (unsigned char)p;
      }
    }
  }
  __syncthreads();
}

// a row of a ragged batch's table that does not fit the plan is skipped (the Python wrapper refuses such a batch; the arena is sized
// by the plan's frame count)
__device__ __forceinline__ bool yl_row_fits(const int* __restrict__ U, int b, const Plan& P) {
  return !U || (U[b * 4 + 2] >= 1 && U[b * 4 + 2] <= P.nframes && U[b * 4 + 3] >= 0 && U[b * 4 + 3] <= P.nframes);
}

// LDS: floats sl[4][SP] so[4][SP]; bytes s_pred[4][CH]
__global__ void __launch_bounds__(64) yaapt_long_spec_post_kernel(const float* __restrict__ cand, float* __restrict__ spec_out,
                                                                 float* __restrict__ scal, int* __restrict__ status,
                                                                 const int* __restrict__ U, float* arena_all, int CH, const Plan P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (!yl_row_fits(U, blockIdx.x, P)) return;
  float* arena = arena_all + (size_t)blockIdx.x * YL_ARENA * P.nframes;
  const int SP = CH + YL_HALO;
  float* sl = lds;
  float* so = sl + 4 * SP;
  unsigned char* s_pred = (unsigned char*)(so + 4 * SP);
#define YAAPT_ARENA arena
#define YAAPT_SPEC_PATH1()                                                          \
  auto tr = [&](int i, int j, int q) {                                              \
    const float d = fabsf(so[j * SP + q] - so[i * SP + (q - 1)]) / f0min;           \
    return k1 * (0.05f * d + d * d);                                                \
  };                                                                                \
  path1_long<4, 0>(vcm, vcp, nullptr, nf, nv, CH, sl, so, nullptr, SP, s_pred, tr, pred, path)
#include "../yaapt_spec_select_body.h"
#undef YAAPT_SPEC_PATH1
#undef YAAPT_ARENA
}

// yaapt_frame_means_kernel in chunks of CH frames: s_tail holds one chunk's tails, wave 0 carries prev / h0 / h1 across the chunks
__global__ void __launch_bounds__(256) yaapt_long_frame_means_kernel(const float* __restrict__ filt, float* __restrict__ fmean,
                                                                    const int* __restrict__ U, int CH, const Plan P) {
  __shared__ float s_tail[YL_CHUNK_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, sig = blockIdx.y;
  if (!yl_row_fits(U, b, P)) return;
  const float* x = filt + ((size_t)b * 2 + sig) * P.Lz;
  float* m = fmean + ((size_t)b * 2 + sig) * P.nframes;
  const int ov = P.tda_len - P.frame_jump;
  const int T = ulen(U, b, 3, P.tda_nframes);
  auto head = [&](int k, int j) { return (k < T && j < ov) ? x[(size_t)k * P.frame_jump + j] : 0.f; };
  float h0 = head(0, lane), h1 = head(0, lane + 64);
  float prev = 0.f;
  for (int c0 = 0; c0 < T; c0 += CH) {
    const int n = min(CH, T - c0);
    __syncthreads();                                   // wave 0 has walked the previous chunk's tails
    for (int k = c0 + wave; k < c0 + n; k += 4) {
      float part = 0.f;
      for (int j = ov + lane; j < P.tda_len; j += 64) part += x[(size_t)k * P.frame_jump + j];
      part = wsum(part);
      if (lane == 0) s_tail[k - c0] = part;
    }
    __syncthreads();
    if (wave == 0) {
      for (int k = c0; k < c0 + n; ++k) {
        const float n0 = head(k + 1, lane), n1 = head(k + 1, lane + 64);   // prefetch
        float v0 = h0, v1 = h1;
        if (k > 0) {
          if (lane < ov) v0 = v0 - prev;
          if (lane + 64 < ov) v1 = v1 - prev;
        }
        const float mean = (wsum(v0 + v1) + s_tail[k - c0]) / (float)P.tda_len;
        if (lane == 0) m[k] = mean;
        prev = mean;
        h0 = n0;
        h1 = n1;
      }
    }
  }
}

// ---- the wide pair: a frame that overlaps more than its predecessor (tda_len - frame_jump > 128, the reference's defaults among them) ----
// time_track's frames are overlapping views of ONE buffer and crs_corr subtracts each frame's mean in place, so sample j of frame k
// has lost the means of every earlier frame that covers it, oldest first, each subtraction rounded (n = tda_len, J = frame_jump):
//     v = x[k J + j];   for i = D .. 1:  if (k - i >= 0 && j < n - i J) v = v - mean[k - i];      D = ceil(n / J) - 1
//     mean[k] = mean_j(v);   d[j] = v - mean[k]
// yaapt_long_frame_means_kernel is the case D = 1 with at most 128 overlapping samples.  Here the buffer itself is walked: the ring holds
// the samples of the frame at hand that earlier frames have touched (its first ov = n - J samples, the part on the critical path) as the
// reference's buffer holds them, and a step of the walk, mean[k] in hand, turns it into frame k + 1's head:
//     in flight   positions (k + 1) J .. k J + ov     ring <- ring - mean[k]
//     raw         positions max(..) .. k J + n        ring <- x - mean[k]        min(J, ov) <= 512 samples, loaded one frame ahead
// and sums the new head on the way, so that  mean[k + 1] = (head sum + tail sum) / n  needs one wave reduction and no barrier: position p is
// always handled by lane p & 63, a lane reads from the ring only what it stored there itself.  The recurrence-free tails (j >= ov) are
// reduced a chunk ahead by all four waves, as in yaapt_long_frame_means_kernel.
constexpr int YL_WIDE_DEPTH = 7;      // the earlier frames a frame may overlap: tda_len <= 8 frame_jump
constexpr int YL_RING = 1024;         // >= tda_len
constexpr int YL_RAW = 8;             // raw samples per lane that enter a head: min(frame_jump, ov) <= tda_len / 2 <= 512

__device__ __forceinline__ int yl_own(int lo, int lane) { return lo + ((lane - lo) & 63); }   // the first position >= lo that `lane` handles

__global__ void __launch_bounds__(256) yaapt_long_wide_frame_means_kernel(const float* __restrict__ filt, float* __restrict__ fmean,
                                                                         const int* __restrict__ U, int CH, const Plan P) {
  __shared__ float s_tail[YL_CHUNK_MAX];
  __shared__ float s_ring[YL_RING];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, sig = blockIdx.y;
  if (!yl_row_fits(U, b, P)) return;
  const float* x = filt + ((size_t)b * 2 + sig) * P.Lz;
  float* m = fmean + ((size_t)b * 2 + sig) * P.nframes;
  const int n = P.tda_len, J = P.frame_jump, ov = n - J;
  const int nr = min(J, ov);
  const int T = ulen(U, b, 3, P.tda_nframes);
  // the raw samples of the step out of frame k: positions k J + n - nr .. k J + n, inside frame k; needed when there is a frame k + 1
  auto raw = [&](int k, float* r) {
    const int hi = k * J + n, p0 = yl_own(hi - nr, lane);
#pragma unroll
    for (int i = 0; i < YL_RAW; ++i) r[i] = (k + 1 < T && p0 + 64 * i < hi) ? x[p0 + 64 * i] : 0.f;
  };
  float cur[YL_RAW], nxt[YL_RAW];
  float hsum = 0.f;                                    // the head sum of the frame to walk next
  if (wave == 0) {
    float part = 0.f;
    for (int p = lane; p < ov; p += 64) {              // frame 0's head is untouched
      const float v = x[p];
      s_ring[p] = v;
      part += v;
    }
    hsum = wsum(part);
    raw(0, cur);
  }
  for (int c0 = 0; c0 < T; c0 += CH) {
    const int nc = min(CH, T - c0);
    __syncthreads();                                   // wave 0 has walked the previous chunk's tails
    for (int k = c0 + wave; k < c0 + nc; k += 4) {
      float part = 0.f;
      for (int j = ov + lane; j < n; j += 64) part += x[(size_t)k * J + j];
      part = wsum(part);
      if (lane == 0) s_tail[k - c0] = part;
    }
    __syncthreads();
    if (wave == 0) {
      for (int k = c0; k < c0 + nc; ++k) {
        raw(k + 1, nxt);                               // prefetch
        const float mean = (hsum + s_tail[k - c0]) / (float)n;
        if (lane == 0) m[k] = mean;
        float part = 0.f;
        if (k + 1 < T) {
          for (int p = yl_own((k + 1) * J, lane); p < k * J + ov; p += 64) {
            const float v = s_ring[p & (YL_RING - 1)] - mean;
            s_ring[p & (YL_RING - 1)] = v;
            part += v;
          }
          const int hi = k * J + n, p0 = yl_own(hi - nr, lane);
#pragma unroll
          for (int i = 0; i < YL_RAW; ++i) {
            if (p0 + 64 * i < hi) {
              const float v = cur[i] - mean;
              s_ring[(p0 + 64 * i) & (YL_RING - 1)] = v;
              part += v;
            }
          }
        }
        hsum = wsum(part);
#pragma unroll
        for (int i = 0; i < YL_RAW; ++i) cur[i] = nxt[i];
      }
    }
  }
}

// yaapt_nccf_kernel (csrc/yaapt.hip) with the frame rebuilt from every earlier mean that covers a sample, oldest first: the same statements
__global__ void __launch_bounds__(256) yaapt_long_wide_nccf_kernel(const float* __restrict__ filt, const float* __restrict__ fmean,
                                                                  const float* __restrict__ spec, float* __restrict__ scal,
                                                                  float* __restrict__ tp, float* __restrict__ tm,
                                                                  int* __restrict__ status, const int* __restrict__ U, const Plan P) {
  // frame k - i covers the first n - i J samples of frame k (none from i = D + 1 on: the entry point holds D to YL_WIDE_DEPTH)
#define YAAPT_NCCF_PREVIOUS_MEANS()                                            \
  const int J = P.frame_jump;                                                  \
  float mp[YL_WIDE_DEPTH];                                                     \
  _Pragma("unroll") for (int i = 1; i <= YL_WIDE_DEPTH; ++i) mp[i - 1] = (k - i >= 0 && n - i * J > 0) ? fm[k - i] : 0.f
#define YAAPT_NCCF_HEAD(v, j)                                                  \
  _Pragma("unroll") for (int i = YL_WIDE_DEPTH; i >= 1; --i)                   \
    if (k - i >= 0 && j < n - i * J) v = v - mp[i - 1]
#include "../yaapt_nccf_body.h"
#undef YAAPT_NCCF_HEAD
#undef YAAPT_NCCF_PREVIOUS_MEANS
}

// LDS: floats sl[6][SP] so[6][SP] se[SP]; bytes s_pred[6][CH]
__global__ void __launch_bounds__(64) yaapt_long_refine_dp_kernel(const float* __restrict__ tp, const float* __restrict__ tm,
                                                                 const float* __restrict__ spec, const float* __restrict__ energy,
                                                                 const int* __restrict__ vuv, float* __restrict__ f0,
                                                                 const float* __restrict__ scal, int* __restrict__ status,
                                                                 float* __restrict__ refined, const int* __restrict__ U, float* arena_all,
                                                                 int CH, const Plan P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (!yl_row_fits(U, blockIdx.x, P)) return;
  float* arena = arena_all + (size_t)blockIdx.x * YL_ARENA * P.nframes;
  const int SP = CH + YL_HALO;
  float* sl = lds;
  float* so = sl + NC * SP;
  float* se = so + NC * SP;
  unsigned char* s_pred = (unsigned char*)(se + SP);
#define YAAPT_ARENA arena
#define YAAPT_REFINE_PATH1()                                                                                                      \
  auto tr = [&](int i, int j, int q) {                                                                                            \
    const float p1 = so[j * SP + q], p2 = so[i * SP + (q - 1)];                                                                   \
    float v = 1.f;                                                                                                                \
    if (p1 > 0.f && p2 > 0.f) v = w1 * (fabsf(p1 - p2) / mean_pitch);                                                             \
    else if ((p1 == 0.f && p2 > 0.f) || (p1 > 0.f && p2 == 0.f)) v = w2 * (1.f - tmin(1.f, fabsf(se[q - 1] - se[q])));            \
    else if (p1 == 0.f && p2 == 0.f) v = w3;                                                                                      \
    return v / w4;                                                                                                                \
  };                                                                                                                              \
  path1_long<NC, 1>(rm, rp, en, nf, nf, CH, sl, so, se, SP, s_pred, tr, pred, path)
#include "../yaapt_refine_body.h"
#undef YAAPT_REFINE_PATH1
#undef YAAPT_ARENA
}

static int yl_chunk(int chunk_frames) {   // -> the chunk to run with, 0 = refused
  if (chunk_frames == 0) return YL_CHUNK_DEFAULT;
  if (chunk_frames < YL_CHUNK_STEP || chunk_frames > YL_CHUNK_MAX || chunk_frames % YL_CHUNK_STEP) return 0;
  return chunk_frames;
}

}  // namespace sat

using namespace sat;

extern "C" size_t sat_yaapt_long_workspace_bytes(const sat_yaapt_plan* plan, int B, int chunk_frames) {
  if (!plan || B <= 0 || plan->nframes <= 0 || !yl_chunk(chunk_frames)) return 0;
  return align_up((yaapt_ws_floats(*plan, B) + (size_t)B * YL_ARENA * (size_t)plan->nframes) * sizeof(float), 256);
}

extern "C" int sat_yaapt_long_f32(const sat_yaapt_plan* plan, const float* wav, const int32_t* utt_dims, float* f0, int32_t* status,
                                  const float* hann, const float* kaiser, const float* twiddle, void* workspace, size_t workspace_bytes,
                                  int B, int chunk_frames, void* stream) {
  SAT_REQUIRE(plan && wav && f0 && status && hann && kaiser && twiddle && workspace, "yaapt_long: null pointer");
  const Plan& P = *plan;
  const int32_t* U = utt_dims;
  const int ok = yaapt_check_plan(P, B, false);
  if (ok != SAT_OK) return ok;
  // frames that overlap more than their predecessor run the wide pair of kernels: up to YL_WIDE_DEPTH earlier frames
  const int depth = P.frame_jump > 0 ? (P.tda_len + P.frame_jump - 1) / P.frame_jump - 1 : YL_WIDE_DEPTH + 1;
  SAT_REQUIRE(depth <= YL_WIDE_DEPTH,"yaapt_long: tda_frame_length / frame_space combination not supported: a frame of %d samples at a "
              "hop of %d overlaps %d earlier frames (depth %d), at most %d are supported (tda_len <= %d * frame_jump)", P.tda_len,
              P.frame_jump, depth, depth, YL_WIDE_DEPTH, YL_WIDE_DEPTH + 1);
  const bool wide = P.tda_len - P.frame_jump > 128;
  SAT_REQUIRE(P.nframes >= 4, "yaapt_long: %d frames not supported (4 frames at least)", P.nframes);
  // the prefilter kernel's buffer descriptors cover a block's 32 utterances (64 filtered rows) with 31-bit offsets; 32767 is what the
  // compaction's short frame indices take, far above it
  SAT_REQUIRE((size_t)32 * P.n * 4 < ((size_t)1 << 31) && (size_t)64 * P.Lz * 4 < ((size_t)1 << 31) && P.nframes <= 32767,
              "yaapt_long: %d frames not supported: utterance too long for the prefilter's 31-bit row offsets (64 * Lz * 4 < 2^31: "
              "at most %d padded samples, about 26 200 frames at a 20 ms hop)", P.nframes, (1 << 23) - 1);
  const int CH = yl_chunk(chunk_frames);
  SAT_REQUIRE(CH != 0, "yaapt_long: chunk_frames %d not supported (0 = the default %d, or a multiple of 64 in 64 .. %d)", chunk_frames,
              YL_CHUNK_DEFAULT, YL_CHUNK_MAX);
  SAT_REQUIRE_WORKSPACE(workspace_bytes >= sat_yaapt_long_workspace_bytes(plan, B, chunk_frames), "yaapt_long: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const YaaptBuffers W = yaapt_carve(P, B, workspace);
  float* arena = (float*)workspace + yaapt_ws_floats(P, B);
  const size_t SP = (size_t)CH + YL_HALO;
  const size_t post_lds = 2 * 4 * SP * sizeof(float) + 4 * (size_t)CH;
  const size_t dp_lds = (2 * NC + 1) * SP * sizeof(float) + NC * (size_t)CH;
  static std::atomic<uint64_t> attr_done{0};      // per device
  int dev;
  if (attr_needed_on_current_device(attr_done, &dev)) {
    SAT_HIP(hipFuncSetAttribute((const void*)yaapt_long_spec_post_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    SAT_HIP(hipFuncSetAttribute((const void*)yaapt_long_refine_dp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done_on_device(attr_done, dev);
  }
  const int front = yaapt_launch_front(P, wav, U, status, hann, kaiser, twiddle, W, B, s);
  if (front != SAT_OK) return front;
  hipLaunchKernelGGL(yaapt_long_spec_post_kernel, dim3(B), dim3(64), post_lds, s, W.cand, W.spec, W.scal, status, U, arena, CH, P);
  SAT_LAUNCH_CHECK("yaapt_long_spec_post_kernel");
  if (wide) {
    hipLaunchKernelGGL(yaapt_long_wide_frame_means_kernel, dim3(B, 2), dim3(256), 0, s, W.filt, W.fmean, U, CH, P);
    SAT_LAUNCH_CHECK("yaapt_long_wide_frame_means_kernel");
    hipLaunchKernelGGL(yaapt_long_wide_nccf_kernel, dim3(P.nframes, 2, B), dim3(256), 0, s, W.filt, W.fmean, W.spec, W.scal, W.tp, W.tm,
                       status, U, P);
    SAT_LAUNCH_CHECK("yaapt_long_wide_nccf_kernel");
  } else {
    hipLaunchKernelGGL(yaapt_long_frame_means_kernel, dim3(B, 2), dim3(256), 0, s, W.filt, W.fmean, U, CH, P);
    SAT_LAUNCH_CHECK("yaapt_long_frame_means_kernel");
    const int nccf = yaapt_launch_nccf(P, U, status, W, B, s);
    if (nccf != SAT_OK) return nccf;
  }
  hipLaunchKernelGGL(yaapt_long_refine_dp_kernel, dim3(B), dim3(64), dp_lds, s, W.tp, W.tm, W.spec, W.energy, W.vuv, f0, W.scal, status,
                     W.refined, U, arena, CH, P);
  SAT_LAUNCH_CHECK("yaapt_long_refine_dp_kernel");
  return SAT_OK;
}
