// The statements of the NCCF kernel, shared by yaapt_nccf_kernel (csrc/yaapt.hip: a frame overlaps its predecessor only) and
// yaapt_long_wide_nccf_kernel (csrc/yaapt_long/yaapt_long.hip: a frame overlaps up to seven predecessors).  The two differ only in how
// the frame that crs_corr sees is rebuilt from the frame means, which the including kernel supplies:
//   YAAPT_NCCF_PREVIOUS_MEANS()   declarations, once per block; in scope: fm (the signal's means), k, n, P
//   YAAPT_NCCF_HEAD(v, j)         the in-place subtractions of the earlier frames on sample j of frame k, applied to the float v
// The including kernel declares: filt, fmean, spec, scal, tp, tm, status, U, P.  One block of 256 threads per (frame, signal, utterance).
  __shared__ float d[1024];
  __shared__ float phi[1024];
  __shared__ float red[8];
  __shared__ int s_first;
  const int tid = threadIdx.x;
  const int k = blockIdx.x, sig = blockIdx.y, b = blockIdx.z;
  const int nf = P.nframes;                       // row stride
  if (k >= ulen(U, b, 2, nf)) return;
  const size_t oidx = ((size_t)b * 2 + sig) * nf + k;
  const float sp = spec[(size_t)b * nf + k];
  const float pstd = scal[b * 4 + 0];
  const float fthr = 5.0f * pstd;
  const float rlo = tmax(sp - 2.0f * pstd, P.f0_min);
  const float rhi = tmin(sp + 2.0f * pstd, P.f0_max);
  const float fa = floorf(P.fs / rhi), fb = floorf(P.fs / rlo);
  float pitch = 0.f, merit = 0.f;
  const int n = P.tda_len;
  if (!(fa != fa) && !(fb != fb)) {
    const int lag_min = (int)fa - P.nccf_center;
    const int lag_max = (int)fb + P.nccf_center;
    const int N = n - lag_max;
    // The reference walks the frames in order and ends at the first that fails: scal[1] keeps the smallest (frame, code), both
    // signals of a frame have the same lags and so the same code; yaapt_refine_dp_kernel turns it into the utterance's status
    if (N <= 0 || lag_min < 1) {
      if (tid == 0) atomicMin((int*)scal + b * 4 + 1, k * 4 + 2);  // the reference asserts N > 0 (yaapt.py:586)
    } else if (lag_max < lag_min) {
      // the spectral pitch lies outside [f0_min, f0_max] by more than two deviations: the reference asks stride_matrix for
      // lag_max - lag_min < 0 rows and fails (yaapt.py:594)
      if (tid == 0) atomicMin((int*)scal + b * 4 + 1, k * 4 + 3);
    } else {
      const float* x = filt + ((size_t)b * 2 + sig) * P.Lz + (size_t)k * P.frame_jump;
      const float* fm = fmean + ((size_t)b * 2 + sig) * nf;
      const float mk = fm[k];
      YAAPT_NCCF_PREVIOUS_MEANS();
      for (int j = tid; j < n; j += 256) {
        float v = x[j];
        YAAPT_NCCF_HEAD(v, j);
        d[j] = v - mk;
        phi[j] = 0.f;
      }
      __syncthreads();
      float part = 0.f;
      for (int j = tid; j < N; j += 256) part += d[j] * d[j];
      const float pw = block_sum256(part, red);
      const int nl = lag_max - lag_min;
      for (int l = tid; l < nl; l += 256) {
        const float* row = d + lag_min + l;
        float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
        int j = 0;
        for (; j + 4 <= N; j += 4) {
          n0 = fmaf(row[j], d[j], n0); q0 = fmaf(row[j], row[j], q0);
          n1 = fmaf(row[j + 1], d[j + 1], n1); q1 = fmaf(row[j + 1], row[j + 1], q1);
          n2 = fmaf(row[j + 2], d[j + 2], n2); q2 = fmaf(row[j + 2], row[j + 2], q2);
          n3 = fmaf(row[j + 3], d[j + 3], n3); q3 = fmaf(row[j + 3], row[j + 3], q3);
        }
        for (; j < N; ++j) { n0 = fmaf(row[j], d[j], n0); q0 = fmaf(row[j], row[j], q0); }
        const float nume = (n0 + n1) + (n2 + n3);
        const float den = (q0 + q1) + (q2 + q3);
        phi[lag_min + l] = nume / sqrtf(den * pw + 0.0f);
      }
      __syncthreads();
      // cmp_rate: first index with phi[n] > phi[n-1], > phi[n+1], > nccf_thresh1 inside [lag_min+c, lag_max-c]
      const int c = P.nccf_center;
      int first = 1 << 30;
      float amax = 0.f;  // phi is zero outside the lag window
      for (int i = tid; i < n; i += 256) {
        const float v = phi[i];
        amax = fmaxf(amax, v);   // NaN entries are skipped by fmaxf, like they never win a '>' test
        if (i >= lag_min + c && i <= lag_max - c && v > phi[i - 1] && v > phi[i + 1] && v > P.nccf_thresh1)
          first = min(first, i);
      }
      amax = block_max256(amax, red);
      first = wmin_i(first);
      if (tid == 0) s_first = 1 << 30;
      __syncthreads();
      if ((tid & 63) == 0) atomicMin(&s_first, first);
      __syncthreads();
      first = s_first;
      if (first < (1 << 30)) {
        bool take = amax > P.nccf_thresh2;
        if (!take) {
          const float v = phi[first];
          take = true;  // argmax(phi[first-c : first+c+1]) == c
          for (int i = first - c; i < first; ++i) take = take && (phi[i] < v);
          for (int i = first + 1; i <= first + c; ++i) take = take && (phi[i] <= v);
        }
        if (take) {
          pitch = (float)((double)P.fs / (double)(first + 1));
          merit = phi[first];
          if (merit > 1.0f) merit = merit / merit;
        }
      }
    }
  }
  if (tid == 0) {
    const float diff = fabsf(pitch - sp);
    const float m1 = diff < fthr ? 1.f : 0.f;
    const float match = (1.f - diff / fthr) * m1;
    tp[oidx] = pitch;
    tm[oidx] = (P.merit_boost1 * merit) * match;
  }
