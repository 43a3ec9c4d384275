// The statements of spec_track after the per-frame candidates (selection, smoothing, Viterbi, interpolation), #included into the body of
// yaapt_spec_post_kernel (csrc/yaapt.hip: the arrays in the block's LDS) and of yaapt_long_spec_post_kernel (csrc/yaapt_long/: the arrays
// in the workspace), the form of csrc/xvector_chain_body.h: one text, so the two kernels do the same arithmetic in the same order.
// The including kernel defines, before the #include:
//   cand, spec_out, scal, status, U, P      its parameters
//   YAAPT_ARENA                             float*: where the per-utterance arrays live (53 bytes per frame of the utterance)
//   YAAPT_SPEC_PATH1()                      the transition functor of dynamic5 and the path1 call over (vcm, vcp, nf, nv, pred, path);
//                                           k1 and f0min are in scope
  const int b = blockIdx.x;
  const int nfs = P.nframes;                      // row stride of the per-frame arrays in global memory
  const int nf = ulen(U, b, 2, nfs);              // frames of this utterance (also the row pitch of the arena's arrays)
  const int lane = threadIdx.x;
  float* vcp = YAAPT_ARENA;
  float* vcm = vcp + 4 * (size_t)nf;
  float* ta = vcm + 4 * (size_t)nf;
  float* tb = ta + nf;
  float* spec = tb + nf;
  short* vidx = (short*)(spec + nf);
  short* index = vidx + nf;
  unsigned char* pred = (unsigned char*)(index + nf);
  unsigned char* path = pred + 4 * (size_t)nf;
  const float* cp = cand + (size_t)b * 8 * nfs;
  const float* cm = cp + 4 * (size_t)nfs;
  for (int f = lane; f < nf; f += 64) spec[f] = cp[f];
  // a shorter utterance of a ragged batch whose last spectral frame ends inside its own padded length: the reference fails on the
  // negative zero extension (yaapt.py:206-210).  yaapt_run refuses it for the plan's own length; only a kernel sees the others
  if (U && lane == 0 && P.nframe_size + (nf - 1) * P.frame_jump < U[b * 4 + 1]) atomicMax(&status[b], 3);
  // ... or whose tda frame count differs from its analysis frame count (yaapt_run refuses that too for the plan's own length: the
  // NCCF kernel walks the analysis frames and would read frame means that were never written): status 4, a refusal after the fact
  if (U && lane == 0 && U[b * 4 + 3] != nf) atomicMax(&status[b], 4);
  if (lane == 0) ((int*)scal)[b * 4 + 1] = 0x7fffffff;   // first frame on which the reference's time_track fails, and how (nccf kernel)
  const int nv = compact_frames(nf, [&](int f) { return cp[f] > 0.f; }, vidx);
  __syncthreads();
  for (int i = lane; i < nv; i += 64) {
    const int f = vidx[i];
    for (int c = 0; c < 4; ++c) { vcp[c * nf + i] = cp[(size_t)c * nfs + f]; vcm[c * nf + i] = cm[(size_t)c * nfs + f]; }
  }
  __syncthreads();
  float pitch_avg, pitch_std;
  if (nv == 0) {
    // the reference fails here (medfilt of an empty tensor, yaapt.py:257 -> :54-69); report it
    if (lane == 0) atomicMax(&status[b], 1);
    pitch_avg = 150.f;
    pitch_std = NAN;
  } else {
    const float avg_v = mean_par(vcp, nv);
    const float std_v = std_unbiased_par(vcp, nv);
    const float ref = 0.8f * avg_v;
    for (int i = lane; i < nv; i += 64) {
      int bi = 0;
      float bv = fabsf(vcp[i] - ref) * (3.f - vcm[i]);
      for (int c = 1; c < 4; ++c) {
        const float d = fabsf(vcp[c * nf + i] - ref) * (3.f - vcm[c * nf + i]);
        if (d < bv) { bv = d; bi = c; }   // first minimum
      }
      index[i] = (short)bi;
      ta[i] = vcp[bi * nf + i];
    }
    __syncthreads();
    const int mk = P.median_value - 2 > 1 ? P.median_value - 2 : 1;
    medfilt_par(ta, tb, nv, mk);
    __syncthreads();
    for (int i = lane; i < nv; i += 64) vcp[index[i] * nf + i] = tb[i];
    __syncthreads();
    const float k1 = (P.dp5_k1 * std_v) / avg_v;
    if (nv > 2) {
      // dynamic5 (yaapt.py:506-523): local = 1 - merit (in place), trans = k1*(0.05*d + d*d), d = |p_j(t) - p_i(t-1)|/f0_min
      for (int c = 0; c < 4; ++c)
        for (int i = lane; i < nv; i += 64) vcm[c * nf + i] = 1.f - vcm[c * nf + i];
      __syncthreads();
      const float f0min = P.f0_min;
      YAAPT_SPEC_PATH1();
      for (int t = lane; t < nv; t += 64) tb[t] = vcp[path[t] * nf + t];
      __syncthreads();
      medfilt_par(tb, ta, nv, mk);
    } else {
      for (int i = lane; i < nv; i += 64) ta[i] = 150.f;
    }
    __syncthreads();
    pitch_avg = mean_par(ta, nv);
    pitch_std = tmax(std_unbiased_par(ta, nv), pitch_avg * P.spec_pitch_min_std);
    for (int i = lane; i < nv; i += 64) spec[vidx[i]] = ta[i];
  }
  __syncthreads();
  if (lane == 0) {
    if (spec[0] < pitch_avg / 2.f) spec[0] = pitch_avg;
    if (spec[nf - 1] < pitch_avg / 2.f) spec[nf - 1] = pitch_avg;
  }
  __syncthreads();
  // F.interpolate(non-zero values, size=nf, mode='linear', align_corners=False)
  const int nz = compact_frames(nf, [&](int f) { return spec[f] != 0.f; }, vidx);
  __syncthreads();
  for (int i = lane; i < nz; i += 64) tb[i] = spec[vidx[i]];
  __syncthreads();
  if (nz == nf) {
    for (int f = lane; f < nf; f += 64) ta[f] = tb[f];
  } else {
    const float scale = (float)nz / (float)nf;
    for (int f = lane; f < nf; f += 64) {
      // torch's CPU kernel contracts both expressions into fused multiply-adds (checked bit for
      // bit against F.interpolate): src = fma(scale, f + 0.5, -0.5), out = fma(l0, x0, l1*x1)
      float src = fmaf(scale, (float)f + 0.5f, -0.5f);
      if (src < 0.f) src = 0.f;
      int i0 = (int)floorf(src);
      if (i0 > nz - 1) i0 = nz - 1;
      float l1 = src - (float)i0;
      l1 = fminf(fmaxf(l1, 0.f), 1.f);
      const int i1 = i0 + (i0 < nz - 1 ? 1 : 0);
      const float l0 = 1.f - l1;
      ta[f] = fmaf(l0, tb[i0], l1 * tb[i1]);
    }
  }
  __syncthreads();
  if (lane == 0 && nf >= 4) { ta[0] = ta[2]; ta[1] = ta[3]; }
  __syncthreads();
  float* out = spec_out + (size_t)b * nfs;
  for (int f = lane; f < nf; f += 64) out[f] = ta[f];
  if (lane == 0) scal[b * 4 + 0] = pitch_std;
