// The statements of refine + dynamic + path1 -> final pitch, #included into the body of yaapt_refine_dp_kernel (csrc/yaapt.hip: the arrays
// in the block's LDS) and of yaapt_long_refine_dp_kernel (csrc/yaapt_long/: the arrays in the workspace), the form of
// csrc/xvector_chain_body.h: one text, so the two kernels do the same arithmetic in the same order.
// The including kernel defines, before the #include:
//   tp, tm, spec, energy, vuv, f0, scal, status, refined, U, P      its parameters
//   YAAPT_ARENA                             float*: where the per-utterance arrays live (63 bytes per frame of the utterance)
//   YAAPT_REFINE_PATH1()                    the transition functor of dynamic() and the path1 call over (rm, rp, en, nf, pred, path);
//                                           mean_pitch and w1 .. w4 are in scope
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  const int nfs = P.nframes;                      // row stride in global memory
  const int nf = ulen(U, b, 2, nfs);              // frames of this utterance (also the row pitch of the arena's arrays)
  if (lane == 0) {                                // the first frame the NCCF kernel could not do, if any: 2 or 3
    const int key = ((const int*)scal)[b * 4 + 1];
    if (key != 0x7fffffff) atomicMax(&status[b], key & 3);
  }
  float* rp = YAAPT_ARENA;
  float* rm = rp + NC * (size_t)nf;
  float* ta = rm + NC * (size_t)nf;
  float* en = ta + nf;
  unsigned char* pred = (unsigned char*)(en + nf);
  unsigned char* path = pred + NC * (size_t)nf;
  const float* tp1 = tp + ((size_t)b * 2 + 0) * nfs;
  const float* tp2 = tp + ((size_t)b * 2 + 1) * nfs;
  const float* tm1 = tm + ((size_t)b * 2 + 0) * nfs;
  const float* tm2 = tm + ((size_t)b * 2 + 1) * nfs;
  const float* sp = spec + (size_t)b * nfs;
  const int* vv = vuv + (size_t)b * nfs;
  const int nt = ulen(U, b, 3, P.tda_nframes);
  // concatenate the two tracks (rows 0 and 3 carry the single NCCF candidate), order by merit
  // descending with a stable sort (torch CPU argsort keeps equal keys in index order)
  for (int k = lane; k < nf; k += 64) {
    en[k] = energy[(size_t)b * nfs + k];
    float p[NC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, m[NC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k < nt) { p[0] = tp1[k]; m[0] = tm1[k]; p[3] = tp2[k]; m[3] = tm2[k]; }
    int ord[NC];
    for (int i = 0; i < NC; ++i) {
      int pos = i;
      // key = -m ascending, NaN last; insertion keeps earlier rows first on ties
      while (pos > 0) {
        const float a = m[ord[pos - 1]], c = m[i];
        const bool a_nan = a != a, c_nan = c != c;
        const bool c_before_a = c_nan ? false : (a_nan ? true : (c > a));
        if (!c_before_a) break;
        ord[pos] = ord[pos - 1];
        --pos;
      }
      ord[pos] = i;
    }
    // values: flip(sort ascending) ; NaN (sorted last ascending) comes first after the flip
    float ms[NC];
    {
      float t[NC];
      for (int i = 0; i < NC; ++i) t[i] = m[i];
      for (int i = 1; i < NC; ++i) {
        const float x = t[i];
        int j = i - 1;
        while (j >= 0 && ((t[j] != t[j]) ? !(x != x) : (x == x && t[j] > x))) { t[j + 1] = t[j]; --j; }
        t[j + 1] = x;
      }
      for (int i = 0; i < NC; ++i) ms[i] = t[NC - 1 - i];
    }
    for (int i = 0; i < NC; ++i) { rp[i * nf + k] = p[ord[i]]; rm[i * nf + k] = ms[i]; }
  }
  __syncthreads();
  // best_pitch = medfilt(time_pitch[0], median_value) * vuv
  medfilt_par(rp, ta, nf, P.median_value);
  __syncthreads();
  const float th2 = P.nlfer_thresh2;
  double acc = 0.0;
  int cnt = 0;
  for (int k = lane; k < nf; k += 64) {
    const float best = ta[k] * (vv[k] ? 1.f : 0.f);
    ta[k] = best;
    if (best > 0.f) { acc += (double)best; ++cnt; }
    const float e = en[k];
    const float tp0 = rp[k];
    const bool i1 = e <= th2;
    const bool i2 = (e > th2) && (tp0 > 0.f);
    const bool i3 = (e > th2) && (tp0 <= 0.f);
    bool mm[NC];
    for (int r = 0; r < NC; ++r) mm[r] = (r >= 1 && r <= NC - 2) && (rp[r * nf + k] == 0.f) && i2;
    if (i1) for (int r = 0; r < NC; ++r) { rp[r * nf + k] = 0.f; rm[r * nf + k] = P.merit_pivot; }
    if (i2) { rp[(NC - 1) * nf + k] = 0.f; rm[(NC - 1) * nf + k] = 1.0f - rm[k]; }
    for (int r = 0; r < NC; ++r) if (mm[r]) rm[r * nf + k] = 0.f;
    if (i3) {
      rp[k] = sp[k];
      rm[k] = tmin(1.f, e / 2.0f);
      for (int r = 1; r < NC; ++r) { rp[r * nf + k] = 0.f; rm[r * nf + k] = 1.0f - rm[k]; }
    }
    rp[(NC - 2) * nf + k] = best;
    if (best > 0.f) rm[(NC - 2) * nf + k] = rm[k];
    else rm[(NC - 2) * nf + k] = 1.0f - tmin(1.f, e / 2.0f);
    rp[(NC - 3) * nf + k] = sp[k];
    rm[(NC - 3) * nf + k] = e / 5.0f;
    // refine()'s result for the tests (f0.workspace_views: "refined" = pitch[6], merit[6]): nothing else shows most of its branches,
    // the final track picks one row per frame
    float* rd = refined + (size_t)b * 2 * NC * nfs;
    for (int r = 0; r < NC; ++r) { rd[(size_t)r * nfs + k] = rp[r * nf + k]; rd[(size_t)(NC + r) * nfs + k] = rm[r * nf + k]; }
    for (int r = 0; r < NC; ++r) rm[r * nf + k] = 1.f - rm[r * nf + k];   // local cost of dynamic()
  }
  // dynamic (yaapt.py:321-370)
  acc = wsum_d(acc);
  cnt = (int)wsum((float)cnt);
  const float mean_pitch = (float)(acc / (double)cnt);
  __syncthreads();
  const float w1 = P.dp_w1, w2 = P.dp_w2, w3 = P.dp_w3, w4 = P.dp_w4;
  YAAPT_REFINE_PATH1();
  float* out = f0 + (size_t)b * nfs;
  for (int k = lane; k < nf; k += 64) out[k] = rp[path[k] * nf + k];
  for (int k = nf + lane; k < nfs; k += 64) out[k] = 0.f;     // shorter utterance of a ragged batch: zero-padded track
