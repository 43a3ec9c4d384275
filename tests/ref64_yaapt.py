"""Plain float64 restatements of the arithmetic stages of YAAPT (csrc/yaapt.hip, oracle/yaapt.py), for tests.

Each function takes the float32 band-limited signals (and, where a stage reads them, the float32 results of the stage
before it) AS GIVEN, computes the stage's quantity in float64 numpy, and returns with it
  * the sums of magnitudes its error bound needs, assembled into the bound with the rounding counts of `Roundings`,
  * the margins of the comparisons that turn the quantity into a decision (voiced / unvoiced, the peak set, the NCCF lag):
    a decision is `certain` when every comparison that settles it clears the bound, and only then may a float32
    implementation be required to agree with it.
Nothing here is tuned to an implementation: the counts in `Roundings` are read off the summation order of the code under
test (tests/test_hip_yaapt_stages.py for the kernels, tests/test_ref64_yaapt.py for the float32 oracle) and U = 2^-24.
Pinned on the CPU against the float32 oracle by tests/test_ref64_yaapt.py.

Error model (first order in U; the counts are rounded up to absorb the second order).  A sum of terms t_i that collects
k roundings has error <= k U sum |t_i|.

The FFT gets a RUNNING bound instead of a closed one: `fft_running` walks the 13 radix-2 decimation-in-time stages in
float64 and carries, next to every node's value, a bound E on the float32 node's distance from it.  A butterfly
a +- w b with a twiddle rounded once to float32 (|dw| <= U) and the four-multiply complex product (error <= sqrt(5) U |w b|,
Brent, Percival and Zimmermann 2007; a fused product is below that) gives
    E(w b) <= E_b + (|b| + E_b) `cmul` U,   cmul = 1 + sqrt(5) rounded up to 3.25
    E(a +- w b) <= E_a + E(w b) + U (|a +- w b| + E_a + E(w b))                    (the two component additions)
and a butterfly whose b is an exact zero copies a exactly (the zero padding).  The closed form of this recurrence,
|dX_k| <= 13 (cmul + 1) U sum_j |x_j|, is what one would write down by hand; it assumes every partial DFT as large as
the sum of its samples' magnitudes, which overstates the error at a weak harmonic's bin by the ratio of the frame's
strongest component to it, and the SHC multiplies four such bins.  The float32 oracle's FFT is torch's: it is judged by
the same recurrence, on the stated assumption that a mixed-radix pass merges radix-2 levels without adding roundings to
any of them; the CPU pin would show a ratio above 1 if that were wrong.

Underflow.  The model above holds for normal numbers only; below 2^-126 a float32 operation is off by up to the
subnormal spacing, or by the whole value where subnormals are flushed: TINY = 2^-126 per operation either way.  Silence
after a burst takes the band-limited signals there (the filters' tails decay through the subnormals to zero).  Every
bound therefore carries the absolute floor FLOOR = 2^-100 (more than 10^7 operations at TINY each, more than any stage
spends on one value) next to its relative part, and the NCCF, whose sums of squares underflow long before the samples
do, counts TINY per product into the relative error of its energies: where that reaches 1 the bound is infinite."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
FLOOR = 2.0 ** -100
FFT_N = 8192


class Roundings:
    """rounding counts of one implementation: `cmul` (twiddle times node, see the error model), `hyp` (|X| from re, im) are
    plain counts, the others map the number of terms of a sum to the roundings it collects"""

    def __init__(self, cmul, hyp, nl_sum, en_mean, sp_mean, shc_sum, shc_avg, fm_head, fm_tail, dot, pw):
        self.cmul, self.hyp, self.nl_sum, self.en_mean, self.sp_mean = cmul, hyp, nl_sum, en_mean, sp_mean
        self.shc_sum, self.shc_avg, self.fm_head, self.fm_tail, self.dot, self.pw = shc_sum, shc_avg, fm_head, fm_tail, dot, pw


def tables(plan):
    """the float32 window tables both implementations build (taken as given)"""
    hann = torch.hann_window(plan.frame_size + 2)[1:-1].numpy()
    kaiser = torch.kaiser_window(plan.nframe_size, periodic=True, beta=0.5).numpy()
    return hann, kaiser


def _f64(x):
    return np.asarray(x, dtype=np.float64)


_REV = None


def fft_running(x, ein, R, nbins, chunk=32):
    """x [F, n <= 8192] float64 real frames (zero-padded to 8192 here), ein [F, n] bounds on the float32 samples' distance
    from them -> (X [F, nbins] complex128, E [F, nbins]): bins 0 .. nbins-1 of the 8192-point DFT and the running bound of
    the error model on the float32 radix-2 FFT's bins.  X is numpy's float64 transform; the recurrence needs the nodes'
    MAGNITUDES only, takes them from a single-precision walk through the stages (each within 2^-17 of the float64 node
    relative to the bound it enters) and is inflated by 1.001 for it.  From the stage on whose blocks are longer than
    2 nbins only the first nbins nodes of each block are walked: the others feed no wanted bin."""
    global _REV
    if _REV is None:
        j = np.arange(FFT_N)
        _REV = sum(((j >> b) & 1) << (12 - b) for b in range(13))
    F, n = x.shape
    X = np.fft.rfft(x, FFT_N)[:, :nbins]
    E = np.zeros((F, nbins))
    cu, u = np.float32(R.cmul * U), np.float32(U)
    for f0 in range(0, F, chunk):
        xs = np.zeros((min(chunk, F - f0), FFT_N), np.float32)
        es = np.zeros_like(xs)
        xs[:, :n], es[:, :n] = x[f0:f0 + chunk], ein[f0:f0 + chunk]
        v, e = xs[:, _REV].astype(np.complex64), es[:, _REV]
        width = 1                                          # nodes kept per block
        for s in range(1, 14):
            h = 1 << (s - 1)
            v, e = v.reshape(v.shape[0], -1, 2, width), e.reshape(e.shape[0], -1, 2, width)
            a, b, ea, eb = v[:, :, 0], v[:, :, 1], e[:, :, 0], e[:, :, 1]
            t = np.exp(-2j * np.pi * np.arange(width) / (2 * h)).astype(np.complex64) * b
            absb = np.abs(b)
            et = eb + (absb + eb) * cu
            copy = (absb == 0) & (eb == 0)
            hi_ = a + t
            e_hi = np.where(copy, ea, ea + et + u * (np.abs(hi_) + ea + et))
            if 2 * h >= 2 * nbins and width >= nbins:      # the low half (bins h .. 2h-1 of the block) feeds no wanted bin
                v, e = hi_, e_hi
            elif h >= nbins:                               # this stage's blocks outgrow the wanted bins: keep the first nbins
                v, e = hi_[:, :, :nbins], e_hi[:, :, :nbins]
                width = min(width, nbins)
            else:
                lo_ = a - t
                e_lo = np.where(copy, ea, ea + et + u * (np.abs(lo_) + ea + et))
                v, e = np.concatenate((hi_, lo_), axis=2), np.concatenate((e_hi, e_lo), axis=2)
                width = 2 * h
            v, e = v.reshape(v.shape[0], -1), e.reshape(e.shape[0], -1)
        E[f0:f0 + chunk] = e[:, :nbins] * 1.001
    return X, E


# ---- NLFER energy ----------------------------------------------------------------------------------------------------
def nlfer_raw(filt, plan, R):
    """filt [>= L] float32 -> e_raw [nframes] = sum_k |X[nl_lo:nl_hi]| of the hann-windowed 8192-point spectrum, its bound,
    and A = sum |windowed sample| per frame"""
    hann, _ = tables(plan)
    idx = (np.arange(plan.nframes) * plan.frame_jump)[:, None] + np.arange(plan.frame_size)[None, :]
    fr = _f64(filt)[idx] * _f64(hann)                      # exact: 24 x 24 bits
    A = np.abs(fr).sum(1)
    X, E = fft_running(fr, U * np.abs(fr), R, plan.nl_hi)  # the window product: one rounding per sample
    e = np.abs(X[:, plan.nl_lo:plan.nl_hi]).sum(1)
    nb = plan.nl_hi - plan.nl_lo
    bound = E[:, plan.nl_lo:plan.nl_hi].sum(1) + (R.hyp + R.nl_sum(nb)) * U * e + FLOOR
    return e, bound, A


def energy_norm(e_raw, R):
    """e_raw [nframes] as given -> energy = e / mean(e) and its bound (the mean's roundings, two divisions)"""
    e = _f64(e_raw)
    energy = e / e.mean()
    return energy, (R.en_mean(e.size) + 2) * U * np.abs(energy) + FLOOR


def energy_decision(filt, plan, R):
    """the whole chain from the filtered signal: energy, its bound, and the margin |energy - nlfer_thresh1| of the
    voiced / unvoiced decision"""
    e, de, _ = nlfer_raw(filt, plan, R)
    energy, dn = energy_norm(e, R)
    bound = de / e.mean() + energy * (de.sum() / e.sum()) + dn
    return energy, bound, np.abs(energy - plan.p["nlfer_thresh1"])


# ---- SHC and its peaks -----------------------------------------------------------------------------------------------
def shc(filt2, frames, plan, R):
    """filt2 float32, zero-extended so that every frame has nframe_size samples; frames = indices of the frames above
    the NLFER threshold -> (shc [len(frames), max_shc], bound): kaiser window, mean removal, |rfft| shifted by half_wl,
    product over the harmonics, sum over the window"""
    _, kaiser = tables(plan)
    frames = np.asarray(frames, dtype=np.int64)
    n = plan.nframe_size
    idx = (frames * plan.frame_jump)[:, None] + np.arange(n)[None, :]
    xw = _f64(filt2)[idx] * _f64(kaiser)
    s = xw - xw.mean(1, keepdims=True)
    nh = plan.nharm
    n_mag = plan.min_shc * (nh + 1) + (plan.max_shc - plan.min_shc) * (nh + 1) + plan.wl
    nb = n_mag - plan.half_wl
    # input: the window product U |xw| and the subtraction U |s| per sample, through the FFT's running bound; the mean is
    # ONE float32 number (sp_mean roundings on sum |xw| / n) taken off every sample, an exact common shift dm whose
    # transform is dm times the Dirichlet kernel of the n-sample window
    X, E = fft_running(s, U * (np.abs(xw) + np.abs(s)), R, nb)
    dm = (R.sp_mean(n) + 1) * U * np.abs(xw).sum(1) / n
    k = np.arange(nb)
    with np.errstate(all="ignore"):
        dirichlet = np.where(k == 0, float(n), np.abs(np.sin(np.pi * k * n / FFT_N) / np.sin(np.pi * k / FFT_N)))
    mag = np.zeros((frames.size, n_mag))
    dmag = np.zeros_like(mag)
    mag[:, plan.half_wl:] = np.abs(X)
    dmag[:, plan.half_wl:] = E + dm[:, None] * dirichlet[None, :] + R.hyp * U * np.abs(X) + FLOOR
    rows = plan.max_shc - plan.min_shc + 1
    r = np.arange(rows)[:, None]
    w = np.arange(plan.wl)[None, :]
    prod = np.ones((frames.size, rows, plan.wl))
    hi = np.ones_like(prod)
    for h in range(nh + 1):
        ix = (plan.min_shc + r) * (h + 1) + w
        prod *= mag[:, ix]
        hi *= (mag + dmag)[:, ix]
    out = np.zeros((frames.size, plan.max_shc))
    bound = np.zeros_like(out)
    out[:, plan.min_shc - 1:plan.max_shc] = prod.sum(2)
    bound[:, plan.min_shc - 1:plan.max_shc] = (hi - prod + nh * U * hi).sum(2) + R.shc_sum(plan.wl) * U * hi.sum(2) + FLOOR
    return out, bound


def _compare(diff, tol):
    """-> (holds in float64, certain): a comparison `diff > 0` whose operands carry a combined error `tol`; a NaN operand
    fails it for certain, as in float32"""
    if diff != diff:
        return False, True
    return diff > 0, abs(diff) > tol


def peaks(shc_row, dshc_row, plan, R):
    """peaks() of oracle/yaapt.py (yaapt.py:383-497) on one SHC vector in float64 ->
    dict(pitch [4] float32, merit [4], dmerit [4], certain, why): `certain` is False as soon as one comparison that
    settles the candidate list (normalisation, mean test, a peak's window, the merit threshold, the order of the kept
    merits) lies inside the error bound"""
    p = plan.p
    mp = plan.maxpeaks
    lo, hi, c = plan.pk_min_lag, plan.pk_max_lag, plan.pk_center
    why = []
    default = dict(pitch=np.zeros(mp, np.float32), merit=np.ones(mp), dmerit=np.zeros(mp))
    # Two bounds per bin.  `ddata` bounds the normalised value itself (it carries the error of the maximum it is divided
    # by) and goes to the reported merits and to the test of the mean against 1 / shc_thresh1.  `dcmp` serves every
    # comparison BETWEEN normalised values: all are divided by the same float32 maximum, a correctly rounded division is
    # monotone, so the order of two bins is the order of their unnormalised values, up to one rounding each.
    data, ddata, dcmp = shc_row.copy(), dshc_row.copy(), dshc_row.copy()
    mx, dmx = data[lo:hi + 1].max(), dshc_row[lo:hi + 1].max()
    if abs(mx - 1e-14) <= dmx:
        why.append("max")
    if mx > 1e-14:
        data = data / mx
        ddata = (dshc_row + data * dmx) / max(mx - dmx, 1e-300) + U * data
        dcmp = dshc_row / mx + U * data
    cnt = hi - lo + 1
    avg = data[lo:hi + 1].mean()
    sum_u = (R.shc_avg(cnt) + 1) * U * avg
    davg, davg_cmp = ddata[lo:hi + 1].mean() + sum_u, dcmp[lo:hi + 1].mean() + sum_u
    ok, sure = _compare(avg - 1 / p["shc_thresh1"], davg)
    if not sure:
        why.append("avg")
    if ok:
        return dict(default, certain=not why, why=why)
    t2 = p["shc_thresh2"]
    bins = []
    for n in range(lo + c + 1, hi - c + 1):
        v = data[n]
        conds = [(v - t2 * avg, dcmp[n] + t2 * davg_cmp + U * t2 * avg)]
        conds += [(v - data[i], dcmp[n] + dcmp[i]) for i in range(n - c, n + c + 1) if i != n]
        res = [_compare(d, t) for d, t in conds]
        holds = all(h for h, _ in res)
        fails_for_sure = any((not h) and s for h, s in res)
        if not fails_for_sure and not all(s for _, s in res):
            why.append(f"peak{n}")
        if holds:
            bins.append(n)
    merits = [data[n] for n in bins]
    if bins:
        k = int(np.argmax(merits))
        ratio = merits[k] / avg
        dratio = (dcmp[bins[k]] + ratio * davg_cmp) / avg + 2 * U * ratio
    else:
        ratio, dratio = 0.0, 0.0
    ok, sure = _compare(p["shc_thresh1"] - ratio, dratio)
    if not sure:
        why.append("merit")
    if ok:
        return dict(default, certain=not why, why=why)
    order = sorted(range(len(bins)), key=lambda i: -merits[i])          # stable, descending
    for a, b in zip(order[:mp], order[1:mp + 1]):
        if merits[a] - merits[b] <= dcmp[bins[a]] + dcmp[bins[b]]:
            why.append("order")
    order = order[:mp]
    numpeaks = len(order)
    pt = np.zeros(mp, np.float32)
    mt, dm = np.zeros(mp), np.zeros(mp)
    for j, i in enumerate(order):
        pt[j] = np.float32(float(bins[i]) * plan.delta)
        mt[j], dm[j] = merits[i], ddata[bins[i]]
    extra = float(np.float32(p["merit_extra"]))
    if numpeaks > 0:
        if pt[0] > p["f0_double"]:
            numpeaks = min(numpeaks + 1, mp)
            pt[numpeaks - 1], mt[numpeaks - 1], dm[numpeaks - 1] = pt[0] / np.float32(2), extra, 0.0
        if pt[0] < p["f0_half"]:
            numpeaks = min(numpeaks + 1, mp)
            pt[numpeaks - 1], mt[numpeaks - 1], dm[numpeaks - 1] = pt[0] * np.float32(2), extra, 0.0
        pt[numpeaks:], mt[numpeaks:], dm[numpeaks:] = pt[0], mt[0], dm[0]
        return dict(pitch=pt, merit=mt, dmerit=dm, certain=not why, why=why)
    return dict(default, certain=not why, why=why)


# ---- frame means of time_track's in-place subtraction ----------------------------------------------------------------
def frame_means(x, prev_means, plan, R):
    """x float32 [>= (T-1) hop + n]; prev_means [T] float32 = the means the implementation itself produced (frame k uses
    prev_means[k-1] as given, so every frame is checked on its own and an error does not travel down the recurrence)
    -> (mean [T], bound [T]):  mean_k = (sum_{j<ov} (x_j - mean_{k-1}) + sum_{j>=ov} x_j) / n"""
    T, n, hop = plan.tda_nframes, plan.tda_len, plan.frame_jump
    ov = n - hop
    idx = (np.arange(T) * hop)[:, None] + np.arange(n)[None, :]
    fr = _f64(x)[idx]
    prev = np.concatenate(([0.0], _f64(prev_means)[:T - 1]))
    head = fr[:, :ov] - prev[:, None]
    tail = fr[:, ov:]
    S = head.sum(1) + tail.sum(1)
    bound = U * (R.fm_head(ov) * np.abs(head).sum(1) + R.fm_tail(n - ov) * np.abs(tail).sum(1) + 2 * np.abs(S)) / n
    return S / n, bound + U * np.abs(S / n) + FLOOR


def demeaned_frame(x, k, means, plan):
    """the float32 frame crs_corr sees: (x_j - mean_{k-1} for j < ov, k > 0) - mean_k.  Two correctly rounded float32
    subtractions per sample: reproduced here bit for bit"""
    n, hop = plan.tda_len, plan.frame_jump
    ov = n - hop
    v = np.asarray(x[k * hop:k * hop + n], dtype=np.float32).copy()
    if k > 0:
        v[:ov] = v[:ov] - np.float32(means[k - 1])
    return v - np.float32(means[k])


# ---- NCCF ------------------------------------------------------------------------------------------------------------
def lag_window(sp, pstd, plan):
    """the lag window of time_track (yaapt.py:696-709) in float32, as both implementations compute it -> (lag_min,
    lag_max) or None when a bound is NaN (the frame is skipped)"""
    sp, pstd = np.float32(sp), np.float32(pstd)
    with np.errstate(all="ignore"):
        lo, hi = sp - np.float32(2.0) * pstd, sp + np.float32(2.0) * pstd
        lo = lo if (lo != lo or lo > np.float32(plan.p["f0_min"])) else np.float32(plan.p["f0_min"])
        hi = hi if (hi != hi or hi < np.float32(plan.p["f0_max"])) else np.float32(plan.p["f0_max"])
        a, b = np.floor(np.float32(plan.fs) / hi), np.floor(np.float32(plan.fs) / lo)
    if a != a or b != b:
        return None
    return int(a) - plan.nccf_center, int(b) + plan.nccf_center


def nccf_phi(d, lag_min, lag_max, R):
    """d [n] float32 de-meaned frame -> (phi [n], bound [n]), zero outside [lag_min, lag_max):
    phi[l] = sum_{j<N} d[l+j] d[j] / sqrt(sum d[l+j]^2 * sum d[j]^2), N = n - lag_max"""
    n = d.size
    N = n - lag_max
    assert N > 0 and lag_min >= 1
    d64 = _f64(d)
    x = d64[:N]
    rows = np.lib.stride_tricks.sliding_window_view(d64[lag_min:lag_max + N], N)[:lag_max - lag_min]
    phi, bound = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        nume, absn = rows @ x, np.abs(rows) @ np.abs(x)
        den, pw = (rows * rows).sum(1), x @ x
        root = np.sqrt(den * pw)
        v = nume / root
        # both energies are sums of squares: relative `dot` / `pw` roundings plus TINY per product; their product one more
        # rounding; 1 / sqrt(1 - r) - 1 of the total r, infinite from r = 1 on; the root and the division one rounding each
        r = (R.dot(N) * U + N * TINY / den) + (R.pw(N) * U + N * TINY / pw) + (U + TINY / (den * pw))
        grow = np.where(r < 1, 1 / np.sqrt(np.maximum(1 - r, 1e-300)) - 1, np.inf)
        grow = np.where(np.isnan(r), np.inf, grow)
        # numerator: `dot` roundings on sum |terms|, TINY per product
        dv = (R.dot(N) * U * absn + N * TINY) / root + np.abs(v) * (grow + 2 * U)
        dv = np.where(np.isnan(dv), np.inf, dv)
    phi[lag_min:lag_max], bound[lag_min:lag_max] = v, dv
    return phi, bound


def nccf_pick(phi, dphi, lag_min, lag_max, plan):
    """cmp_rate (yaapt.py:609-673) as the reference can return it: the FIRST index of [lag_min + c, lag_max - c] above both
    neighbours and nccf_thresh1, kept if max(phi) > nccf_thresh2 or if it is the maximum of its window
    -> (index or None, certain)"""
    p = plan.p
    c = plan.nccf_center
    certain = True
    first = None
    for i in range(lag_min + c, lag_max - c + 1):
        v = phi[i]
        res = [_compare(v - phi[i - 1], dphi[i] + dphi[i - 1]), _compare(v - phi[i + 1], dphi[i] + dphi[i + 1]),
               _compare(v - p["nccf_thresh1"], dphi[i])]
        holds = all(h for h, _ in res)
        if not any((not h) and s for h, s in res) and not all(s for _, s in res):
            certain = False
        if holds:
            first = i
            break
    if first is None:
        return None, certain
    amax = max(0.0, float(np.nanmax(phi)))
    ok, sure = _compare(amax - p["nccf_thresh2"], float(np.nanmax(dphi)))
    certain = certain and sure
    if ok:
        return first, certain
    v = phi[first]
    res = [_compare(v - phi[i], dphi[first] + dphi[i]) for i in range(first - c, first + c + 1) if i != first]
    certain = certain and (all(s for _, s in res) or any((not h) and s for h, s in res))
    return (first if all(h for h, _ in res) else None), certain


def nccf_pitch(first, plan):
    return np.float32(0.0) if first is None else np.float32(plan.fs / float(first + 1))


def nccf_merit(phi, dphi, first, pitch, sp, pstd, plan):
    """the weighted merit of time_track (yaapt.py:716-727) for the candidate at index `first` (None: no candidate) ->
    (tm, bound); NaN where pitch_std is NaN"""
    merit, dmerit = (0.0, 0.0) if first is None else (min(float(phi[first]), 1.0), float(dphi[first]))
    boost = float(np.float32(1 + plan.p["merit_boost"]))
    with np.errstate(all="ignore"):
        fthr = 5.0 * float(pstd)
        diff = abs(float(pitch) - float(sp))
        q = diff / fthr
        match = (1.0 - q) * (1.0 if diff < fthr else 0.0)
        tm = boost * merit * match
        dmatch = U * (2 * abs(q) + abs(1.0 - q))            # 5 * pitch_std, the division, the subtraction
        bound = boost * (dmerit * abs(match) + merit * dmatch) + 3 * U * abs(tm)
    return tm, bound


# ---- an implementation's stage outputs held against the above ---------------------------------------------------------
# Each judge takes one utterance's float32 results (numpy) of an implementation and returns
#   ratio   the largest |value - float64 value| / bound (inf for a NaN on one side only),
#   exempt  the frames whose float64 decision lies inside the bound (either outcome is legitimate there),
#   wrong   the frames whose decision is certain in float64 and differs: must be empty.
def _ratio(got, want, bound):
    got, want, bound = _f64(got), _f64(want), _f64(bound)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if (nan_g != nan_w).any():
        return float("inf")
    err = np.abs(got - want)[~nan_w]
    b = bound[~nan_w]
    with np.errstate(all="ignore"):
        r = np.where(b > 0, err / np.maximum(b, 1e-300), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def judge_e_raw(filt, e_raw, plan, R):
    e, bound, _ = nlfer_raw(filt, plan, R)
    return dict(ratio=_ratio(e_raw, e, bound + U * e))              # + the float32 store


def judge_energy_norm(e_raw, energy, R):
    want, bound = energy_norm(e_raw, R)
    return dict(ratio=_ratio(energy, want, bound))


def judge_vuv(filt, energy, vuv, plan, R):
    """energy and the voiced / unvoiced decision against the float64 chain from the filtered signal"""
    want, bound, margin = energy_decision(filt, plan, R)
    sure = margin > bound
    dec = want > plan.p["nlfer_thresh1"]
    vuv = np.asarray(vuv).astype(bool)
    return dict(ratio=_ratio(energy, want, bound), exempt=np.flatnonzero(~sure).tolist(),
                wrong=np.flatnonzero(sure & (vuv != dec)).tolist())


def judge_cand(filt2, vuv, cand_pitch, cand_merit, plan, R):
    """the candidates of the frames the implementation itself found above the NLFER threshold: pitches equal to the
    float64 peak list where that is certain, merits within the bound there"""
    frames = np.flatnonzero(np.asarray(vuv).astype(bool))
    need = plan.nframe_size + (plan.nframes - 1) * plan.frame_jump
    x = np.zeros(max(need, len(filt2)), np.float32)
    x[:len(filt2)] = filt2
    out = dict(ratio=0.0, exempt=[], wrong=[])
    if frames.size == 0:
        return out
    s, ds = shc(x, frames, plan, R)
    for i, f in enumerate(frames.tolist()):
        pk = peaks(s[i], ds[i], plan, R)
        if not pk["certain"]:
            out["exempt"].append(f)
            continue
        if not np.array_equal(np.asarray(cand_pitch[:, f], np.float32), pk["pitch"]):
            out["wrong"].append((f, np.asarray(cand_pitch[:, f]).tolist(), pk["pitch"].tolist()))
            continue
        out["ratio"] = max(out["ratio"], _ratio(cand_merit[:, f], pk["merit"], pk["dmerit"]))
    return out


def judge_fmean(x, fmean, plan, R):
    want, bound = frame_means(x, fmean, plan, R)
    return dict(ratio=_ratio(np.asarray(fmean)[:plan.tda_nframes], want, bound))


def judge_nccf(x, fmean, spec_pitch, pitch_std, tp, tm, plan, R):
    """one signal's NCCF candidates: the lag equal to the float64 pick where that is certain; the weighted merit at the
    lag the implementation chose within the bound (NaN where pitch_std is NaN).  `unbounded` lists the uncertain frames
    whose bound is infinite (see Underflow in the module text) apart from the `exempt` ones, whose bound is finite"""
    out = dict(ratio=0.0, exempt=[], unbounded=[], wrong=[])
    for k in range(plan.tda_nframes):
        win = lag_window(spec_pitch[k], pitch_std, plan)
        got_p = np.float32(tp[k])
        if win is None:
            phi = dphi = None
            want_first, sure = None, True
        else:
            d = demeaned_frame(x, k, fmean, plan)
            phi, dphi = nccf_phi(d, win[0], win[1], R)
            want_first, sure = nccf_pick(phi, dphi, win[0], win[1], plan)
        got_first = None
        if got_p != 0:
            got_first = int(round(plan.fs / float(got_p))) - 1
            inside = win is not None and win[0] <= got_first < win[1]
            if not inside or nccf_pitch(got_first, plan) != got_p:
                out["wrong"].append((k, float(got_p), "not a lag of the window"))
                continue
        if not sure:
            # no finite bound: the frame's sums of squares underflow float32 (silence after a burst), kept apart
            unbounded = bool(np.isinf(dphi[win[0]:win[1]]).any())
            out["unbounded" if unbounded else "exempt"].append(k)
        elif got_first != want_first:
            out["wrong"].append((k, float(got_p), float(nccf_pitch(want_first, plan))))
            continue
        want_tm, bound = nccf_merit(phi, dphi, got_first, got_p, spec_pitch[k], pitch_std, plan)
        out["ratio"] = max(out["ratio"], _ratio([tm[k]], [want_tm], [bound + U * abs(want_tm)]))
    return out
