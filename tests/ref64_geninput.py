"""Float64 restatement of the generator-input launch (include/satools_hip_geninput.h; csrc/geninput/generator_input.hip) and of the
host side of the reference's SpeakerCMVN, for tests/test_hip_geninput.py, tests/test_hip_variants.py and tests/test_variants_host.py.
numpy only.

The normalised value q = (v - mean) / std is two correctly rounded float32 operations on exact inputs: with u = 2^-24,
fl(v - mean) = (v - mean)(1 + e1), |e1| <= u, and the quotient adds |e2| <= u, so |got - q| <= (2 u + u^2) |q| < 3 u |q|: NORM_BOUND.
Everything else the launch produces is a copy or a gather: equality."""
import numpy as np

U = 2.0 ** -24
NORM_BOUND = 3 * U          # times |q|


def interp_index(T, T_f0):
    """source index of F.interpolate(mode='nearest') for T_f0 -> T, in the float32 arithmetic torch and the kernels use"""
    scale = np.float32(T_f0) / np.float32(T)
    s = np.floor(np.arange(T, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(s, T_f0 - 1)


def normalise(f0, mean, std):
    """voiced (v - mean) / std in float64, zeros kept; mean / std broadcast against f0"""
    f0 = np.asarray(f0, dtype=np.float64)
    q = (f0 - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return np.where(f0 != 0, q, 0.0)


def transform32(norm, quant_bins=0, noise=None):
    """quantiser and noise ON the float32 normalised values, in float32 as torch does them: exact functions of their input for the
    power-of-two bin counts in use (x * bins, round half to even, / bins) and one rounded addition"""
    v = np.asarray(norm, dtype=np.float32).copy()
    if quant_bins > 0:
        b = np.float32(quant_bins)
        with np.errstate(invalid="ignore"):
            q = (np.rint(v * b) / b).astype(np.float32)
        v = np.where(v != 0, q, v)
    if noise is not None:
        v = np.where(v != 0, (v + np.asarray(noise, dtype=np.float32)).astype(np.float32), v)
    return v.astype(np.float32)


def slice_rows(S, R, slice_stat):
    """statistics row of every batch row b = s R + r; -1 for a row of a skipped slice"""
    return np.repeat(np.zeros(S, dtype=np.int64) if slice_stat is None else np.asarray(slice_stat, dtype=np.int64), R)


def generator_input(bn, f0, stats, slice_stat=None, spk=None):
    """-> (x float64 [B, C_bn + 1 + n_spk, T] with the NORMALISED F0 row (no quantiser, no noise), f0_norm float64 like f0).
    bn [B, C_bn, T], f0 [S, R, T_f0], stats [n_stats, 2], spk [B, n_spk] or None"""
    bn, f0, stats = np.asarray(bn), np.asarray(f0), np.asarray(stats, dtype=np.float64)
    S, R, T_f0 = f0.shape
    B, C_bn, T = bn.shape
    assert S * R == B
    k = slice_rows(S, R, slice_stat)
    norm = normalise(f0.reshape(B, T_f0), stats[k, 0][:, None], stats[k, 1][:, None])
    rows = [bn.astype(np.float64), norm[:, interp_index(T, T_f0)][:, None, :]]
    if spk is not None:
        rows.append(np.repeat(np.asarray(spk, dtype=np.float64)[:, :, None], T, axis=2))
    return np.concatenate(rows, axis=1), norm.reshape(S, R, T_f0)


def speaker_moments(total, total_sq, frames):
    """SpeakerCMVN.compute_global_stats: Python-float mean and variance of the accumulated sums, then the reference's float32 roundings
    (torch.tensor(mean); sqrt(tensor(var + 1e-6)): the sum in float64, rounded to float32, then a float32 square root)"""
    mean = total / frames
    var = total_sq / frames - mean ** 2
    return np.float32(mean), np.sqrt(np.float32(var + 1e-6))


def speaker_table(state, n_spk):
    """the unpickled SpeakerCMVN state {"speaker_stats": {index string: {"mean", "std", ...}}, "stats_computed": {index string: bool}} ->
    float32 [n_spk, 2] = {mean, std}; NaN rows for speakers without computed statistics"""
    t = np.full((n_spk, 2), np.nan, dtype=np.float32)
    for key, done in state["stats_computed"].items():
        if done:
            st = state["speaker_stats"][key]
            t[int(key)] = (np.float32(float(st["mean"])), np.float32(float(st["std"])))
    return t
