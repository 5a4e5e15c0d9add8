"""Long-double restatement of the levels and loudness family: what standard.normalize, rms, crest_factor, fade,
apply_gain, detrend, envelope and lufs_integrated compute, written from their definitions (not from the reference's
code) in numpy's long double.  The generator judges the reference against it, the GPU tests the device.

The least-squares polynomial is formed in a basis orthonormal on the sample grid (the discrete Chebyshev polynomials by
their three-term recurrence), the windowed sums from a long-double prefix sum, the second-order sections by the
transposed direct form II recursion sample by sample, the analytic signal by fft64_cases.oracle_hilbert."""

import numpy as np

import fft64_cases as f64c
import levels_cases as lc

LD = np.longdouble


def gram_basis(n, order):
    """P (order + 1, n) long double: the polynomials orthonormal on 0 .. n - 1, degree by degree."""
    order = min(order, n - 1)
    t = np.arange(n, dtype=LD) - (LD(n) - 1) / 2
    k = np.arange(order + 1, dtype=LD)
    beta = np.sqrt(k * k * (LD(n) * LD(n) - k * k) / (4 * (4 * k * k - 1)))
    P = np.empty((order + 1, n), LD)
    P[0] = 1 / np.sqrt(LD(n))
    for j in range(order):
        P[j + 1] = (t * P[j] - (beta[j] * P[j - 1] if j else 0)) / beta[j + 1]
    return P


def trend(x, order):
    """The least-squares polynomial of every column of x (n, C), long double."""
    P = gram_basis(len(x), order)
    return P.T @ (P @ x.astype(LD))


def detrend(x, order):
    return x.astype(LD) - trend(x, order)


def rms(x, common=False, centred=True):
    """sqrt(mean (x - mean)^2) per column; common: of the flattened array, for every column."""
    x = x.astype(LD)
    if common:
        x = x.reshape(-1, 1)
    d = x - np.mean(x, axis=0) if centred else x
    return np.sqrt(np.mean(d * d, axis=0))


def peak(x):
    return np.max(np.abs(x.astype(LD)), axis=0)


def normalize(x, dbfs, peak_normalization, each_channel):
    factor = LD(10) ** (LD(dbfs) / 20)
    if peak_normalization:
        d = peak(x) if each_channel else np.max(peak(x))
    else:
        d = rms(x) if each_channel else rms(x, common=True)[0]
    return x.astype(LD) * (factor / d)


def gain(x, gain_db):
    return x.astype(LD) * LD(10) ** (np.atleast_1d(np.asarray(gain_db, dtype=LD)) / 20)


def fade_table(kind, l_samples):
    """The rising curve, long double: linear in amplitude, linear in dB from -100, or log10 of a line from 1 to
    50 sqrt(10) normalised to end at 1."""
    r = np.arange(l_samples, dtype=LD) / max(l_samples - 1, 1)
    if kind == "Linear":
        return r
    if kind == "Exponential":
        return LD(10) ** ((-100 + 100 * r) / 20)
    if kind == "Logarithmic":
        top = 50 * np.sqrt(LD(10))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.log10(1 + (top - 1) * r) / np.log10(1 + (top - 1) * r[-1])
    raise ValueError(kind)


def fade(x, kind, l_samples, at_start, at_end, swapped=False):
    """Both ends act on the same samples.  swapped: the wrong oracle (the curve runs the other way)."""
    y = x.astype(LD).copy()
    if kind == "NoFade" or l_samples == 0:
        return y
    table = fade_table(kind, l_samples)[:, None]
    if swapped:
        table = table[::-1]
    if at_start:
        y[:l_samples] *= table
    if at_end:
        y[len(y) - l_samples:] *= table[::-1]
    return y


def moving_mean_square(x, window, with_detrend=True):
    """Mean over the last `window` samples (zeros before the first) of the squared linearly detrended signal."""
    d = detrend(x, 1) if with_detrend else x.astype(LD)
    cs = np.concatenate([np.zeros((1, x.shape[1]), LD), np.cumsum(d * d, axis=0)])
    n = np.arange(1, len(x) + 1)
    return (cs[n] - cs[np.maximum(n - window, 0)]) / window


def envelope_analytic(x, with_detrend=True):
    d = detrend(x, 1) if with_detrend else x.astype(LD)
    return np.abs(f64c.oracle_hilbert(d))


def biquad(kind, f_hz, gain_db, q, fs):
    """The Audio EQ Cookbook's high shelf and high pass as (b0, b1, b2, a0, a1, a2), long double."""
    w = 2 * np.pi * LD(f_hz) / fs
    cw, alpha = np.cos(w), np.sin(w) / (2 * LD(q))
    if kind == "highpass":
        return np.array([(1 + cw) / 2, -(1 + cw), (1 + cw) / 2, 1 + alpha, -2 * cw, 1 - alpha], LD)
    A = LD(10) ** (LD(gain_db) / 40)
    r = 2 * np.sqrt(A) * alpha
    return np.array([A * ((A + 1) + (A - 1) * cw + r), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - r),
                     (A + 1) - (A - 1) * cw + r, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - r], LD)


def k_weighting(fs):
    return [biquad("highshelf", 1500, 4.0, np.sqrt(LD(2)) / 2, fs), biquad("highpass", 38.1, 0.0, 0.5, fs)]


def sos_filter(x, sections):
    """The cascade from rest, all columns at once, sample by sample (transposed direct form II)."""
    y = x.astype(LD)
    for s in sections:
        b0, b1, b2, a1, a2 = s[0] / s[3], s[1] / s[3], s[2] / s[3], s[4] / s[3], s[5] / s[3]
        z1 = np.zeros(y.shape[1], LD)
        z2 = np.zeros(y.shape[1], LD)
        out = np.empty_like(y)
        for i in range(len(y)):
            xi = y[i]
            yi = b0 * xi + z1
            z1 = b1 * xi - a1 * yi + z2
            z2 = b2 * xi - a2 * yi
            out[i] = yi
        y = out
    return y


def block_count(n, tg, step):
    return max(0, -(-(n - tg) // step))


def lufs_blocks(x, fs, tg=None, step=None):
    """-> (z (blocks, C), peak (blocks, C)): mean square and peak of every block of the K-weighted signal."""
    tg0, step0 = lc.lufs_blocks(fs)
    tg, step = tg or tg0, step or step0
    y = sos_filter(x, k_weighting(fs))
    nb = block_count(len(x), tg, step)
    z = np.empty((nb, x.shape[1]), LD)
    pk = np.empty((nb, x.shape[1]), LD)
    for b in range(nb):
        seg = y[b * step:b * step + tg]
        z[b] = np.mean(seg * seg, axis=0)
        pk[b] = np.max(np.abs(seg), axis=0)
    return z, pk


def lufs_gating(z):
    """-> (loudness, block loudness, mask of the absolute gate, mask of both gates, relative gate); NaN without blocks."""
    z = np.asarray(z)
    w = np.array(lc.LUFS_WEIGHTS, z.dtype)[:z.shape[1]]
    if z.shape[0] == 0:
        return float("nan"), np.zeros(0), np.zeros(0, bool), np.zeros(0, bool), float("nan")

    def loud(p):
        with np.errstate(divide="ignore", invalid="ignore"):
            return -0.691 + 10 * np.log10(p @ w)

    lj = loud(z)
    above = lj > -70
    gate = loud(np.mean(z[above], axis=0)) - 10 if above.any() else float("nan")
    both = lj > max(gate, -70) if above.any() else above
    value = loud(np.mean(z[both], axis=0)) if both.any() else float("nan")
    return float(value), lj, above, both, float(gate)


def relative_to_peak(got, want):
    """max |got - want| per column over the column's peak |want|, the worst column."""
    want = np.asarray(want)
    err = np.max(np.abs(np.asarray(got).astype(want.dtype) - want), axis=0)
    pk = np.max(np.abs(want), axis=0)
    return float(np.max(np.where(pk > 0, err / np.where(pk > 0, pk, 1), err)))


def reduction_depth(n):
    """The longest chain of additions a term of a length-n reduction passes in the kernels: PER_LANE in a lane, log2(NT) in
    the tree, then the workgroups' partials the same way (ceil(n_wg / NT) in a lane, log2(NT) in the tree)."""
    n_wg = -(-n // lc.SPAN)
    lg = int(np.log2(lc.NT))
    return min(lc.PER_LANE, -(-n // lc.NT)) + lg + -(-n_wg // lc.NT) + lg
