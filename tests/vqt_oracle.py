"""The variable-Q transform of the reference (transforms/transforms.py:812-923, transforms/_transforms.py:327-383) stage
by stage as direct sums in np.longdouble, independent of the package.  Beside each value its absolute companion A: the
same sums with |h|, |k| and |x| in place of the taps, the kernels and the samples -- what the running forward error
bound of a chain of dot products is measured in.  The tap tables are built in float64 exactly as the reference and scipy
build them (firwin, get_window, the complex exponentials) and only then widened, so the device and the oracle sum the
same numbers.

P(x, up, down) is scipy.signal.resample_poly with its default filter for an integer ratio, one of `up`, `down` being 1:
    r = max(up, down), h = up * firwin(20 r + 1, 1 / r, window=("kaiser", 5.0)), n_out = ceil(n_in * up / down)
    out[m] = sum_k h[k] xu[m * down + 10 r - k]
with xu the input with up - 1 zeros after every sample and zero outside it; r = 1 is a copy.  The interpolator sums only
the 21 terms that meet a sample (the others are products with exact zeros)."""

import numpy as np
from scipy.signal import firwin, get_window

LD = np.longdouble
U53 = 2.0 ** -53


def rate_taps(up: int, down: int):
    r = max(up, down)
    if r == 1:
        return None
    h = firwin(20 * r + 1, 1.0 / r, window=("kaiser", 5.0))
    h *= up
    return h


def _accumulate(x, a, n_out, terms, complex_taps=False):
    """sum over (tap (n_out,), index (n_out,)) of tap * x[index] along axis 0, terms outside x being zero; and the same
    with |tap| and the companion a."""
    n = x.shape[0]
    y = np.zeros((n_out,) + x.shape[1:], dtype=np.clongdouble if complex_taps or np.iscomplexobj(x) else LD)
    ya = np.zeros((n_out,) + x.shape[1:], dtype=LD)
    tail = (None,) * (x.ndim - 1)
    for tap, idx in terms:
        ok = (idx >= 0) & (idx < n)
        i = np.where(ok, idx, 0)
        t = np.where(ok, tap, 0)[(slice(None),) + tail]
        y += t * x[i]
        ya += np.abs(t) * a[i]
    return y, ya


def resample(x, a, up: int, down: int):
    """P along axis 0 of the longdouble (or clongdouble) array x and of its companion a -> (y, ya, terms per value)."""
    assert up == 1 or down == 1
    h = rate_taps(up, down)
    if h is None:
        return x.copy(), a.copy(), 1
    h = h.astype(LD)
    n, r = x.shape[0], max(up, down)
    n_out = -(-n * up // down)
    m = np.arange(n_out)
    if down > 1:
        terms = ((np.full(n_out, h[k]), m * down + 10 * r - k) for k in range(len(h)))
        return _accumulate(x, a, n_out, terms) + (len(h),)
    hp = np.concatenate([h, np.zeros(up - 1, dtype=LD)])  # (taps past 20 up meet nothing)
    q, p = m // up, m % up
    terms = ((hp[p + up * j], q + 10 - j) for j in range(21))
    return _accumulate(x, a, n_out, terms) + (21,)


def resample_poly(x, up: int, down: int):
    """P of a float64 or complex128 array along axis 0 -> (value, A) in longdouble."""
    x = np.asarray(x)
    xl = x.astype(np.clongdouble if np.iscomplexobj(x) else LD)
    y, ya, _ = resample(xl, np.abs(xl), up, down)
    return y, ya


def kernels(q, highest_f, bins, mid_fs, window, gamma):
    freqs = highest_f * 2 ** (-1 / bins * np.arange(bins))
    factor = 2 ** (1 / bins) - 1
    lengths = np.round(q * mid_fs / ((freqs * factor) + gamma)).astype(int)
    out = []
    for ind in range(len(lengths)):
        w = get_window(window, lengths[ind], fftbins=False)
        w /= w.sum()
        out.append(w * np.exp(1j * freqs[ind] * 2 * np.pi / mid_fs * np.arange(-lengths[ind] // 2, lengths[ind] // 2)))
    return out


def setup(fs, octaves, a4_tuning):
    highest_f = a4_tuning * 2 ** (octaves[1] - 4 + 2 / 12)
    d = int((fs // 2) / (highest_f * 1.1))
    return highest_f, d, fs // d


def vqt(x, fs, q=1, gamma=50, octaves=(1, 5), bins_per_octave=24, a4_tuning=440, window="hann"):
    """-> (f, value (F, N, C) clongdouble, A (F, N, C) longdouble, c (F,) int64): the transform of x (N, C) float64, its
    absolute companion and per row the number of terms summed along an element's chain plus 2 per stage."""
    x = np.asarray(x, dtype=np.float64)
    n, n_ch = x.shape
    highest_f, d, mid_fs = setup(fs, octaves, a4_tuning)
    ks = kernels(q, highest_f, bins_per_octave, mid_fs, window, gamma / fs * mid_fs)
    n_oct, bins = octaves[1] - octaves[0] + 1, bins_per_octave
    td = x.astype(LD)
    td, ta, c_td = resample(td, np.abs(td), 1, d)
    c_td += 2
    rows, rows_a, counts = [], [], []
    for oc in range(n_oct):
        m = td.shape[0]
        for k in ks:
            kl = k.astype(np.clongdouble)
            L, h = len(k), (len(k) - 1) // 2
            idx = np.arange(m)
            z, za = _accumulate(td, ta, m, ((np.full(m, kl[l]), idx + h - l) for l in range(L)), complex_taps=True)
            c = c_td + L + 2
            if oc > 0:
                z, za, t = resample(z, za, 2 ** oc, 1)
                c += t + 2
            z, za, t = resample(z, za, d, 1)
            c += t + 2
            assert z.shape[0] >= n  # (the reference's zero-padding branch is never taken)
            rows.append(z[:n])
            rows_a.append(za[:n])
            counts.append(c)
        td, ta, t = resample(td, ta, 1, 2)
        c_td += t + 2
    f = a4_tuning * 2 ** (np.arange(octaves[0] - 4 - 9 / 12, octaves[1] - 4 + 2 / 12, 1 / 12))
    return f, np.stack(rows[::-1]), np.stack(rows_a[::-1]), np.array(counts[::-1], dtype=np.int64)


def bound(a, c):
    """2 c 2^-53 A: the running forward bound of the chain (any summation order, with or without fused multiply-adds),
    the factor 2 for the companion's own rounding."""
    return 2.0 * np.asarray(c, dtype=np.float64).reshape((-1,) + (1,) * (a.ndim - 1)) * U53 * a.astype(np.float64)
