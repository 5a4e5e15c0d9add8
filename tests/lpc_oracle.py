"""Restatements of the reference's linear prediction (transforms/transforms.py:1199-1283, helpers/ar_estimation.py,
standard/_framed_signal_representation.py) in numpy, vectorised over the (frame, channel) pairs and written for any
floating dtype: with np.float64 they are the restatement the host tests hold to the fixtures, with np.longdouble (x87,
80 bit) the oracle that tools/gen_golden_lpc.py and the host tests judge the reference itself against.  The windowed
frames are float64 data in both (one product per sample, which the reference, this file and the device round alike);
everything after them runs in `dtype`."""

import numpy as np

EPS64 = np.finfo(np.float64).eps


def frames_of(x, L, hop):
    """_get_framed_signal(x, L, hop, keep_last_frames=True): (L, ceil(N / hop), C), zeros past the end."""
    n, n_ch = x.shape
    n_frames = -(-n // hop)
    padded = np.zeros((max(n, (n_frames - 1) * hop + L), n_ch))  # (hop > L: samples between frames are skipped)
    padded[:n] = x
    return np.stack([padded[f * hop:f * hop + L] for f in range(n_frames)], axis=1)


def windowed_frames(x, window, hop):
    return frames_of(np.asarray(x, dtype=np.float64), len(window), hop) * np.asarray(window)[:, None, None]


def autocorrelation(td, order, dtype=np.float64):
    """The biased autocorrelation r[k] = sum_n x[n] x[n + k] / L, k = 0 .. order, of every column of td (L, ...)."""
    t = td.astype(dtype)
    L = t.shape[0]
    return np.stack([(t[:L - k] * t[k:]).sum(axis=0) / dtype(L) for k in range(order + 1)])


def levinson(r, dtype=np.float64):
    """_levison_durbin_recursion without its raise: (a with a[0] = 1, prediction error, singular) -- singular: the
    prediction error was <= 0 after some order, in some column."""
    r = np.asarray(r).astype(dtype)
    E = r[0].copy()
    c = r[1:]
    a = np.zeros_like(c)
    singular = False
    with np.errstate(invalid="ignore", divide="ignore"):
        for m in range(c.shape[0]):
            value = c[m].copy()
            for lag in range(m):
                value += a[lag] * c[m - lag - 1]
            k = -value / E
            E = E * (dtype(1.0) - k * k)
            singular |= bool(np.any(E <= 0))
            old = a[:m].copy()
            a[:m] = old + k * old[::-1]
            a[m] = k
    return np.concatenate([np.ones_like(r[:1]), a]), E, singular


def yule_walker(td, order, dtype=np.float64):
    a, E, singular = levinson(autocorrelation(td, order, dtype), dtype)
    return a, E, singular


def burg(td, order, dtype=np.float64):
    """_burg_ar_estimation on (L, frames, channels): (a of order + 1 rows, den)."""
    t = td.astype(dtype)
    a = np.zeros((order + 1,) + t.shape[1:], dtype=dtype)
    a[0] = 1
    prev = a.copy()
    f, b = t[1:], t[:-1]
    den = (f * f + b * b).sum(axis=0)
    for i in range(order):
        rc = (dtype(-2.0) * (b * f).sum(axis=0)) / (den + dtype(EPS64))
        prev, a = a, prev
        for j in range(1, i + 2):
            a[j] = prev[j] + rc * prev[i - j + 1]
        f, b = f + rc * b, b + rc * f
        den = (dtype(1.0) - rc * rc) * den - b[-1] ** 2 - f[0] ** 2
        f, b = f[1:], b[:-1]
    return a, den


def all_pole(a, src, dtype=np.float64):
    """lfilter([1], a[:, f, c], src[:, f, c]) from zero state for every pair."""
    a = a.astype(dtype)
    s = src.astype(dtype)
    order = a.shape[0] - 1
    y = np.zeros((s.shape[0] + order,) + s.shape[1:], dtype=dtype)  # `order` zeros in front
    taps = a[1:][::-1] / a[0]  # taps[j] multiplies y[n - order + j]
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(s.shape[0]):
            y[n + order] = s[n] / a[0] - (taps * y[n:n + order]).sum(axis=0)
    return y[order:]


def overlap_add(frames, window, hop, n_out, dtype=np.float64):
    """_reconstruct_framed_signal(frames, hop, window, n_out): (n_out, C)."""
    L, n_frames, n_ch = frames.shape
    w = np.asarray(window).astype(dtype)
    total = (n_frames - 1) * hop + L
    td = np.zeros((total, n_ch), dtype=dtype)
    env = np.zeros(total, dtype=dtype)
    fw = frames.astype(dtype) * w[:, None, None]
    for f in range(n_frames):
        td[f * hop:f * hop + L] += fw[:, f]
        env[f * hop:f * hop + L] += w * w
    td /= np.maximum(env, dtype(1e-4))[:, None]
    out = np.zeros((n_out, n_ch), dtype=dtype)
    out[:min(n_out, total)] = td[:n_out]
    return out


def peak_constrained(y):
    """Signal.from_time_data: divided by the largest magnitude where that is above 1."""
    peak = np.max(np.abs(y))
    return y / peak if peak > 1.0 else y


def synthesize(a, sources, window, hop, n_out, dtype=np.float64):
    return peak_constrained(overlap_add(all_pole(a, sources, dtype), window, hop, n_out, dtype))


def coefficient_error(a, ref):
    """The largest |a - ref| over each pair's largest |ref|, over the pairs whose reference is finite; NaN positions
    must agree (asserted)."""
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), "NaN positions differ"
    ok = ~np.isnan(ref[-1])  # (a pair is NaN from row 1 on, or finite)
    if not ok.any():
        return 0.0
    a, ref = a[:, ok], ref[:, ok]
    return float(np.max((np.abs(a - ref).max(axis=0) / np.abs(ref).max(axis=0)).astype(np.float64)))


def variance_error(v, ref):
    """The largest relative error; NaN positions must agree, and a zero must be met by a zero."""
    v, ref = np.asarray(v), np.asarray(ref)
    assert v.shape == ref.shape, (v.shape, ref.shape)
    assert np.array_equal(np.isnan(v), np.isnan(ref)), "NaN positions differ"
    zero = ref == 0
    assert np.array_equal(v[zero], ref[zero]), "a variance that is 0 in the reference is not 0"
    ok = ~np.isnan(ref) & ~zero
    if not ok.any():
        return 0.0
    return float(np.max(np.abs((v[ok] - ref[ok]) / ref[ok]).astype(np.float64)))


def channel_error(y, ref):
    """The largest |y - ref| over each channel's peak |ref|."""
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    return float(np.max((np.abs(y - ref).max(axis=0) / np.abs(ref).max(axis=0)).astype(np.float64)))
