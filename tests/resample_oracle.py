"""Rational-ratio resampling as a direct sum in np.longdouble, written from its definition and independent of the package:
    r = max(up, down), half = 10 r, h = up * firwin(20 r + 1, 1 / r, window=("kaiser", 5.0)), n_out = ceil(n up / down)
    y[m] = sum_n x[n] h[m down + half - n up]
(scipy.signal.resample_poly with its default filter).  The sum runs input sample by input sample: sample n adds
x[n] h[k] to every output m for which k = m down + half - n up is a tap.  Beside each value its absolute companion
A[m] = sum_n |x[n]| |h[k]|, what the running forward bound of a dot product is measured in (tests/vqt_oracle.py).  The
taps are built in float64 exactly as scipy builds them (and multiplied by `scale` in float64, as the package folds a
rescaling into them) and only then widened, so the device and the oracle sum the same numbers.

The device is held to |device - oracle| <= 2 (J + 2) 2^-53 A[m] with J = ceil((20 r + 1) / up) the terms of one output at
most: the bound of a sum of J products in any order, with or without fused multiply-adds, the factor 2 for the
companion's own rounding.  A result rounded to float32 once adds 2^-24 |oracle|."""

import numpy as np

import vqt_oracle

LD = np.longdouble
U53 = vqt_oracle.U53
U24 = 2.0 ** -24


def taps(up: int, down: int, scale: float = 1.0) -> np.ndarray:
    h = vqt_oracle.rate_taps(up, down)
    return h * scale if scale != 1.0 else h


def terms(up: int, down: int) -> int:
    return -(-(20 * max(up, down) + 1) // up)


def resample_poly(x, up: int, down: int, scale: float = 1.0):
    """(value, A) in longdouble of the float64 array x (n, C), up and down coprime and not both 1."""
    x = np.asarray(x, dtype=np.float64)
    xl, xa = x.astype(LD), np.abs(x).astype(LD)
    h = taps(up, down, scale).astype(LD)
    ha = np.abs(h)
    n, ntaps, half = x.shape[0], len(h), 10 * max(up, down)
    n_out = -(-n * up // down)
    y = np.zeros((n_out, x.shape[1]), dtype=LD)
    a = np.zeros((n_out, x.shape[1]), dtype=LD)
    for i in range(n):
        # the outputs sample i reaches: 0 <= m down + half - i up < ntaps
        lo = max(0, -(-(i * up - half) // down))
        hi = min(n_out - 1, (i * up - half + ntaps - 1) // down)
        if hi < lo:
            continue
        k = np.arange(lo, hi + 1) * down + half - i * up
        y[lo:hi + 1] += h[k][:, None] * xl[i][None, :]
        a[lo:hi + 1] += ha[k][:, None] * xa[i][None, :]
    return y, a


def bound(a, up: int, down: int, value=None):
    """2 (J + 2) 2^-53 A, plus 2^-24 |value| where the result is rounded to float32 (value given)"""
    lim = vqt_oracle.bound(a, terms(up, down) + 2)
    return lim if value is None else lim + U24 * np.abs(value).astype(np.float64)


def worst_ratio(got, value, lim) -> float:
    """largest |got - value| / lim over every element (none is skipped: where the bound is zero the error must be too)"""
    err = np.abs(got.astype(LD) - value).astype(np.float64)
    assert err.shape == lim.shape, (err.shape, lim.shape)
    assert not err[lim == 0].any()
    return float((err / np.where(lim > 0, lim, 1.0)).max()) if err.size else 0.0
