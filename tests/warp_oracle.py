"""The all-pass table of transforms.warp and transforms.laguerre restated in numpy, in long double by default, and the
shapes the tests sweep.

    c[i][j] = p c[i-1][j] + c[i-1][j-1] + q c[i][j-1]   (i, j >= 1),     out[j][ch] = sum_i c[i][j] x[i][ch]

with a given first row and first column (c[0][0] from the column).  The table is swept by anti-diagonals -- cell (i, j)
needs only the two diagonals before its own -- so a 2500 x 2500 table costs 5000 vector steps and no 2500 x 2500 array.
warp(lambda) is p = -lambda, q = lambda, the unit pulse as first row and (-lambda)^i as first column; laguerre(f) is
p = -f, q = f, sqrt(1 - f^2) (-f)^i as first column and sqrt(1 - f^2) f^j as first row.  The boundary rows are running
products, as the reference's lfilter calls make them.

The case lists are built from the constants of csrc/warp_plan.hpp: the tile sides TI and TJ, the channel group G and
the wave width."""

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def plan_constants():
    text = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "warp_plan.hpp")).read()
    c = {k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("WAVE", "WAVES", "TI", "G", "STAGGER")}
    assert re.search(r"constexpr int TJ = WAVE \* WAVES;", text)
    c["TJ"] = c["WAVE"] * c["WAVES"]
    return c


K = plan_constants()
TI, TJ, G, WAVE = K["TI"], K["TJ"], K["G"], K["WAVE"]

# the rectangular (n_in, n_out) shapes of the issue: one cell; one row past a tile; one column past a tile; two tiles and
# a cell each way; three full tile rows of an incomplete tile column
RECT_SHAPES = [(1, 1), (TI + 1, 5), (5, TJ + 1), (2 * TI + 1, 2 * TJ + 1), (3 * TI, TJ - 1)]
SQUARE_SIZES = [1, 2, WAVE - 1, WAVE, WAVE + 1, TJ - 1, TJ, TJ + 1, 2 * TJ + 1]
CHANNELS = [1, G, G + 1]
LAMBDAS = [0.0, 0.5, -0.876, 0.99]


def running_powers(first, ratio, n, dtype=np.float64):
    """first, first ratio, first ratio^2, ... as running products in `dtype`"""
    v = np.full(n, dtype(ratio), dtype=dtype)
    v[0] = dtype(first)
    return np.multiply.accumulate(v)


def warp_tables(lam, n_in, n_out, dtype=np.float64):
    """(p, q, row0, col0) of warp(lambda)"""
    row0 = np.zeros(n_out, dtype=dtype)
    row0[0] = 1
    return -lam, lam, row0, running_powers(1.0, -lam, n_in, dtype)


def laguerre_tables(f, n_in, n_out, dtype=np.float64):
    """(p, q, row0, col0) of laguerre(f)"""
    s = np.sqrt(dtype(1) - dtype(f) * dtype(f))
    return -f, f, running_powers(s, f, n_out, dtype), running_powers(s, -f, n_in, dtype)


def allpass_table(x, p, q, row0, col0, n_out=None, dtype=LD):
    """out (n_out, channels) of (n_in, channels) samples"""
    x = np.asarray(x, dtype=dtype)
    if x.ndim == 1:
        x = x[:, None]
    n_in, n_ch = x.shape
    row0, col0 = np.asarray(row0, dtype=dtype), np.asarray(col0, dtype=dtype)
    n_out = len(row0) if n_out is None else n_out
    assert len(row0) == n_out and len(col0) == n_in
    p, q = dtype(p), dtype(q)
    out = np.zeros((n_out, n_ch), dtype=dtype)
    d1, d2 = np.zeros(n_in, dtype=dtype), np.zeros(n_in, dtype=dtype)  # diagonal k - 1 and k - 2, indexed by i
    for k in range(n_in + n_out - 1):
        lo, hi = max(0, k - n_out + 1), min(k, n_in - 1)
        d = np.zeros(n_in, dtype=dtype)
        a, b = max(lo, 1), min(hi, k - 1)  # the computed cells of the diagonal: i >= 1 and j = k - i >= 1
        if a <= b:
            d[a:b + 1] = p * d1[a - 1:b] + d2[a - 1:b] + q * d1[a:b + 1]
        if lo == 0:
            d[0] = row0[k]
        if hi == k:
            d[k] = col0[k]
        idx = np.arange(lo, hi + 1)
        out[k - idx] += d[idx, None] * x[idx]
        d2, d1 = d1, d
    return out


def warp(x, lam, dtype=LD):
    x = np.asarray(x)
    return allpass_table(x, *warp_tables(lam, len(x), len(x), dtype), dtype=dtype)


def laguerre(x, f, dtype=LD):
    x = np.asarray(x)
    return allpass_table(x, *laguerre_tables(f, len(x), len(x), dtype), dtype=dtype)


def channel_error(got, want):
    """the largest |got - want| of any channel over that channel's peak |want|"""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    peak = np.abs(want).max(axis=0)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and (peak > 0).all()
    return float((np.abs(got - want).max(axis=0) / peak).max())


def decaying_noise(n, n_ch, seed):
    """noise under an exponential envelope that falls by 60 dB over the length, rounded to float32"""
    rng = np.random.default_rng(seed)
    env = np.exp(-6.9 * np.arange(n) / max(n, 2))[:, None]
    return (rng.standard_normal((n, n_ch)) * env).astype(np.float32)


_sweep = {}


def sweep_reference(n_in, n_out, lam):
    """(x, (p, q, row0, col0), long-double out) of one sweep shape at G + 1 channels, computed once and shared: the
    table does not depend on the channels, a case with fewer channels takes the leading columns.  Odd n_in take warp's
    boundary rows, even n_in laguerre's."""
    key = (n_in, n_out, lam)
    if key not in _sweep:
        x = decaying_noise(n_in, G + 1, 1000 * n_in + n_out).astype(np.float64)
        tables = warp_tables(lam, n_in, n_out) if n_in % 2 else laguerre_tables(lam, n_in, n_out)
        want = allpass_table(x, *tables)
        for a in (x, want, tables[2], tables[3]):
            a.setflags(write=False)
        _sweep[key] = (x, tables, want)
    return _sweep[key]
