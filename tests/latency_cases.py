"""The signals of the latency tests and of tools/gen_golden_latency.py, and the loader of tests/golden/latency/cases.npz.

One family: white noise of a seeded generator; every channel is the noise delayed by l + f samples -- the fraction f by a
33-tap Hann-windowed sinc, the integer l by where the channel is cut out of the longer noise -- plus independent noise
of 0.01, rounded to float32.  A pair case compares `in1` (each channel delayed by its own l + f) with `in2` (the same
channels undelayed); a case without `in2` has its channels cut from ONE noise, channel 0 undelayed.  The impulse responses
are a unit impulse, a smaller neighbour and noise of 1e-3."""

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "latency", "cases.npz")
FS = 48000
STORED_UP_TO = 1000
POINTS = (0, 1, 2, 3)
TAPS = 33

# name: n, lags, fractions; `cut`: in1 keeps its first `cut` samples; `self`: no in2, channel 0 is the undelayed one
CASES = {
    "c1": dict(n=100, lags=[5, -9, 30], fractions=[0.4, 0.7, 0.2], seed=1),
    "c2": dict(n=4096, lags=[7, -5, 40], fractions=[0.25, 0.5, 0.8], seed=2),
    "c3": dict(n=4097, lags=[7, -5, 40], fractions=[0.25, 0.5, 0.8], seed=3),
    "c4": dict(n=20000, lags=[900, -333], fractions=[0.35, 0.65], seed=4),
    "c5": dict(n=4096, lags=[0, 112], fractions=[0.3, 0.6], seed=5),
    # the peaks of c5 lie 113 rows apart (112.6 rounds up), its window has 513 rows; one row less gives the power of two
    "c5p": dict(n=4096, lags=[0, 111], fractions=[0.3, 0.6], seed=5),
    "c6": dict(n=20000, lags=[4000, -4000], fractions=[0.3, 0.6], seed=6),
    "c7": dict(n=4096, lags=[7, -5, 40], fractions=[0.25, 0.5, 0.8], seed=2, cut=3277),
    "c8": dict(n=500, lags=[0, 3, 11, 25], fractions=[0.0, 0.3, 0.6, 0.2], seed=8, self=True),
    "c8two": dict(n=500, lags=[0, 11], fractions=[0.0, 0.6], seed=9, self=True),
}
# name: n, channels, peak row, the neighbour's value
IRS = {
    "ir600": dict(n=600, channels=2, peak=37, neighbour=0.45, seed=600),
    "ir4097": dict(n=4097, channels=1, peak=120, neighbour=-0.3, seed=4097),
}


def shifted(base: np.ndarray, fraction: float) -> np.ndarray:
    """base delayed by `fraction` samples, same length: the Hann-windowed sinc of TAPS taps centred on its middle."""
    if fraction == 0.0:
        return base.copy()
    k = np.arange(TAPS) - TAPS // 2
    h = np.sinc(k - fraction) * np.hanning(TAPS)
    return np.convolve(base, h)[TAPS // 2:TAPS // 2 + len(base)]


def make_pair(n, lags, fractions, seed, cut=None, self=False):
    """(in1, in2) float64 arrays holding float32 values; in2 is None for a `self` case."""
    rng = np.random.default_rng(seed)
    margin = max(abs(int(v)) for v in lags) + TAPS
    n_ch = len(lags)
    base = rng.standard_normal((n + 2 * margin, 1 if self else n_ch))
    in1 = np.empty((n, n_ch))
    for c, (lag, fr) in enumerate(zip(lags, fractions)):
        b = base[:, 0 if self else c]
        in1[:, c] = shifted(b, fr)[margin - lag:margin - lag + n]
    in1 += 0.01 * rng.standard_normal(in1.shape)
    in1 = in1.astype(np.float32).astype(np.float64)
    if self:
        return in1, None
    in2 = base[margin:margin + n] + 0.01 * rng.standard_normal((n, n_ch))
    in2 = in2.astype(np.float32).astype(np.float64)
    return (in1[:cut] if cut else in1), in2


def make_ir(n, channels, peak, neighbour, seed):
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.standard_normal((n, channels))
    x[peak] += 1.0
    x[peak + 1] += neighbour
    return x.astype(np.float32).astype(np.float64)


def probe(x: np.ndarray) -> np.ndarray:
    return np.concatenate([x[:16, 0], [x.sum()]])


_GOLDEN = None


def golden():
    """(arrays, meta) of the fixture, loaded once: stored signals widened to float64, the long ones rebuilt from their
    seeds and proved by their probes.  arrays[name + "_in1"], [name + "_in2"] (absent for a `self` case), arrays[ir name]."""
    global _GOLDEN
    if _GOLDEN is None:
        f = np.load(PATH)
        meta = json.loads(str(f["meta"]))
        z = {k: f[k] for k in f.files if k != "meta"}

        def restore(key, build):
            if key in z:
                z[key] = z[key].astype(np.float64)
            else:
                x = build()
                assert np.array_equal(probe(x), z[key + "_probe"]), f"the seeded signal {key} changed"
                z[key] = x

        for name, p in meta["signals"].items():
            restore(name + "_in1", lambda: make_pair(**p)[0])
            if not p.get("self"):
                restore(name + "_in2", lambda: make_pair(**p)[1])
        for name, p in meta["irs"].items():
            restore(name, lambda: make_ir(**p))
        _GOLDEN = (z, meta)
    return _GOLDEN


def pair_of(z, name):
    return z[name + "_in1"], z.get(name + "_in2")
