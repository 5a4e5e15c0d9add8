"""The cases of the variable-Q transform tests (tests/test_vqt_host.py, tests/test_vqt_gpu.py) and of
tools/gen_golden_vqt.py, which runs the reference on them and writes tests/golden/vqt/cases.npz.

CASES have golden data.  EDGES are judged against the oracle only: lengths around the tiles of the three kernels at three
channels (a workgroup of k_vqt_interp takes 1020 output samples of a row at the last stage's U = d = 3 and three channels; one
of k_vqt_decimate and k_vqt_bank takes 64 samples at the decimated rate when there are more than two channels, 128 at
two, 256 at one), d = 3, one octave pair."""

import os
import zlib

import numpy as np

import vqt_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "vqt", "cases.npz")

INTERP_TILE = 1020  # of the last stage at d = 3 and three channels (backend._vqt_interp_tile(3, 3))
SAMPLE_TILE = 64  # at three channels

CASES = {
    # d = 22, L 70 .. 127, octave lengths 219, 110, 55, 28, 14: the bottom octave is shorter than every kernel
    "default": dict(n=4801, c=2, fs=48000, kw={}),
    # constant-Q: d = 14
    "cqt": dict(n=3000, c=1, fs=16000, kw=dict(octaves=[2, 4], bins_per_octave=12, gamma=0)),
    # L 10 .. 16, odd bin count, a window with a parameter
    "kaiser": dict(n=700, c=3, fs=8000, kw=dict(octaves=[1, 3], bins_per_octave=7, q=0.5, window=("kaiser", 6.0))),
    # shorter than the first decimation filter
    "short": dict(n=50, c=1, fs=48000, kw={}),
    # d = 1: the rate-1 stages are copies
    "d1": dict(n=600, c=2, fs=8000, kw=dict(octaves=[4, 6])),
}

_EDGE_KW = dict(octaves=[5, 6], bins_per_octave=6)  # fs = 16000: d = 3
EDGES = {f"interp_{n}": dict(n=n, c=3, fs=16000, kw=_EDGE_KW)
         for n in (INTERP_TILE - 1, INTERP_TILE, INTERP_TILE + 1, 2 * INTERP_TILE + 1)}
# ceil(n / 3) = 63, 64, 65, 129 samples after the first decimation
EDGES.update({f"tile_{n}": dict(n=n, c=3, fs=16000, kw=_EDGE_KW) for n in (189, 192, 195, 387)})
EDGES["tile_c1_771"] = dict(n=771, c=1, fs=16000, kw=_EDGE_KW)  # 257 samples at one channel: a second workgroup
EDGES["tile_c2_387"] = dict(n=387, c=2, fs=16000, kw=_EDGE_KW)  # 129 at two channels

ALL = {**CASES, **EDGES}
STORE_WHOLE_UP_TO = 200_000  # bytes of a case's result stored whole; larger ones store subset()

RATIOS = [(1, 22), (1, 2), (16, 1), (22, 1), (1, 1)]  # (up, down) of the resampler tests
RATIO_LENGTHS = [1, 21, 219]


def signal(name: str) -> np.ndarray:
    """(n, c) float64: unit noise and two tones an octave apart, seeded by the case's name."""
    p = ALL[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    t = np.arange(p["n"])[:, None] / p["fs"]
    hi = vqt_oracle.setup(p["fs"], p["kw"].get("octaves", [1, 5]), p["kw"].get("a4_tuning", 440))[0]
    return rng.standard_normal((p["n"], p["c"])) + np.sin(2 * np.pi * hi / 3 * t) + 0.5 * np.cos(2 * np.pi * hi / 6 * t + 1.0)


def ratio_signal(n: int, complex_: bool = False) -> np.ndarray:
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal((n, 2))
    return x + 1j * rng.standard_normal((n, 2)) if complex_ else x


def subset(name: str):
    """(rows, samples) stored for a case too large to store whole: the top, middle and bottom row of every octave; the
    first and the last 64 samples and 64 spread between them."""
    p = ALL[name]
    octaves = p["kw"].get("octaves", [1, 5])
    bins = p["kw"].get("bins_per_octave", 24)
    rows = sorted({o * bins + r for o in range(octaves[1] - octaves[0] + 1) for r in (0, bins // 2, bins - 1)})
    n = p["n"]
    samples = sorted(set(range(min(64, n))) | set(range(max(0, n - 64), n)) | set(np.linspace(0, n - 1, 64).astype(int).tolist()))
    return np.array(rows), np.array(samples)


def n_rows(name: str) -> int:
    p = ALL[name]
    octaves = p["kw"].get("octaves", [1, 5])
    return (octaves[1] - octaves[0] + 1) * p["kw"].get("bins_per_octave", 24)


def stored_whole(name: str) -> bool:
    p = ALL[name]
    return 16 * n_rows(name) * p["n"] * p["c"] <= STORE_WHOLE_UP_TO


_expected = {}


def expected(name: str, f32: bool = False):
    """The oracle's (f, value, A, c) of a case, computed once; f32: of the samples rounded to float32."""
    key = (name, f32)
    if key not in _expected:
        x = signal(name)
        if f32:
            x = x.astype(np.float32).astype(np.float64)
        _expected[key] = vqt_oracle.vqt(x, ALL[name]["fs"], **ALL[name]["kw"])
    return _expected[key]
