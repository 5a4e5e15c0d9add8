"""The cases of the resampler tests (tests/test_resample_host.py, tests/test_resample_gpu.py, the emulation
tests/host_san/resample_plan_san.cpp) and of tools/gen_golden_resample.py, which runs the reference's `resample` on
GOLDEN and writes tests/golden/resample/cases.npz.

Every ratio is run at the LENGTHS and, per channel count, at the lengths on either side of the edge of the kernel's output
tile (csrc/resample_plan.hpp, restated by plan() below and compared with the header by the host test): the longest input
whose output stays below one tile, the shortest that fills it and the shortest that goes past it.  Where up > down not
every output length exists, and the second and third may be one length."""

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "resample", "cases.npz")

NT, PASSES, LDS_DOUBLES, MAX_RATE = 256, 4, 20480, 640  # csrc/resample_plan.hpp

# the last is the one ratio here whose sums run in several chunks (12801 terms: the window is staged 3 to 11 times)
RATIOS = [(3, 2), (2, 3), (7, 5), (160, 147), (147, 160), (80, 441), (640, 147), (147, 640), (1, 2), (2, 1), (1, 50), (100, 1),
          (1, 640)]
LENGTHS = [1, 2, 20, 21, 257, 1000]
CHANNELS = [1, 2, 3, 5]
RESIDENT_RATIOS = [(160, 147), (147, 160), (80, 441)]


def ch_group(n_ch: int) -> int:
    return 1 if n_ch == 1 else 2 if n_ch == 2 else 4


def terms(up: int, down: int) -> int:
    """J: the terms of one output at most, ceil((20 r + 1) / up)"""
    return -(-(20 * max(up, down) + 1) // up)


def plan(up: int, down: int, n_ch: int) -> dict:
    """make_plan of the header"""
    cg, j = ch_group(n_ch), terms(up, down)
    js = j | 1
    w = (LDS_DOUBLES - up * js) // cg

    def adv(tile):
        return -(-(tile - 1) * down // up)

    tile = PASSES * NT // cg
    while tile > 1 and adv(tile) + j > w and adv(tile) > w // 2:
        tile >>= 1
    jc = min(j, w - adv(tile))
    return dict(cg=cg, J=j, JS=js, tile=tile, adv=adv(tile), jc=jc, chunks=-(-j // jc), span=adv(tile) + jc,
                lds_bytes=8 * (up * js + (adv(tile) + jc) * cg))


def n_out(n: int, up: int, down: int) -> int:
    return -(-n * up // down)


def edge_lengths(up: int, down: int, n_ch: int) -> list:
    tile = plan(up, down, n_ch)["tile"]
    fills = -(-(tile - 1) * down // up) + 1 if tile > 1 else 1  # the shortest n with n_out >= tile: n up > (tile - 1) down
    while n_out(fills, up, down) < tile:
        fills += 1
    while fills > 1 and n_out(fills - 1, up, down) >= tile:
        fills -= 1
    past = fills
    while n_out(past, up, down) <= tile:
        past += 1
    return sorted({n for n in (fills - 1, fills, past) if n >= 1})


def lengths(up: int, down: int, n_ch: int) -> list:
    return sorted(set(LENGTHS) | set(edge_lengths(up, down, n_ch)))


def all_lengths(up: int, down: int) -> list:
    return sorted(set().union(*(lengths(up, down, c) for c in CHANNELS)))


def signal(n: int, n_ch: int = 5, seed: int = 0) -> np.ndarray:
    """(n, n_ch) float64 holding float32 values: noise on an offset.  The first columns of a wider signal of the same
    length and seed are the same numbers."""
    rng = np.random.default_rng(7000 + 13 * seed + n)
    x = 0.25 * rng.standard_normal((n, 5)) + 0.1
    return x.astype(np.float32).astype(np.float64)[:, :n_ch].copy()


# ---- the cases run through the reference: name -> (fs, new fs, type, rescaling, constrain_amplitude) ------------------
# (constrain_amplitude None: the type's default, False for a Signal and True for an ImpulseResponse)
GOLDEN_N, GOLDEN_CH = 1500, 2
GOLDEN = {
    "up_44100_48000": (44100, 48000, "Signal", False, None),
    "down_48000_44100": (48000, 44100, "Signal", False, None),
    "third_48000_16000": (48000, 16000, "Signal", False, None),
    "triple_16000_48000": (16000, 48000, "Signal", False, None),
    "down_44100_8000": (44100, 8000, "Signal", False, None),
    "rescaled_44100_48000": (44100, 48000, "Signal", True, None),
    "ir_48000_44100": (48000, 44100, "ImpulseResponse", False, None),
    # the input's peak is just below 1 and the filter's ringing takes the output past it: the constraint normalises
    "overshoot_44100_48000": (44100, 48000, "Signal", False, True),
}


def golden_signal(name: str) -> np.ndarray:
    kind = GOLDEN[name][2]
    x = signal(GOLDEN_N, GOLDEN_CH, seed=1 + list(GOLDEN).index(name))
    if kind == "ImpulseResponse":  # a decaying response
        x = x * np.exp(-np.arange(GOLDEN_N) / 200.0)[:, None]
        x = x.astype(np.float32).astype(np.float64)
    if name.startswith("overshoot"):  # a square wave at a quarter of Nyquist on a little noise, peak 0.999
        sq = np.sign(np.sin(2 * np.pi * np.arange(GOLDEN_N) / 16.0 + 0.1))[:, None]
        x = sq + 0.01 * x
        x = (0.999 * x / np.abs(x).max()).astype(np.float32).astype(np.float64)
    return x


def golden_input(dsp, name: str):
    """the case's input as an object of the package `dsp` (this one, or the reference)"""
    fs, _, kind, _, constrain = GOLDEN[name]
    kw = {} if constrain is None else dict(constrain_amplitude=constrain)
    return getattr(dsp, kind)(None, golden_signal(name), fs, **kw)
