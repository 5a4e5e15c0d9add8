"""The cases of the levels and loudness family (standard.normalize, rms, crest_factor, fade, apply_gain, detrend,
envelope, lufs_integrated; csrc/kernels_level.hpp): shared by tools/gen_golden_levels.py, which runs the reference on
them, and by tests/test_levels_host.py and tests/test_levels_gpu.py.  The inputs are rebuilt from their seeds: float32
values held in float64, so that a host signal and a device-resident one hold the same numbers."""

from collections import OrderedDict

import numpy as np

FS = 8000
# the kernels' constants (csrc/kernels_level.hpp); the host test compares them with the header and with backend.LEVEL_*
NT = 256
PER_LANE = 16
SPAN = NT * PER_LANE
TILE = 1024
VEC_BYTES = 16
MAX_ORDER = 8
U = 2.0 ** -53


def noise(seed, n, n_ch, offset=0.25, slope=0.2, curve=0.0, level=0.2):
    """Noise on a trend: per channel an offset, a slope and a cubic bend over the signal, so that the mean, the line and
    the higher orders all matter; float32 values in float64."""
    rng = np.random.default_rng(seed)
    t = np.linspace(-1.0, 1.0, n)[:, None] if n > 1 else np.zeros((1, 1))
    k = 1.0 + np.arange(n_ch)[None, :] / max(n_ch, 1)
    x = level * rng.standard_normal((n, n_ch)) + offset * k + slope * k * t + curve * (t ** 3 - 0.4 * t ** 2)
    return x.astype(np.float32).astype(np.float64)


def burst(seed, n, n_ch, stop):
    """Noise on a line up to sample `stop`, exact zeros behind it."""
    x = noise(seed, n, n_ch, offset=0.0, slope=0.0)
    x[stop:] = 0.0
    return x


# name -> (seed, n, n_ch, norm_dbfs, peak_normalization, each_channel)
NORMALIZE = OrderedDict([
    ("peak_all", (11, 1001, 2, -6.0, True, False)),
    ("peak_each", (12, 1001, 2, -1.5, True, True)),
    ("rms_all", (13, 1001, 2, -20.0, False, False)),
    ("rms_each", (14, 1001, 2, -23.0, False, True)),
])

# name -> (seed, n, n_ch, gain_db): one gain or one per channel
GAIN = OrderedDict([
    ("one", (21, 513, 2, -4.5)),
    ("each", (22, 513, 3, [3.0, -7.25, 0.0])),
])

# name -> (seed, n, n_ch, fade type name, length in samples (None: the default 2.5 %), at_start, at_end).  The length in
# seconds handed to fade is (samples + 0.5) / FS, which int() turns back into the samples.
FADE = OrderedDict([
    ("lin_both_default", (31, 1200, 2, "Linear", None, True, True)),
    ("exp_start", (32, 1000, 2, "Exponential", 300, True, False)),
    ("log_end", (33, 1000, 3, "Logarithmic", 301, False, True)),
    ("lin_one_sample", (34, 600, 1, "Linear", 1, True, True)),
    ("exp_all_but_one", (35, 601, 2, "Exponential", 600, True, True)),
    ("log_overlap", (36, 900, 2, "Logarithmic", 600, True, True)),
    ("no_fade", (37, 500, 2, "NoFade", 100, True, True)),
])


def fade_seconds(samples):
    return None if samples is None else (samples + 0.5) / FS


# detrend: every order on one signal with a bent trend
DETREND = (41, 1000, 2)
DETREND_ORDERS = tuple(range(MAX_ORDER + 1))


def detrend_input():
    seed, n, n_ch = DETREND
    return noise(seed, n, n_ch, curve=0.6)


# analytic envelope: lengths of fft64_cases.HILBERT_CASES, whose bound ds_hilbert is held to: name -> (seed, n, n_ch)
ENVELOPE_ANALYTIC = OrderedDict([("n4095", (51, 4095, 1)), ("n5000", (52, 5000, 1))])
# boxcar envelope: name -> (seed, n, n_ch, window, burst stop or None)
ENVELOPE_BOXCAR = OrderedDict([
    ("w1", (61, 1300, 1, 1, None)),
    ("w64", (62, 1300, 2, 64, None)),
    ("w300_burst", (63, 1300, 1, 300, 400)),
])


def boxcar_input(name):
    seed, n, n_ch, _, stop = ENVELOPE_BOXCAR[name]
    return noise(seed, n, n_ch) if stop is None else burst(seed, n, n_ch, stop)


# ---- loudness ------------------------------------------------------------------------------------------------------
LUFS_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)


def lufs_blocks(fs):
    tg = int(0.4 * fs + 0.5)
    return tg, int(0.25 * tg + 0.5)


def programme(seed, fs, n_ch, sections):
    """Sections of (samples, kind, amplitude): a 997 Hz tone (1 kHz would fold oddly at low rates) or noise; float32
    values in float64.  Channel c is scaled by 1 - 0.1 c."""
    rng = np.random.default_rng(seed)
    parts, start = [], 0
    for n, kind, amp in sections:
        t = (start + np.arange(n)) / fs
        parts.append(amp * np.sin(2 * np.pi * 997.0 * t) if kind == "tone" else amp * rng.standard_normal(n))
        start += n
    x = np.concatenate(parts)[:, None] * (1.0 - 0.1 * np.arange(n_ch))[None, :]
    return x.astype(np.float32).astype(np.float64)


_TG8, _STEP8 = lufs_blocks(8000)
# name -> (seed, fs, n_ch, sections)
LUFS = OrderedDict([
    ("programme_11025", (71, 11025, 1, [(9000, "tone", 0.5), (8000, "tone", 0.02), (5000, "noise", 1e-5), (8000, "tone", 0.3)])),
    ("programme_8000", (72, 8000, 2, [(5000, "tone", 0.5), (4000, "tone", 0.02), (5000, "noise", 1e-5), (6000, "tone", 0.3)])),
])
# the lengths around one block at 8000 Hz: no block, no block, one, one (the second full block is lost to the ceil), two
LUFS_EDGE_LENGTHS = (_TG8 - 1, _TG8, _TG8 + 1, _TG8 + _STEP8, _TG8 + _STEP8 + 1)
for _n_ch in (2, 5):
    for _n in LUFS_EDGE_LENGTHS:
        LUFS[f"edge_{_n}_{_n_ch}ch"] = (73 + _n_ch, 8000, _n_ch, [(_n, "tone", 0.25)])


def lufs_input(name):
    seed, fs, n_ch, sections = LUFS[name]
    return programme(seed, fs, n_ch, sections), fs


# the wrong oracles the generator shows to miss their bound: family -> what is wrong
WRONG_ORACLES = OrderedDict([
    ("rms", "the mean is not removed"),
    ("fade", "the start and the end of the fade are swapped"),
    ("lufs", "the block is taken as four steps at 11025 Hz (4412 samples, not 4410)"),
    ("envelope", "the line is not removed"),
])
