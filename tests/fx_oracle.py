"""Long-double restatement of the audio effects' recursions (effects.Compressor, DigitalDelay, Chorus, Distortion,
Tremolo and the gate of standard.activity_detector), written from the behaviour the issue describes and the reference
shows when it is run.  What the host builds as small tables -- follower coefficients, linear levels and offsets, the
chorus index table, the modulator -- comes in as float64 values; every sample operation is np.longdouble.

BOUND = 1e-12 of each channel's peak is what the reference and the device are both held to.  The follower maps are
contractive, so the rounding of one float64 step, about 3 * 2^-53 g, accumulates to at most 3 * 2^-53 / c_min: 5e-14 at
the smallest coefficient of the cases, c_min >= 0.007 (tools/gen_golden_fx.py asserts it).  The rest of the margin covers
one- or two-ulp log10, pow and atan and the RMS restore."""

import numpy as np

LD = np.longdouble
BOUND = 1e-12
C_MIN = 0.007


def stream_error(got, want) -> float:
    """Largest deviation in units of its channel's peak; non-finite values must sit at the same places."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~np.isfinite(want)
    if bad.any():
        assert np.array_equal(bad, ~np.isfinite(got)), "non-finite values at different places"
        got, want = np.where(bad, 0, got), np.where(bad, 0, want)
    peak = np.max(np.abs(want), axis=0)
    peak = np.where(peak > 0, peak, 1)
    return float(np.max(np.abs(got - want) / peak))


def coefficient(samples) -> float:
    """float64, as the host computes it: 1 - exp(ln 0.05 / samples), 1 for 0 samples."""
    with np.errstate(divide="ignore"):
        return float(1 - np.exp(np.log(1 - 0.95) / np.float64(samples)))


def knee(d, T, R, W, downward: bool, unreachable_branch: bool = False):
    """The compression curve in dB the reference's loop reaches (its array branch).  unreachable_branch: the formula of
    its `type(x) is float` branch instead, which differs in the knee section (a deliberately wrong oracle)."""
    T, R, W = LD(T), LD(R), LD(W)
    y = LD(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if downward:
            if d - T < -W / 2:
                y = d
            if abs(d - T) <= W / 2:
                y = d - (1 / R - 1) * (d - T - W / 2) ** 2 / 2 / W if unreachable_branch else \
                    d + (1 / R - 1) * (d - T + W / 2) ** 2 / 2 / W
            if d - T > W / 2:
                y = T + (d - T) / R
        else:
            if d - T < -W / 2:
                y = T + (d - T) / R
            if abs(d - T) <= W / 2:
                y = d - (1 / R - 1) * (d - T - W / 2) ** 2 / 2 / W
            if d - T > W / 2:
                y = d
    return y


def std(td):
    td = np.asarray(td, dtype=LD)
    return np.sqrt(np.mean((td - np.mean(td, axis=0)) ** 2, axis=0))


def compress(x, fs, threshold_dbfs=-10, attack_time_ms=0.5, release_time_ms=20, ratio=3, relative=True, knee_db=0,
             pre_gain_db=0, post_gain_db=0, make_up=True, downward=True, wrong=None):
    """-> (y, the smallest |level - threshold| in dB over the samples).  wrong: None, or one of the deliberately wrong
    variants 'swap' (attack and release exchanged), 'knee' (the unreachable knee branch), 'post' (the final gain taken
    from post_gain_db)."""
    pre = LD(10 ** (pre_gain_db / 20))
    td = np.asarray(x, dtype=LD) * pre
    rms, peak = std(td), np.max(np.abs(td), axis=0)
    if relative:
        td = td / peak
    ca = LD(coefficient(int(attack_time_ms * 1e-3 * fs)))
    cr = LD(coefficient(int(release_time_ms * 1e-3 * fs)))
    if wrong == "swap":
        ca, cr = cr, ca
    floor = LD(10 ** (-300.0 / 10))
    out = np.empty_like(td)
    nearest = np.inf
    for ch in range(td.shape[1]):
        g = LD(1)
        for i in range(td.shape[0]):
            samp = td[i, ch] ** 2
            d = 10 * np.log10(max(samp, floor))
            nearest = min(nearest, abs(float(d) - threshold_dbfs))
            f = LD(10) ** ((knee(d, threshold_dbfs, ratio, knee_db, downward, wrong == "knee") - d) / 20)
            c = ca if f > g else cr
            g = c * f + (1 - c) * g
            out[i, ch] = td[i, ch] * g
    if relative:
        out = out * peak
    if make_up:
        out = out * (rms / std(out))
    return out * (LD(10 ** (post_gain_db / 20)) if wrong == "post" else pre), nearest


def detector_coefficient(time_ms, fs) -> float:
    with np.errstate(divide="ignore"):
        return float(1 - np.exp(np.log(1 - 0.95) / (time_ms / 1e3) / fs))


def detect(x, fs, threshold_dbfs=-20, relative=True, release_time_ms=25):
    """x (N,) one channel -> (mask (N,) bool, the smallest |10 log10 g - threshold| in dB)."""
    td = np.asarray(x, dtype=LD)
    if relative:
        td = td / np.max(np.abs(td))
    p = td ** 2
    cr = LD(detector_coefficient(release_time_ms, fs))
    g = np.zeros(len(p), dtype=LD)
    for i in range(1, len(p)):
        c = cr if p[i - 1] > 0 else LD(0)
        g[i] = c * p[i] + (1 - c) * g[i - 1]
    with np.errstate(divide="ignore"):
        level = 10 * np.log10(g)
    finite = np.isfinite(level)
    nearest = float(np.min(np.abs(level[finite] - threshold_dbfs))) if finite.any() else np.inf
    return level > threshold_dbfs, nearest


def delay_lengths(fs, delay_ms, feedback):
    d = int(np.round(delay_ms * 1e-3 * fs))
    return d, int(d * (1 + feedback * 15))


def delay_samples(x, d: int, pad: int, feedback, saturation="digital"):
    """The delay line with the delay and the padding in samples."""
    x = np.asarray(x, dtype=LD)
    peak = np.max(np.abs(x), axis=0)
    td = np.concatenate([x, np.zeros((pad, x.shape[1]), dtype=LD)])
    fb = LD(feedback)
    for i in range(d, len(td)):
        v = td[i - d].copy()  # (with d = 0 the sample itself, before it is overwritten)
        td[i] = td[i] + fb * (v if saturation == "digital" else LD(0.5) * np.arctan(2 * v))
    with np.errstate(divide="ignore", invalid="ignore"):
        return td * (peak / np.max(np.abs(td), axis=0))


def delay(x, fs, delay_ms=300, feedback=0.1, saturation="digital"):
    return delay_samples(x, *delay_lengths(fs, delay_ms, feedback), feedback, saturation)


def chorus(x, delays, mix):
    """delays (N, V) integer samples: the index table the host builds."""
    x = np.asarray(x, dtype=LD)
    n = len(x)
    max_delay = int(np.abs(delays).max())
    td = np.concatenate([x, np.zeros((max_delay, x.shape[1]), dtype=LD)])
    peak = np.max(np.abs(td), axis=0)
    new = np.zeros_like(td)
    for i in range(n):
        new[i] = td[i]
        for v in range(delays.shape[1]):
            new[i] = new[i] + td[i + int(delays[i, v])]  # (a negative index counts from the end)
    new = (new * LD(mix) + td * LD(1 - mix))[:n]
    return new * (peak / np.max(np.abs(new), axis=0))


def _clip(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def curve(kind: str, x, level, offset):
    """level and offset linear float64 (the host's 10 ** (dB / 20))."""
    level, offset = LD(level), LD(offset)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = x / np.max(np.abs(x), axis=0)
        if kind == "Arctan":
            return np.arctan(norm * level + offset) * (2 / LD(np.pi))
        if kind == "HardClip":
            return _clip(norm * level + offset, LD(-1), LD(1))
        if kind == "SoftClip":
            u = (norm * LD(2 / 3) + offset) * level
            return _clip(u - u ** 3 / 3, LD(-2 / 3), LD(2 / 3))
    assert kind == "NoDistortion", kind
    return x


def distort(x, kinds, levels_db, mixes, offsets_db, post_gain_db=0):
    """kinds: DistortionType names; mixes as fractions."""
    x = np.asarray(x, dtype=LD)
    peak = np.max(np.abs(x), axis=0)
    out = np.zeros_like(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        for kind, lv, w, off in zip(kinds, levels_db, mixes, offsets_db):
            if w == 0.0:
                continue
            comp = curve(kind, x, 10 ** (np.float64(lv) / 20), 10 ** (np.float64(off) / 20)) * LD(w)
            out = out + comp * (peak / np.max(np.abs(comp), axis=0))
    return out * LD(10 ** (post_gain_db / 20))


def tremolo(x, modulator):
    return np.asarray(x, dtype=LD) * np.asarray(modulator, dtype=LD)[:, None]
