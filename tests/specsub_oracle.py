"""Long-double restatement of effects.SpectralSubtractor, written from the behaviour the issue lists and the reference
shows when it is run.  What the host builds as tables comes in as float64 values (the clipped window of scipy, a given
spectrum); every sample operation is np.longdouble, the transform included: a radix-2 one of its own, since numpy's FFT
may compute in double.  Besides the result, `subtract` returns what decides a comparison discretely:
  gate margins   |level - threshold| in dB of every (frame, channel), level = 10 log10(max(var, tiny));
  clip margins   of every bin with max(|X|^e, t) > 0 the value (|X|^e - t) / max(|X|^e, t): positive for a bin that is
                 not clipped -- then it is the issue's (|X|^e - t) / |X|^e -- and negative for a clipped one.
A case is only used when no gate margin is below MARGIN_DB and no clip margin, of either sign, is nearer to 0 than
MARGIN_CLIP (the issue asks this of the unclipped bins; the clipped ones are held to it as well, since a bin that is
clipped by a hair in one arithmetic is unclipped by a hair in another).

The bound.  error = max |got - want| per channel over that channel's peak (fx_oracle.stream_error).  A result passes
within max(4 x the reference's own error on that case, FLOOR(W)), FLOOR(W) = C log2(W) 2^-53, u = 2^-53:
  * transforms: a radix-2 transform of N points in floating point has the norm-wise forward error log2(N) eta,
    eta = mu + gamma_4 (sqrt 2 + mu) with twiddles good to mu = u and gamma_4 = 4 u, so eta = 6.7 u (Higham, Accuracy and
    Stability of Numerical Algorithms, theorem 24.2).  The packed real transform is log2(W) - 1 such stages and the
    split, the inverse the same: 2 x 6.7 = 13.4 log2(W) u of the frame's l2 norm; the transform is unitary up to its
    scale, so per sample that is 13.4 log2(W) u of the frame's RMS, which is at most the channel's peak;
  * overlap-add: sample y = (sum_f v_f w_f) / (sum_f w_f^2) over K <= 4 covering frames; an error d in every v_f arrives
    as d (sum w_f) / (sum w_f^2).  For the Hann window at 50 % and 75 % overlap, the shapes held to the floor alone,
    sum w = 1 and 2, sum w^2 >= 0.5 and = 1.5: a factor of at most 2.  The sums and the division add (2 K + 1) u <= 9 u;
  * per bin: sqrt, the subtraction, the root and the scaling are about 6 u of the bin, plus u / (2 sqrt(m)) from the
    cancellation at a clip margin m; only bins near the noise level come near the clip, and in the cases the noise is
    1 % of the peak: under one more log2(W) u of the peak.  The adaptive average is contractive (forgetting factor 0.9:
    ten roundings' worth of the noise level), the peak restore two more roundings.
  Together 2 x 13.4 + 9 / log2(W) + 1 + ... <= 38 log2(W) u for W >= 4; C = 40.
Windows whose overlap-added square comes near zero inside the kept samples (no overlap, 30 % overlap) amplify every
rounding, the reference's as much as the device's, far beyond the floor: those are golden cases, where four times the
reference's recorded error is the larger bound."""

import numpy as np

import fx_oracle as fo

LD = np.longdouble
C = 40.0
MARGIN_DB = 1e-6
MARGIN_CLIP = 1e-6
TINY = np.finfo(np.float64).tiny
PI = 4 * np.arctan(LD(1))
stream_error = fo.stream_error


def floor(window: int) -> float:
    return C * np.log2(window) * 2.0 ** -53


def bound(window: int, reference_error: float = 0.0) -> float:
    return max(4 * reference_error, floor(window))


def fft(x, inverse: bool = False):
    """Radix-2 decimation in time over axis 0 in complex long double (unnormalised in both directions)."""
    x = np.asarray(x, dtype=np.clongdouble)
    n = x.shape[0]
    assert n >= 1 and n & (n - 1) == 0
    if n == 1:
        return x.copy()
    even, odd = fft(x[0::2], inverse), fft(x[1::2], inverse)
    k = np.arange(n // 2, dtype=LD)
    ang = (2 if inverse else -2) * PI * k / n
    w = (np.cos(ang) + 1j * np.sin(ang)).reshape((-1,) + (1,) * (x.ndim - 1))
    return np.concatenate([even + w * odd, even - w * odd])


def rfft(x):
    return fft(x)[: x.shape[0] // 2 + 1]


def irfft(spec):
    """numpy's irfft: the imaginary parts of the first and the last bin do not count."""
    spec = np.array(spec, dtype=np.clongdouble)
    spec[0], spec[-1] = spec[0].real, spec[-1].real
    full = np.concatenate([spec, np.conj(spec[-2:0:-1])])
    return fft(full, inverse=True).real / full.shape[0]


def closest_power_of_2(number) -> int:
    p = np.log2(number)
    return int(2 ** (int(np.floor(p)) if p - int(p) < 0.5 else int(np.ceil(p))))


def frames_of(td, window: int, step: int):
    """(W, ceil(L / step), C): the frames of `td`, zero-padded at the end."""
    length, n_ch = td.shape
    n_frames = -(-length // step)
    padded = np.zeros(((n_frames - 1) * step + window, n_ch), dtype=LD)
    padded[:length] = td
    return np.stack([padded[f * step: f * step + window] for f in range(n_frames)], axis=1)


def welch_psd(x, window, window_length: int, overlap_percent: float):
    """What the reference's Welch estimate returns for FFTBackward scaling, which it counts among the amplitude scalings:
    the ROOT of the mean squared magnitude (the mean of every windowed frame removed first).  The subtractor raises it to
    e / 2 all the same ("it is already raised to the power of 2"): kept."""
    step = window_length - int(overlap_percent / 100 * window_length)
    fr = frames_of(np.asarray(x, dtype=LD)[:, None], window_length, step) * np.asarray(window, dtype=LD)[:, None, None]
    fr = fr - np.mean(fr, axis=0)
    return np.sqrt(np.mean(np.abs(rfft(fr)) ** 2, axis=1)[:, 0])


def subtract(x, window, step: int, mode: str, threshold_db=-40.0, forgetting=0.9, factor=2.0, exponent=2.0, table=None,
             env_floor=None):
    """x (n, C) -> (y (n, C) long double, gate margins (F, C) in dB, clip margins: a flat array).  window: the clipped
    float64 window; table (bins,) or (C, bins): |PSD|^(e / 2) in long double or float64 (static mode)."""
    x = np.asarray(x, dtype=LD)
    x = x[:, None] if x.ndim == 1 else x
    n, n_ch = x.shape
    w = np.asarray(window, dtype=LD)
    W = len(w)
    e, ff, fac = LD(exponent), LD(forgetting), LD(factor)
    padded = np.zeros((n + 2 * W, n_ch), dtype=LD)
    padded[W:W + n] = x
    fr = frames_of(padded, W, step)
    F = fr.shape[1]
    var = np.mean((fr - np.mean(fr, axis=0)) ** 2, axis=0)
    level = 10 * np.log10(np.maximum(var, LD(TINY)))
    gate = level < threshold_db
    spec = rfft(fr * w[:, None, None])
    mag = np.abs(spec)
    power = mag ** e
    if mode == "adaptive":
        term = np.zeros_like(power)
        for c in range(n_ch):
            noise = np.zeros(W // 2 + 1, dtype=LD)
            for f in range(F):
                if gate[f, c]:
                    noise = noise * ff + mag[:, f, c] * (1 - ff)
                term[:, f, c] = fac * noise ** e
    else:
        t = np.asarray(table, dtype=LD)
        term = np.broadcast_to(fac * np.broadcast_to(t, (n_ch, W // 2 + 1)).T[:, None, :], power.shape)
    rest = power - term
    scale = np.maximum(power, term)
    clip_margins = (rest[scale > 0] / scale[scale > 0]).astype(np.float64)
    now = np.maximum(rest, 0) ** (1 / e)
    phase = np.where(mag > 0, spec / np.where(mag > 0, mag, 1), 1)
    out = irfft(now * phase) * w[:, None, None]
    total = (F - 1) * step + W
    td, env = np.zeros((total, n_ch), dtype=LD), np.zeros(total, dtype=LD)
    for f in range(F):
        td[f * step: f * step + W] += out[:, f]
        env[f * step: f * step + W] += w * w
    if env_floor is not None:
        env = np.maximum(env, LD(env_floor))
    ok = env > TINY
    td[ok] /= env[ok, None]
    y = td[W:W + n]
    with np.errstate(all="ignore"):
        y = y * (np.max(np.abs(x), axis=0) / np.max(np.abs(y), axis=0))
    return y, np.abs(level - threshold_db).astype(np.float64), clip_margins


def detector_table(x, fs, window_type_window, window_length: int, overlap_percent: float, threshold_db, release_ms, exponent):
    """(C, bins) |PSD|^(e / 2) of every channel's noise part as static mode finds it: the activity detector's mask
    (fx_oracle.detect; the nearest level to its threshold comes back too) and the Welch estimate with the UNCLIPPED
    window `window_type_window`."""
    x = np.asarray(x, dtype=LD)
    rows, nearest = [], np.inf
    for c in range(x.shape[1]):
        mask, near = fo.detect(x[:, c], fs, threshold_db, True, release_ms)
        nearest = min(nearest, near)
        rows.append(np.abs(welch_psd(x[~mask, c], window_type_window, window_length, overlap_percent)) ** (LD(exponent) / 2))
    return np.stack(rows), nearest
