"""normalize, fade, rms, crest_factor, apply_gain and lufs_integrated (API mirror of dsptoolbox/standard/gain_and_level.py).

Every per-sample operation runs on the device in float64 (csrc/kernels_level.hpp); there is no host path.  A host signal
goes up once as (samples, channels) float64 and its result comes down once; a device-resident signal is read where it
lies.  Results that are signals (normalize, fade, apply_gain) of a resident signal stay resident, as a new float32
planar buffer; the measures (rms, crest_factor, lufs_integrated) bring down a few numbers per channel.  The host keeps
what the reference does on a handful of values: decibel conversions, the fade table (built by the reference's numpy
expressions, so the faded samples agree bit for bit), the two gates of the loudness measure.

Kept from the reference: rms, crest_factor and RMS normalisation use numpy's std, the centred value (with
`each_channel=False` one mean over all channels); a silent channel normalises to inf / NaN samples; fade with both ends
applies both tables to the same samples, the start first; lufs_integrated returns NaN when the signal holds no block.
`crest_factor(use_true_peak=True)` needs the resampler, which is not built."""

from __future__ import annotations

import numpy as np

from .. import backend
from .._lib import DevicePlanar
from .._db import from_db, to_db
from .enums import BiquadEqType, FadeType

__all__ = ["normalize", "fade", "rms", "crest_factor", "apply_gain", "lufs_integrated"]


def _samples(sig):
    return sig.device_samples if sig.on_device else sig.time_data


def _result(sig, y):
    return sig._device_result(y) if isinstance(y, DevicePlanar) else sig.copy_with_new_time_data(y)


def _bands(sig, function, *args):
    """A MultiBandSignal of function(band, *args) for every band (no band is copied first: resident bands stay where
    they are)."""
    from ..classes import MultiBandSignal
    return MultiBandSignal([function(b, *args) for b in sig.bands], sig.same_sampling_rate, dict(sig.info))


def normalize(sig, norm_dbfs: float, peak_normalization: bool = True, each_channel: bool = False):
    """Normalise a Signal or every band of a MultiBandSignal to `norm_dbfs`: at the peak, or at the (centred) RMS value;
    each channel on its own, or all by the peak / RMS value over all channels."""
    from ..classes import MultiBandSignal, Signal
    if isinstance(sig, Signal):
        norm = ("peak_" if peak_normalization else "rms_") + ("each" if each_channel else "all")
        return _result(sig, backend.level_apply(_samples(sig), norm=norm, norm_factor=from_db(norm_dbfs, True)))
    if isinstance(sig, MultiBandSignal):
        return _bands(sig, normalize, norm_dbfs, peak_normalization, each_channel)
    raise TypeError("Type of signal is not valid. Use either Signal or MultiBandSignal")


def _fade_table(fade_type: FadeType, l_samples: int) -> np.ndarray:
    """The rising fade of `l_samples` values, by the numpy expressions of the reference (helpers/gain_and_level.py)."""
    if fade_type == FadeType.Exponential:
        return 10 ** (np.linspace(-100, 0, l_samples) / 20)
    if fade_type == FadeType.Linear:
        return np.linspace(0, 1, l_samples)
    if fade_type == FadeType.Logarithmic:
        table = np.log10(np.linspace(1, 50 * 10**0.5, l_samples))
        table /= table[-1]
        return table
    raise ValueError("No valid fade")


def fade(sig, fade_type: FadeType, length_fade_seconds: float | None = None, at_start: bool = True, at_end: bool = True):
    """Fade the start, the end or both of a Signal in or out over `length_fade_seconds` (default: 2.5 % of the signal)."""
    assert at_start or at_end, "At least start or end of signal should be faded"
    if length_fade_seconds is None:
        length_fade_seconds = sig.time_vector_s[-1] * 0.025
    assert length_fade_seconds < sig.time_vector_s[-1], "Fade length should not be longer than the signal itself"
    l_samples = 0
    if fade_type != FadeType.NoFade:
        assert length_fade_seconds > 0, "Only positive lengths"
        l_samples = int(length_fade_seconds * sig.sampling_rate_hz)
        assert len(sig) > l_samples, "Signal is shorter than the desired fade"
        table = _fade_table(fade_type, l_samples)
    if l_samples == 0:  # nothing to multiply: a copy -- made where the samples are, a host signal's without the device
        return _result(sig, backend.level_apply(sig.device_samples)) if sig.on_device \
            else sig.copy_with_new_time_data(sig.time_data.copy())
    return _result(sig, backend.level_apply(_samples(sig), fade=table, at_start=at_start, at_end=at_end))


def _per_band(sig, measure) -> np.ndarray:
    """measure(signal) -> (channels,) of a Signal, or stacked to (bands, channels) over a MultiBandSignal."""
    from ..classes import MultiBandSignal, Signal
    if isinstance(sig, Signal):
        return measure(sig)
    if isinstance(sig, MultiBandSignal):
        return np.stack([measure(b) for b in sig.bands]).reshape(sig.number_of_bands, sig.number_of_channels)
    raise TypeError("Passed signal should be either a Signal or MultiBandSignal type")


def _rms_and_peak(sig) -> tuple:
    """Per channel sqrt(mean (x - mean)^2) and max |x|, from one pass pair on the device."""
    stats = backend.level_stats(_samples(sig), 0)
    return np.sqrt(stats[:, 0] / len(sig)), stats[:, 2]


def rms(sig, in_dbfs: bool = True) -> np.ndarray:
    """The RMS value (numpy's std) of every channel, (channels,) or (bands, channels), in dBFS or linear."""
    values = _per_band(sig, lambda s: _rms_and_peak(s)[0])
    return np.atleast_1d(20.0 * np.log10(values) if in_dbfs else values)


def crest_factor(sig, in_db: bool = True, use_true_peak: bool = False) -> np.ndarray:
    """Peak over RMS value of every channel, (channels,) or (bands, channels), in dB or as a ratio."""
    if use_true_peak:
        raise NotImplementedError("crest_factor: the true peak needs the resampler (standard.resample), which is not built")

    def ratio(s):
        values, peak = _rms_and_peak(s)
        return peak / values

    from ..classes import MultiBandSignal
    crest = _per_band(sig, ratio)
    if in_db:
        crest = to_db(crest, True)
        if isinstance(sig, MultiBandSignal):  # kept from the reference: it converts the bands' values, then the table again
            crest = to_db(crest, True)
    return np.atleast_1d(crest)


def _scaled_filter(filt, factor):
    """A copy of the filter with `factor` on its numerator: the gain of a zpk form, and the last section of an sos form
    or, without one, the b coefficients."""
    out = filt.copy()
    if out.has_zpk:
        z, p, k = out.zpk
        out.zpk = [z, p, k * factor]
    if out.has_sos:
        sos = out.sos.copy()
        sos[-1, :3] = sos[-1, :3] * factor
        out.sos = sos
    else:
        b, a = out.ba
        out.ba = [b * factor, a]
    return out


def apply_gain(target, gain_db):
    """Gain in dB on a Signal or MultiBandSignal (one value, or one per channel) or on the coefficients of a Filter or
    of the filters of a FilterBank (one value, or one per filter)."""
    from ..classes import Filter, FilterBank, MultiBandSignal, Signal
    factors = from_db(np.atleast_1d(gain_db), True)
    if isinstance(target, Signal):
        if len(factors) not in (1, target.number_of_channels):
            raise ValueError(f"{len(factors)} gains do not match {target.number_of_channels} channels")
        imaginary = target.time_data_imaginary if target.is_complex_signal else None
        new_sig = _result(target, backend.level_apply(_samples(target), gain=factors))
        if imaginary is not None:
            new_sig.time_data_imaginary = backend.level_apply(imaginary, gain=factors)
        return new_sig
    if isinstance(target, MultiBandSignal):
        return _bands(target, apply_gain, gain_db)
    if isinstance(target, Filter):
        return _scaled_filter(target, factors[0] if len(factors) == 1 else factors)
    if isinstance(target, FilterBank):
        assert len(factors) in (1, target.number_of_filters), "one gain, or one per filter of the bank"
        new_bank = target.copy()
        new_bank.filters = [_scaled_filter(f, g) for f, g in zip(target.filters, np.broadcast_to(factors, (target.number_of_filters,)))]
        return new_bank
    raise TypeError("No valid type was passed")


# Rec. ITU-R BS.1770-5: block length and overlap, gates, channel weights (L, R, C, Ls, Rs)
_LUFS_BLOCK_S = 400e-3
_LUFS_OVERLAP = 0.75
_LUFS_GATE_ABSOLUTE = -70
_LUFS_GATE_RELATIVE = 10
_LUFS_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)


def _k_weighting_sos(fs_hz: int) -> np.ndarray:
    """The two biquads of the K-weighting at any rate: the high shelf of the head, the RLB high pass."""
    from ..classes import Filter
    from .other import merge_filters
    k_filter = merge_filters([
        Filter.biquad(eq_type=BiquadEqType.Highshelf, frequency_hz=1500, gain_db=4.0, q=2**0.5 / 2.0, sampling_rate_hz=fs_hz),
        Filter.biquad(eq_type=BiquadEqType.Highpass, frequency_hz=38.1, gain_db=0.0, q=0.5, sampling_rate_hz=fs_hz)])
    return k_filter.sos


def _lufs_blocks(fs_hz: int) -> tuple:
    """(block, step) in samples; the block is not always four steps (11025 Hz: 4410 and 1103)."""
    block = int(_LUFS_BLOCK_S * fs_hz + 0.5)
    return block, int((1.0 - _LUFS_OVERLAP) * block + 0.5)


def _lufs_gating(z: np.ndarray) -> float:
    """The integrated loudness from the block mean squares z (blocks, channels): absolute gate, relative gate, mean."""
    weights = np.array(_LUFS_WEIGHTS)[: z.shape[1]]

    def loudness(power):
        return -0.691 + 10.0 * np.log10(power @ weights)

    with np.errstate(divide="ignore", invalid="ignore"):
        if z.shape[0] == 0:
            return float("nan")
        block_loudness = loudness(z)
        gate = loudness(np.mean(z[block_loudness > _LUFS_GATE_ABSOLUTE, :], axis=0)) - _LUFS_GATE_RELATIVE
        return float(loudness(np.mean(z[block_loudness > max(gate, _LUFS_GATE_ABSOLUTE), :], axis=0)))


def lufs_integrated(s) -> float:
    """Integrated loudness in LUFS after Rec. ITU-R BS.1770-5, for up to 5 channels in the order L, R, C, Ls, Rs.  The
    K-weighting is designed at the signal's rate from the biquad parameters of the 48 kHz coefficients."""
    assert s.number_of_channels <= 5, "Not implemented for more channels than 5"
    fs_hz = s.sampling_rate_hz
    block, step = _lufs_blocks(fs_hz)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (the mean of no block: NaN, as the reference returns)
        return _lufs_gating(backend.loudness_blocks(_samples(s), _k_weighting_sos(fs_hz), block, step))
