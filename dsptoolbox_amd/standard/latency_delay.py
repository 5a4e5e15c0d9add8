"""latency, fractional_delay and delay (API mirror of dsptoolbox/standard/latency_delay.py).

latency: the cross-correlation of every channel pair is formed, searched for its peak and, for the sub-sample form,
Hilbert-transformed around the peaks on the device (backend.latency_peaks); the host turns the 2 p + 2 values per
channel that come down into the root (backend._fractional_index) and picks the correlation coefficient of the rounded
lag.  delay is host arithmetic.

fractional_delay: the Kaiser-windowed sinc filter of every delayed channel is built on the device (k_delay_taps)
and applied there in float64 (k_delay_sum); the host only splits the delay into its integer part and fraction, with
the reference's float64 operations.  Output lengths, the pass-through of a zero delay, the zero padding of channels
left out of `channels` and the normalisation of constrained signals are the reference's."""

from __future__ import annotations

from warnings import warn

import numpy as np

from .. import backend


def _delay_rows(n_ch: int, channels, delay_samples: float, order: int):
    """Per channel: (shift, frac) of the reference's output -- the filtered channels move by integer_delay,
    the others pass through unshifted.  Returns (shift, frac, integer_delay)."""
    integer_delay, frac = backend._delay_split(delay_samples, order)
    shift = np.zeros(n_ch, dtype=np.int64)
    fr = np.full(n_ch, -1.0)
    shift[channels] = integer_delay
    fr[channels] = frac
    return shift, fr, integer_delay


def fractional_delay(sig, delay_seconds: float, channels=None, keep_length: bool = False, order: int = 30,
                     side_lobe_suppression_db: float = 60):
    """Apply a fractional time delay to a Signal or to every band of a MultiBandSignal.  The output has
    N + order + integer_delay samples (N with `keep_length`); channels not in `channels` are zero-padded at the
    end.  A device-resident signal that does not constrain its amplitude gives a device-resident result."""
    from ..classes import MultiBandSignal, Signal
    assert delay_seconds >= 0, "Delay must be positive"
    if isinstance(sig, Signal):
        if delay_seconds == 0:
            return sig.copy()
        if sig.time_data_imaginary is not None:
            warn("Imaginary time data will be ignored in this function. Delay it manually by creating another "
                 "signal object, if needed.")
        n, n_ch = sig.length_samples, sig.number_of_channels
        delay_samples = delay_seconds * sig.sampling_rate_hz
        if keep_length:
            assert delay_samples < n, "Delay too large for the given signal"
        if channels is None:
            channels = np.arange(n_ch)
        channels = np.atleast_1d(np.asarray(channels).squeeze())
        assert np.all(channels < n_ch) and len(np.unique(channels)) == len(channels), \
            "There is at least an invalid channel number"
        if order < 1 or order > backend.DELAY_MAX_ORDER:
            raise NotImplementedError(f"fractional delay filters of order 1 to {backend.DELAY_MAX_ORDER} are built")
        shift, frac, integer_delay = _delay_rows(n_ch, channels, delay_samples, order)
        out_len = n if keep_length else n + order + integer_delay
        src = np.arange(n_ch)[:, None]
        if sig.on_device and not sig.constrain_amplitude:
            dev = backend.delay_sum_device(sig.device_samples, n, src, shift[:, None], frac[:, None], 1.0, order,
                                           side_lobe_suppression_db, out_len)
            return sig._device_result(dev)
        y, _ = backend.delay_sum(sig.time_data, n, src, shift[:, None], frac[:, None], 1.0, order,
                                 side_lobe_suppression_db, out_len)
        return sig.copy_with_new_time_data(y)
    elif isinstance(sig, MultiBandSignal):
        out_sig = sig.copy()
        out_sig.bands = [fractional_delay(b, delay_seconds, channels, keep_length, order, side_lobe_suppression_db)
                         for b in sig.bands]
        return out_sig
    else:
        raise TypeError("Passed signal should be either type Signal or MultiBandSignal")


def _fractional_latency(td1: np.ndarray, td2, polynomial_points: int) -> np.ndarray:
    """_fractional_latency of the reference (helpers/latency.py:101-149) for two arrays: float lags, (channels,)."""
    peaks, window, near, _ = backend.latency_peaks(td1, td2, polynomial_points)
    return td1.shape[0] - backend.fractional_peak_rows(peaks, window, near, polynomial_points) - 1


def _latency_of_arrays(td1: np.ndarray, td2, p: int):
    """(lags, correlations) of latency for one Signal's arrays; td2 None compares channel 0 with the others."""
    from_first = td2 is None
    n1 = td1.shape[0]
    if from_first:
        # channel 0 goes up once, as the single column every pair shares
        peaks, window, near, r = backend.latency_peaks(td1[:, 1:], td1[:, :1], p, pearson=True, reverse_pairs=True)
        peaks = peaks[::-1]
        near = None if near is None else near[::-1]
        n_und = n1
    else:
        peaks, window, near, r = backend.latency_peaks(td1, td2, p, pearson=True)
        n_und = td2.shape[0]
    if p == 0:
        lags = (n1 - peaks - 1).astype(int)
    else:
        lags = n1 - backend.fractional_peak_rows(peaks, window, near, p) - 1
    rounded = np.round(lags, 0).astype(np.int_)
    # _get_correlation_of_latencies: the delayed signal loses |lag| samples, both are cut to the shorter; fewer than
    # two samples make pearsonr raise there, which sets every coefficient to 0
    n_del = np.where(rounded > 0, n1, n_und)
    overlap = np.minimum(n_del - np.abs(rounded), np.where(rounded > 0, n_und, n1))
    if np.any(overlap < 2):
        warn("An error occured while computing the correlations. They are set to 0.")
        return lags, np.zeros(len(lags))
    candidate = rounded - (n1 - 1 - peaks) + (1 if p > 0 else 0)  # the device's lags: the peak's own and one either side
    assert np.all((candidate >= 0) & (candidate < r.shape[1])), "the rounded lag is one of the device's candidates"
    return lags, r[np.arange(len(lags)), candidate]


def latency(in1, in2=None, polynomial_points: int = 0):
    """Latency between two signals by the correlation method, (lags in samples, correlation coefficients); `in1` is the
    delayed version of `in2` for a positive lag.  Without `in2`, channel 0 of `in1` is the undelayed one and the lags
    of the other channels are returned (length channels - 1).  polynomial_points > 0 gives sub-sample lags from the
    zero crossing of the Hilbert transform of the correlation around its peak, fitted with 2 p points (float lags;
    integer lags, dtype int, for 0); where the root finding fails the integer lag is returned with a warning.  The
    coefficients are Pearson's r of the two channels after the rounded lag is taken out.  MultiBandSignal: (band,
    channel) arrays.

    Two things are the reference's and kept: with `in2` None the lags come out in REVERSED channel order (entry j is
    the lag of channel C - 1 - j: scipy's 2-D correlate flips the column axis), and the coefficient of entry j is still
    computed between channel 0 and channel j + 1 with that entry's lag -- so they are poor for more than two channels.
    With two channels neither shows.  Non-finite samples raise ValueError (numpy's argmax on NaN is not reproduced)."""
    from ..classes import MultiBandSignal, Signal
    assert polynomial_points >= 0, "Polynomial points has to be at least 0"
    if isinstance(in1, Signal):
        if in2 is not None:
            assert in1.sampling_rate_hz == in2.sampling_rate_hz, "Sampling rates must match"
            assert in1.number_of_channels == in2.number_of_channels, "Number of channels between the two signals must match"
            assert isinstance(in2, Signal), "Both signals must be of type Signal"
            td2 = in2.time_data
        else:
            assert in1.number_of_channels > 1, "Signal must have at least 2 channels to compare"
            td2 = None
        return _latency_of_arrays(in1.time_data, td2, int(polynomial_points))
    elif isinstance(in1, MultiBandSignal):
        if in2 is not None:
            assert isinstance(in2, MultiBandSignal), "Both signals must be of type Signal"
            assert in1.sampling_rate_hz == in2.sampling_rate_hz, "Sampling rates must match"
        n_out = in1.number_of_channels - (1 if in2 is None else 0)
        lags = np.zeros((in1.number_of_bands, n_out), dtype=int if polynomial_points == 0 else float)
        correlations = np.zeros((in1.number_of_bands, n_out), dtype=np.float64)
        for band in range(in1.number_of_bands):
            lags[band, :], correlations[band, :] = latency(in1.bands[band], None if in2 is None else in2.bands[band],
                                                           polynomial_points=polynomial_points)
        return lags, correlations
    else:
        raise TypeError("Signals must either be type Signal or MultiBandSignal")


def _pad_trim(vector: np.ndarray, desired_length: int, in_the_end: bool = True) -> np.ndarray:
    """helpers/other.py:216-259 along axis 0 of an (N, C) array: zeros added, or rows cut, at the end or at the start."""
    diff = desired_length - vector.shape[0]
    if diff == 0:
        return vector.copy()
    if diff > 0:
        zeros = np.zeros((diff, vector.shape[1]), dtype=vector.dtype)
        return np.concatenate([vector, zeros] if in_the_end else [zeros, vector])
    return (vector[:desired_length] if in_the_end else vector[-desired_length:] if desired_length > 0
            else vector[:0]).copy()


def delay(sig, delay_samples: int, channels=None, keep_length: bool = False):
    """Delay a Signal, or every band of a MultiBandSignal, by an integer number of samples through zero-padding.  The
    output has N + delay_samples samples (N with `keep_length`); channels not in `channels` are zero-padded at the end.
    A delay of 0 returns a copy."""
    from ..classes import MultiBandSignal, Signal
    if isinstance(sig, Signal):
        if delay_samples == 0:
            return sig.copy()
        if keep_length:
            assert delay_samples < sig.time_data.shape[0], "Delay too large for the given signal"
        if channels is None:
            channels = np.arange(sig.number_of_channels)
        channels = np.atleast_1d(np.asarray(channels).squeeze())
        assert np.all(channels < sig.number_of_channels) and len(np.unique(channels)) == len(channels), \
            "There is at least an invalid channel number"
        n_new = delay_samples + sig.time_data.shape[0]
        # the reference's setdiff1d(channels, all channels) is empty for valid channels: the channels left out are
        # simply those of the whole array padded at the end
        new_time_data = _pad_trim(sig.time_data, n_new, in_the_end=True)
        new_time_data[:, channels] = _pad_trim(sig.time_data[:, channels], n_new, in_the_end=False)
        if keep_length:
            new_time_data = new_time_data[: sig.time_data.shape[0], :]
        return sig.copy_with_new_time_data(new_time_data)
    elif isinstance(sig, MultiBandSignal):
        out_sig = sig.copy()
        out_sig.bands = [delay(b, delay_samples, channels, keep_length) for b in sig.bands]
        return out_sig
    else:
        raise TypeError("Passed signal should be either type Signal or MultiBandSignal")
