"""fractional_delay (API mirror of dsptoolbox/standard/latency_delay.py:159-285).

The Kaiser-windowed sinc filter of every delayed channel is built on the device (k_delay_taps) and applied there in
float64 (k_delay_sum); the host only splits the delay into its integer part and fraction, with the reference's
float64 operations.  Output lengths, the pass-through of a zero delay, the zero padding of channels left out of
`channels` and the normalisation of constrained signals are the reference's."""

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
