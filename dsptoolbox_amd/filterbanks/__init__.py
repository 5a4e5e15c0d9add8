"""filterbanks: the block-streaming FIR classes of the reference's filterbanks module
(dsptoolbox/filterbanks/__init__.py:78-83) on the device FIR kernels, and the fractional-octave
Butterworth bank (filterbanks/filterbanks.py:336-413) on the device IIR kernels."""

import numpy as np

from ..classes.filter import Filter
from ..classes.filterbank import FilterBank
from ..classes.fir_filter_realtime import (FIRFilterOverlapSave, FIRUniformPartitioned,
                                           FIRUniformPartitionedMultichannel)
from ..standard.enums import FilterPassType, IirDesignMethod
from ..tools import fractional_octave_frequencies


def fractional_octave_bands(frequency_range_hz=[31.5, 16e3], octave_fraction: int = 1, filter_order: int = 6,
                            sampling_rate_hz: int | None = None):
    """A FilterBank of Butterworth band passes, one per fractional-octave band of ANSI S1.11-2004 within the range
    (a band whose upper edge lies above Nyquist becomes a high pass).  Returns (bank, exact mid-band frequencies,
    (lower, upper) band edges)."""
    assert sampling_rate_hz is not None, "A sampling rate must be passed for the filter bank"
    frequency_range_hz = np.atleast_1d(np.squeeze(frequency_range_hz))
    frequency_range_hz.sort()
    assert len(frequency_range_hz) == 2, "Frequency range must contain exactly two entries"
    assert frequency_range_hz[-1] < sampling_rate_hz // 2, \
        "The highest frequency in the range is higher than the nyquist frequency"
    _, center_freqs_hz, (lower_hz, upper_hz) = fractional_octave_frequencies(
        octave_fraction, frequency_range_hz, return_cutoff=True)
    bank = FilterBank()
    for lo, hi in zip(lower_hz, upper_hz):
        if hi > sampling_rate_hz // 2:
            top, freqs = FilterPassType.Highpass, lo
        else:
            top, freqs = FilterPassType.Bandpass, [lo, hi]
        bank.add_filter(Filter.iir_filter(order=filter_order, frequency_hz=freqs, type_of_pass=top,
                                          filter_design_method=IirDesignMethod.Butterworth,
                                          sampling_rate_hz=sampling_rate_hz))
    return bank, center_freqs_hz, (lower_hz, upper_hz)


__all__ = ["FIRFilterOverlapSave", "FIRUniformPartitioned", "FIRUniformPartitionedMultichannel",
           "fractional_octave_bands"]
