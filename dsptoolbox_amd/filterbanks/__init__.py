"""filterbanks: the block-streaming FIR classes of the reference's filterbanks module
(dsptoolbox/filterbanks/__init__.py:78-83) on the device FIR kernels, the fractional-octave
Butterworth bank (filterbanks/filterbanks.py:336-413) on the device IIR kernels, and the auditory gammatone bank
(filterbanks/filterbanks.py:217-303, filterbanks/_filterbank.py:664-701) on the complex-coefficient IIR kernels, and the
structure filters the reference exports here (filterbanks/__init__.py:75-86) -- LatticeLadderFilter, WarpedFIR, WarpedIIR,
KautzFilter -- on the structure-filter kernels, and the Linkwitz-Riley crossover bank (filterbanks/filterbanks.py:37-78,
filterbanks/_filterbank.py:45-405) on the device IIR kernels, and the realtime filters -- StateVariableFilter, ParallelFilter,
IIRFilter, FIRFilter, StateSpaceFilter, FilterChain on the realtime-filter kernels (classes/realtime_filters.py), and the
host-only ExponentialAverageFilter."""

import numpy as np

from ..classes.filter import Filter
from ..classes.filterbank import FilterBank
from ..classes.fir_filter_realtime import (FIRFilterOverlapSave, FIRUniformPartitioned,
                                           FIRUniformPartitionedMultichannel)
from ..classes.realtime_filters import (ExponentialAverageFilter, FilterChain, FIRFilter, IIRFilter, ParallelFilter,
                                        StateSpaceFilter, StateVariableFilter)
from ..classes.structure_filters import KautzFilter, LatticeLadderFilter, WarpedFIR, WarpedIIR
from ..standard.enums import FilterCoefficientsType, FilterPassType, IirDesignMethod
from ..tools import erb_frequencies, fractional_octave_frequencies
from ._linkwitz_riley import LRFilterBank


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


def linkwitz_riley_crossovers(crossover_frequencies_hz, order, sampling_rate_hz: int) -> LRFilterBank:
    """A Linkwitz-Riley crossover bank: len(crossover_frequencies_hz) + 1 bands whose sum is an all-pass.  order: one
    value or one per crossover -- 2 (Sallen-Key sections with Q = 0.5, the high band phase-inverted), a multiple of 4
    (Butterworth filters of half the order twice; bands cross at -6 dB, slope 6 dB / octave per order) or odd (one
    Butterworth filter per side, bands cross at -3 dB; not a Linkwitz-Riley crossover, but the magnitudes still
    reconstruct)."""
    return LRFilterBank(crossover_frequencies_hz, order, sampling_rate_hz)


class GammaToneFilterBank(FilterBank):
    """The bank of auditory_filters_gammatone: a FilterBank of complex sos filters that also carries the centre
    frequencies, the complex poles and the normalisations of its bands.  Unlike the reference's constructor this one
    does not run an impulse through the bank: the values that pass prepares are only used by reconstruct."""

    def __init__(self, filters: list, info: dict, frequencies, coefficients, normalizations):
        super().__init__(filters, same_sampling_rate=True, info=info)
        self._frequencies = frequencies
        self._coefficients = coefficients
        self._normalizations = normalizations
        self._delay = 0.004  # the target delay of the reconstruction, in seconds

    def reconstruct(self, signal):
        raise NotImplementedError(
            "GammaToneFilterBank.reconstruct is not built: the reference's own delays, phase factors and gains "
            "evaluate to NaN (it searches the band envelopes of an impulse before the impulse's position, where they "
            "are zero), so there is no result to reproduce")


def auditory_filters_gammatone(frequency_range_hz=[20, 20000], resolution: float = 1,
                               sampling_rate_hz: int | None = None) -> GammaToneFilterBank:
    """The fourth-order gammatone analysis bank of V. Hohmann (Acta Acust. united Ac. 88, 2002), one band per
    `resolution` ERB between the two frequencies, reference frequency 1 kHz.  Band k is four identical complex
    one-pole sections 1 / (1 - a_k z^-1), the last one scaled by the band's normalisation; its output is complex
    (Signal.time_data_imaginary).  Filtering runs on the device (backend.iir_sos_filter_complex)."""
    assert sampling_rate_hz is not None, "A sampling rate must be passed to create the filter bank"
    assert np.max(frequency_range_hz) <= sampling_rate_hz // 2, \
        "Highest frequency should not be higher than the nyquist frequency"
    frequencies_hz = erb_frequencies(frequency_range_hz, resolution)
    # Hohmann 2002: the ERB of the auditory filter at each frequency, Eq. (13); the bandwidth parameter of an
    # order-4 filter with that ERB, Eqs. (14.2), (14.3); the pole's radius, Eq. (14.1), and angle, Eq. (10)
    erb_hz = 24.7 + frequencies_hz / 9.265
    a_gamma = np.pi * 720 * 2 ** (-6) / 36  # pi (2 n - 2)! 2^-(2 n - 2) / ((n - 1)!)^2 at n = 4
    radius = np.exp(-2 * np.pi * (erb_hz / a_gamma) / sampling_rate_hz)
    coefficients = radius * np.exp(1j * (2 * np.pi * frequencies_hz / sampling_rate_hz))  # Eq. (1)
    normalizations = 2 * (1 - np.abs(coefficients)) ** 4  # section 2.2
    filters = []
    for pole, norm in zip(coefficients, normalizations):
        sos = np.zeros((4, 6), dtype=np.complex128)
        sos[:, 0] = 1.0
        sos[:, 3] = 1.0
        sos[:, 4] = -pole
        sos[3, 0] = norm
        band = Filter({FilterCoefficientsType.Sos: sos}, sampling_rate_hz)
        band.warning_if_complex = False
        filters.append(band)
    return GammaToneFilterBank(filters, info={"Type of filter bank": "Gammatone filter bank"},
                               frequencies=frequencies_hz, coefficients=coefficients, normalizations=normalizations)


__all__ = ["FIRFilterOverlapSave", "FIRUniformPartitioned", "FIRUniformPartitionedMultichannel",
           "fractional_octave_bands", "auditory_filters_gammatone", "GammaToneFilterBank", "LatticeLadderFilter", "WarpedFIR",
           "WarpedIIR", "KautzFilter", "linkwitz_riley_crossovers", "LRFilterBank", "StateSpaceFilter", "IIRFilter",
           "FIRFilter", "StateVariableFilter", "ParallelFilter", "FilterChain", "ExponentialAverageFilter"]
