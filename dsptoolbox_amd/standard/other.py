"""detrend, envelope and merge_filters (API mirror of dsptoolbox/standard/other.py).

detrend removes the least-squares polynomial of every channel on the device (csrc/kernels_level.hpp): the fit runs in
the discrete Chebyshev polynomials orthonormal on the sample grid, so no power of the sample index is ever summed.
Orders up to 8 are built.  A device-resident signal is read where it lies and its result stays resident.

envelope always removes the least-squares line first, as the reference does.  The analytic envelope is the magnitude
of the float64 Hilbert transform of transforms.hilbert, within that transform's length bounds; the boxcar envelope is
the causal moving RMS value over `window_length_samples`.  Where the reference's FFT convolution can leave a tiny
negative mean square and a NaN after the root, the device sums non-negative squares and clamps at zero: the envelope
of finite samples is finite and not negative.  merge_filters is host arithmetic on coefficients."""

from __future__ import annotations

import numpy as np

from .. import backend
from .._lib import DevicePlanar
from .enums import FilterCoefficientsType

__all__ = ["detrend", "envelope", "merge_filters"]


def _samples(sig):
    return sig.device_samples if sig.on_device else sig.time_data


def detrend(sig, polynomial_order: int = 0):
    """Remove the least-squares polynomial of `polynomial_order` (0: the mean) from every channel of a Signal or of the
    bands of a MultiBandSignal."""
    from ..classes import MultiBandSignal, Signal
    if isinstance(sig, Signal):
        assert polynomial_order >= 0, "Polynomial order should be positive"
        if polynomial_order > backend.LEVEL_MAX_ORDER:
            raise NotImplementedError(f"detrend: polynomial orders up to {backend.LEVEL_MAX_ORDER} are built on the "
                                      f"device, not {polynomial_order}")
        y = backend.level_apply(_samples(sig), order=int(polynomial_order))
        return sig._device_result(y) if isinstance(y, DevicePlanar) else sig.copy_with_new_time_data(y)
    if isinstance(sig, MultiBandSignal):
        return MultiBandSignal([detrend(b, polynomial_order) for b in sig.bands], sig.same_sampling_rate, dict(sig.info))
    raise TypeError("Pass either a Signal or a MultiBandSignal")


def envelope(signal, analytic: bool = True, window_length_samples: int | None = None) -> np.ndarray:
    """The envelope of the linearly detrended signal: |hilbert| (analytic) or the RMS value over a causal boxcar window,
    as (samples, channels), or (samples, bands, channels) for a MultiBandSignal of one sampling rate."""
    from ..classes import MultiBandSignal, Signal
    if isinstance(signal, Signal):
        if analytic:
            return backend.envelope_analytic(_samples(signal))
        assert window_length_samples is not None, "Some window length must be passed"
        assert window_length_samples > 0, "Window length must be more than 1 sample"
        return backend.moving_rms(_samples(signal), window_length_samples)
    if isinstance(signal, MultiBandSignal):
        assert signal.same_sampling_rate, "This is only available for constant sampling rate bands"
        env = np.zeros((len(signal.bands[0]), signal.number_of_bands, signal.number_of_channels), float)
        for ind, b in enumerate(signal.bands):
            env[:, ind, :] = envelope(b, analytic=analytic, window_length_samples=window_length_samples)
        return env
    raise TypeError("Signal must be type Signal or MultiBandSignal")


def merge_filters(filters):
    """One Filter for a list of filters or a FilterBank applied one after the other: the convolution of FIR filters,
    the concatenated second-order sections of IIR filters."""
    from scipy.signal import convolve
    from ..classes import Filter, FilterBank
    filts = filters.filters if isinstance(filters, FilterBank) else filters
    assert len(filts) > 1, "There must be at least two filters to combine"
    assert all(filts[0].sampling_rate_hz == f.sampling_rate_hz for f in filts), "Sampling rates do not match"
    if filts[0].is_fir:
        assert all(f.is_fir for f in filts), "Some filter is not FIR"
        b = filts[0].ba[0].copy()
        for f in filts[1:]:
            b = convolve(b, f.ba[0], mode="full", method="auto")
        return Filter.from_ba(b, [1.0], filts[0].sampling_rate_hz)
    assert all(f.is_iir for f in filts), "Some filter is not IIR"
    sos = np.concatenate([f.get_coefficients(FilterCoefficientsType.Sos) for f in filts], axis=0)
    return Filter.from_sos(sos, filts[0].sampling_rate_hz)
