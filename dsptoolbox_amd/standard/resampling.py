"""resample and resample_filter (API mirror of dsptoolbox/standard/resampling.py).

resample converts a signal to another sampling rate by the ratio of the two rates in lowest terms, up / down, with the
filter scipy.signal.resample_poly designs by default.  The polyphase sum runs on the device in float64
(csrc/kernels_resample.hpp, one launch); there is no host path.  A host signal goes up once as (samples, channels) float64
and its result comes down once; a device-resident signal is read where it lies and its result stays resident, as a new
float32 planar buffer at the new rate.  The reduced ratio is bounded by backend.RESAMPLE_MAX_RATE (44100 <-> 192000 is
inside, 44100 -> 44101 is not); beyond it the call raises NotImplementedError before anything reaches the device.

resample_filter is host float64 design code on a handful of poles and zeros: the reference's numpy and scipy operations
in the reference's order."""

from __future__ import annotations

from fractions import Fraction

import numpy as np
from scipy.signal import bilinear_zpk

from .. import backend
from .enums import FilterCoefficientsType

__all__ = ["resample", "resample_filter"]


def resample(sig, desired_sampling_rate_hz: int, rescaling: bool = False):
    """The signal at `desired_sampling_rate_hz`, of the same type (an ImpulseResponse stays one) and with the same
    amplitude constraint.  With `rescaling` the samples are multiplied by down / up, which keeps the magnitude of the
    unscaled spectrum; the factor is folded into the filter's taps on the host (one rounding per tap), so host and
    resident signals take the same single launch and no further pass over the samples.  Equal rates return a copy.
    Signals with imaginary time data raise NotImplementedError."""
    if sig.sampling_rate_hz == desired_sampling_rate_hz:
        return sig.copy()
    if sig.is_complex_signal:
        raise NotImplementedError("resample: signals with imaginary time data are not run on the device")
    up, down = Fraction(int(desired_sampling_rate_hz), int(sig.sampling_rate_hz)).as_integer_ratio()
    scale = down / up if rescaling else 1.0
    if sig.on_device:
        new_sig = sig._device_result(backend.resample_poly_device(sig.device_samples, up, down, scale))
    else:
        new_sig = sig.copy_with_new_time_data(backend.resample_poly(sig.time_data, up, down, scale))
    new_sig.sampling_rate_hz = desired_sampling_rate_hz
    return new_sig


def resample_filter(filter, new_sampling_rate_hz: int):
    """The filter at another sampling rate: its poles and zeros go to the s-plane by the inverse bilinear map at the old
    rate and come back by scipy's bilinear_zpk at the new one.  Good where poles and zeros lie at low normalised
    frequencies (about 0.1); higher ones are distorted by the bilinear map's frequency warping."""
    from ..classes import Filter
    z, p, k = filter.get_coefficients(FilterCoefficientsType.Zpk)
    extra_poles = max(0, len(z) - len(p))
    extra_zeros = max(0, len(p) - len(z))
    fs2 = 2 * filter.sampling_rate_hz
    p = fs2 * (p - 1) / (p + 1)
    z = z[z != -1.0]  # zeros at Nyquist lie at infinity in the s-plane
    z = fs2 * (z - 1) / (z + 1)
    if extra_poles:
        p = np.hstack([p, [-fs2] * (len(z) - len(p))])
    if extra_zeros:
        z = np.hstack([z, [-fs2] * (len(p) - len(z))])
    k /= np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
    z, p, k = bilinear_zpk(z, p, k, new_sampling_rate_hz)
    return Filter.from_zpk(z, p, k, new_sampling_rate_hz)
