"""tools: the fractional-octave band arithmetic of the reference's tools.fractional_octave_frequencies
(dsptoolbox/tools.py:186-255), after the band definitions of IEC 61260-1:2014 / ANSI S1.11-2004,
erb_frequencies (dsptoolbox/tools.py:261-336), fractional_octave_smoothing (dsptoolbox/tools.py:22-23) on the
device, and the decibel conversions to_db and from_db (dsptoolbox/helpers/gain_and_level.py:28-46, 158-200)."""

import numpy as np

from ._db import from_db, to_db  # noqa: F401
from .backend import fractional_octave_smoothing  # noqa: F401


def get_smoothing_factor_ema(relaxation_time_s: float, sampling_rate_hz: int, accuracy: float = 0.95):
    """alpha of the exponential moving average y[n] = alpha x[n] + (1 - alpha) y[n - 1] whose step response is within
    `accuracy` (in ]0, 1[) of 1 after the relaxation time (dsptoolbox/helpers/smoothing.py:132-166)."""
    from .classes.realtime_filters import _get_smoothing_factor_ema
    return _get_smoothing_factor_ema(relaxation_time_s, sampling_rate_hz, accuracy)

# base-ten octave ratio and reference frequency of IEC 61260-1 (5.2, 5.4)
_G = 10 ** (3 / 10)
_F_REF = 1000.0
# the standard's nominal mid-band frequencies (IEC 61260-1, Annex E): octave and one-third-octave bands
_NOMINAL = {
    1: [31.5, 63, 125, 250, 500, 1e3, 2e3, 4e3, 8e3, 16e3],
    3: [25, 31.5, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500,
        3150, 4000, 5000, 6300, 8000, 10000, 12500, 16000, 20000],
}


def fractional_octave_frequencies(num_fractions=1, frequency_range=(20, 20e3), return_cutoff=False):
    """Nominal and exact mid-band frequencies of 1/num_fractions-octave bands within frequency_range, and -- with
    return_cutoff -- the band edges (lower, upper) = exact * G^(-+1 / (2 num_fractions)).

    For octaves and thirds the bands are the standard's: band x has the exact mid-band frequency
    1000 G^(x / b), x the index whose nominal frequency is that of the table, and only bands whose nominal
    frequency lies inside the range are kept.  Other fractions have no nominal frequencies (an empty array)
    and exact frequencies 1000 * 2^(x / b) for x from -round(b log2(1000 / f_low)) to round(b log2(f_high / 1000)).

    Returns (nominal, exact) or (nominal, exact, (lower, upper))."""
    f_lims = np.asarray(frequency_range)
    if f_lims.size != 2:
        raise ValueError("You need to specify a lower and upper limit frequency.")
    if f_lims[0] > f_lims[1]:
        raise ValueError("The second frequency needs to be higher than the first.")
    b = num_fractions
    if b in _NOMINAL:
        nominal = np.asarray(_NOMINAL[b], dtype=float)
        # odd b: mid-band frequencies at integer band indices relative to 1 kHz
        exact = _F_REF * _G ** (np.around(b * np.log(nominal / _F_REF) / np.log(_G)) / b)
        keep = (nominal >= f_lims[0]) & (nominal <= f_lims[1])
        nominal, exact = nominal[keep], exact[keep]
    else:
        nominal = np.array([])
        x_hi = np.around(b * np.log2(f_lims[1] / _F_REF))
        x_lo = np.around(b * np.log2(_F_REF / f_lims[0]))
        exact = _F_REF * 2 ** (np.arange(-x_lo, x_hi + 1) / b)
    if not return_cutoff:
        return nominal, exact
    return nominal, exact, (exact * _G ** (-1 / 2 / b), exact * _G ** (1 / 2 / b))


# the ERB-number scale of Hohmann 2002, Eq. (16): erb(f) = _ERB_L log(1 + f _ERB_Q)
_ERB_L = 9.2645
_ERB_Q = 0.00437


def _hz_to_erb(f):
    return _ERB_L * np.sign(f) * np.log(1 + np.abs(f) * _ERB_Q)


def erb_frequencies(freq_range_hz=[20, 20000], resolution: float = 1, reference_frequency_hz: float = 1000):
    """Frequencies in Hz spaced by `resolution` units of the ERB-number scale (V. Hohmann, "Frequency analysis and
    synthesis using a gammatone filterbank", Acta Acust. united Ac. 88, 2002, Eq. 16).  The grid passes through the
    reference frequency and holds every point of it inside the range, whose two limits may come in either order."""
    if not isinstance(freq_range_hz, (list, tuple, np.ndarray)) or len(freq_range_hz) != 2:
        raise ValueError("freq_range must be an array like of length 2")
    if freq_range_hz[0] > freq_range_hz[1]:
        freq_range_hz = [freq_range_hz[1], freq_range_hz[0]]
    if resolution <= 0:
        raise ValueError("Resolution must be larger than zero")
    erb_lo, erb_hi = _hz_to_erb(np.asarray(freq_range_hz))
    erb_ref = _hz_to_erb(reference_frequency_hz)
    # whole steps that fit below and above the reference
    steps_below = int(np.floor((erb_ref - erb_lo) / resolution))
    steps_above = int(np.floor((erb_hi - erb_ref) / resolution))
    erb = np.arange(-steps_below, steps_above + 1) * resolution + erb_ref
    return 1 / _ERB_Q * np.sign(erb) * (np.exp(np.abs(erb) / _ERB_L) - 1)
