"""Decibel conversions (dsptoolbox/helpers/gain_and_level.py:28-46, 158-200): exported as tools.to_db and
tools.from_db; a module of their own because the standard package needs them while the backend is still importing."""

import numpy as np


def from_db(x, amplitude_output: bool):
    """Values in dB as amplitudes (10^(x / 20)) or, amplitude_output False, as powers (10^(x / 10))."""
    return 10 ** (x / (20.0 if amplitude_output else 10.0))


def to_db(x, amplitude_input: bool, dynamic_range_db: float | None = None,
          min_value: float | None = float(np.finfo(np.float64).smallest_normal)):
    """Amplitudes (20 log10 |x|) or, amplitude_input False, powers (10 log10 |x|) in dB.  |x| is clipped from below
    first, at `min_value` or -- with `dynamic_range_db`, which wins -- that many dB below its largest value; with both
    None nothing is clipped and a zero gives -inf."""
    factor = 20.0 if amplitude_input else 10.0
    magnitude = np.abs(x)
    if dynamic_range_db is not None:
        min_value = np.max(magnitude) * 10.0 ** (-abs(dynamic_range_db) / factor)
    if min_value is None:
        return factor * np.log10(magnitude)
    return factor * np.log10(np.clip(magnitude, a_min=min_value, a_max=None))
