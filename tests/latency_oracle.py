"""numpy / scipy restatement of the reference's latency family (standard.latency, standard/latency_delay.py:15-156;
_latency, standard/_standard_backend.py:14-34; helpers/latency.py; _remove_ir_latency_from_phase_min_phase,
helpers/minimum_phase.py:82-117; find_ir_latency and group_delay's latency removal, transfer_functions.py:862-915,
1380-1406), with the intermediate values the tests judge the device by: the correlation, the shared window, the
Hilbert transform of the window and the neighbourhood of every peak."""

import warnings

import numpy as np
from scipy.fft import next_fast_len
from scipy.interpolate import interp1d
from scipy.signal import correlate, hilbert
from scipy.stats import pearsonr

from test_phase_host import ref_group_delay_direct, ref_minimum_group_delay, ref_min_phase_spectrum

FAILED = "Fractional latency detection failed for channel {}. Integer latency is returned"
MARGIN = 200


def xcorr(td1, td2):
    """(L, channels) full-mode correlation as the reference forms it; td2 None: channel 0 against the others through
    scipy's 2-D form, whose output column j belongs to channel C - 1 - j."""
    if td2 is None:
        return correlate(td1[:, :1], np.atleast_2d(td1[:, 1:]))
    return np.stack([correlate(td2[:, i], td1[:, i]) for i in range(td2.shape[1])], axis=1)


def integer_latency(td1, td2):
    return td1.shape[0] - np.argmax(np.abs(xcorr(td1, td2)), axis=0) - 1


def peak_window(time_data):
    """(d, lo, window): every channel's argmax |x|, the shared window's first row and the window's rows."""
    d = np.argmax(np.abs(time_data), axis=0).astype(int)
    window = time_data[:np.max(d) + MARGIN]
    lo = max(np.min(d) - MARGIN, 0)
    return d, lo, window[lo:]


def root_of(h_col, d, p, ch=0):
    """One channel's sub-sample row inside the window from the Hilbert transform's imaginary part h_col and the
    integer peak row d: helpers/latency.py:46-97."""
    sel = h_col[d:d + 2]
    move_back = int(sel[0] * sel[1] > 0)
    d = d - move_back
    if h_col[d] * h_col[d + 1] > 0:
        warnings.warn(FAILED.format(ch))
        return float(d + move_back)
    pol = np.polyfit(np.arange(-p + 1, p + 1), h_col[d - p + 1:d + p + 1], deg=2 * p - 1)
    roots = np.roots(pol)
    roots = roots[(roots == roots.real) & (roots <= 1) & (roots >= 0)].real
    if len(roots) == 0:
        warnings.warn(FAILED.format(ch))
        return float(d + move_back)
    return d + roots[0]


def fractional_peak(time_data, p, detail=False):
    """_get_fractional_impulse_peak_index.  detail: also (d, lo, h), the peak rows of the whole array, the window's
    first row and imag(hilbert(window))."""
    d, lo, window = peak_window(time_data)
    h = hilbert(window, axis=0).imag
    rows = np.array([root_of(h[:, c], d[c] - lo, p, c) for c in range(time_data.shape[1])]) + lo
    return (rows, d, lo, h) if detail else rows


def neighbourhood(h, d_window, p):
    """(C, 2 p + 2): h[d - p .. d + p + 1] per channel, NaN outside the window."""
    out = np.full((h.shape[1], 2 * p + 2), np.nan)
    for c in range(h.shape[1]):
        for j in range(2 * p + 2):
            r = d_window[c] - p + j
            if 0 <= r < h.shape[0]:
                out[c, j] = h[r, c]
    return out


def fractional_latency(td1, td2, p):
    return td1.shape[0] - fractional_peak(xcorr(td1, td2), p) - 1


def correlation_of_latencies(time_data, other, lat):
    """_get_correlation_of_latencies."""
    one = time_data.shape[1] == 1
    out = np.zeros(len(lat))
    for ch in range(len(lat)):
        t = time_data[:, 0] if one else time_data[:, ch]
        if lat[ch] > 0:
            und, dl = t, other[:, ch]
        else:
            und, dl = other[:, ch], t
        dl = dl[abs(lat[ch]):]
        n = min(len(dl), len(und))
        out[ch] = pearsonr(dl[:n], und[:n])[0]
    return out


def latency(td1, td2, p):
    """standard.latency for one Signal's arrays: (lags, correlations)."""
    lags = integer_latency(td1, td2) if p == 0 else fractional_latency(td1, td2, p)
    try:
        return lags, correlation_of_latencies(td2 if td2 is not None else td1[:, :1], td1 if td2 is not None else td1[:, 1:],
                                              np.round(lags, 0).astype(np.int_))
    except Exception:
        warnings.warn("An error occured while computing the correlations. They are set to 0.")
        return lags, np.zeros(len(lags))


def min_phase_rows(x, padding_factor):
    """_min_phase_ir_from_real_cepstrum: all next_fast_len(N padding_factor) rows."""
    return np.real(np.fft.ifft(ref_min_phase_spectrum(x, padding_factor), axis=0))


def find_ir_latency(x, compare_to_min_phase_ir=True):
    if compare_to_min_phase_ir:
        return latency(x, min_phase_rows(x, 8)[:len(x)], 1)[0]
    return fractional_peak(x, 1)


def wrap_phase(x):
    return (x + np.pi) % (2 * np.pi) - np.pi


def latency_free_phase(x, fs):
    """(f, phase) of group_delay(analytic_computation=False, remove_ir_latency=True) before the unwrap."""
    n = next_fast_len(x.shape[0] * 8, True)
    td = np.concatenate([x, np.zeros((n - len(x), x.shape[1]))])
    f = np.fft.rfftfreq(n, 1 / fs)
    lat = fractional_latency(x, min_phase_rows(x, 1), 1)
    return f, wrap_phase(np.angle(np.fft.rfft(td, axis=0)) + 2 * np.pi * f[:, None] * (lat / fs)[None, :])


def group_delay_latency_free(x, fs):
    f, ph = latency_free_phase(x, fs)
    return f, ref_group_delay_direct(ph, f[1] - f[0])


def excess_group_delay_latency_free(x, fs, analytic):
    """excess_group_delay(remove_ir_latency=True); the analytic form is test_phase_host.ref_group_delay's."""
    from test_phase_host import ref_group_delay
    f_min, min_gd = ref_minimum_group_delay(x, fs, 1)
    f, gd = ref_group_delay(x, fs, analytic=True, latency=True) if analytic else group_delay_latency_free(x, fs)
    if len(f) != len(f_min):
        gd = interp1d(f, gd, kind="linear", copy=False, bounds_error=False, assume_sorted=True, fill_value=(0.0, 0.0),
                      axis=0)(f_min)
    return f_min, gd - min_gd
