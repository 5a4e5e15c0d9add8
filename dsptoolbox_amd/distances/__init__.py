"""distances: how far one signal is from another (API mirror of dsptoolbox/distances/distances.py: log_spectral
:23-105, itakura_saito :108-191, snr :194-222, si_sdr :225-272, fw_snr_seg :275-387).  snr and si_sdr are float64
reductions on the device in a fixed summation order; fw_snr_seg is one device call from the samples to the value
per channel (the gammatone bank, the framing, one float64 transform per frame, band and channel, the weighted
reduction); log_spectral and itakura_saito stand on Signal.get_spectrum() -- the device's Welch or FFT path -- and
integrate the few thousand selected bins on the host."""

import numpy as np
from scipy.integrate import simpson
from scipy.signal import windows

from .. import backend
from ..classes.signal import Signal
from ..filterbanks import auditory_filters_gammatone
from ..standard.enums import SpectrumMethod
from ..transfer_functions import find_nearest_points_index_in_vector


def _band_limited_power_spectra(insig1: Signal, insig2: Signal, method, f_range_hz, energy_normalization: bool,
                                spectrum_parameters):
    """What log_spectral and itakura_saito share: the checks, both power spectra on the selected bins (each column
    divided by its sum when asked for) and the frequencies of those bins."""
    assert insig1.sampling_rate_hz == insig2.sampling_rate_hz, "Sampling rates do not match"
    assert insig1.number_of_channels == insig2.number_of_channels, "Signals have different channel numbers"
    if spectrum_parameters is None:
        spectrum_parameters = {}
    fs_hz = insig1.sampling_rate_hz
    if f_range_hz is None:
        f_range_hz = [0, fs_hz // 2]
    else:
        assert len(f_range_hz) == 2, "f_range_hz must only have a lower and an upper limit"
        f_range_hz = np.sort(f_range_hz)
        assert f_range_hz[1] <= fs_hz // 2, "Upper bound for frequency must be smaller than the nyquist frequency"
        assert not any(f_range_hz < 0), "Frequencies in range must be positive"
    insig1.set_spectrum_parameters(method=method, **spectrum_parameters)
    insig2.set_spectrum_parameters(method=method, **spectrum_parameters)
    f, spec1 = insig1.get_spectrum()
    f, spec2 = insig2.get_spectrum()
    psd1, psd2 = np.abs(spec1), np.abs(spec2)
    if insig1.spectrum_scaling.is_amplitude_scaling():
        psd1, psd2 = psd1 ** 2, psd2 ** 2
    lo, hi = find_nearest_points_index_in_vector(f_range_hz, f)
    psd1, psd2 = psd1[lo:hi].copy(), psd2[lo:hi].copy()
    if energy_normalization:
        psd1 /= np.sum(psd1, axis=0)
        psd2 /= np.sum(psd2, axis=0)
    return f[lo:hi], psd1, psd2


def log_spectral(insig1: Signal, insig2: Signal, method: SpectrumMethod = SpectrumMethod.WelchPeriodogram,
                 f_range_hz=[20, 20000], energy_normalization: bool = True, spectrum_parameters: dict | None = None):
    """Log-spectral distance per channel: sqrt of the integral over frequency of (10 log10(P1 / P2))^2."""
    f, p1, p2 = _band_limited_power_spectra(insig1, insig2, method, f_range_hz, energy_normalization, spectrum_parameters)
    return np.array([np.sqrt(simpson((10 * np.log10(p1[:, n] / p2[:, n])) ** 2, x=f)) for n in range(p1.shape[1])])


def itakura_saito(insig1: Signal, insig2: Signal, method: SpectrumMethod = SpectrumMethod.WelchPeriodogram,
                  f_range_hz=[20, 20000], energy_normalization: bool = True, spectrum_parameters: dict | None = None):
    """Itakura-Saito measure per channel, with the reference's base-ten logarithm: the integral over frequency of
    P1 / P2 - log10(P1 / P2) - 1.  Not symmetric in its two signals."""
    f, p1, p2 = _band_limited_power_spectra(insig1, insig2, method, f_range_hz, energy_normalization, spectrum_parameters)
    return np.array([simpson(p1[:, n] / p2[:, n] - np.log10(p1[:, n] / p2[:, n]) - 1, x=f) for n in range(p1.shape[1])])


def _moments(a: Signal, b: Signal, par=None) -> np.ndarray:
    if a.on_device and b.on_device:
        return backend.pair_moments_device(a.device_samples, b.device_samples, par)
    return backend.pair_moments(a.time_data, b.time_data, par)


def snr(signal: Signal, noise: Signal) -> np.ndarray:
    """Signal-to-noise ratio per channel, 20 log10(rms(signal) / rms(noise)) with the reference's rms, which is the
    standard deviation.  A noise with one channel is the noise of every channel of the signal.  Two passes on the
    device: the sums give the means, then the squares are summed about them."""
    assert signal.sampling_rate_hz == noise.sampling_rate_hz, "Sampling rates do not match"
    if noise.number_of_channels != 1:
        assert signal.number_of_channels == noise.number_of_channels, "Signals have different channel numbers"
    n = len(signal)
    m = _moments(signal, noise)
    par = np.stack([np.zeros(m.shape[0]), m[:, 3] / n, m[:, 4] / n], axis=1)
    m = _moments(signal, noise, par)
    return np.atleast_1d(20 * np.log10(np.sqrt(m[:, 0] / n) / np.sqrt(m[:, 1] / n)))


def si_sdr(target_signal: Signal, modified_signal: Signal) -> np.ndarray:
    """Scale-invariant signal-to-distortion ratio per channel (Le Roux et al., arXiv:1811.02508):
    10 log10(|alpha s|^2 / |alpha s - shat|^2), alpha = <s, shat> / <s, s>.  A target with one channel is the target
    of every channel of the modified signal.  Two passes on the device: the inner products give alpha, then the
    residual is summed term by term."""
    assert modified_signal.sampling_rate_hz == target_signal.sampling_rate_hz, "Sampling rates do not match"
    if target_signal.number_of_channels != 1:
        assert modified_signal.number_of_channels == target_signal.number_of_channels, \
            "Signals have different channel numbers"
    assert len(modified_signal) == len(target_signal), "Length of signals do not match"
    m = _moments(target_signal, modified_signal)
    alpha = m[:, 2] / m[:, 0]
    r = _moments(target_signal, modified_signal, np.stack([alpha, np.zeros_like(alpha), np.zeros_like(alpha)], axis=1))
    return 10 * np.log10(alpha ** 2 * m[:, 0] / r[:, 5])


def fw_snr_seg(x: Signal, xhat: Signal, f_range_hz=[20, 10e3], snr_range_db=[-10, 35], gamma: float = 0.2) -> np.ndarray:
    """Frequency-weighted segmental SNR (Y. Hu and P. C. Loizou, "Evaluation of Objective Quality Measures for Speech
    Enhancement", IEEE TASLP 16(1), 2008) of xhat against x per channel: gammatone bands between the two
    frequencies, 75 ms Hamming frames at half overlap, per frame the band spectra's log ratio weighted by |X|^gamma,
    clipped to snr_range_db, averaged over the frames.  An x with one channel is the original of every channel of
    xhat.  A frame in which a band's spectrum sums to zero makes the result NaN, as in the reference."""
    assert x.sampling_rate_hz == xhat.sampling_rate_hz, "Sampling rates do not match"
    fs_hz = x.sampling_rate_hz
    assert len(x) == len(xhat), "Signal lengths do not match"
    if x.number_of_channels != xhat.number_of_channels:
        assert x.number_of_channels == 1, "Invalid number of channels for this measurement"
    assert len(f_range_hz) == 2, "Frequency range must have lower and upper bounds"
    f_range = np.sort(np.asarray(f_range_hz))
    assert f_range[1] < fs_hz // 2, \
        f"Upper frequency range {f_range[1]} must be smaller than nyquist frequency {fs_hz // 2}"
    assert f_range[0] > 0, "Frequency range must be positive"
    assert len(snr_range_db) == 2, "SNR range must have lower and upper bounds"
    snr_range_db = np.sort(np.asarray(snr_range_db))
    length_samp = int(75e-3 * fs_hz)
    length_samp += length_samp % 2  # an even window, so that the hop is half of it
    window = windows.hamming(length_samp, sym=False)
    assert 0.1 <= gamma <= 2, f"{gamma} is not in the valid range for gamma [0.1, 5]"
    bank = auditory_filters_gammatone(frequency_range_hz=f_range, resolution=1, sampling_rate_hz=fs_hz)
    sections = [f._device_sections() for f in bank.filters]
    if x.is_complex_signal or xhat.is_complex_signal:
        raise NotImplementedError("complex input samples are not run through the device recursion (its input is real)")
    if x.on_device and xhat.on_device:
        return backend.fw_snr_seg(x.device_samples, xhat.device_samples, sections, window, snr_range_db, gamma)
    return backend.fw_snr_seg(x.time_data, xhat.time_data, sections, window, snr_range_db, gamma)


__all__ = ["log_spectral", "itakura_saito", "snr", "si_sdr", "fw_snr_seg"]
