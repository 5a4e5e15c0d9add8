"""transforms: the inverse STFT (dsptoolbox/transforms/transforms.py:444-586, SURVEY.md section 8(f)
row 1) and the STFT consumers log_mel_spectrogram / mfcc / chroma_stft (:113-203, :335-441, :589-684,
row 4) on the device, and hilbert / cepstrum / from_complex_cepstrum (:59-110, :763-809) on the float64 any-length
transform (ds_hilbert, ds_cepstrum, ds_from_cepstrum), and lpc (:1199-1283) on the linear-prediction kernels (ds_lpc,
ds_lpc_synth), and warp / laguerre / warp_filter (:955-1196, transforms/_transforms.py:386-463) on the all-pass table
kernel (ds_allpass_table).  Same signature, parameter handling and quirks as the reference;
the frame-wise inverse FFTs and the windowed overlap-add with the squared-window envelope
(standard/_framed_signal_representation.py:70-137) run in the HIP library (ds_istft).  The continuous wavelet
transform cwt with Wavelet / MorletWavelet (:687-760, transforms/_transforms.py:29-301) lives in _wavelets.py.
dft (:1286-1327) is the direct sum at arbitrary frequencies (ds_dft).  vqt (:812-923, transforms/_transforms.py:327-383)
runs its decimators, its kernel bank and its polyphase interpolators in float64 on the device (ds_vqt)."""

from __future__ import annotations

import numpy as np
from scipy.signal import get_window

from .. import backend
from ..classes.filter import Filter
from ..classes.multibandsignal import MultiBandSignal
from ..classes.signal import Signal
from ..standard.enums import FilterCoefficientsType, Window
from ._wavelets import MorletWavelet, Wavelet, cwt  # noqa: F401

__all__ = ["istft", "mel_filterbank", "log_mel_spectrogram", "mfcc", "chroma_stft", "cwt", "Wavelet", "MorletWavelet",
           "dft", "hilbert", "cepstrum", "from_complex_cepstrum", "lpc", "warp", "laguerre", "warp_filter", "vqt"]


def dft(signal: Signal, frequency_vector_hz) -> np.ndarray:
    """DFT for any set of frequencies: the (frequency bin, channel) complex128 spectrum of the direct sum, on the
    device in float64.  The samples of a device-resident signal are read where they are."""
    freqs = np.asarray(frequency_vector_hz, dtype=np.float64)
    if signal.on_device and not signal.is_complex_signal:
        return backend.dft(signal.device_samples, freqs, signal.sampling_rate_hz)
    return backend.dft(signal.time_data, freqs, signal.sampling_rate_hz)


def _pad_trim(td: np.ndarray, desired_length: int) -> np.ndarray:
    """helpers/other.py:216-259 for (N, C) data, at the end."""
    n = td.shape[0]
    if n >= desired_length:
        return td[:desired_length].copy()
    return np.concatenate([td, np.zeros((desired_length - n, td.shape[1]), dtype=td.dtype)])


def istft(stft, original_signal: Signal | None = None, parameters: dict | None = None,
          sampling_rate_hz: int | None = None, window_length_samples: int | None = None,
          window_type=None, overlap_percent: int | None = None,
          fft_length_samples: int | None = None, padding: bool | None = None,
          scaling=None) -> Signal:
    """Complex STFT (frequency, time frame, channel) -> time signal (Griffin & Lim)."""
    resident = isinstance(stft, backend.DeviceSTFT)  # Signal.get_spectrogram(on_device=True): stays in HBM
    if not resident:
        stft = np.asarray(stft)
    assert len(stft.shape) == 3, f"{len(stft.shape)} is not a valid number of dimensions. It must be 3"
    if original_signal is not None:
        assert parameters is None, "A signal was passed. No parameters dictionary should be passed"
        parameters = original_signal._spectrogram_parameters.copy()
    elif parameters is not None:
        pass
    else:
        assert ((window_length_samples is not None) and (window_type is not None)
                and (overlap_percent is not None) and (padding is not None)
                and (scaling is not None)), \
            "At least one of the needed parameters needed was passed as None"
        parameters = {"window_length_samples": window_length_samples, "window_type": window_type,
                      "overlap_percent": overlap_percent, "fft_length_samples": fft_length_samples,
                      "padding": padding, "scaling": scaling}
    W = parameters["window_length_samples"]
    window = get_window(parameters["window_type"].to_scipy_format(), W)
    sc = parameters["scaling"]
    # irfft(..., n=None) takes n = 2 (bins - 1)
    nfft = parameters["fft_length_samples"]
    nfft_eff = 2 * (stft.shape[0] - 1) if nfft is None else int(nfft)
    norm = sc.fft_norm()
    scale = {"backward": 1.0 / nfft_eff, "forward": 1.0, "ortho": nfft_eff ** -0.5}[norm]
    if sc.has_physical_units():
        scale = scale / float(np.asarray(sc.get_scaling_factor(nfft, sampling_rate_hz, window)).ravel()[0])
    step = int((1 - parameters["overlap_percent"] / 100) * len(window))
    n_frames = stft.shape[1]
    pad = bool(parameters["padding"])
    if resident:
        from .._lib import DevicePlanar
        dev = backend._istft_device(stft, nfft_eff, W, step, window, scale, frame_offset=0 if pad else 1,
                                    n_frames_total=n_frames if pad else n_frames + 2)
        cut = int(parameters["overlap_percent"] / 100 * len(window)) if pad else step
        length = dev.n_samples - 2 * cut
        want = len(original_signal) if original_signal is not None else length
        if cut > 0 and 0 < want <= length:
            # trimming both ends (and to the original length) is a view of the same device samples
            view = DevicePlanar(dev.owner, dev.n_ch, want, dev.ld, 4 * cut)
            if original_signal is not None:
                return original_signal._device_result(view)
            return Signal.from_planar_f32(view, sampling_rate_hz)
        td = backend._interleaved_f64(dev.to_planar())  # (padding would need zeros behind the samples: host)
    else:
        td = backend._istft(stft, nfft_eff, W, step, window, scale, frame_offset=0 if pad else 1,
                            n_frames_total=n_frames if pad else n_frames + 2)
    if pad:
        overlap = int(parameters["overlap_percent"] / 100 * len(window))
        td = td[overlap:-overlap, :]
    else:
        td = td[step:-step, :]
    if original_signal is not None:
        td = _pad_trim(td, len(original_signal))
        return original_signal.copy_with_new_time_data(td)
    return Signal(None, time_data=td, sampling_rate_hz=sampling_rate_hz)


def _hz2mel(f):
    """helpers/frequency_conversion.py:7-25"""
    return 2595 * np.log10(1 + f / 700)


def _mel2hz(mel):
    """helpers/frequency_conversion.py:28-46"""
    return 700 * (10 ** (mel / 2595) - 1)


def mel_filterbank(f_hz, range_hz=None, n_bands: int = 40, normalize: bool = True):
    """Equidistant mel triangle filters (bands, frequency) and their centre frequencies in mel
    (transforms/transforms.py:206-277).  Host-side parameter preparation."""
    f_hz = np.squeeze(f_hz)
    assert f_hz.ndim == 1, "f_hz should be a 1D-array"
    n_bands = int(n_bands)
    if range_hz is None:
        range_hz = f_hz[[0, -1]]
    else:
        range_hz = np.atleast_1d(np.asarray(range_hz).squeeze())
        assert len(range_hz) == 2, "range_hz should be an array with exactly two values!"
        range_hz = np.sort(range_hz)
        assert range_hz[-1] <= f_hz[-1], (
            f"Upper frequency in range {range_hz[-1]} is bigger than nyquist frequency {f_hz[-1]}")
        assert range_hz[0] >= 0, "Lower frequency in range must be positive"
    range_mel = _hz2mel(range_hz)
    mel_center_freqs = np.linspace(range_mel[0], range_mel[1], n_bands + 2, endpoint=True)
    bands_hz = _mel2hz(mel_center_freqs)
    inds = np.array([np.argmin(np.abs(b - f_hz)) for b in bands_hz], dtype=int)
    mel_filters = np.zeros((n_bands, len(f_hz)))
    for n in range(n_bands):
        ni = n + 1
        mel_filters[n, inds[ni - 1]:inds[ni]] = np.linspace(0, 1, inds[ni] - inds[ni - 1], endpoint=False)
        mel_filters[n, inds[ni]:inds[ni + 1]] = np.linspace(1, 0, inds[ni + 1] - inds[ni], endpoint=False)
        if normalize:
            mel_filters[n, :] /= np.sum(mel_filters[n, :])
    return mel_filters, mel_center_freqs[1:-1]


def _band_power(signal: Signal, filters, f_hz_check, to_db: bool, dct_abs: bool):
    par = signal._spectrogram_parameters
    return backend._spectrogram_band_power(
        signal.device_samples if signal.on_device else signal.time_data, signal.sampling_rate_hz,
        par["window_length_samples"], par["window_type"],
        par["overlap_percent"], par["fft_length_samples"], par["detrend"], par["padding"], par["scaling"],
        filters, to_db, dct_abs)


def _spectrogram_axes(signal: Signal):
    par = signal._spectrogram_parameters
    plan = backend._stft_plan(len(signal), signal.number_of_channels, signal.sampling_rate_hz, par["window_length_samples"],
                              par["window_type"], par["overlap_percent"], par["fft_length_samples"], par["detrend"],
                              par["padding"], par["scaling"])  # from the shape alone: the samples stay where they are
    return plan.time_s, plan.freqs_hz, plan.B


def log_mel_spectrogram(s: Signal, channel: int = 0, range_hz=None, n_bands: int = 40,
                        generate_plot: bool = True, stft_parameters: dict | None = None):
    """-> (time_s, f_mel, log_mel_sp (bands, time frame, channel)); STFT, |.|^2, the mel filter
    contraction and the dB conversion run on the device."""
    if generate_plot:
        raise NotImplementedError("plotting is outside the GPU hot path: pass generate_plot=False")
    if stft_parameters is not None:
        s.set_spectrogram_parameters(**stft_parameters)
    time_s, f_hz, n_bins = _spectrogram_axes(s)
    mfilt, f_mel = mel_filterbank(f_hz, range_hz, n_bands, normalize=True)
    assert mfilt.shape[1] == n_bins, \
        "the frequency vector (window length) and the STFT (fft length) have different bin counts"
    _, _, log_mel_sp = _band_power(s, mfilt, f_hz, True, False)
    return time_s, f_mel, log_mel_sp


def mfcc(signal: Signal, channel: int = 0, mel_filters=None, generate_plot: bool = True,
         stft_parameters: dict | None = None):
    """-> (time_s, f_mel, mfcc (cepstral coefficients, time frame, channel))."""
    if generate_plot:
        raise NotImplementedError("plotting is outside the GPU hot path: pass generate_plot=False")
    if stft_parameters is not None:
        signal.set_spectrogram_parameters(**stft_parameters)
    time_s, f, n_bins = _spectrogram_axes(signal)
    if mel_filters is None:
        mel_filters, f_mel = mel_filterbank(f, None, n_bands=40)
    else:
        mel_filters = np.asarray(mel_filters)
        f_mel = np.array([0, mel_filters.shape[0]])
    assert mel_filters.shape[1] == n_bins, (
        f"Shape of the mel filter matrix {mel_filters.shape} does not match the STFT")
    _, _, out = _band_power(signal, mel_filters, f, True, True)
    return time_s, f_mel, out


def _pitch2frequency(tuning_a_hz: float = 440):
    """transforms/_transforms.py:10-26: frequencies of the MIDI pitches 0..127 (0 is C0)."""
    return tuning_a_hz * 2 ** ((np.arange(128) - 69) / 12)


def chroma_stft(signal: Signal, tuning_a_hz: float = 440, compression: float = 0.5, plot_channel: int = -1):
    """Chroma features and pitch log-STFT (transforms/transforms.py:589-684).
    -> (time_s, chroma_stft (12 notes C..B, time frame, channel), pitch_stft (128, time frame,
    channel)).  The STFT, |.|^2 and the contraction onto the quarter-tone pitch bands run on the
    device (the spectrogram never leaves it); the octave sums over the 128 pitch rows and the
    logarithmic compression are done on the (128, F, C) result."""
    assert tuning_a_hz > 0, "Tuning A4 must be greater than zero"
    assert compression > 0, "Compression factor must be greater than zero"
    if plot_channel != -1:
        raise NotImplementedError("plotting is outside the GPU hot path: pass plot_channel=-1")
    time_s, f, n_bins = _spectrogram_axes(signal)
    pitch_frequencies = _pitch2frequency(tuning_a_hz)
    pitch_transformation = np.zeros((len(pitch_frequencies), len(f)))
    for ind, fn in enumerate(pitch_frequencies):
        pitch_transformation[ind, (f >= fn * 2 ** (-1 / 24)) & (f < fn * 2 ** (1 / 24))] = 1
    assert pitch_transformation.shape[1] == n_bins, \
        "the frequency vector (window length) and the STFT (fft length) have different bin counts"
    _, _, pitch_stft = _band_power(signal, pitch_transformation, f, False, False)
    n_notes = 12
    chroma_transformation = np.zeros((n_notes, len(pitch_frequencies)))
    for i in range(n_notes):
        chroma_transformation[i, i::n_notes] = 1
    chroma = np.tensordot(chroma_transformation, pitch_stft, (1, 0))
    return time_s, np.log(1 + compression * chroma), np.log(1 + compression * pitch_stft)


def hilbert(signal: Signal | MultiBandSignal) -> Signal | MultiBandSignal:
    """The analytic signal: the real part in `time_data`, the imaginary part in `time_data_imaginary`.  The transform,
    the one-sided mask and the inverse transform run on the device in float64 for any length."""
    if isinstance(signal, Signal):
        return signal.copy_with_new_time_data(backend.hilbert(signal.time_data))
    if type(signal) is MultiBandSignal:
        new_mb = signal.copy()
        for ind, b in enumerate(new_mb):
            new_mb.bands[ind] = hilbert(b)
        return new_mb
    raise TypeError("Signal does not have a valid type")


def cepstrum(signal: Signal, complex: bool = True) -> np.ndarray:
    """The cepstrum in the quefrency domain, (quefrency, channel) complex128: ifft(log(fft(x))) with the principal
    logarithm, or the real cepstrum ifft(log|fft(x)|) when `complex` is False."""
    return backend.cepstrum(signal.time_data, complex)


def from_complex_cepstrum(cepstrum: np.ndarray, sampling_rate_hz: int) -> Signal:
    """The real signal of a complex cepstrum of shape (quefrency, channel)."""
    ceps = np.asarray(cepstrum)
    return Signal.from_time_data(backend.from_complex_cepstrum(ceps[:, None] if ceps.ndim == 1 else ceps), sampling_rate_hz)


def lpc(signal: Signal, order: int, window_length_samples: int, synthesize_encoded_signal: bool = False,
        use_burg_method: bool = False, hop_size_samples: int | None = None, window_type: Window = Window.Hann):
    """Linear-predictive coding of every windowed frame: (a, variances) with a of shape (coefficient, frame, channel),
    a[0] = 1, and variances (frame, channel); or, with `synthesize_encoded_signal`, only the Signal resynthesized from
    them with white noise as the source (drawn by np.random.normal as the reference draws it, channel outer, frame
    inner).  Yule-Walker (biased autocorrelation, Levinson-Durbin) or Burg's method; the hop defaults to half the window.
    Framing, windowing, the estimators, the all-pole filters and the overlap-add run on the device in float64; the
    samples of a device-resident real signal are read where they lie.

    Kept from the reference: there are ceil(len(signal) / hop) frames, the last ones zero-padded; Burg returns
    window_length_samples + 1 coefficient rows (zeros after row `order`) and as "variance" the running denominator of
    its recursion, not divided by the frame length; a frame that is all zeros after windowing gives NaN coefficients and
    variance with Yule-Walker and [1, 0, ...], 0 with Burg; ValueError("Invalid prediction error: Singular Matrix")
    when a Yule-Walker prediction error is <= 0."""
    L = int(window_length_samples)
    hop = L // 2 if hop_size_samples is None else int(hop_size_samples)
    order = int(order)
    if order < 1:
        raise ValueError("lpc: the order must be at least 1")
    if order >= L:
        raise ValueError(f"lpc: the order ({order}) must be below the window length ({L})")
    if hop < 1:
        raise ValueError("lpc: the hop size must be at least 1")
    if signal.is_complex_signal:
        raise ValueError("lpc: the signal must be real")
    window = get_window(window_type.to_scipy_format(), L, fftbins=True)
    n = len(signal)
    n_frames = backend._lpc_frames(n, hop)
    backend._lpc_guard(n_frames, signal.number_of_channels, L, order)
    samples = signal.device_samples if signal.on_device else signal.time_data
    a, var = backend.lpc(samples, order, window, hop, "burg" if use_burg_method else "yule_walker")
    if not synthesize_encoded_signal:
        if use_burg_method:  # the reference's array has window_length + 1 rows (helpers/ar_estimation.py:168-170)
            a = np.concatenate([a, np.zeros((L - order,) + a.shape[1:])])
        return a, var
    sources = np.empty((L, n_frames, a.shape[2]))
    for channel in range(a.shape[2]):
        for n_window in range(n_frames):
            sources[:, n_window, channel] = np.random.normal(0.0, var[n_window, channel] ** 0.5, L)
    y = backend.lpc_synthesize(a, sources, window, hop, n)
    return Signal.from_time_data(y, signal.sampling_rate_hz)


def _get_warping_factor(warping_factor: float | str, fs_hz: int) -> float:
    """A float is asserted to lie in ]-1, 1[; "bark" / "erb" give the factor of the bilinear approximation of that scale
    after Smith & Abel (1999), eq. 26 and 30, and "bark-" / "erb-" its negative, for de-warping.  Any other string is
    a ValueError, any other type (an int, a numpy float) a TypeError.  As in the reference the formulas receive the
    sampling rate in Hz although they were fitted to kHz: "bark" is about -0.876 and "erb" about -0.777 at every audio
    rate."""
    if type(warping_factor) is float:
        assert np.abs(warping_factor) < 1.0, "Warping factor has to be in ]-1; 1["
        return warping_factor
    if type(warping_factor) is not str:
        raise TypeError("Invalid type for warping factor")
    name = warping_factor.lower()
    sign = -1.0 if name[-1:] in ("k", "b") else 1.0  # a trailing "-" (any other last character) inverts
    if "bark" in name:
        return sign * (1.0674 * (2.0 / np.pi * np.arctan(0.06583 * fs_hz)) ** 0.5 - 0.1916)
    if "erb" in name:
        return sign * (0.7446 * (2.0 / np.pi * np.arctan(0.1418 * fs_hz)) ** 0.5 + 0.03237)
    raise ValueError("Warping factor approximation is not supported")


def _find_ir_start(ir: np.ndarray, threshold_dbfs: float = -20) -> int:
    """room_acoustics/_room_acoustics.py:88-115: walking back from the peak of a 1-D response, the first sample whose
    magnitude is below the peak by the threshold (0 if there is none)."""
    mag = np.abs(ir)
    peak = int(np.argmax(mag))
    below = np.nonzero(mag[:peak + 1] < mag[peak] * 10 ** (-np.abs(threshold_dbfs) / 20.0))[0]
    return int(below[-1]) if len(below) else 0


def warp(ir: Signal, warping_factor: float | str, shift_ir: bool, total_length: int | None = None):
    """The frequency-warped impulse response (a warped FIR filter, Haermae et al. 2000): sample i of every channel
    weights the all-pass (z^-1 - lambda) / (1 - lambda z^-1) applied i times to a unit pulse.  A negative factor
    pre-warps (more resolution at low frequencies), the same positive factor de-warps.  "bark", "erb" take the factor
    from the sampling rate (see _get_warping_factor; "bark-", "erb-" de-warp) and the factor is returned beside the
    Signal.  `shift_ir` rolls every channel so that the sample before it first comes within 20 dB of its peak is
    first (the operation is not shift-invariant).  `total_length` truncates the input, and with it the output.

    The table of all-pass responses and its contraction with the samples run on the device in float64, one launch per
    anti-diagonal of tiles; nothing is printed.  The samples of a device-resident signal are read where they lie unless
    `shift_ir` is set: the roll is done on the host and materialises them there.  NotImplementedError beyond
    backend.WARP_MAX_SIDE samples."""
    approximation = type(warping_factor) is str
    factor = _get_warping_factor(warping_factor, ir.sampling_rate_hz)
    n = len(ir) if total_length is None else len(range(len(ir))[:total_length])
    backend._warp_check(n, n, ir.number_of_channels)
    if ir.on_device and not shift_ir and not ir.is_complex_signal:
        from .._lib import DevicePlanar
        dev = ir.device_samples
        samples = dev if n == dev.n_samples else DevicePlanar(dev.owner, dev.n_ch, n, dev.ld, dev.offset_bytes)
    else:
        samples = ir.time_data.copy()
        if shift_ir:
            for ch in range(ir.number_of_channels):
                samples[:, ch] = np.roll(samples[:, ch], -_find_ir_start(samples[:, ch], -20))
        samples = samples[:n]
    warped = ir.copy_with_new_time_data(backend.warp_time_series(samples, factor))
    return (warped, factor) if approximation else warped


def laguerre(signal: Signal, warping_factor: float) -> Signal:
    """The discrete Laguerre transform in the time domain (Zoelzer, DAFX, chapter 11): the same frequency mapping as
    `warp`, with orthonormal basis functions.  Applying it with `warping_factor` and then with `-warping_factor`
    undoes it up to the truncation to the signal's length.  The table of basis functions and its contraction with the
    samples run on the device in float64; the samples of a device-resident signal are read where they lie.
    AssertionError for |warping_factor| >= 1, NotImplementedError beyond backend.WARP_MAX_SIDE samples."""
    assert np.abs(warping_factor) < 1.0, "Warping factor cannot be larger than 1."
    backend._warp_check(len(signal), len(signal), signal.number_of_channels)
    samples = signal.device_samples if signal.on_device and not signal.is_complex_signal else signal.time_data
    return signal.copy_with_new_time_data(backend.laguerre_transform(samples, float(warping_factor)))


def warp_filter(filter: Filter, warping_factor: float) -> Filter:
    """The filter with z^-1 replaced by (z^-1 - lambda) / (1 - lambda z^-1): every pole and zero r moves to
    (lambda + r) / (1 + lambda r), and the shorter of the two lists is filled up with `warping_factor`.  The gain is
    kept.  Host arithmetic on zpk; the result is Filter.from_zpk, so the stable-poles rule of Filter applies."""
    assert abs(warping_factor) < 1.0, "Warping factor must be less than 1."
    z, p, k = filter.get_coefficients(FilterCoefficientsType.Zpk)
    z, p = np.atleast_1d(z), np.atleast_1d(p)
    z, p = (warping_factor + z) / (1 + warping_factor * z), (warping_factor + p) / (1 + warping_factor * p)
    fill = [warping_factor] * abs(len(p) - len(z))
    if len(p) > len(z):
        z = np.hstack([z, fill])
    elif len(z) > len(p):
        p = np.hstack([p, fill])
    return Filter.from_zpk(z, p, k, filter.sampling_rate_hz)


def vqt(signal: Signal, channel=None, q: float = 1, gamma: float = 50, octaves: list = [1, 5], bins_per_octave: int = 24,
        a4_tuning: int = 440, window: str | tuple = "hann", *, on_device: bool = False):
    """Variable-Q transform: (f, vqt) with the coefficients (frequency, time sample, channel) complex128 at the input
    rate, the lowest frequency first.  `gamma = 0` gives the constant-Q transform.  The signal is decimated by
    d = int((fs // 2) / (1.1 highest_f)) and then by 2 per octave; every octave is convolved (same mode) with the same
    `bins_per_octave` windowed complex exponentials (window from scipy.signal.get_window, normalised to a unit sum,
    length round(q mid_fs / (f_i (2^(1/bins) - 1) + gamma mid_fs / fs))); every row is brought back to the input rate by
    polyphase interpolation (scipy.signal.resample_poly's default filter) and cut at the signal's length.  All of it runs
    on the device in float64; the samples of a device-resident real signal are read where they lie.  With `on_device=True`
    the coefficients stay in HBM as a `backend.DeviceScalogram` (complex128).

    Kept from the reference: `f` has 12 entries per octave whatever `bins_per_octave` is (60 beside 120 rows at the
    defaults); a `channel` subset raises ValueError (the reference's accumulator is sized by all channels);
    ZeroDivisionError when the top octave lies above Nyquist / 1.1; mid_fs = fs // d is an integer, not the true rate.
    NotImplementedError beyond backend.VQT_MAX_DECIMATION, VQT_MAX_OCTAVES, VQT_MAX_KERNEL, VQT_MAX_ROWS and
    VQT_MAX_OUTPUT_BYTES."""
    if channel is None:
        channel = np.arange(signal.number_of_channels)
    channel = np.atleast_1d(channel)
    if len(channel) != signal.number_of_channels:
        raise ValueError("all the input array dimensions except for the concatenation axis must match exactly, but along "
                         f"dimension 2, the array at index 0 has size {signal.number_of_channels} and the array at index "
                         f"1 has size {len(channel)}")
    whole = np.array_equal(channel, np.arange(signal.number_of_channels))
    if signal.on_device and whole and not signal.is_complex_signal:
        samples = signal.device_samples
    else:
        samples = signal.time_data[:, channel]
    coefficients = backend.vqt(samples, signal.sampling_rate_hz, q, gamma, octaves, bins_per_octave, a4_tuning, window,
                               on_device=on_device)
    f = a4_tuning * 2 ** (np.arange(octaves[0] - 4 - 9 / 12, octaves[1] - 4 + 2 / 12, 1 / 12))
    return f, coefficients
