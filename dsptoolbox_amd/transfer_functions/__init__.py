"""compute_transfer_function and spectral_deconvolve
(API mirror of dsptoolbox/transfer_functions/transfer_functions.py:419-539 and
:61-184; regularisation window helpers/windows.py:8-76, band detection
helpers/other.py:9-41), window_frequency_dependent (:1288-1377) and complex_smoothing (:1788-1876); the real-cepstrum
minimum-phase family min_phase_ir / minimum_phase / minimum_group_delay and group_delay / excess_group_delay
(:789-1083) on the float64 any-length transform (ds_min_phase, ds_group_delay_phase) and the direct DFT (ds_dft);
find_ir_latency (:1380-1406) on the latency entries (ds_latency)."""

import numpy as np
from scipy.fft import next_fast_len
from scipy.signal.windows import get_window

from .. import backend
from ..classes import ImpulseResponse, Signal, Spectrum
from ..standard.enums import SpectrumMethod, Window
from ..standard.latency_delay import _fractional_latency, latency
from .enums import SmoothingDomain, TransferFunctionType

__all__ = ["compute_transfer_function", "spectral_deconvolve", "window_frequency_dependent", "complex_smoothing",
           "min_phase_ir", "group_delay", "minimum_phase", "minimum_group_delay", "excess_group_delay",
           "find_ir_latency", "min_phase_from_mag", "lin_phase_from_mag", "TransferFunctionType", "SmoothingDomain"]


def compute_transfer_function(output: Signal, input: Signal, window_length_samples: int,
                              mode: TransferFunctionType = TransferFunctionType.H2) -> Spectrum:
    """Welch H1 / H2 / H3 transfer functions with coherence.  A one-channel
    input is the input of every output channel.  Window, overlap, detrend,
    average and scaling are taken from the INPUT signal's spectrum parameters."""
    assert input.sampling_rate_hz == output.sampling_rate_hz, "Sampling rates do not match"
    assert len(input) == len(output), "Signal lengths do not match"
    if input.number_of_channels != 1:
        assert input.number_of_channels == output.number_of_channels, \
            "Channel number does not match between signals"
    par = input._spectrum_parameters.copy()
    assert type(par) is dict, "Spectrum parameters should be passed as a dictionary"
    for k in ("window_length_samples", "method", "smoothing", "pad_to_fast_length"):
        par.pop(k)
    if not isinstance(mode, TransferFunctionType):
        raise ValueError("Unsupported transfer function type")
    W = int(window_length_samples)
    # device-resident samples (Signal.to_device / from_planar_f32): the fp32 kernels read them in place -- unless the
    # precision rule sends this shape through the float64 kernels, which take the host arrays.  One plan serves the
    # question and whichever route answers it; with invalid parameters there is none and the reference's assertion
    # comes from the host function.
    plan = None
    if output.on_device and not output.is_complex_signal and not input.is_complex_signal:
        plan = output._welch_plan({**par, "window_length_samples": W})
    if plan is None:
        # small problems run in float64 end to end like the reference (backend.TF_PRECISION)
        tf, coherence = backend.welch_transfer_function(
            output.time_data, input.time_data, input.sampling_rate_hz, window_length_samples,
            mode.name, precision=backend.TF_PRECISION, **par)
    elif backend._welch_route(plan, "tf", (input.number_of_channels, output.number_of_channels), "resident",
                              backend.TF_PRECISION) == backend.ROUTE_RESIDENT:
        tf, coherence = backend._tf_resident(plan, output.device_samples, input.to_device().device_samples, mode.name,
                                             narrow=True)
        return Spectrum._from_device_result(np.fft.rfftfreq(W, 1 / input.sampling_rate_hz), tf, coherence)
    else:
        tf, coherence = backend._tf_host(plan, output.time_data, input.time_data, mode.name, backend.TF_PRECISION)
    spec = Spectrum(np.fft.rfftfreq(window_length_samples, 1 / input.sampling_rate_hz), tf)
    spec.set_coherence(coherence)
    return spec


# ---- spectral deconvolution --------------------------------------------------
def _to_db_amplitude(x):
    tiny = float(np.finfo(np.float64).smallest_normal)
    return 20.0 * np.log10(np.clip(np.abs(x), a_min=tiny, a_max=None))


def find_frequencies_above_threshold(spec, f, threshold_db, normalize=True):
    d = _to_db_amplitude(spec)
    if normalize:
        d = d - np.max(d)
    fr = f[d > threshold_db]
    return [fr[0], fr[-1]]


def find_nearest_points_index_in_vector(points, vector):
    points = np.atleast_1d(np.array(points))
    return np.array([np.argmin(np.abs(p - vector)) for p in points], dtype=np.int_)


def _inverse_hann_band(ids, length: int):
    """1 - (0 .. Hann rise .. 1 .. Hann fall .. 0) over the four bin indices."""
    i0, i1, i2, i3 = [int(i) for i in ids]
    nl, nh = i1 - i0, i3 - i2
    low = get_window("hann", nl * 2, fftbins=True)[:nl] if nl > 0 else np.ones(nl)
    high = get_window("hann", nh * 2, fftbins=True)[nh:] if nh > 1 else np.ones(nh)
    w = np.concatenate((np.zeros(i0), low, np.ones(i2 - i1), high, np.zeros(length - i3)))
    return 1 - w


def _spectral_deconvolve_scaled(output, input, apply_regularization, start_stop_hz, threshold_db, padding,
                                keep_original_length, multichannel):
    """spectral_deconvolve for signals whose spectrum parameters ask for a scaling other than the plain
    transform (FFTForward / FFTOrthogonal norms, amplitude or power spectra in physical units): the
    reference divides whatever `get_spectrum` returns (transfer_functions.py:142-177, classes/signal.py:
    899-938 -- power scalings make both spectra real, |X|^2 k).  Transforms on the device
    (Signal.get_spectrum), the B x C division in float64 on the host, the inverse transform of any length
    on the device."""
    fs_hz = output.sampling_rate_hz
    original_length = output.time_data.shape[0]
    n_time = original_length * 2 if padding else original_length

    def spectrum_of(sig):
        td = sig.time_data
        if padding:
            td = np.concatenate((td, np.zeros_like(td)), axis=0)
        tmp = Signal(None, td, fs_hz)
        tmp._spectrum_parameters = dict(sig._spectrum_parameters)
        tmp.spectrum_method = SpectrumMethod.FFT
        return tmp.get_spectrum()

    _, denum_fft = spectrum_of(input)
    freqs_hz, num_fft = spectrum_of(output)
    if apply_regularization:
        if start_stop_hz is None:
            start_stop_hz = find_frequencies_above_threshold(denum_fft[:, 0], freqs_hz, threshold_db)
        if len(start_stop_hz) == 2:
            start_stop_hz = np.array([start_stop_hz[0] / np.sqrt(2), start_stop_hz[0], start_stop_hz[1],
                                      np.min([start_stop_hz[1] * np.sqrt(2), fs_hz / 2])])
        elif len(start_stop_hz) != 4:
            raise ValueError("start_stop_hz vector should have 2 or 4 values")
        ids = find_nearest_points_index_in_vector(start_stop_hz, freqs_hz)
        eps = _inverse_hann_band(ids, len(freqs_hz)) * 10 ** (30 / 20)
        den = denum_fft[:, :1] if multichannel else denum_fft
        prod = num_fft * (np.conj(den) / (np.abs(den) ** 2 + eps[:, None]))
    else:
        prod = num_fft / (denum_fft[:, :1] if multichannel else denum_fft)
    # np.fft.irfft(prod, n=n_time): the spectrum is cropped or zero-padded to n_time // 2 + 1 bins
    nb = n_time // 2 + 1
    spec = np.zeros((nb, prod.shape[1]), dtype=np.complex128)
    spec[: min(nb, prod.shape[0])] = prod[:nb]
    delta = np.zeros((n_time, prod.shape[1]))
    delta[0, :] = 1.0
    new_time_data = backend.spectral_division(delta, n_time, spec, n_time)
    new_sig = ImpulseResponse(None, new_time_data, fs_hz, constrain_amplitude=False)
    if padding and keep_original_length:
        new_sig.time_data = new_sig.time_data[:original_length].copy()
    return new_sig


def spectral_deconvolve(output: Signal, input: Signal, apply_regularization: bool = True,
                        start_stop_hz=None, threshold_db: float = -30.0, padding: bool = False,
                        keep_original_length: bool = False) -> ImpulseResponse:
    """Impulse response by (regularised) spectral division output / input."""
    assert len(output) == len(input), "Lengths do not match for spectral deconvolution"
    multichannel = input.number_of_channels == 1
    if not multichannel:
        assert output.number_of_channels == input.number_of_channels, \
            "The number of channels do not match."
    assert output.sampling_rate_hz == input.sampling_rate_hz, "Sampling rates do not match"
    if not apply_regularization:
        assert start_stop_hz is None, \
            "No start_stop_hz vector can be passed when using standard mode"
    # Only the spectrum METHOD is forced (transfer_functions.py:142-143): each signal's own scaling still
    # and smoothing still apply inside get_spectrum (classes/signal.py:899-938).  The defaults (FFTBackward, no
    # smoothing) give the plain transform and take the fused device path below; anything else goes through the
    # general one.
    plain = all(s._spectrum_parameters["scaling"].fft_norm() == "backward"
                and not s._spectrum_parameters["scaling"].has_physical_units()
                and s._spectrum_parameters["smoothing"] == 0 for s in (output, input))
    if not plain:
        return _spectral_deconvolve_scaled(output, input, apply_regularization, start_stop_hz, threshold_db,
                                           padding, keep_original_length, multichannel)
    fs_hz = output.sampling_rate_hz
    original_length = len(output)
    n_time = original_length * 2 if padding else original_length
    n_fft = (next_fast_len(n_time, True)
             if input._spectrum_parameters["pad_to_fast_length"] else n_time)
    if output.on_device and n_fft == n_time and not output.is_complex_signal and not input.is_complex_signal:
        # device-resident samples: spectrum of the input, regularised inverse, division and inverse transform on the
        # device; only the input's spectrum comes down for the band detection (and a (bins,) eps goes up)
        freqs_dev = np.fft.rfftfreq(n_fft, 1 / fs_hz)

        def eps_of(den, band=start_stop_hz):
            if band is None:  # band from the FIRST denominator channel only
                band = find_frequencies_above_threshold(den[:, 0], freqs_dev, threshold_db)
            if len(band) == 2:
                band = np.array([band[0] / np.sqrt(2), band[0], band[1], np.min([band[1] * np.sqrt(2), fs_hz / 2])])
            elif len(band) != 4:
                raise ValueError("start_stop_hz vector should have 2 or 4 values")
            return _inverse_hann_band(find_nearest_points_index_in_vector(band, freqs_dev), len(freqs_dev)) * 10 ** (30 / 20)

        n_out = original_length if (padding and keep_original_length) else n_time
        dev = backend.spectral_division_device(output.device_samples, input.to_device().device_samples, n_fft, n_out,
                                               eps_of if apply_regularization else None)
        return ImpulseResponse.from_planar_f32(dev, fs_hz)
    # rfft(n=n_fft) zero pads, so the optional x2 padding needs no copy
    denum_fft = backend.rfft_spectrum(input.time_data, n_fft)
    freqs_hz = np.fft.rfftfreq(n_fft, 1 / fs_hz)
    eps = None
    if apply_regularization:
        if start_stop_hz is None:  # band from the FIRST denominator channel only
            start_stop_hz = find_frequencies_above_threshold(denum_fft[:, 0], freqs_hz,
                                                             threshold_db)
        if len(start_stop_hz) == 2:
            start_stop_hz = np.array([start_stop_hz[0] / np.sqrt(2), start_stop_hz[0],
                                      start_stop_hz[1],
                                      np.min([start_stop_hz[1] * np.sqrt(2), fs_hz / 2])])
        elif len(start_stop_hz) != 4:
            raise ValueError("start_stop_hz vector should have 2 or 4 values")
        ids = find_nearest_points_index_in_vector(start_stop_hz, freqs_hz)
        eps = _inverse_hann_band(ids, len(freqs_hz)) * 10 ** (30 / 20)
    inverse = backend.regularized_inverse(denum_fft, eps)  # (B, Cx)
    if n_fft == n_time:
        new_time_data = backend.spectral_division(
            output.time_data, n_fft, inverse[:, 0] if multichannel else inverse, n_time)
    else:
        # The signal length is not a fast length: the reference transforms with n_fft =
        # next_fast_len(n_time) points but inverts with np.fft.irfft(..., n=n_time)
        # (_transfer_functions.py:37-41), and numpy then CROPS the spectrum to n_time//2 + 1 bins
        # and runs an n_time-point inverse (the bins keep their values but not their spacing).
        # Reproduced literally: forward spectrum on the device, the cropped product as a
        # per-channel "inverse spectrum" against a unit impulse (whose rfft is 1): the device
        # computes irfft_{n_time}(1 * product).
        num_fft = backend.rfft_spectrum(output.time_data, n_fft)               # (n_fft//2 + 1, C)
        prod = (num_fft * (inverse[:, :1] if multichannel else inverse))[: n_time // 2 + 1]
        delta = np.zeros((n_time, prod.shape[1]))
        delta[0, :] = 1.0
        new_time_data = backend.spectral_division(delta, n_time, prod, n_time)
    new_sig = ImpulseResponse(None, new_time_data, fs_hz, constrain_amplitude=False)
    if padding and keep_original_length:
        new_sig.time_data = new_sig.time_data[:original_length].copy()
    return new_sig


# ---- frequency-dependent windowing and complex smoothing (direct sums on the device) -----------------------------
def _fdw_parameters(time_data: np.ndarray, fs: int, cycles, end_window_value_db: float):
    """(f, alpha, peak, half) of window_frequency_dependent in the reference's statements
    (transfer_functions.py:1335-1358): the bins above DC, the Gaussian exponent factor per bin, the peak sample per
    channel and half the signal's span."""
    length = time_data.shape[0]
    end_window_value = 10 ** (end_window_value_db / 20.0)
    f = np.fft.rfftfreq(length, 1 / fs)[1:]
    cycles_per_freq_samples = np.round(fs / f * cycles).astype(int)
    if np.any(cycles_per_freq_samples == 0):
        raise ValueError("cycles gives a window of zero samples for the highest bins")
    half = (length - 1) / 2
    alpha_factor = np.log(1 / (end_window_value) ** 2) ** 0.5 * half
    peak = np.argmax(np.abs(time_data), axis=0)
    alpha = (alpha_factor / cycles_per_freq_samples) ** 2.0
    return f, alpha, peak, half


def window_frequency_dependent(ir: ImpulseResponse, cycles: int, end_window_value_db: float = -50.0) -> Spectrum:
    """The spectrum of an impulse response under a Gaussian window per frequency bin, centred on each channel's peak
    and `cycles` periods of the bin's frequency wide where it reaches `end_window_value_db`.  The windowed sums run on
    the device in float64 (ds_dft); window terms below 2^-70 are skipped."""
    assert type(ir) is ImpulseResponse, "This is only valid for an impulse response"
    assert end_window_value_db < 0.0, "Window ends must be less than 0 dB"
    fs = ir.sampling_rate_hz
    f, alpha, peak, half = _fdw_parameters(ir.time_data, fs, cycles, end_window_value_db)
    spec = backend.windowed_dft(ir.time_data, f, fs, alpha, peak, half)
    return Spectrum(np.hstack([0.0, f]), np.pad(spec, ((1, 0), (0, 0))))


def complex_smoothing(ir: ImpulseResponse, octave_fraction: float, smoothing_domain: SmoothingDomain,
                      window: Window = Window.Hann) -> Spectrum:
    """Complex smoothing of an impulse response's spectrum over +- 1 / (2 octave_fraction) octave around every bin
    (Hatziantoniou and Mourjopoulos), in the chosen domain, on the device (ds_complex_smooth)."""
    assert octave_fraction > 0.0, "Octave fraction must be greater than 0"
    if not isinstance(smoothing_domain, SmoothingDomain):
        raise ValueError("Invalid smoothing domain")
    f, sp = ir.get_spectrum()
    window_values = window(3000, True).astype(np.float64, order="C")
    return Spectrum(f, backend.complex_smoothing(sp, f, octave_fraction, smoothing_domain, window_values))


_NO_EQUIRIPPLE = ("use_real_cepstrum=False (scipy's equiripple / Hilbert design method, scipy.signal.minimum_phase) is "
                  "not built on the device")


def _pad_trim(td: np.ndarray, desired_length: int) -> np.ndarray:
    """helpers/other.py:216-259 for (N, C) data, at the end."""
    n = td.shape[0]
    if n >= desired_length:
        return td[:desired_length].copy()
    return np.concatenate([td, np.zeros((desired_length - n, td.shape[1]), dtype=td.dtype)])


def _group_delay_units(gd: np.ndarray, delta_f: float) -> np.ndarray:
    """The device returns -gradient(unwrap(phase)) / (2 pi delta_f), seconds.  The reference's _group_delay_direct
    (standard/_standard_backend.py:57-63) reads a frequency step of exactly 1 as "no step given" and returns
    -gradient(unwrap(phase)) with no 1 / (2 pi): radians per bin.  A one-second signal (fs == N; 6000 samples at 48 kHz
    with padding_factor 8) meets that branch, and so does this."""
    return gd * (2.0 * np.pi) if delta_f == 1 else gd


def min_phase_ir(sig: ImpulseResponse, use_real_cepstrum: bool = True, padding_factor: int = 8,
                 alpha: float = 1.0) -> ImpulseResponse:
    """The same impulse response with minimum phase by the real-cepstrum method: transform, log magnitude, inverse
    transform, cepstral fold, transform, exp and inverse transform run on the device in float64 at the length
    next_fast_len(len * padding_factor).  The alpha ** n scaling before and after stays on the host."""
    assert type(sig) is ImpulseResponse, "This is only valid for an impulse response"
    assert padding_factor > 1, "Padding factor should be at least 1"
    assert alpha <= 1.0 and alpha > 0.0, "Alpha must be in the range ]0, 1]"
    if not use_real_cepstrum:
        raise NotImplementedError(_NO_EQUIRIPPLE)
    new_time_data = sig.time_data.copy()
    if alpha != 1.0:
        new_time_data *= (alpha ** (np.arange(new_time_data.shape[0])))[:, None]
    n = new_time_data.shape[0]
    # the reference keeps all n_fft rows until the end and crops to len(sig) last: the rows past it are never seen
    new_time_data = backend.min_phase(new_time_data, backend.min_phase_fft_length(n, padding_factor), "ir", n_out=n)
    if alpha != 1.0:
        new_time_data *= (alpha ** (-np.arange(new_time_data.shape[0])))[:, None]
    return sig.copy_with_new_time_data(new_time_data[: len(sig)])


def _group_delay_analytic(b: np.ndarray, n_freq: int, fs: int) -> np.ndarray:
    """_group_delay_filter([b, [1]], n_freq, fs) (classes/filter_helpers.py:167-205) for the columns of b: the
    quotient of the direct DFTs of n b[n] and b[n] at omega = linspace(0, pi, n_freq) -- for an odd length these are
    not FFT bins -- evaluated on the device (ds_dft); the quotient, the non-finite -> 0 rule and / fs on the host."""
    freqs = np.linspace(0, np.pi, n_freq) / np.pi * (fs / 2)
    ramp = np.arange(b.shape[0], dtype=np.float64)[:, None]
    sp = backend.dft(np.concatenate([b * ramp, b], axis=1), freqs, fs)
    with np.errstate(divide="ignore", invalid="ignore"):
        gd = np.real(sp[:, :b.shape[1]] / sp[:, b.shape[1]:])  # - len(a) + 1 = 0 for a = [1]
    gd[~np.isfinite(gd)] = 0
    return gd / fs


_NO_PUBLIC_LATENCY_FREE = ("group_delay(analytic_computation=False, remove_ir_latency=True) is not built into the public "
                           "function (DESIGN section 20): transfer_functions._group_delay computes it on the device")


def group_delay(signal: Signal, analytic_computation: bool = True, smoothing: int = 0,
                remove_ir_latency: bool = False):
    """_group_delay below, except that the numerical form with remove_ir_latency still raises NotImplementedError here
    (and so in excess_group_delay at its default analytic_computation=False): the refusal is part of what the package
    has promised so far, and is lifted separately."""
    if not analytic_computation and remove_ir_latency:
        raise NotImplementedError(_NO_PUBLIC_LATENCY_FREE)
    return _group_delay(signal, analytic_computation, smoothing, remove_ir_latency)


def _group_delay(signal: Signal, analytic_computation: bool = True, smoothing: int = 0, remove_ir_latency: bool = False):
    """Group delay in seconds (numerical form with a frequency step of exactly 1 Hz: radians per bin, as the reference
    returns it there), (frequency vector, (gd, channel) matrix).  analytic_computation: the quotient form of
    https://www.dsprelated.com/freebooks/filters/Phase_Group_Delay.html from two direct DFTs on the device; otherwise
    the gradient of the unwrapped phase of the spectrum, transform to gradient on the device (ds_group_delay_phase).
    remove_ir_latency (impulse responses, zero-padded to next_fast_len(8 N)): the analytic form starts each channel
    one sample before its peak; the numerical form takes out the sub-sample latency against the minimum-phase
    equivalent (padding factor 1) as a linear phase BEFORE the unwrap, wrapped again as the reference does
    (ds_group_delay_phase_lat)."""
    length_time_signal = (next_fast_len(signal.time_data.shape[0] * 8, True) if remove_ir_latency
                          else signal.time_data.shape[0])
    td = _pad_trim(signal.time_data, length_time_signal)
    fs = signal.sampling_rate_hz
    f = np.fft.rfftfreq(td.shape[0], 1 / fs)
    if not analytic_computation:
        latency_samples = None
        if remove_ir_latency:
            assert type(signal) is ImpulseResponse, "This is only valid for an impulse response"
            # _remove_ir_latency_from_phase_min_phase (helpers/minimum_phase.py:82-117): all n_fft rows of the
            # minimum-phase response are compared, not the first N
            n_min = backend.min_phase_fft_length(signal.time_data.shape[0], 1)
            min_ir = backend.min_phase(signal.time_data, n_min, "ir", n_out=n_min)
            latency_samples = _fractional_latency(signal.time_data, min_ir, 1)
        group_delays = _group_delay_units(backend.group_delay_phase(td, f[1] - f[0], latency_samples, fs), f[1] - f[0])
    elif remove_ir_latency:
        group_delays = np.zeros((length_time_signal // 2 + 1, td.shape[1]))
        for n in range(signal.number_of_channels):
            b = td[:, n]
            b = b[max(int(np.argmax(np.abs(b))) - 1, 0):]
            group_delays[:, n] = _group_delay_analytic(b[:, None], len(f), fs)[:, 0]
    else:
        group_delays = _group_delay_analytic(td, len(f), fs)
    if smoothing != 0:
        group_delays = backend.fractional_octave_smoothing(group_delays, None, smoothing)
    return f, group_delays


def _min_phase_frequencies(n_fft: int, fs: int) -> np.ndarray:
    f = np.fft.fftfreq(n_fft, 1 / fs)
    if n_fft % 2 == 0:
        f[n_fft // 2] *= -1
    return f[f >= 0]


def minimum_phase(signal: ImpulseResponse, use_real_cepstrum: bool = True, padding_factor: int = 8):
    """(frequency vector, (phase, channel) matrix) of the minimum-phase equivalent by the real-cepstrum method, on the
    non-negative bins of the length next_fast_len(len * padding_factor)."""
    assert type(signal) is ImpulseResponse, "This is only valid for an impulse response"
    if not use_real_cepstrum:
        raise NotImplementedError(_NO_EQUIRIPPLE)
    n_fft = backend.min_phase_fft_length(signal.time_data.shape[0], padding_factor)
    return _min_phase_frequencies(n_fft, signal.sampling_rate_hz), backend.min_phase(signal.time_data, n_fft, "phase")


def minimum_group_delay(signal: ImpulseResponse, smoothing: int = 0, padding_factor: int = 8):
    """(frequency vector, (gd, channel) matrix in seconds) of the minimum-phase equivalent: its phase is unwrapped
    and differentiated on the device.  At a frequency step of exactly 1 Hz the reference returns radians per bin; so
    does this (_group_delay_units)."""
    assert type(signal) is ImpulseResponse, "This is only valid for an impulse response"
    n_fft = backend.min_phase_fft_length(signal.time_data.shape[0], padding_factor)
    f = _min_phase_frequencies(n_fft, signal.sampling_rate_hz)
    min_gd = _group_delay_units(backend.min_phase(signal.time_data, n_fft, "group_delay", delta_f=f[1] - f[0]), f[1] - f[0])
    if smoothing != 0:
        min_gd = backend.fractional_octave_smoothing(min_gd, None, smoothing)
    return f, min_gd


def excess_group_delay(signal: ImpulseResponse, smoothing: int = 0, remove_ir_latency: bool = False,
                       analytic_computation: bool = False):
    """(frequency vector, (excess gd, channel) matrix in seconds): the group delay less the minimum group delay (no
    zero-padding for the minimum-phase equivalent).  Where the two frequency vectors differ the group delay is
    interpolated linearly onto the minimum group delay's, 0 outside, on the host.  The numerical form with
    remove_ir_latency raises NotImplementedError as group_delay does; _excess_group_delay computes it."""
    assert type(signal) is ImpulseResponse, "This is only valid for an impulse response"
    if not analytic_computation and remove_ir_latency:
        raise NotImplementedError(_NO_PUBLIC_LATENCY_FREE)
    return _excess_group_delay(signal, smoothing, remove_ir_latency, analytic_computation)


def _excess_group_delay(signal: ImpulseResponse, smoothing: int = 0, remove_ir_latency: bool = False,
                        analytic_computation: bool = False):
    assert type(signal) is ImpulseResponse, "This is only valid for an impulse response"
    f_min, min_gd = minimum_group_delay(signal, smoothing=0, padding_factor=1)
    f, gd = _group_delay(signal, smoothing=0, analytic_computation=analytic_computation,
                         remove_ir_latency=remove_ir_latency)
    if len(f) != len(f_min):
        from scipy.interpolate import interp1d
        gd = interp1d(f, gd, kind="linear", copy=False, bounds_error=False, assume_sorted=True, fill_value=(0.0, 0.0),
                      axis=0)(f_min)
    ex_gd = gd - min_gd
    if smoothing != 0:
        ex_gd = backend.fractional_octave_smoothing(ex_gd, None, smoothing)
    return f_min, ex_gd


def find_ir_latency(ir: ImpulseResponse, compare_to_min_phase_ir: bool = True) -> np.ndarray:
    """The sub-sample position of each channel's peak, in samples: the latency of the response against its own
    minimum-phase equivalent (padding factor 8; `latency` with one polynomial point), or, compare_to_min_phase_ir
    False, the zero crossing of the Hilbert transform around the peak of the time data itself."""
    assert type(ir) is ImpulseResponse, "This is only valid for an impulse response"
    if compare_to_min_phase_ir:
        return latency(ir, min_phase_ir(ir), 1)[0]
    peaks, window, near, _ = backend.latency_peaks(ir.time_data, None, 1)
    return backend.fractional_peak_rows(peaks, window, near, 1)


def min_phase_from_mag(spectrum: Spectrum, sampling_rate_hz: int, ir_length_samples: int | None = None):
    raise NotImplementedError("min_phase_from_mag is not built: it needs Spectrum.get_interpolated_spectrum, which "
                              "this package does not have")


def lin_phase_from_mag(spectrum: Spectrum, sampling_rate_hz: int, group_delay_ms: float | None = None,
                       check_causality: bool = True, minimum_group_delay_factor: float = 1.0):
    raise NotImplementedError("lin_phase_from_mag is not built: it needs Spectrum.get_interpolated_spectrum, which "
                              "this package does not have")
