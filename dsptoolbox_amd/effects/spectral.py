"""Spectral subtraction on the device: `SpectralSubtractor`, the denoiser of the reference's effects module
(effects/effects.py:138-550), with its constructor, setters, assertions, warnings and defaults.

Every sample is computed by the HIP kernels of csrc/kernels_specsub.hpp in float64 (there is no CPU path); the host builds
the clipped window and, in static mode, the noise spectrum (through `activity_detector` and `Signal.get_spectrum`).  The
bands of a `MultiBandSignal` with one rate and length are streams of one call in adaptive mode and with a given spectrum
(host bands always, resident bands when they are consecutive slices of one buffer); the detector-driven static mode builds
a noise spectrum per band and makes one call per band.  What is kept from the reference is listed in the README ("Kept from
the reference") and in DESIGN section 25.
"""

from warnings import warn

import numpy as np

from .. import backend
from ..classes import Signal
from ..standard.enums import SpectrumMethod, SpectrumScaling, Window
from . import AudioEffect, _result, _samples

__all__ = ["SpectralSubtractor"]


def _closest_power_of_2(number) -> int:
    """The power of two closest to `number` in log2 (the reference's `_get_next_power_2`, mode "closest")."""
    assert number > 0, "Only positive numbers are valid"
    p = np.log2(number)
    p = np.floor(p).astype(int) if p - int(p) < 0.5 else np.ceil(p).astype(int)
    return int(2**p)


class SpectralSubtractor(AudioEffect):
    """Classical spectral subtraction (a denoiser): adaptive, with a noise estimate that follows the quiet frames, or
    static, with one noise spectrum per channel (from `activity_detector` and a Welch estimate, or passed in).  Windows
    are powers of two up to 16384 samples; each channel's peak is kept.  Nothing is printed."""

    def __init__(self, adaptive_mode: bool = True, threshold_rms_dbfs: float = -40, block_length_s: float = 0.1,
                 spectrum_to_subtract=False):
        super().__init__("Spectral Subtraction (Denoiser)")
        self.__set_parameters(adaptive_mode, threshold_rms_dbfs, block_length_s, spectrum_to_subtract)
        self.set_advanced_parameters()

    def __set_parameters(self, adaptive_mode, threshold_rms_dbfs, block_length_s, spectrum_to_subtract):
        if adaptive_mode is not None:
            assert type(adaptive_mode) is bool, "Adaptive mode must be of boolean type"
            self.adaptive_mode = adaptive_mode
        if threshold_rms_dbfs is not None:
            assert type(threshold_rms_dbfs) in (int, float), "Threshold must be of type int or float"
            if threshold_rms_dbfs >= 0:
                warn("Threshold is positive. This might be a wrong input")
            self.threshold_rms_dbfs = threshold_rms_dbfs
        if block_length_s is not None:
            assert type(block_length_s) in (int, float), "Block length should be of type int or float"
            self.block_length_s = block_length_s
        if spectrum_to_subtract is not None:
            if np.any(spectrum_to_subtract):
                assert type(spectrum_to_subtract) is np.ndarray, "Spectrum to subtract must be of type numpy.ndarray"
                spectrum_to_subtract = np.squeeze(spectrum_to_subtract)
                assert spectrum_to_subtract.ndim == 1, "Spectrum to subtract could not be broadcasted to a 1D-Array"
                if self.adaptive_mode:
                    warn("A spectrum to subtract was passed but adaptive mode was selected. This is unsupported. "
                         "Setting adaptive mode to False")
                    self.adaptive_mode = False
            self.spectrum_to_subtract = spectrum_to_subtract

    def set_advanced_parameters(self, overlap_percent: int = 50, window_type: Window = Window.Hann,
                                noise_forgetting_factor: float = 0.9, subtraction_factor: float = 2,
                                subtraction_exponent: float = 2, ad_attack_time_ms: float = 0.5,
                                ad_release_time_ms: float = 30):
        """Window overlap in percent and type, the forgetting factor of the adaptive noise average in ]0, 1], how many
        times the noise is subtracted and at which exponent (2: power, 1: amplitude subtraction), and the activity
        detector's times (static mode)."""
        assert (0 <= overlap_percent) and (100 > overlap_percent), "Overlap should be in [0, 100["
        self.overlap = overlap_percent / 100
        self.window_type = window_type
        assert (0 < noise_forgetting_factor) and (noise_forgetting_factor <= 1), "Noise forgetting factor must be in ]0, 1]"
        self.noise_forgetting_factor = noise_forgetting_factor
        assert subtraction_factor > 0, "The subtraction factor must be positive"
        self.subtraction_factor = subtraction_factor
        assert subtraction_exponent > 0, "Subtraction exponent should be above zero"
        self.subtraction_exponent = subtraction_exponent
        assert ad_attack_time_ms >= 0, "Attack time for activity detector must be 0 or above"
        self.ad_attack_time_ms = ad_attack_time_ms
        assert ad_release_time_ms >= 0, "Release time for activity detector must be 0 or above"
        self.ad_release_time_ms = ad_release_time_ms

    def set_parameters(self, adaptive_mode=None, threshold_rms_dbfs=None, block_length_s=None, spectrum_to_subtract=False):
        """Change parameters; `None` keeps a value (`spectrum_to_subtract` defaults to `False`: no spectrum)."""
        self.__set_parameters(adaptive_mode, threshold_rms_dbfs, block_length_s, spectrum_to_subtract)
        assert self.adaptive_mode is not None, "None is not a valid value"
        assert self.threshold_rms_dbfs is not None, "None is not a valid value"
        assert self.block_length_s is not None, "None is not a valid value"
        assert self.spectrum_to_subtract is not None, "None is not a valid value"

    def _compute_window(self, sampling_rate_hz):
        """Window length (the power of two closest to the block, or 2 (len - 1) of a given spectrum) and the step in
        samples; the clipped window itself is built by backend.fx_specsub."""
        if not np.any(self.spectrum_to_subtract):
            self.window_length = _closest_power_of_2(self.block_length_s * sampling_rate_hz)
        else:
            self.window_length = (len(self.spectrum_to_subtract) - 1) * 2
        self.step_size = int(self.window_length * (1 - self.overlap))

    @property
    def _bands_in_one_call(self):  # the detector's noise spectrum is a per-band table
        return bool(self.adaptive_mode or np.any(self.spectrum_to_subtract))

    def _subtract(self, x, mode, table=None):
        return backend.fx_specsub(x, self.window_type, self.window_length, self.step_size, mode, self.threshold_rms_dbfs,
                                  self.noise_forgetting_factor, self.subtraction_factor, self.subtraction_exponent, table,
                                  env_floor=1e-4 if mode == "adaptive" else None)

    def _process(self, x, fs_hz):
        self._compute_window(fs_hz)
        if self.adaptive_mode:
            return self._subtract(x, "adaptive")
        # (a given spectrum is the squared magnitude: it serves every stream as it is)
        return self._subtract(x, "static", np.abs(self.spectrum_to_subtract) ** (self.subtraction_exponent / 2))

    def _apply_this_effect(self, signal: Signal) -> Signal:
        if self._bands_in_one_call:
            return super()._apply_this_effect(signal)
        from ..standard.activity import activity_detector
        x = _samples(signal)
        self._compute_window(signal.sampling_rate_hz)
        backend._specsub_guard(signal.number_of_channels, len(signal), self.window_length, self.step_size)
        table = np.empty((signal.number_of_channels, self.window_length // 2 + 1))
        for n in range(signal.number_of_channels):
            _, noise = activity_detector(signal, channel=n, threshold_dbfs=self.threshold_rms_dbfs,
                                         attack_time_ms=self.ad_attack_time_ms, release_time_ms=self.ad_release_time_ms)
            noise["noise"].set_spectrum_parameters(method=SpectrumMethod.WelchPeriodogram,
                                                   window_length_samples=self.window_length,
                                                   overlap_percent=self.overlap * 100, window_type=self.window_type,
                                                   scaling=SpectrumScaling.FFTBackward)
            _, noise_psd = noise["noise"].get_spectrum()
            table[n] = np.abs(noise_psd).squeeze() ** (self.subtraction_exponent / 2)  # (the PSD is a squared magnitude)
        return _result(signal, self._subtract(x, "static", table))
