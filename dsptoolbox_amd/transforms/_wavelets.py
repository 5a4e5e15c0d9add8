"""Wavelets and the continuous wavelet transform (transforms/transforms.py:687-760 and transforms/_transforms.py:29-301
of the reference).  The wavelets are built on the host in float64 exactly as the reference builds them (the linear
interpolation vectorised: the same operations per element); the convolutions and the synchrosqueezing run in the HIP
library (ds_cwt, ds_cwt_dev, ds_cwt_squeeze_dev)."""

from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from .. import backend
from ..classes.signal import Signal


class Wavelet:
    """Base class for a wavelet function."""

    def __init__(self):
        """Constructor for the base wavelet class. It's not supposed to be used directly."""
        pass

    def get_base_wavelet(self):
        """Abstract method to get the mother wavelet. It must be implemented in each Wavelet class."""
        raise NotImplementedError("Wavelet function has not been implemented")

    def get_wavelet(self, f, fs):
        """Abstract method to get the sampled wavelet. It must be implemented in each Wavelet class."""
        raise NotImplementedError("Wavelet function has not been implemented")

    def get_center_frequency(self):
        """Returns the center frequency of the wavelet (normalized, i.e., with fs=1)."""
        x, func = self.get_base_wavelet()
        ind = np.argmax(np.abs(np.fft.fft(func)))
        domain = x[-1] - x[0]
        return ind / domain

    def get_scale_lengths(self, frequencies: NDArray[np.float64], fs: int):
        """Returns the lengths in samples of the wavelets of the queried frequencies."""
        scales = np.atleast_1d(self.get_center_frequency() / frequencies * fs)
        x, _ = self.get_base_wavelet()
        return (scales * (x[-1] - x[0]) + 1).astype(int)


class MorletWavelet(Wavelet):
    """Complex morlet wavelet."""

    def __init__(self, b: float | None = None, h: float | None = None, scale: float = 1.0,
                 precision_bounds: float = 1e-5, step: float = 5e-3, interpolation: bool = True):
        """Complex morlet wavelet with bandwidth `b` or full width at half maximum `h` (b = h**2 / (4 ln 2), `h`
        overrides `b`), base wavelet `scale`, bounds where the gaussian falls to `precision_bounds`, base sampling
        `step` and linear interpolation (`interpolation`) when it is resampled for a frequency."""
        assert b is not None or h is not None, "Either b or h must be passed"
        if h is not None:
            self.b = h**2 / np.log(2) / 4
        else:
            self.b = b
        self.scale = scale

        t = np.sqrt(self.b * np.log(1 / precision_bounds))
        self.bounds = [-t, t]

        self.step = step
        self.interpolation = interpolation

    def _get_x(self) -> NDArray[np.float64]:
        """Returns x vector for the mother wavelet."""
        return np.arange(self.bounds[0], self.bounds[1] + self.step, self.step)

    def get_base_wavelet(self) -> tuple[NDArray[np.float64], NDArray[np.float64]]:
        """Return complex morlet wavelet."""
        x = self._get_x()
        return x, 1 / np.sqrt(np.pi * self.b) * np.exp(2j * np.pi / self.scale * x) * np.exp(-(x**2) / self.b)

    def get_center_frequency(self) -> float:
        """Return center frequency for the complex morlet wavelet."""
        return 1 / self.scale

    def get_wavelet(self, f: float | NDArray[np.float64], fs: int):
        """The wavelet scaled for frequency `f` at sampling rate `fs` (a list of them for several frequencies),
        linearly interpolated from the base wavelet when `interpolation` is set."""
        scales = np.atleast_1d(self.get_center_frequency() / f * fs)
        x, base = self.get_base_wavelet()
        wave = []

        for scale in scales:
            inds = np.arange(scale * (x[-1] - x[0]) + 1) / (scale * self.step)
            if self.interpolation:
                wavef = self._get_interpolated_wave(base, inds)
            else:
                inds = inds.astype(int)
                inds = inds[inds < len(base)]
                wavef = base[inds]
            if len(scales) == 1:
                return wavef
            wave.append(wavef)
        return wave

    def _get_interpolated_wave(self, base: NDArray[np.float64], inds: NDArray[np.float64]):
        """Linear interpolation of the base wavelet at `inds` (the reference's per-sample loop, vectorised); the
        last sample is base[trunc[-1]]."""
        trunc = inds.astype(int)
        trunc = trunc[trunc < len(base)]
        accumulator = np.zeros(len(trunc), dtype=np.complex128)
        i = trunc[:-1]
        accumulator[:-1] = base[i] + (base[i + 1] - base[i]) * (inds[: len(i)] - i)
        accumulator[-1] = base[trunc[-1]]
        return accumulator


def _normalised_wavelets(wavelet, frequencies, fs):
    waves = []
    for f in frequencies:
        wv = np.array(wavelet.get_wavelet(f, fs))
        wv /= np.abs(wv).sum()
        waves.append(wv)
    return waves


def cwt(signal: Signal, frequencies: NDArray[np.float64], wavelet: Wavelet | MorletWavelet,
        channel: NDArray[np.float64] | None = None, synchrosqueezed: bool = False,
        apply_synchrosqueezed_normalization: bool = False, *, on_device: bool = False):
    """Scalogram (frequency, time sample, channel) of `signal` by the continuous wavelet transform: row f is the
    "same"-mode convolution of the channels `channel` (None: all) with wavelet.get_wavelet(f, fs) normalised to a
    unit sum of magnitudes.  `synchrosqueezed` reassigns it by the phase transform (delta_w = 0.05), each row scaled
    by (f / fs)**1.5 when `apply_synchrosqueezed_normalization`.

    Computed on the device in fp32 / complex64 (the squeeze in float64).  Returns the reference's complex128 array,
    or with `on_device=True` a `backend.DeviceScalogram` left in HBM (complex64, complex128 when squeezed).  A
    device-resident signal is read in place; a host signal is uploaded into a temporary buffer."""
    if channel is None:
        channel = np.arange(signal.number_of_channels)
    channel = np.atleast_1d(channel)
    fs = signal.sampling_rate_hz
    waves = _normalised_wavelets(wavelet, frequencies, fs)
    lens, _ = backend._cwt_taps(waves)  # (the tap-length limit before anything touches the device)
    n = len(signal)
    if synchrosqueezed and n < 2:
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")
    if len(waves) == 0:
        empty = np.zeros((0, n, len(channel)), dtype=np.complex128)
        return empty if not on_device else backend.DeviceScalogram(
            backend.DeviceBuffer(backend.get_context(), 16), empty.shape, np.complex128)

    if signal.on_device:
        x_dev, chans = signal.device_samples, channel
    elif on_device or synchrosqueezed:
        from .._lib import DevicePlanar
        td = signal.time_data[:, channel]
        x_dev = DevicePlanar.from_planar(backend.get_context(), backend._planar_f32(td))  # (not kept by the signal)
        chans = np.arange(td.shape[1])
    else:
        return backend.cwt_host(signal.time_data[:, channel], waves)

    scal = backend.cwt_device(x_dev, chans, waves)
    if synchrosqueezed:
        scal = backend.cwt_squeeze_device(scal, np.asarray(frequencies), fs,
                                          apply_frequency_normalization=apply_synchrosqueezed_normalization)
    return scal if on_device else scal.to_host()
