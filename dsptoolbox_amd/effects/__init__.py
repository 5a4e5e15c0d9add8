"""Audio effects on the device (API mirror of dsptoolbox/effects/effects.py): Compressor, Distortion, Tremolo, Chorus
and DigitalDelay here and SpectralSubtractor in the submodule `effects.spectral`, with the reference's constructors,
setters, assertions and defaults.

Every sample is computed by the HIP kernels of csrc/kernels_fx.hpp (the subtractor's: csrc/kernels_specsub.hpp) in float64
(there is no CPU path); the host builds only what the reference builds as small tables: LFO waveforms, the chorus index
table, the tremolo modulator and the follower coefficients.  `apply()` takes a `Signal` or a `MultiBandSignal`.  A
device-resident signal is read where it lies and its result stays resident.  The bands of a `MultiBandSignal` with one rate
and length go through the kernels as bands x channels streams of one call where the effect has no per-band table
(Compressor, Distortion, DigitalDelay; host bands always, resident bands when they are consecutive slices of one buffer, as
a filter bank leaves them); Tremolo and Chorus build their tables band by band, as the reference's loop draws their
phases, and make one call per band.

What the reference does and a reader might not expect is kept: the compressor ignores `mix_percent`
and `post_gain_db` and applies `pre_gain_db` twice; distortion components are peak-restored one by one, so mix weights
only switch a component off at 0; an ndarray modulator never passes the type checks.

The names this module exports are pinned by the effects suite; `SpectralSubtractor` is reached as
`dsp.effects.spectral.SpectralSubtractor` (the submodule is imported with the package).
"""

from enum import Enum, auto
from warnings import warn

import numpy as np

from .. import backend
from .._lib import DevicePlanar
from ..classes import MultiBandSignal, Signal
from ._lfo import LFO, get_frequency_from_musical_rhythm, get_time_period_from_musical_rhythm

__all__ = ["AudioEffect", "Compressor", "Distortion", "DistortionType", "Tremolo", "Chorus", "DigitalDelay", "LFO",
           "get_frequency_from_musical_rhythm", "get_time_period_from_musical_rhythm"]


class DistortionType(Enum):
    Arctan = auto()
    HardClip = auto()
    SoftClip = auto()
    NoDistortion = auto()


def _samples(signal: Signal):
    if signal.is_complex_signal:
        raise NotImplementedError("effects: complex samples are not run on the device (the recursions are real)")
    return signal.device_samples if signal.on_device else signal.time_data


def _result(signal: Signal, y) -> Signal:
    return signal._device_result(y) if isinstance(y, DevicePlanar) else signal.copy_with_new_time_data(y)


def _consecutive(planars):
    """The bands' planars as one DevicePlanar of bands x channels rows, when they are consecutive slices of one buffer
    with one pitch (a filter bank's output); None otherwise."""
    first = planars[0]
    step = 4 * first.n_ch * first.ld
    for b, p in enumerate(planars):
        if p.owner is not first.owner or p.ld != first.ld or p.offset_bytes != first.offset_bytes + b * step:
            return None
    return DevicePlanar(first.owner, first.n_ch * len(planars), first.n_samples, first.ld, first.offset_bytes)


class AudioEffect:
    """Base class: `apply()` dispatches a Signal or the bands of a MultiBandSignal to `_process()`."""

    _bands_in_one_call = False  # the effect has no per-band table: bands x channels are streams of one call

    def __init__(self, description: str | None = None):
        self.description = description

    def apply(self, signal):
        if isinstance(signal, Signal):
            return self._apply_this_effect(signal)
        if type(signal) is MultiBandSignal:
            return MultiBandSignal(self._apply_bands(signal), signal.same_sampling_rate, dict(signal.info))
        raise TypeError("Audio effect can only be applied to Signal or MultiBandSignal")

    def _apply_bands(self, mbs) -> list:
        bands = list(mbs.bands)
        if not (self._bands_in_one_call and mbs.same_sampling_rate and len(bands) > 1):
            return [self.apply(b) for b in bands]
        n_ch = mbs.number_of_channels
        if mbs.on_device:
            x = _consecutive([b.device_samples for b in bands])
            if x is None:
                return [self.apply(b) for b in bands]
            y = self._process(x, mbs.sampling_rate_hz)
            return [b._device_result(DevicePlanar(y.owner, n_ch, y.n_samples, y.ld, 4 * i * n_ch * y.ld))
                    for i, b in enumerate(bands)]
        y = self._process(np.concatenate([_samples(b) for b in bands], axis=1), mbs.sampling_rate_hz)
        return [b.copy_with_new_time_data(y[:, i * n_ch:(i + 1) * n_ch]) for i, b in enumerate(bands)]

    def _apply_this_effect(self, signal: Signal) -> Signal:
        return _result(signal, self._process(_samples(signal), signal.sampling_rate_hz))

    def _process(self, x, fs_hz: int):
        """x (samples, streams) float64 or a DevicePlanar -> the processed samples, in kind."""
        return x


class Compressor(AudioEffect):
    """Dynamic range compressor (a multi-band one on a MultiBandSignal): threshold in dBFS, attack and release in ms,
    ratio >= 1, the threshold relative to each channel's peak or absolute."""

    _bands_in_one_call = True

    def __init__(self, threshold_dbfs: float = -10, attack_time_ms: float = 0.5, release_time_ms: float = 20,
                 ratio: float = 3, relative_to_peak_level: bool = True):
        super().__init__("Compressor")
        self.__set_parameters(threshold_dbfs, attack_time_ms, release_time_ms, ratio, relative_to_peak_level)
        self.set_advanced_parameters()

    def __set_parameters(self, threshold_dbfs, attack_time_ms, release_time_ms, ratio, relative_to_peak_level):
        if threshold_dbfs is not None:
            if threshold_dbfs > 0:
                warn("Threshold is above 0 dBFS, this might lead to unexpected results")
            self.threshold_dbfs = threshold_dbfs
        if attack_time_ms is not None:
            assert attack_time_ms >= 0, "Attack time has to be 0 or above"
            self.attack_time_ms = attack_time_ms
        if release_time_ms is not None:
            assert release_time_ms >= 0, "Release time has to be 0 or above"
            self.release_time_ms = release_time_ms
        if ratio is not None:
            assert ratio >= 1, "Compression ratio must be above 1"
            self.ratio = ratio
        if relative_to_peak_level is not None:
            self.relative_to_peak_level = relative_to_peak_level

    def set_parameters(self, threshold_dbfs=None, attack_time_ms=None, release_time_ms=None, ratio=None,
                       relative_to_peak_level=None):
        """Change parameters; `None` keeps a value."""
        self.__set_parameters(threshold_dbfs, attack_time_ms, release_time_ms, ratio, relative_to_peak_level)

    def set_advanced_parameters(self, knee_factor_db: float = 0, pre_gain_db: float = 0, post_gain_db: float = 0,
                                mix_percent: float = 100, automatic_make_up_gain: bool = True,
                                downward_compression: bool = True):
        """Knee width in dB, gains, make-up gain (the RMS of the input is restored) and the direction.  As in the
        reference, `mix_percent` and `post_gain_db` are stored and have no effect, and `pre_gain_db` is applied before
        and once more after the compression."""
        assert knee_factor_db >= 0, "Knee factor must be 0 or above"
        self.knee_factor_db = knee_factor_db
        assert mix_percent > 0 and mix_percent <= 100, "Mix percent must be in ]0, 100]"
        self.mix = mix_percent / 100
        self.pre_gain_db = pre_gain_db
        self.post_gain_db = post_gain_db
        self.automatic_make_up_gain = automatic_make_up_gain
        self.downward_compression = downward_compression

    def show_compression(self):
        raise NotImplementedError("plots are outside the GPU hot path")

    def _process(self, x, fs_hz):
        gain = 1.0 if self.pre_gain_db is None else 10 ** (self.pre_gain_db / 20)
        return backend.fx_compress(x, self.threshold_dbfs, self.ratio, self.knee_factor_db,
                                   int(self.attack_time_ms * 1e-3 * fs_hz), int(self.release_time_ms * 1e-3 * fs_hz),
                                   pre_gain=gain, final_gain=gain, downward=self.downward_compression,
                                   relative=self.relative_to_peak_level, make_up=self.automatic_make_up_gain)


class Distortion(AudioEffect):
    """Non-linear distortion: one curve mixed with the clean signal, or a list of curves.  Each channel's peak is kept."""

    _bands_in_one_call = True

    def __init__(self, distortion_level: float = 20, post_gain_db: float = 0,
                 type_of_distortion: DistortionType = DistortionType.Arctan):
        super().__init__("Distortion")
        self.set_advanced_parameters(type_of_distortion=type_of_distortion, distortion_levels_db=distortion_level,
                                     post_gain_db=post_gain_db)

    def set_advanced_parameters(self, type_of_distortion=DistortionType.Arctan, distortion_levels_db=20, mix_percent=100,
                                offset_db=-np.inf, post_gain_db: float = 0):
        """Curves (one DistortionType or a list), their levels in dB, mix weights in percent (summing to 100) and
        offsets in dB (-inf: none).  A single curve gets the clean signal beside it with the rest of the weight."""
        mix_percent = np.atleast_1d(mix_percent)
        assert np.all(mix_percent <= 100), "No value of mix_percent can be greater than 100"
        if type(type_of_distortion) is not list:
            type_of_distortion = [type_of_distortion]
        kinds = []
        for dist in type_of_distortion:
            if not isinstance(dist, DistortionType):
                raise ValueError("The type of distortion is not implemented.")
            kinds.append(backend.FX_CURVES[dist.name])
        self.mix = mix_percent / 100
        self.distortion_levels = np.atleast_1d(distortion_levels_db)
        self.offset_db = np.atleast_1d(offset_db)
        if len(kinds) == 1:
            kinds.append(backend.FX_CURVES["NoDistortion"])
            self.mix = np.append(self.mix, 1 - self.mix[0])
            self.distortion_levels = np.append(self.distortion_levels, 0)
            self.offset_db = np.append(self.offset_db, -np.inf)
        n = len(kinds)
        assert n == len(self.mix), "Length of mix_percent does not match distortions"
        assert np.isclose(np.sum(self.mix), 1), "mix_percent does not sum up to 100"
        assert n == len(self.distortion_levels), "Length of distortion_levels does not match distortions"
        assert n == len(self.offset_db), "Length of offset_db does not match distortions"
        self.__kinds = kinds
        self.post_gain_db = post_gain_db

    def _process(self, x, fs_hz):
        levels = [10 ** (v / 20) for v in self.distortion_levels]
        offsets = [10 ** (v / 20) for v in self.offset_db]
        gain = 1.0 if self.post_gain_db is None else 10 ** (self.post_gain_db / 20)
        return backend.fx_distort(x, self.__kinds, levels, offsets, list(self.mix), gain)


class Tremolo(AudioEffect):
    """Amplitude modulation by an LFO: every channel times |waveform depth + 1|."""

    def __init__(self, depth: float = 0.5, modulator=None):
        super().__init__("Modulation effect: Tremolo")
        if modulator is None:
            modulator = LFO(1, "harmonic")
        self.__set_parameters(depth, modulator)

    def __set_parameters(self, depth, modulator):
        if modulator is not None:
            # (the reference compares the type with a numpy type alias, which no object has: only an LFO passes)
            assert type(modulator) is LFO, "Unsupported modulator type. Use LFO or numpy.ndarray"
            self.modulator = modulator
        if depth is not None:
            assert depth > 0 and depth <= 1, "Depth must be in ]0, 1]"
            self.depth = depth

    def set_parameters(self, depth=None, modulator=None):
        """Change parameters; `None` keeps a value."""
        self.__set_parameters(depth, modulator)

    def _process(self, x, fs_hz):
        n = backend._samples_shape(backend._fx_samples(x))[0]
        return backend.fx_tremolo(x, np.abs(self.modulator.get_waveform(fs_hz, n) * self.depth + 1))


class Chorus(AudioEffect):
    """Chorus / flanger: voices whose delay (base delay plus depth times an LFO, in ms) varies over time are added to
    the signal; the number of voices is the longest of the parameters.  Peaks and duration are kept."""

    def __init__(self, depths_ms=5, base_delays_ms=15, modulators=None, mix_percent: float = 100):
        super().__init__("Modulation effect: Chorus/Flanger")
        if modulators is None:
            modulators = LFO(2, "harmonic", random_phase=True)
        self.__set_parameters(depths_ms, base_delays_ms, modulators, mix_percent)

    def __set_parameters(self, depths_ms, base_delays_ms, modulators, mix_percent):
        if base_delays_ms is not None:
            base_delays_ms = np.atleast_1d(base_delays_ms)
            nv_base = len(base_delays_ms)
        else:
            nv_base = len(self.base_delays_ms)
        if depths_ms is not None:
            depths_ms = np.atleast_1d(depths_ms)
            nv_depths = len(depths_ms)
        else:
            nv_depths = len(self.depths_ms)
        if modulators is not None:
            nv_mod = len(modulators) if type(modulators) in (list, tuple) else 1
        else:
            nv_mod = len(self.modulators)
        self.number_of_voices = max(nv_base, nv_depths, nv_mod)

        if base_delays_ms is not None:
            assert np.all(base_delays_ms > 0), "Base delays must be above 0"
            assert len(base_delays_ms) in (1, self.number_of_voices), "Base delays can only be length 1 or number of voices"
            self.base_delays_ms = base_delays_ms
            if len(self.base_delays_ms) == 1:
                self.base_delays_ms = np.repeat(self.base_delays_ms, self.number_of_voices)
        if modulators is not None:
            # (an ndarray fails here as in the reference, whose comparison with a numpy type alias is never true)
            assert type(modulators) in (LFO, list, tuple), "Unsupported modulators type. Use LFO or numpy.ndarray"
            if type(modulators) is LFO:
                self.modulators = [modulators] * self.number_of_voices
            else:
                assert len(modulators) in (1, self.number_of_voices), \
                    f"The number of modulators signals does not match the number of voices {self.number_of_voices}"
                assert all(type(i) is LFO for i in modulators), "All modulators signals have to be of type LFO"
                self.modulators = modulators
                if len(self.modulators) == 1:
                    self.modulators = [self.modulators[0]] * self.number_of_voices
        if depths_ms is not None:
            self.depths_ms = np.atleast_1d(depths_ms)
            assert len(self.depths_ms) in (1, self.number_of_voices), \
                f"Depth must be of length 1 or number of voices {self.number_of_voices}"
            if len(self.depths_ms) == 1:
                self.depths_ms = np.repeat(self.depths_ms, self.number_of_voices)
        if mix_percent is not None:
            mix_percent /= 100
            assert mix_percent <= 1 and mix_percent > 0, "Mix percent must be below 100 and above 0"
            self.mix = mix_percent

    def set_parameters(self, depths_ms=None, base_delays_ms=None, modulators=None, mix_percent=None):
        """Change parameters; `None` keeps a value."""
        self.__set_parameters(depths_ms, base_delays_ms, modulators, mix_percent)

    def _delay_table(self, fs_hz, n: int) -> np.ndarray:
        """(n, voices) delays in samples: the reference's rounding, on the host."""
        modulation = np.zeros((n, self.number_of_voices))
        for ind, m in enumerate(self.modulators):
            modulation[:, ind] = m.get_waveform(fs_hz, n) * self.depths_ms[ind] + self.base_delays_ms[ind]
        return np.round(modulation * 1e-3 * fs_hz).astype(int)

    def _process(self, x, fs_hz):
        n = backend._samples_shape(backend._fx_samples(x))[0]
        return backend.fx_chorus(x, self._delay_table(fs_hz, n), self.mix)


class DigitalDelay(AudioEffect):
    """Feedback delay: repetitions `delay_time_ms` apart, each `feedback` times the one before, optionally through an
    arctan saturation.  The result is longer than the input by int(delay (1 + 15 feedback)) samples; peaks are kept."""

    _bands_in_one_call = True

    def __init__(self, delay_time_ms: float = 300, feedback: float = 0.1):
        super().__init__("Digital Delay")
        self.__set_parameters(delay_time_ms, feedback)
        self.set_advanced_parameters()

    def __set_parameters(self, delay_time_ms, feedback):
        assert delay_time_ms > 0, "Delay time must be larger than 0"
        self.delay_ms = delay_time_ms
        assert feedback > 0, "Feedback must be larger than one"
        self.feedback = feedback

    def set_parameters(self, delay_time_ms=None, feedback=None):
        """Change both parameters (as in the reference, `None` fails the comparison)."""
        self.__set_parameters(delay_time_ms, feedback)

    def set_advanced_parameters(self, saturation: str | None = None):
        """`None` or 'digital': a linear delay line; 'arctan': 0.5 atan(2 v) in the feedback path.  A callable ends at
        `.lower()` with AttributeError, as in the reference."""
        if saturation is None:
            saturation = "digital"
        saturation = saturation.lower()
        if saturation not in backend.FX_SATURATIONS:
            raise TypeError("'str' object is not callable")  # (what the reference ends with for an unknown name)
        self.saturation = saturation

    def plot_delay(self):
        raise NotImplementedError("plots are outside the GPU hot path")

    def _process(self, x, fs_hz):
        delay_samples = int(np.round(self.delay_ms * 1e-3 * fs_hz).astype(int))
        padding = int(delay_samples * (1 + self.feedback * 15))
        return backend.fx_delay(x, delay_samples, padding, self.feedback, self.saturation)


from . import spectral  # noqa: E402,F401  (effects.spectral.SpectralSubtractor; after the base class it builds on)
