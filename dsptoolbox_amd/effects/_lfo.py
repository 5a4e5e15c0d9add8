"""Low-frequency oscillators and the musical-rhythm helpers of the effects module (API mirror of
dsptoolbox/effects/_effects.py:289-551).  Waveforms are small host tables in numpy: they draw from
numpy's global generator with the reference's arguments, as often and in the same order, so that a
seeded run gives the reference's phases."""

import numpy as np


def get_frequency_from_musical_rhythm(note, bpm):
    """Frequency in Hz of a note value at `bpm` in 4/4: 'quarter', 'half', 'whole', 'eighth', 'sixteenth', '32th',
    'quintuplet'; a '3' in the string makes it a triplet, 'dotted' a dotted value."""
    assert type(note) is str and type(bpm) in (float, int), "Wrong data types for note duration and bpm"
    factor = 0
    for word, value in (("quarter", 1), ("half", 2), ("whole", 4), ("eighth", 1 / 2), ("sixteenth", 1 / 4),
                        ("32th", 1 / 8), ("quintuplet", 1 / 5)):
        if word in note:
            factor = value
    if "3" in note:
        factor *= 2 / 3
    if "dotted" in note:
        factor *= 1.5
    if factor == 0:
        raise ValueError("No valid note description was passed")
    return 60 / bpm / factor


def get_time_period_from_musical_rhythm(note, bpm):
    """Period in seconds of the same note value."""
    return 1 / get_frequency_from_musical_rhythm(note, bpm)


def _phase(random_phase, low=-np.pi, high=np.pi):
    return np.random.uniform(low, high) if random_phase else 0


def _harmonic(freq, fs, length, random_phase, smooth):
    norm_freq = freq / fs
    shift = _phase(random_phase)
    return np.sin(norm_freq * 2 * np.pi * np.arange(length) + shift)


def _square(freq, fs, length, random_phase, smooth):
    shift = _phase(random_phase)
    x = np.sin(freq / fs * 2 * np.pi * np.arange(length) + shift)
    if smooth == 0:
        return np.sign(x)
    smooth *= 0.25 / 10
    return np.arctan(x / smooth)


def _sawtooth(freq, fs, length, random_phase, smooth):
    norm_freq = freq / fs
    if smooth == 0:
        shift = _phase(random_phase, 0, 1)
        x = norm_freq * np.arange(length) + shift
        return (x % 1 - 0.5) * 2
    shift = _phase(random_phase)
    x = np.pi * norm_freq * np.arange(length) + shift
    smooth = max(1, (12 - smooth) ** 1.5)
    waveform = np.arcsin(np.tanh(np.cos(x) * smooth) * np.sin(x))
    waveform /= np.abs(np.max(waveform))
    return waveform


def _triangle(freq, fs, length, random_phase, smooth):
    shift = _phase(random_phase)
    x = np.sin(freq / fs * 2 * np.pi * np.arange(length) + shift)
    if smooth == 0:
        waveform = 2 / np.pi * np.arcsin(x)
    else:
        smooth *= 0.08 / 10
        waveform = 1 - 2 / np.pi * np.arccos((1 - smooth) * x)
    waveform /= np.max(np.abs(waveform))
    return waveform


_OSCILLATORS = {"harmonic": _harmonic, "sawtooth": _sawtooth, "square": _square, "triangle": _triangle}


class LFO:
    """Low-frequency oscillator: `frequency_hz` a number or a (note, bpm) pair, `waveform` one of 'harmonic',
    'sawtooth', 'square', 'triangle', an optional random phase per call and a smoothing amount for the waveforms with
    corners (0: none)."""

    def __init__(self, frequency_hz, waveform: str = "harmonic", random_phase: bool = False, smooth: float = 0):
        self.__set_parameters(frequency_hz, waveform, random_phase, smooth)

    def __set_parameters(self, frequency_hz, waveform, random_phase, smooth):
        if frequency_hz is not None:
            if type(frequency_hz) in (float, int):
                self.frequency_hz = np.abs(frequency_hz)
            elif type(frequency_hz) in (tuple, list):
                assert len(frequency_hz) == 2, "frequency_hz as tuple must have length 2"
                self.frequency_hz = get_frequency_from_musical_rhythm(frequency_hz[0], frequency_hz[1])
            else:
                raise TypeError("frequency_hz does not have a valid type")
        if waveform is not None:
            waveform = waveform.lower()
            if waveform not in _OSCILLATORS:
                raise ValueError("Selected waveform is not valid")
            self.oscillator = _OSCILLATORS[waveform]
        if smooth is not None:
            self.smooth = smooth
        if random_phase is not None:
            self.random_phase = random_phase

    def set_parameters(self, frequency_hz=None, waveform=None, random_phase=None, smooth=None):
        """Change parameters; `None` keeps a value."""
        self.__set_parameters(frequency_hz, waveform, random_phase, smooth)

    def get_waveform(self, sampling_rate_hz: int, length_samples=None):
        """`length_samples` values of the waveform at the sampling rate (None: one period)."""
        if length_samples is None:
            length_samples = int(sampling_rate_hz / self.frequency_hz)
        return self.oscillator(self.frequency_hz, sampling_rate_hz, length_samples, self.random_phase, self.smooth)

    def plot_waveform(self):
        raise NotImplementedError("plots are outside the GPU hot path")
