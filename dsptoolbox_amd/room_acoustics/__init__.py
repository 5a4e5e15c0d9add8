"""room_acoustics: applying a room impulse response to a signal
(dsptoolbox/room_acoustics/room_acoustics.py:216-266) -- the full
linear convolution runs on the device through the FIR block-convolution path (ds_fir_ola; impulse
responses longer than 8193 taps take its four-step-FFT overlap-save branch) -- and making one:
Room, ShoeboxRoom (_rooms.py) and generate_synthetic_rir (room_acoustics.py:300-451), whose image-source sum
runs on the device (backend.image_source_rir)."""

from __future__ import annotations

import numpy as np

from .. import backend
from ..classes.filter import Filter
from ..classes.impulse_response import ImpulseResponse
from ..classes.signal import Signal
from ..standard.enums import FilterPassType, IirDesignMethod
from ._rooms import Room, ShoeboxRoom

__all__ = ["convolve_rir_on_signal", "generate_synthetic_rir", "Room", "ShoeboxRoom"]


def convolve_rir_on_signal(signal: Signal, rir: Signal, keep_peak_level: bool = True,
                           keep_length: bool = True) -> Signal:
    """Convolve every channel of `signal` with the single-channel `rir`."""
    assert rir.number_of_channels == 1, "RIR should not contain more than one channel."
    assert rir.sampling_rate_hz == signal.sampling_rate_hz, "The sampling rates do not match"
    x = signal.time_data
    h = rir.time_data[:, 0]
    # mode="full": the causal convolution of the signal followed by len(h) - 1 zeros
    xfull = np.concatenate([x, np.zeros((len(h) - 1, x.shape[1]))], axis=0)
    new_time_data = backend.fir_filter_bank(xfull, [h], backend.DS_FB_PARALLEL)[0]
    if keep_length:
        new_time_data = new_time_data[: len(signal), ...]
    if keep_peak_level:
        old_peak_levels = np.max(np.abs(signal.time_data), axis=0)
        new_peak_levels = np.max(np.abs(new_time_data), axis=0)
        new_time_data *= (old_peak_levels / new_peak_levels)[None, ...]
    return signal.copy_with_new_time_data(new_time_data)


def _add_reverberant_tail_noise(rir: np.ndarray, mixing_time_s: float, t60: float, sr: int) -> np.ndarray:
    """Decaying noise in the empty samples of the late part (room_acoustics/_room_acoustics.py:840-886), host
    arithmetic.  The noise is np.random.normal from numpy's global state, drawn once with the reference's arguments,
    so a seeded state gives the reference's samples."""
    ind_direct = np.squeeze(np.where(rir != 0))[0]
    noise_length = len(rir) - ind_direct - int(mixing_time_s * sr)
    noise = np.abs(np.random.normal(0, 1, noise_length))
    noise *= np.exp(-(0.02 * 343 / t60) * np.arange(noise_length) / sr)
    noise /= np.max(noise)
    # half the median of what the image sources left in 100 samples around the start of the noise
    window = rir[-noise_length - 50: -noise_length + 50]
    noise *= np.median(window[window != 0]) * 0.5
    empty = rir[-noise_length:] == 0
    rir[-noise_length:][empty] += noise[empty]
    return rir


def generate_synthetic_rir(room: ShoeboxRoom, source_position, receiver_position, sampling_rate_hz: int,
                           total_length_seconds: float = 0.5, add_noise_reverberant_tail: bool = False,
                           apply_bandpass: bool = False, use_detailed_absorption: bool = False,
                           max_order: int | None = None) -> ImpulseResponse:
    """A room impulse response of a shoebox room by the image-source model (Brinkmann, Erbes, Weinzierl 2018:
    "Extending the closed form image source model for source directivity"), summed on the device.

    use_detailed_absorption: one device call sums every octave band of room.detailed_absorption; band `ind` of the
    zero-phase order-12 Linkwitz-Riley split of band ind's response is kept and the bands are added.
    add_noise_reverberant_tail: decaying noise after the mixing time (room.mixing_time_s, or the physical one for 1000
    reflections).  apply_bandpass: an order-12 Butterworth band pass from 20 Hz to 0.9 (sr // 2).  max_order caps the
    lattice.  IndexError where the reference raises it (a source beyond its buffer, in elongated rooms); ValueError
    when source and receiver coincide."""
    assert sampling_rate_hz is not None, "Sampling rate can not be None"
    assert type(room) is ShoeboxRoom, "Room must be of type ShoeboxRoom"
    source_position = np.asarray(source_position)
    receiver_position = np.asarray(receiver_position)
    assert room.check_if_in_room(source_position), "Source is not located inside the room"
    assert room.check_if_in_room(receiver_position), "Receiver is not located inside the room"
    total_length_samples = int(total_length_seconds * sampling_rate_hz)

    def bands_rir(alphas):
        out = backend.image_source_rir(room.dimensions_m, alphas, source_position, receiver_position, room.t60_s,
                                       max_order, sampling_rate_hz, total_length_samples)
        return np.nan_to_num(out, copy=False, nan=0)

    if not use_detailed_absorption:
        rir = bands_rir(np.atleast_1d(room.absorption_coefficient)[None, :])[0]
    else:
        assert hasattr(room, "detailed_absorption"), "Given room has no detailed absorption dictionary"
        from ..filterbanks import linkwitz_riley_crossovers
        freqs = room.detailed_absorption["center_frequencies"][:-1] * np.sqrt(2)
        fb = linkwitz_riley_crossovers(crossover_frequencies_hz=freqs, order=12, sampling_rate_hz=sampling_rate_hz)
        per_band = bands_rir(room.detailed_absorption["absorption_matrix"].T)
        rir = np.zeros(total_length_samples)
        for ind in range(fb.number_of_bands):
            split = fb.filter_signal(ImpulseResponse(None, per_band[ind], sampling_rate_hz), zero_phase=True)
            rir += split.bands[ind].time_data[:, 0]
    if add_noise_reverberant_tail:
        if getattr(room, "mixing_time_s", None) is None:
            room.get_mixing_time("physical", n_reflections=1000)
        rir = _add_reverberant_tail_noise(rir, room.mixing_time_s, room.t60_s, sr=sampling_rate_hz)
    rir_output = ImpulseResponse(None, rir, sampling_rate_hz)
    if apply_bandpass:
        f = Filter.iir_filter(order=12, frequency_hz=[20.0, (sampling_rate_hz // 2) * 0.9],
                              filter_design_method=IirDesignMethod.Butterworth, type_of_pass=FilterPassType.Bandpass,
                              sampling_rate_hz=sampling_rate_hz)
        rir_output = f.filter_signal(rir_output)
    return rir_output
