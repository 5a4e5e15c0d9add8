"""standard.activity_detector (API mirror of dsptoolbox/standard/other.py:55-179): the power gate on the device."""

from warnings import warn

import numpy as np

from .. import backend
from ..classes import Filter, Signal


def _coefficient(time_ms: float, fs_hz: int):
    with np.errstate(divide="ignore"):
        return 1 - np.exp(np.log(1 - 0.95) / (time_ms / 1e3) / fs_hz)


def activity_detector(signal: Signal, threshold_dbfs: float = -20, channel: int = 0, relative_to_peak: bool = True,
                      pre_filter: Filter | None = None, attack_time_ms: float = 1, release_time_ms: float = 25):
    """Split one channel of `signal` into activity and noise by a power threshold in dBFS (relative to the channel's
    peak, or absolute) on the smoothed squared samples.  `pre_filter` is applied zero-phase before the detection only.
    -> (detected signal, {'noise': Signal, 'signal_indices': bool array, 'noise_indices': its inverse}).

    The smoothing runs on the device (ds_fx_detect); the boolean indexing is the host's.  As in the reference, whose loop
    reads its gain array before writing it, the attack time has no effect and sample 0 is never active."""
    assert isinstance(channel, int), "Channel must be type integer. Function is not implemented for multiple channels."
    assert threshold_dbfs < 0, "Threshold must be below zero"
    assert release_time_ms >= 0, "Release time must be positive"
    assert attack_time_ms >= 0, "Attack time must be positive"
    signal = signal.get_channels(channel)
    if pre_filter is not None:
        assert isinstance(pre_filter, Filter), "pre_filter must be of type Filter"
        detect_in = pre_filter.filter_signal(signal, zero_phase=True)
    else:
        detect_in = signal
    if detect_in.is_complex_signal:
        raise NotImplementedError("activity_detector: complex samples are not run on the device")
    x = detect_in.device_samples if detect_in.on_device else detect_in.time_data
    c_release = _coefficient(release_time_ms, signal.sampling_rate_hz)
    signal_indices = backend.fx_detect(x, threshold_dbfs, c_release, relative_to_peak)[:, 0]
    noise_indices = ~signal_indices

    def part(indices, what, advice):
        out = signal.copy()
        out.clear_time_window()
        if np.any(indices):
            out.time_data = signal.time_data[indices, 0]
        else:
            warn(f"No detected {what}, threshold might be too {advice}. It will be a vector filled with zeroes")
            out.time_data = np.zeros(500)
        return out

    detected = part(signal_indices, "activity", "high")
    noise = part(noise_indices, "noise", "low")
    return detected, dict(noise=noise, signal_indices=signal_indices, noise_indices=noise_indices)
