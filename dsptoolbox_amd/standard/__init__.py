from . import enums  # noqa: F401
from .activity import activity_detector  # noqa: F401
from .gain_and_level import apply_gain, crest_factor, fade, lufs_integrated, normalize, rms  # noqa: F401
from .latency_delay import delay, fractional_delay, latency  # noqa: F401
from .other import detrend, envelope, merge_filters  # noqa: F401
from .resampling import resample, resample_filter  # noqa: F401

__all__ = ["latency", "fractional_delay", "delay", "activity_detector", "normalize", "rms", "crest_factor", "fade",
           "apply_gain", "lufs_integrated", "detrend", "envelope", "merge_filters", "resample", "resample_filter"]
