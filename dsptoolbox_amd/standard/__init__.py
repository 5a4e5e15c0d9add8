from . import enums  # noqa: F401
from .activity import activity_detector  # noqa: F401
from .latency_delay import delay, fractional_delay, latency  # noqa: F401

__all__ = ["latency", "fractional_delay", "delay", "activity_detector"]
