from . import enums  # noqa: F401
from .latency_delay import fractional_delay  # noqa: F401

__all__ = ["fractional_delay"]
