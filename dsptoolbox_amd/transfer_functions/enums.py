from enum import Enum, auto


class TransferFunctionType(Enum):
    """H1 = Gxy/Gxx (noise at the output), H2 = Gyy/Gyx (noise at the input),
    H3 = Gxy/|Gxy| * sqrt(Gyy/Gxx) (noise in both)."""

    H1 = auto()
    H2 = auto()
    H3 = auto()


class SmoothingDomain(Enum):
    """Where complex_smoothing averages (transfer_functions/enums.py:18-42 of the reference, same members, same
    order): RealImaginary on the spectrum itself; PowerPhase / MagnitudePhase on power or magnitude and on the unwrapped
    phase; Power / Magnitude on power or magnitude with the phase kept; EquivalentComplex takes the smoothed power and
    the phase of the RealImaginary result (Hatziantoniou and Mourjopoulos)."""

    RealImaginary = auto()
    PowerPhase = auto()
    MagnitudePhase = auto()
    Power = auto()
    Magnitude = auto()
    EquivalentComplex = auto()
