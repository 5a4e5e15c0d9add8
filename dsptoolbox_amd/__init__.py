"""dsptoolbox_amd -- MI355X-native implementation of dsptoolbox's batched
spectral hot path (Welch/H1-H3, STFT, CSM, spectral deconvolution, FIR filter
banks) behind the reference's Signal / Filter / FilterBank API."""

from . import beamforming, distances, effects, filterbanks, room_acoustics, standard, tools, transfer_functions, transforms
from .classes import Filter, FilterBank, ImpulseResponse, MultiBandSignal, Signal, Spectrum
from .standard.enums import (BiquadEqType, FadeType, FilterBankMode, FilterCoefficientsType, FilterPassType,
                             FrequencySpacing, IirDesignMethod, SpectrumMethod, SpectrumScaling, SpectrumType, Window)
from .standard import (activity_detector, apply_gain, crest_factor, delay, detrend, envelope, fade, fractional_delay, latency,
                       lufs_integrated, merge_filters, normalize, resample, rms)
from .transfer_functions.enums import SmoothingDomain, TransferFunctionType

__version__ = "0.1.0"
__all__ = ["Signal", "ImpulseResponse", "Spectrum", "Filter", "FilterBank", "MultiBandSignal",
           "SpectrumMethod", "SpectrumScaling", "SpectrumType", "FrequencySpacing", "Window", "FilterBankMode",
           "FilterPassType", "FilterCoefficientsType", "IirDesignMethod", "BiquadEqType", "TransferFunctionType", "SmoothingDomain",
           "transfer_functions", "transforms", "room_acoustics", "beamforming", "distances", "filterbanks", "tools", "standard",
           "fractional_delay", "latency", "delay", "effects", "activity_detector", "FadeType", "normalize", "rms", "crest_factor",
           "fade", "apply_gain", "lufs_integrated", "detrend", "envelope", "merge_filters", "resample"]
