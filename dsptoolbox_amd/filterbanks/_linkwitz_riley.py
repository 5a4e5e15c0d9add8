"""The Linkwitz-Riley crossover bank of the reference (filterbanks/_filterbank.py:45-405, 652-661, 1307-1345): a tree of
two-way splits, band k being the low side of crossover k after the all-passes (low + high) of every later crossover.
The coefficients are designed on the host with scipy; every recursion runs on the device through backend._sosfilt and
backend._sosfiltfilt."""

from copy import deepcopy
from warnings import warn

import numpy as np
from scipy.signal import bilinear, butter, sosfilt_zi, tf2sos

from .. import backend
from ..classes.impulse_response import ImpulseResponse
from ..classes.multibandsignal import MultiBandSignal
from ..classes.signal import Signal
from ..standard.enums import FilterBankMode


def _second_order_pair(f0: float, sampling_rate_hz: int):
    """The order-2 crossover: Sallen-Key sections with Q = 0.5, omega0^2 / (s + omega0)^2 and -s^2 / (s + omega0)^2 (the
    high band is phase-inverted so that the bands sum to an all-pass), through the bilinear transform pre-warped at
    f0."""
    omega_0 = 2 * np.pi * f0
    a_s = [1, 2 * omega_0, omega_0 ** 2]
    warped = np.pi * f0 / np.tan(np.pi * f0 / sampling_rate_hz)
    low = tf2sos(*bilinear([omega_0 ** 2], a_s, warped))
    high = tf2sos(*bilinear([-1, 0, 0], a_s, warped))
    return low, high


class LRFilterBank:
    """Crossovers at `freqs` of the given order(s): 2 (the pair above), odd (one Butterworth filter per side, bands
    crossing at -3 dB) or a multiple of 4 (two Butterworth filters of half the order in cascade)."""

    def __init__(self, freqs, order=4, sampling_rate_hz: int = 48000, info: dict | None = None):
        freqs = np.atleast_1d(np.asarray(freqs).squeeze())
        order = np.atleast_1d(np.asarray(order).squeeze())
        if len(order) == 1:
            order = np.ones(len(freqs)) * order
        assert np.max(freqs) <= sampling_rate_hz // 2, \
            "Highest frequency is above nyquist frequency for the given sampling rate"
        assert len(freqs) == len(order), "Number of frequencies and number of order of the crossovers do not match"
        for o in order:
            if o % 2 != 0 and o != 1:
                warn("Order of the crossovers is recommended to be even. Odd orders have band crossing at -3 dB and are "
                     "not really Linkwitz-Riley crossovers, although they have perfect magnitude reconstruction.")
        by_frequency = freqs.argsort()
        self.freqs = freqs[by_frequency]
        self.order = order[by_frequency]
        self.number_of_cross = len(freqs)
        self.number_of_bands = self.number_of_cross + 1
        self.sampling_rate_hz = sampling_rate_hz
        edges = np.concatenate([[0], self.freqs, [sampling_rate_hz // 2]])
        self.center_frequencies = (edges[:-1] + edges[1:]) / 2
        self._create_filters_sos()
        self.info = dict(crossover_frequencies=self.freqs, crossover_orders=self.order,
                         number_of_crossovers=self.number_of_cross, number_of_bands=self.number_of_bands,
                         sampling_rate_hz=self.sampling_rate_hz) | (info or {})

    def _create_filters_sos(self):
        """self.sos[i] = [low sos, high sos] of crossover i, ascending in frequency."""
        self.sos = []
        for f0, o in zip(self.freqs, self.order):
            if o == 2:
                self.sos.append(list(_second_order_pair(f0, self.sampling_rate_hz)))
                continue
            if o % 2 == 0:
                assert o % 4 == 0, f"{o} order is not supported for crossover"
            half = o // 2 if o % 2 == 0 else o
            pair = [butter(half, f0, btype=kind, fs=self.sampling_rate_hz, output="sos") for kind in ("lowpass", "highpass")]
            if o % 2 == 0:
                pair = [np.vstack([p, p]) for p in pair]
            self.sos.append(pair)

    def initialize_zi(self, number_of_channels: int = 1):
        """Steady-state filter states per channel: channels_zi[ch] = [splits, all-passes], splits[i] = [low, high] of
        crossover i.  The all-pass list has the reference's layout: while crossover 0's row [[low, high] per
        crossover] is being filled it is appended once per entry, so all-passes[cn] for every cn < number_of_cross is
        that one row and bands share the state of the all-pass at a given crossover."""
        def states(i):
            return [sosfilt_zi(self.sos[i][0]), sosfilt_zi(self.sos[i][1])]

        self.channels_zi = []
        for _ in range(number_of_channels):
            splits, allpasses = [], []
            for i in range(self.number_of_cross):
                splits.append(states(i))
                row = []
                for i2 in range(self.number_of_cross):
                    row.append(states(i2))
                    allpasses.append(row)
            self.channels_zi.append([splits, allpasses])

    def filter_signal(self, s: Signal, mode: FilterBankMode = FilterBankMode.Parallel, activate_zi: bool = False,
                      zero_phase: bool = False):
        """Parallel: a MultiBandSignal of the bands; Summed: their sum (Sequential warns and becomes Summed).
        zero_phase filters every side forward and backward with one Butterworth filter of the pair (so the magnitude
        is that of the crossover) and needs no all-pass compensation; activate_zi keeps the states between calls."""
        if mode == FilterBankMode.Sequential:
            warn("sequential mode is not supported for this filter bank. It is automatically changed to summed")
            mode = FilterBankMode.Summed
        assert s.sampling_rate_hz == self.sampling_rate_hz, "Sampling rates do not match"
        assert not (activate_zi and zero_phase), "Zero phase filtering and activating zi is a valid setting"
        n_cross = self.number_of_cross
        bands = np.zeros((s.time_data.shape[0], s.number_of_channels, self.number_of_bands))
        rest = s.time_data.copy()
        if activate_zi:
            if not hasattr(self, "channels_zi") or len(self.channels_zi) != s.number_of_channels:
                self.initialize_zi(s.number_of_channels)
            for ch in range(s.number_of_channels):
                splits, allpasses = self.channels_zi[ch]
                for cn in range(n_cross):
                    band, rest[:, ch] = self._pair_zi(rest[:, ch], cn, splits[cn])
                    for ap in range(cn + 1, n_cross):
                        band = np.add(*self._pair_zi(band, ap, allpasses[cn][ap]))
                    bands[:, ch, cn] = band
                bands[:, ch, n_cross] = rest[:, ch]
        elif zero_phase:
            for cn in range(n_cross):
                doubled = not (self.order[cn] % 2 == 1 or self.order[cn] == 2)
                rows = self.sos[cn][0].shape[0] // (2 if doubled else 1)
                bands[:, :, cn] = backend._sosfiltfilt(self.sos[cn][0][:rows], rest)
                rest = backend._sosfiltfilt(self.sos[cn][1][:rows], rest)
            bands[:, :, n_cross] = rest
        else:
            for cn in range(n_cross):
                band, rest = self._pair(rest, cn)
                for ap in range(cn + 1, n_cross):
                    band = np.add(*self._pair(band, ap))
                bands[:, :, cn] = band
            bands[:, :, n_cross] = rest
        out = MultiBandSignal(
            bands=[s.copy_with_new_time_data(bands[:, :, n]) for n in range(self.number_of_bands)],
            same_sampling_rate=True,
            info=dict(readme="MultiBandSignal made using Linkwitz-Riley filter bank", filterbank_freqs=self.freqs,
                      filterbank_order=self.order))
        return out.collapse() if mode == FilterBankMode.Summed else out

    def _pair(self, x, cross: int):
        """(low, high) of crossover `cross` on (samples, channels) data, from rest."""
        return backend._sosfilt(self.sos[cross][0], x), backend._sosfilt(self.sos[cross][1], x)

    def _pair_zi(self, x, cross: int, zi: list):
        """(low, high) of crossover `cross` on one channel, continuing from and updating zi = [low state, high state]."""
        out = []
        for side in (0, 1):
            y, zf = backend._sosfilt(self.sos[cross][side], np.ascontiguousarray(x)[:, None], zi[side][:, :, None])
            zi[side] = zf[:, :, 0]
            out.append(y[:, 0])
        return out

    def get_ir(self, length_samples: int, mode: FilterBankMode = FilterBankMode.Parallel, zero_phase: bool = False):
        """The bank's response to a unit pulse of length_samples."""
        d = np.zeros((length_samples, 1))
        d[0] = 1.0
        return self.filter_signal(ImpulseResponse(None, d, self.sampling_rate_hz), mode=mode, zero_phase=zero_phase,
                                  activate_zi=False)

    def copy(self) -> "LRFilterBank":
        return deepcopy(self)
