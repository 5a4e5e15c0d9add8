"""The reference's sample-by-sample realtime filters on the device: StateVariableFilter (classes/sv_filter.py),
ParallelFilter (classes/parallel_filter.py), IIRFilter (classes/iir_filter_realtime.py), FIRFilter
(classes/fir_filter_realtime.py), StateSpaceFilter (classes/state_space_filter.py), FilterChain (classes/filter_chain.py)
and ExponentialAverageFilter (classes/exponential_average_filter.py).

`filter_signal` runs the same recursion in float64 on the device, time-parallel (backend.rtfilt_filter, backend.rtfir_filter,
csrc/kernels_rtfilt.hpp).  Where the reference has no `filter_signal` (IIRFilter, FIRFilter,
StateSpaceFilter, FilterChain) it is an additive method with LatticeLadderFilter's semantics: it starts from the object's
state and leaves the final state there, so two calls continue the recursion and `process_sample` continues after it.
`process_sample`, `reset_state` and `set_n_channels` are the reference's one-sample host float64 arithmetic: one sample is
not a device workload, and it is no fallback for any device path.  Design code (`from_filter*`, `fit_to_ir`) stays float64
on the host.  ExponentialAverageFilter branches on x > state, is not linear and has no device path.

What the device path does not run raises NotImplementedError: more than 64 states or 32 sections, an unstable recursion,
a carry gain above the kernels' limit, more than 4096 FIR taps, complex coefficients or complex input samples."""

from warnings import warn

import numpy as np
import scipy.signal as sig

from .. import backend
from ..standard.enums import FilterCoefficientsType
from .filter import Filter
from .filterbank import FilterBank
from .fir_filter_realtime import RealtimeFilter
from .impulse_response import ImpulseResponse
from .multibandsignal import MultiBandSignal
from .signal import Signal
from .structure_filters import _refuse_complex

_CHANNELS_WARNING = ("Number of channels did not match the filter's state. The right number of channels are automatically "
                     "initiated")


def _dirac(length_samples: int, sampling_rate_hz: int) -> ImpulseResponse:
    d = np.zeros((length_samples, 1))
    d[0] = 1.0
    return ImpulseResponse(None, d, sampling_rate_hz)


def _run(signal: Signal, kind: int, coef, d: int, aux: int = 0, delay: int = 0, fir=None, zi=None, want_zf: bool = False):
    """signal through the packed filter from zi (None: zero state) -> (the new signal, or the four of them for the
    state-variable filter; zf or None).  A device-resident signal is read where it lies and its result stays resident;
    only the states and coefficients cross."""
    if zi is not None and not np.any(zi):
        zi = None
    if signal.on_device:
        out = backend.rtfilt_filter_device(signal.device_samples, kind, coef, d, aux, delay, fir, zi=zi, want_zf=want_zf)
        y, zf = out if want_zf else (out, None)
        return ([signal._device_result(b) for b in y] if isinstance(y, list) else signal._device_result(y)), zf
    out = backend.rtfilt_filter(signal.time_data, kind, coef, d, aux, delay, fir, zi=zi, want_zf=want_zf)
    y, zf = out if want_zf else (out, None)
    return ([signal.copy_with_new_time_data(b) for b in y] if y.ndim == 3 else signal.copy_with_new_time_data(y)), zf


def _run_fir(signal: Signal, b, hist=None) -> Signal:
    if signal.on_device:
        return signal._device_result(backend.rtfir_filter_device(signal.device_samples, b, hist))
    return signal.copy_with_new_time_data(backend.rtfir_filter(signal.time_data, b, hist))


def _last_samples(signal: Signal, count: int):
    """The last min(count, N) samples of every channel as float64 (samples, channels); of a resident signal only those
    come down."""
    count = min(count, signal.time_data.shape[0] if not signal.on_device else signal.device_samples.n_samples)
    if not signal.on_device:
        return np.asarray(signal.time_data[len(signal.time_data) - count:], dtype=np.float64)
    dev = signal.device_samples
    out = np.empty((dev.n_ch, count), dtype=np.float32)
    if count:
        for c in range(dev.n_ch):
            dev.ctx.download(dev.ptr + 4 * (c * dev.ld + dev.n_samples - count), out[c])
    return out.T.astype(np.float64)


# ---- state-variable filter -------------------------------------------------------------------------------------------
class StateVariableFilter(RealtimeFilter):
    """A state-variable filter discretised with the topology-preserving transform (trapezoidal integrators), a 2-pole
    multimode filter (Zavalishin: The Art of VA Filter Design, p. 81; `resonance` is 2R, Q = 1 / resonance).
    `filter_signal` gives the four outputs low pass, high pass, band pass and all-pass as the bands of a MultiBandSignal;
    it starts from `self.state` and leaves the final state there."""

    def __init__(self, frequency_hz: float, resonance: float, sampling_rate_hz: int):
        self.sampling_rate_hz = sampling_rate_hz
        self.set_parameters(frequency_hz, resonance, 1)

    def set_parameters(self, frequency_hz: float, resonance: float, n_channels: int):
        assert frequency_hz > 0 and frequency_hz < self.sampling_rate_hz // 2
        self.g = np.tan(np.pi * frequency_hz / self.sampling_rate_hz)
        self.resonance = resonance
        self.intermediate_value = 1 / (1 + self.resonance * self.g + self.g ** 2)
        self.set_n_channels(n_channels)
        return self

    def set_n_channels(self, n_channels: int):
        assert n_channels > 0
        self.n_channels = n_channels
        self.state = np.zeros((2, self.n_channels))

    def reset_state(self):
        self.state.fill(0)

    def process_sample(self, sample: float, channel: int = 0):
        """-> (low pass, high pass, band pass, all-pass)"""
        yh = (sample - (self.resonance + self.g) * self.state[0, channel] - self.state[1, channel]) * self.intermediate_value
        yb = self.g * yh + self.state[0, channel]
        self.state[0, channel] = self.g * yh + yb
        yl = self.g * yb + self.state[1, channel]
        self.state[1, channel] = self.g * yb + yl
        return yl, yh, yb, yl - self.resonance * yb + yh

    def filter_signal(self, signal: Signal) -> MultiBandSignal:
        assert self.sampling_rate_hz == signal.sampling_rate_hz, "Sampling rates do not match"
        _refuse_complex(signal, np.asarray(self.resonance), np.asarray(self.g))
        if not self.resonance > 0:
            raise NotImplementedError("a state-variable filter with resonance <= 0 is unstable or marginal: the "
                                      "time-parallel carry of the device recursion is exact only for a stable one")
        n, n_ch = signal.time_data.shape if not signal.on_device else (signal.device_samples.n_samples,
                                                                       signal.device_samples.n_ch)
        if n < n_ch:
            raise ValueError("a signal with fewer samples than channels is not filtered (the reference's output array has "
                             "the wrong shape there)")
        if self.n_channels != n_ch:
            self.set_n_channels(n_ch)
        coef = np.array([self.g, self.resonance, self.intermediate_value], dtype=np.float64)
        bands, zf = _run(signal, backend.RTFILT_SVF, coef, 2, zi=self.state, want_zf=True)
        self.state = zf
        return MultiBandSignal(bands)

    def get_ir(self, length_samples: int) -> MultiBandSignal:
        self.reset_state()
        return self.filter_signal(_dirac(length_samples, self.sampling_rate_hz))

    def plot_magnitude(self, *args, **kwargs):
        raise NotImplementedError("plots are not built in this project")

    def plot_group_delay(self, *args, **kwargs):
        raise NotImplementedError("plots are not built in this project")

    def plot_phase(self, *args, **kwargs):
        raise NotImplementedError("plots are not built in this project")


# ---- transposed direct form II ---------------------------------------------------------------------------------------
class IIRFilter(RealtimeFilter):
    """An IIR filter as a transposed direct form II of any order up to 64, state (order, channels)."""

    def __init__(self, b, a):
        b /= a[0]
        a /= a[0]
        self.order = max(len(b), len(a)) - 1
        self.b = np.pad(b, ((0, self.order + 1 - len(b))))
        self.a = np.pad(a, ((0, self.order + 1 - len(a))))
        self.set_n_channels(1)

    @staticmethod
    def from_filter(iir: Filter):
        assert iir.is_iir, "Only valid for IIR filters"
        b, a = iir.get_coefficients(FilterCoefficientsType.Ba)
        return IIRFilter(b, a)

    def set_n_channels(self, n_channels: int):
        self.state = np.zeros((self.order, n_channels))

    def reset_state(self):
        self.state.fill(0.0)

    def process_sample(self, x: float, channel: int):
        y = self.b[0] * x + self.state[0, channel]
        for i in range(self.order - 1):
            self.state[i, channel] = x * self.b[i + 1] - y * self.a[i + 1] + self.state[i + 1, channel]
        self.state[-1, channel] = x * self.b[-1] - y * self.a[-1]
        return y

    def _structure(self):
        if self.order > backend.RTFILT_MAX_STATES:
            raise NotImplementedError(f"an IIR filter of an order above {backend.RTFILT_MAX_STATES} is not run on the device "
                                      f"(got {self.order}): the carry's state vector is one value per lane of a wave")
        if self.order and not np.all(np.abs(np.roots(self.a)) < 1.0):
            raise NotImplementedError("an IIR filter with a pole on or outside the unit circle is unstable: the "
                                      "time-parallel carry of the device recursion is exact only for a stable one")
        return backend.RTFILT_TDF2, np.concatenate([self.b, self.a]).astype(np.float64), self.order

    def filter_signal(self, signal: Signal) -> Signal:
        """Additive: the signal through the filter from `self.state`, which is left holding the final state."""
        _refuse_complex(signal, self.b, self.a)
        kind, coef, d = self._structure()  # (raises before any state is touched)
        if self.state.shape[1] != signal.number_of_channels:
            warn(_CHANNELS_WARNING)
            self.set_n_channels(signal.number_of_channels)
        if d == 0:
            return _run_fir(signal, np.asarray(self.b[:1], dtype=np.float64))
        new_signal, zf = _run(signal, kind, coef, d, zi=self.state, want_zf=True)
        self.state = zf
        return new_signal


# ---- direct FIR ------------------------------------------------------------------------------------------------------
class FIRFilter(RealtimeFilter):
    """An FIR filter in the time domain; the state is a circular buffer of the last `order` input samples and
    `current_state_ind`, the index of the newest one, per channel."""

    def __init__(self, b):
        self.order = len(b) - 1
        self.b = b
        self.set_n_channels(1)

    @staticmethod
    def from_filter(fir: Filter):
        assert fir.is_fir, "Only valid for FIR filters"
        b, _ = fir.get_coefficients(FilterCoefficientsType.Ba)
        return FIRFilter(b)

    def set_n_channels(self, n_channels: int):
        self.state = np.zeros((self.order, n_channels))
        self.current_state_ind = np.zeros(n_channels, dtype=np.int_)

    def reset_state(self):
        self.state.fill(0.0)

    def process_sample(self, x: float, channel: int):
        y = self.b[0] * x
        write_index = self.current_state_ind[channel]
        for i in range(self.order):
            read_index = (write_index - i) % self.order
            y += self.state[read_index, channel] * self.b[i + 1]
        write_index = (write_index + 1) % self.order
        self.state[write_index, channel] = x
        self.current_state_ind[channel] = write_index
        return y

    def _history(self):
        """The circular buffer as (channels, order), oldest sample first: x[n - 1 - i] lies at (index - i) % order."""
        order = self.order
        rows = (self.current_state_ind[None, :] - (order - 1 - np.arange(order))[:, None]) % order  # (order, channels)
        return np.take_along_axis(self.state, rows, axis=0).T.astype(np.float64)

    def filter_signal(self, signal: Signal) -> Signal:
        """Additive: the signal through the filter from the state, which is left exactly as the reference's sample loop
        would have left it (it holds input samples: the last `order` of them are put in place on the host)."""
        _refuse_complex(signal, self.b)
        b = np.asarray(self.b, dtype=np.float64)
        if self.state.shape[1] != signal.number_of_channels:
            warn(_CHANNELS_WARNING)
            self.set_n_channels(signal.number_of_channels)
        order = self.order
        hist = self._history() if order and np.any(self.state) else None
        new_signal = _run_fir(signal, b, hist)
        if order:
            n = signal.device_samples.n_samples if signal.on_device else signal.time_data.shape[0]
            tail = _last_samples(signal, order)  # (min(order, n), channels)
            for m in range(len(tail)):  # sample n - len(tail) + m was written at (index + n - len(tail) + m + 1) % order
                rows = (self.current_state_ind + (n - len(tail) + m + 1)) % order
                self.state[rows, np.arange(self.state.shape[1])] = tail[m]
            self.current_state_ind = (self.current_state_ind + n) % order
        return new_signal


# ---- state space -----------------------------------------------------------------------------------------------------
class StateSpaceFilter(RealtimeFilter):
    """A state-space filter y[n] = C x[n] + D u[n], x[n + 1] = A x[n] + B u[n] from the system's matrices (the
    controller-canonical form scipy.signal.tf2ss gives is expected); the state is `self.x` (states, channels)."""

    def __init__(self, A, B, C, D):
        assert A.ndim == 2, "Matrix A should have exactly 2 dimensions"
        assert len(B) == A.shape[1], "Matrix B dimensions are not valid"
        self.A = A.squeeze()
        self.B = B.squeeze()
        self.C = C.squeeze()
        self.D = D.squeeze()
        self.set_n_channels(1)

    @staticmethod
    def from_filter(filt: Filter):
        b, a = filt.get_coefficients(FilterCoefficientsType.Ba)
        return StateSpaceFilter(*sig.tf2ss(b, a))

    @staticmethod
    def from_filter_as_sos_list(filt: Filter):
        sos = filt.get_coefficients(FilterCoefficientsType.Sos)
        return [StateSpaceFilter(*sig.tf2ss(sos[n, :3], sos[n, 3:])) for n in range(sos.shape[0])]

    def reset_state(self):
        self.x.fill(0.0)

    def set_n_channels(self, n_channels: int):
        self.x = np.zeros((self.A.shape[0], n_channels))

    def process_sample(self, x: float, channel: int):
        y = self.C @ self.x[:, channel] + self.D * x
        self.x[:, channel] = self.A @ self.x[:, channel] + self.B * x
        return y

    def _structure(self):
        d = self.A.shape[0]
        if d > backend.RTFILT_MAX_STATES:
            raise NotImplementedError(f"a state-space filter with more than {backend.RTFILT_MAX_STATES} states is not run on "
                                      f"the device (got {d}): the carry's state vector is one value per lane of a wave")
        if not np.all(np.abs(np.linalg.eigvals(self.A)) < 1.0):
            raise NotImplementedError("a state-space filter with an eigenvalue of A on or outside the unit circle is "
                                      "unstable: the time-parallel carry of the device recursion is exact only for a stable "
                                      "one")
        coef = np.concatenate([np.ravel(self.A), np.ravel(self.B), np.ravel(self.C), np.ravel(self.D)]).astype(np.float64)
        return backend.RTFILT_STATE_SPACE, coef, d

    def filter_signal(self, signal: Signal) -> Signal:
        """Additive: the signal through the system from `self.x`, which is left holding the final state."""
        _refuse_complex(signal, self.A, self.B, self.C, self.D)
        kind, coef, d = self._structure()  # (raises before any state is touched)
        if self.x.shape[1] != signal.number_of_channels:
            warn(_CHANNELS_WARNING)
            self.set_n_channels(signal.number_of_channels)
        new_signal, zf = _run(signal, kind, coef, d, zi=self.x, want_zf=True)
        self.x = zf
        return new_signal


# ---- parallel second-order sections ----------------------------------------------------------------------------------
class ParallelFilter(RealtimeFilter):
    """A fixed-pole parallel filter: second-order sections in parallel and an FIR part (B. Bank: Warped, Kautz, and
    Fixed-Pole Parallel Filters: A Review, JAES 2022).  Only real poles or complex poles with positive imaginary part are
    passed (the conjugates are implied).  `filter_signal` runs from rest, as the reference does: the FIR sum, then every
    section over the delayed input in ONE pass of the device recursion."""

    def __init__(self, poles, n_fir: int, sampling_rate_hz: int):
        assert n_fir >= 0, "n_fir must be at least 0"
        assert np.all(np.abs(poles) < 1.0), "At least one pole lies outside the unit circle"
        assert np.all(poles.imag >= 0.0), "Only poles with positive imaginary part are accepted"
        assert np.all(np.abs(poles) > 0.0), "No poles at the origin should be used"
        assert all([np.sum(np.isclose(poles, p)) == 1 for p in poles]), "Pole multiplicity cannot be more than 1"
        assert sampling_rate_hz > 0, "Sampling rate must be greater than 0"
        self.poles = poles
        self.n_fir = n_fir
        self.sampling_rate_hz = sampling_rate_hz
        self.set_parameters()

    def set_parameters(self, delay_iir_samples: int = 0, fir_offset_ms: float = 0.0):
        assert delay_iir_samples >= 0, "Delay should not be negative"
        self.fir_offset_samples = max(1, int(self.sampling_rate_hz * fir_offset_ms / 1e3 + 0.5))
        self.delay_iir_samples = (self.n_fir + 1 + self.fir_offset_samples * (self.n_fir - 1)
                                  if delay_iir_samples is None else delay_iir_samples)
        return self

    def set_coefficients(self, iir_coefficients, fir=None):
        """iir_coefficients (n_sos, 2): the numerators b0, b1 of every section; fir: the FIR coefficients."""
        assert iir_coefficients.ndim == 2
        assert iir_coefficients.shape[0] == self._sos.shape[0]
        for ss in range(self._sos.shape[0]):
            self._sos[ss, :2] = iir_coefficients[ss, :]
        if fir is not None:
            assert fir.ndim == 1
            self._fir_coefficients = fir
        else:
            self._fir_coefficients = np.array([])
        self.n_fir = len(self._fir_coefficients)
        return self

    def fit_to_ir(self, ir: ImpulseResponse):
        """The frequency-domain least-squares fit of the sections' numerators and the FIR part to a single-channel
        (preferably minimum-phase) impulse response.  Design code: float64 on the host."""
        from scipy.linalg import lstsq
        assert ir.number_of_channels == 1, "This is only valid for a single-channel IR"
        freqs, spectrum_channels = ir.get_spectrum()
        freqs = freqs[1:]
        spectrum_channels = spectrum_channels[1:]
        fs_hz = ir.sampling_rate_hz

        comp_inds = self.poles.imag != 0
        poles = np.hstack([self.poles, self.poles[comp_inds].conjugate()])
        self._sos = sig.zpk2sos([], poles, 1.0)
        n_sos = self._sos.shape[0]

        n_parameters = n_sos * 3 + self.n_fir
        M = np.zeros((len(freqs), n_parameters), dtype=np.complex128)
        for ind in range(0, n_sos * 3, 3):
            M[:, ind] = sig.sosfreqz(self._sos[ind // 3, :][None, :], freqs, fs=fs_hz)[1]
            sos_delayed = self._sos[ind // 3, :].copy()  # delayed by one sample
            sos_delayed[0] = 0.0
            sos_delayed[1] = 1.0
            M[:, ind + 1] = sig.sosfreqz(sos_delayed[None, :], freqs, fs=fs_hz)[1]
            sos_delayed = self._sos[ind // 3, :].copy()  # delayed by two samples
            sos_delayed[0] = 0.0
            sos_delayed[1] = 0.0
            sos_delayed[2] = 1.0
            M[:, ind + 2] = sig.sosfreqz(sos_delayed[None, :], freqs, fs=fs_hz)[1]
        if self.delay_iir_samples > 0:
            M[:, :n_sos * 3] *= sig.freqz([0.0] * self.delay_iir_samples + [1.0], [1.0], freqs, fs=fs_hz)[1][:, None]
        for n in range(self.n_fir):  # an impulse at index n of the FIR part
            M[:, n_sos * 3 + n] = sig.freqz(np.hstack([[0.0] * (n * self.fir_offset_samples), [1.0]]), [1.0], freqs,
                                            fs=fs_hz)[1]
        M = np.vstack([np.real(M), np.imag(M)])
        spectrum = spectrum_channels[:, 0]
        spectrum = np.hstack([np.real(spectrum), np.imag(spectrum)])
        solution = lstsq(M, spectrum, overwrite_a=True, overwrite_b=True)[0]

        for ind in range(0, n_sos * 3, 3):
            self._sos[ind // 3, 0] = solution[ind]
            self._sos[ind // 3, 1] = solution[ind + 1]
            self._sos[ind // 3, 2] = solution[ind + 2]
        self._fir_coefficients = solution[n_sos * 3:]

        if self.fir_offset_samples > 1 and self.n_fir > 1:  # the delays between the FIR coefficients
            ff = np.zeros(((self.fir_offset_samples) * (len(self._fir_coefficients) - 1) + 1))
            ff[:: self.fir_offset_samples + 1] = self._fir_coefficients[:-1]
            ff[-1] = self._fir_coefficients[-1]
            self._fir_coefficients = ff

        self._compute_filter_bank()
        return self

    def _compute_filter_bank(self):
        fb = FilterBank([Filter.from_sos(self._sos[n, :][None, ...], self.sampling_rate_hz)
                         for n in range(self._sos.shape[0])])
        if len(self._fir_coefficients) > 0:
            fb.add_filter(Filter.from_ba(self._fir_coefficients, [1.0], self.sampling_rate_hz))
        self.filter_bank = fb
        self.iir = []
        for f in self.filter_bank:
            if not f.is_iir:
                self.fir = FIRFilter(f.get_coefficients(FilterCoefficientsType.Ba)[0])
            else:
                self.iir.append(IIRFilter(*f.get_coefficients(FilterCoefficientsType.Ba)))
        if self.delay_iir_samples > 0:
            self.iir_delay = FIRFilter(np.array(self.delay_iir_samples * [0.0] + [1.0]))

    def filter_signal(self, signal: Signal) -> Signal:
        assert self.sampling_rate_hz == signal.sampling_rate_hz, "Sampling rates do not match"
        sos = np.asarray(self._sos)
        fir = np.asarray(self._fir_coefficients)
        _refuse_complex(signal, sos, fir)
        n_sec = sos.shape[0]
        if n_sec > backend.RTFILT_MAX_STATES // 2:
            raise NotImplementedError(f"a parallel filter with more than {backend.RTFILT_MAX_STATES // 2} sections is not run "
                                      f"on the device (got {n_sec}): the carry's state vector is one value per lane of a "
                                      f"wave")
        coef = np.ascontiguousarray(sos[:, [0, 1, 2, 4, 5]], dtype=np.float64).ravel()
        fir = np.asarray(fir, dtype=np.float64) if self.n_fir > 0 else None
        return _run(signal, backend.RTFILT_PARALLEL, coef, 2 * n_sec, n_sec, int(self.delay_iir_samples), fir)[0]

    def get_ir(self, length_samples: int):
        return self.filter_signal(_dirac(length_samples, self.sampling_rate_hz))

    def set_n_channels(self, n_channels: int):
        for f in self.iir:
            f.set_n_channels(n_channels)
        if self.n_fir > 0:
            self.fir.set_n_channels(n_channels)
        if self.delay_iir_samples > 0:
            self.iir_delay.set_n_channels(n_channels)

    def reset_state(self):
        for f in self.iir:
            f.reset_state()
        if self.n_fir > 1:
            self.fir.reset_state()
        if self.delay_iir_samples > 0:
            self.iir_delay.reset_state()

    def process_sample(self, x: float, channel: int):
        y = 0.0
        if self.n_fir > 1:
            y += self.fir.process_sample(x, channel)
        elif self.n_fir == 1:
            y += self._fir_coefficients[0] * x
        if self.delay_iir_samples > 0:
            x = self.iir_delay.process_sample(x, channel)
        for f in self.iir:
            y += f.process_sample(x, channel)
        return y


# ---- chain -----------------------------------------------------------------------------------------------------------
class FilterChain(RealtimeFilter):
    """A series of realtime filters applied in the given order."""

    def __init__(self, filters: list):
        self.filters = filters

    @property
    def n_filters(self):
        return len(self.filters)

    def set_n_channels(self, n_channels: int):
        for f in self.filters:
            f.set_n_channels(n_channels)

    def reset_state(self):
        for f in self.filters:
            f.reset_state()

    def process_sample(self, x: float, channel: int):
        for f in self.filters:
            x = f.process_sample(x, channel)
        return x

    def filter_signal(self, signal: Signal) -> Signal:
        """Additive: the members' `filter_signal` in order.  A host signal stays a float64 host array between the members;
        a device-resident one stays resident and is rounded to float32 once per member."""
        for i, f in enumerate(self.filters):
            if not callable(getattr(f, "filter_signal", None)) or isinstance(f, StateVariableFilter):
                raise NotImplementedError(f"member {i} of the chain ({type(f).__name__}) has no filter_signal that returns a "
                                          f"Signal")
        for f in self.filters:
            signal = f.filter_signal(signal)
        return signal


# ---- exponential average ---------------------------------------------------------------------------------------------
def _get_smoothing_factor_ema(relaxation_time_s: float, sampling_rate_hz: int, accuracy: float = 0.95):
    """alpha of the exponential moving average y[n] = alpha x[n] + (1 - alpha) y[n - 1] whose step response is within
    `accuracy` (in ]0, 1[) of 1 after the relaxation time: alpha = 1 - (1 - accuracy)^(1 / (time * rate))."""
    factor = np.log(1 - accuracy)
    return 1 - np.exp(factor / relaxation_time_s / sampling_rate_hz)


class ExponentialAverageFilter(RealtimeFilter):
    """A one-pole smoothing filter with one coefficient for rising and one for falling input.  Host arithmetic only: its
    branch on x > state is not linear, so it has no place in the time-parallel recursion, and it has no
    `filter_signal`."""

    def __init__(self, increase_time_s: float, decrease_time_s: float, sampling_rate_hz: int,
                 accuracy_step_response: float = 0.95):
        self.sampling_rate_hz = sampling_rate_hz
        self.increase_coefficient = _get_smoothing_factor_ema(increase_time_s, self.sampling_rate_hz, accuracy_step_response)
        self.decrease_coefficient = _get_smoothing_factor_ema(decrease_time_s, self.sampling_rate_hz, accuracy_step_response)
        self.set_n_channels(1)

    def set_n_channels(self, n_channels: int):
        self.state = np.zeros((1, n_channels))

    def reset_state(self):
        self.state.fill(0.0)

    def process_sample(self, x: float, channel: int):
        if x > self.state:  # ascending
            y = x * self.increase_coefficient + (1 - self.increase_coefficient) * self.state[0, channel]
        else:  # descending
            y = x * self.decrease_coefficient + (1 - self.decrease_coefficient) * self.state[0, channel]
        self.state[0, channel] = y
        return y
