"""The reference's structure filters on the device: LatticeLadderFilter (classes/lattice_ladder_filter.py), WarpedFIR /
WarpedIIR (classes/warped_filters.py) and KautzFilter (classes/kautz_filter.py).

In the reference each is a Python loop over samples, stages and channels.  Here `filter_signal` runs the same
recursion in float64 on the device, time-parallel (backend.sfilt_filter, csrc/kernels_sfilt.hpp);
the coefficient conversions (`from_filter`, the warped-IIR sigmas, the Kautz normalisations, the Kautz pole search) are
design code and stay float64 on the host, as everywhere in this project.  `process_sample` is the reference's one-sample
step as host float64 arithmetic: one sample is not a device workload, and it is no fallback for any device path.

What the device path does not run raises NotImplementedError: more than 64 states, an unstable recursion (the
time-parallel carry is exact only for a stable one), a carry gain above the kernels' limit, complex coefficients or
complex input samples."""

from warnings import warn

import numpy as np

from .. import backend
from ..standard.enums import FilterCoefficientsType
from .filter import Filter
from .fir_filter_realtime import RealtimeFilter
from .impulse_response import ImpulseResponse
from .signal import Signal


def _refuse_complex(signal: Signal, *coefficients):
    if any(c is not None and np.iscomplexobj(c) for c in coefficients):
        raise NotImplementedError("structure filters with complex coefficients are not run on the device (its "
                                  "recursions are real)")
    if signal.is_complex_signal:
        raise NotImplementedError("complex input samples are not run through the device recursion (its input is real)")


def _run(signal: Signal, structure, zi=None, want_zf: bool = False):
    """signal through the packed structure (kind, coef, d, aux) from zi (None: zero state) -> (the new signal, zf or
    None).  A device-resident signal is read where it lies and its result stays resident; only the states cross."""
    kind, coef, d, aux = structure
    if zi is not None and not np.any(zi):
        zi = None
    if signal.on_device:
        out = backend.sfilt_filter_device(signal.device_samples, kind, coef, d, aux, zi=zi, want_zf=want_zf)
        y, zf = out if want_zf else (out, None)
        return signal._device_result(y), zf
    out = backend.sfilt_filter(signal.time_data, kind, coef, d, aux, zi=zi, want_zf=want_zf)
    y, zf = out if want_zf else (out, None)
    return signal.copy_with_new_time_data(y), zf


# ---- lattice / lattice-ladder ----------------------------------------------------------------------------------------
def _step_down(alpha):
    """Oppenheim / Schafer's step-down recursion: alpha (N,) the coefficients of A(z) = 1 - sum alpha_m z^-m ->
    (reflection coefficients k (N,), rows (N, N) with rows[i - 1, m - 1] = alpha_m of the order-i predictor)."""
    n = len(alpha)
    rows = np.zeros((n, n))
    rows[n - 1] = alpha
    k = np.zeros(n)
    k[n - 1] = alpha[n - 1]
    with np.errstate(divide="ignore", invalid="ignore"):  # (|k| = 1 ends in inf or nan, which the callers refuse)
        for i in range(n - 1, 0, -1):  # order i + 1 -> order i
            cur = rows[i, :i + 1]
            rows[i - 1, :i] = (cur[:i] + k[i] * cur[:i][::-1]) / (1.0 - k[i] ** 2)
            k[i - 1] = rows[i - 1, i - 1]
    return k, rows


def _lattice_ladder_from_ba(b, a):
    """k and the ladder taps c_m = b_m + sum_{i > m} c_i alpha^(i)_{i-m} of b / a (a is taken as it is, a[0] = 1)."""
    k, rows = _step_down(-np.asarray(a, dtype=np.float64)[1:])
    c = np.zeros(len(b))
    for m in range(len(b) - 1, -1, -1):
        c[m] = b[m] + sum(c[i] * rows[i - 1, i - 1 - m] for i in range(m + 1, len(b)))
    return k, c


def _lattice_ladder_from_sos(sos):
    """Per second-order section (normalised by its a0): k (K, 2), c (K, 3)."""
    sos = np.asarray(sos, dtype=np.float64)
    sos = sos / sos[:, 3:4]
    k = np.zeros((len(sos), 2))
    c = np.zeros((len(sos), 3))
    a1 = -sos[:, 4]
    k[:, 1] = -sos[:, 5]
    k[:, 0] = (a1 + k[:, 1] * a1) / (1.0 - k[:, 1] ** 2)
    c[:, 2] = sos[:, 2]
    c[:, 1] = sos[:, 1] + c[:, 2] * a1
    c[:, 0] = sos[:, 0] + c[:, 1] * k[:, 0] + c[:, 2] * k[:, 1]
    return k, c


class LatticeLadderFilter(RealtimeFilter):
    """A lattice (FIR: reflection coefficients k only) or lattice-ladder (IIR: k and ladder taps c) filter, the
    structure linear prediction produces.  2-D k (K, 2) with c (K, 3) filters in second-order sections.

    IIR: the first k (and c) coefficient is the first from right (output) to left; FIR: the first k is the first from
    left to right.  `filter_signal` starts from `self.state` and leaves the final state there, so consecutive calls
    continue the recursion; `process_sample` shares that state."""

    def __init__(self, k_coefficients, c_coefficients=None, sampling_rate_hz: int | None = None):
        assert sampling_rate_hz is not None, "Sampling rate cannot be None"
        assert k_coefficients.ndim in (2, 1), "k_coefficients should be a vector or a matrix"
        if k_coefficients.ndim == 2:
            assert c_coefficients is not None, ("Second-order sections are only valid for IIR filters. "
                                                "C coefficients cannot be None")
            assert k_coefficients.shape[1] == 2, ("When k has two dimensions, it is assumed that the "
                                                  "second one has length 2 (second-order section)")
            assert c_coefficients.shape[1] == 3, "Second-order sections should have 3 c coefficients"
            assert c_coefficients.shape[0] == k_coefficients.shape[0], "Number of second-order sections do not match"
            self.iir_filter = True
            self.sos_filtering = True
        else:
            self.sos_filtering = False
            if c_coefficients is not None:
                assert len(c_coefficients) == len(k_coefficients) + 1, \
                    "c_coefficients must have the length len(k_coefficients) + 1"
                self.iir_filter = True
            else:
                self.iir_filter = False
        self.k = k_coefficients
        self.c = c_coefficients
        self.state = None
        self.sampling_rate_hz = sampling_rate_hz
        self.set_n_channels(1)

    @staticmethod
    def from_filter(filt: Filter) -> "LatticeLadderFilter":
        """The lattice(-ladder) representation of an IIR (ba or sos) or FIR filter.  A linear-phase FIR filter has
        reflection coefficients on the unit circle and cannot be converted (assertion)."""
        if filt.is_iir:
            if filt.has_sos:
                k, c = _lattice_ladder_from_sos(filt.get_coefficients(FilterCoefficientsType.Sos))
            else:
                k, c = _lattice_ladder_from_ba(*filt.get_coefficients(FilterCoefficientsType.Ba))
            return LatticeLadderFilter(k, c, filt.sampling_rate_hz)
        b, _ = filt.get_coefficients(FilterCoefficientsType.Ba)
        b = np.asarray(b, dtype=np.float64) / b[0]
        k, _ = _step_down(-b[1:])
        assert np.all(np.abs(k) < 1), "Some reflection coefficient was equal or larger than one, this is not supported"
        return LatticeLadderFilter(k, None, filt.sampling_rate_hz)

    def set_n_channels(self, n_channels: int):
        assert n_channels > 0, "At least one channel must be initialized"
        if self.sos_filtering:
            self.state = np.zeros((self.k.shape[0], 2, n_channels))
        else:
            self.state = np.zeros((len(self.k), n_channels))
        self.n_channels = n_channels

    def reset_state(self):
        self.state.fill(0.0)

    def _structure(self):
        """(kind, packed coefficients, states, aux) for the device; NotImplementedError for what it does not run."""
        k = np.asarray(self.k, dtype=np.float64)
        if not self.iir_filter:
            return backend.SFILT_FIR_LATTICE, k, len(k), 0
        if not np.all(np.abs(k) < 1.0):
            raise NotImplementedError("a lattice-ladder filter with a reflection coefficient |k| >= 1 is unstable: the "
                                      "time-parallel carry of the device recursion is exact only for a stable one")
        c = np.asarray(self.c, dtype=np.float64)
        if self.sos_filtering:
            return backend.SFILT_SOS_LATTICE, np.concatenate([k, c], axis=1).ravel(), 2 * len(k), 0
        return backend.SFILT_IIR_LATTICE, np.concatenate([k, c]), len(k), 0

    def filter_signal(self, signal: Signal) -> Signal:
        assert signal.sampling_rate_hz == self.sampling_rate_hz, "Sampling rates do not match"
        _refuse_complex(signal, self.k, self.c)
        structure = self._structure()  # (raises before any state is touched)
        if self.n_channels != signal.number_of_channels:
            warn("Number of channels did not match the filter's state. The right number of channels are automatically "
                 "initiated")
            self.set_n_channels(signal.number_of_channels)
        zi = np.asarray(self.state, dtype=np.float64).reshape(structure[2], self.n_channels)
        new_signal, zf = _run(signal, structure, zi, want_zf=True)
        self.state = zf.reshape(self.state.shape)
        return new_signal

    def process_sample(self, x: float, channel: int):
        st, k, c = self.state, self.k, self.c
        if not self.iir_filter:
            s0 = x
            for i in range(len(k)):
                s1 = -x * k[i] + st[i, channel]
                x -= st[i, channel] * k[i]
                st[i, channel] = s0
                s0 = s1
            return x
        if self.sos_filtering:
            for sec in range(k.shape[0]):
                x += st[sec, 1, channel] * k[sec, 1]
                x_low = (x * -k[sec, 1] + st[sec, 1, channel]) * c[sec, 2]
                x += st[sec, 0, channel] * k[sec, 0]
                s = x * -k[sec, 0] + st[sec, 0, channel]
                st[sec, 1, channel] = s
                x_low += s * c[sec, 1]
                st[sec, 0, channel] = x
                x = x * c[sec, 0] + x_low
            return x
        last = len(k) - 1
        x_low = 0
        for i in range(last, -1, -1):
            x += st[i, channel] * k[i]
            s = x * -k[i] + st[i, channel]
            if i != last:
                st[i + 1, channel] = s
            x_low += s * c[i + 1]
        st[0, channel] = x
        return x * c[0] + x_low


# ---- warped filters --------------------------------------------------------------------------------------------------
class WarpedFIR(RealtimeFilter):
    """An FIR filter with first-order all-passes (z^-1 - lambda) / (1 - lambda z^-1) in place of its unit delays
    (Karjalainen, Härmä, Laine, Huopaniemi: Warped filters and their audio applications, 1997).  `filter_signal` runs
    from zero state and leaves `self.buffer`, the state of `process_sample`, as it was."""

    def __init__(self, b, warping_factor: float, sampling_rate_hz: int):
        assert abs(warping_factor) < 1.0, "Warping factor must be in range ]-1;1["
        self.sampling_rate_hz = sampling_rate_hz
        self.b = b
        self.warp = warping_factor
        self.N = len(self.b)
        self.order = len(self.b) - 1
        self.set_n_channels(1)

    @staticmethod
    def from_filter(filt: Filter, warping_factor: float):
        assert filt.is_fir, "This is only valid for a FIR filter"
        b, _ = filt.get_coefficients(FilterCoefficientsType.Ba)
        return WarpedFIR(b, warping_factor, filt.sampling_rate_hz)

    def set_n_channels(self, n_channels: int):
        assert n_channels > 0
        self.buffer = np.zeros((self.N, n_channels))

    def reset_state(self):
        self.buffer.fill(0.0)

    def process_sample(self, x: float, channel: int) -> float:
        buf, lam, b = self.buffer, self.warp, self.b
        output = x * b[0]
        residue = x
        for i in range(self.order):
            new_residue = (buf[i + 1, channel] - residue) * lam + buf[i, channel]
            buf[i, channel] = residue
            residue = new_residue
            if i + 1 < len(b):
                output += new_residue * b[i + 1]
        buf[-1, channel] = residue
        return output

    def _structure(self):
        b = np.asarray(self.b, dtype=np.float64)
        return backend.SFILT_WARPED_FIR, np.concatenate([[float(self.warp)], b]), self.N, 0

    def filter_signal(self, signal: Signal) -> Signal:
        assert self.sampling_rate_hz == signal.sampling_rate_hz, "Sampling rates do not match"
        _refuse_complex(signal, self.b, getattr(self, "a", None))
        return _run(signal, self._structure())[0]


class WarpedIIR(WarpedFIR):
    """The warped IIR filter of the same paper: the feedback through the all-pass chain is made computable by the
    sigma coefficients, computed on the host at construction."""

    def __init__(self, b, a, warping_factor: float, sampling_rate_hz: int):
        assert b.ndim == 1, "Coefficients can only have a single dimension"
        assert a.ndim == 1, "Coefficients can only have a single dimension"
        self.N = max(len(a), len(b))
        self.order = self.N - 1
        self.b = b / a[0]
        self.a = a / a[0]
        self.warp = warping_factor
        self.sampling_rate_hz = sampling_rate_hz
        self.set_n_channels(1)
        self.sigmas = self._compute_sigmas()

    @staticmethod
    def from_filter(filt: Filter, warping_factor: float):
        assert filt.is_iir, "This is only valid for a IIR filter"
        b, a = filt.get_coefficients(FilterCoefficientsType.Ba)
        return WarpedIIR(b, a, warping_factor, filt.sampling_rate_hz)

    def _compute_sigmas(self):
        """Karjalainen et al. 1997: S_N = a_N, S_{i-1} = a_{i-1} - lambda S_i; sigma_i = lambda S_{i-1} + S_i, the last
        one lambda a_N, the first one S_1; kept negated behind sigma_0 = 1 / (1 - lambda S_1) for the sample loop."""
        a, lam = self.a, self.warp
        n = len(a)
        sig = np.zeros(n + 1)
        sig[n] = lam * a[n - 1]
        s = a[n - 1]
        for i in range(n - 1, 1, -1):
            s_new = a[i - 1] - lam * s
            sig[i] = lam * s_new + s
            s = s_new
        sig[1] = s
        sig[0] = 1.0 / (1.0 - lam * s)
        sig[1:] *= -1.0
        return sig

    def process_sample(self, x: float, channel: int) -> float:
        x += self.sigmas[1:] @ self.buffer[:len(self.sigmas) - 1, channel]
        x *= self.sigmas[0]
        return super().process_sample(x, channel)

    def poles(self):
        """The poles in the z plane: the denominator is sum a_i w^i in the all-pass variable w = (1 - lambda z) /
        (z - lambda), so each of its roots w is the pole z = (1 + lambda w) / (w + lambda)."""
        w = np.roots(np.asarray(self.a, dtype=np.float64)[::-1])
        return (1.0 + self.warp * w) / (w + self.warp)

    def _structure(self):
        if not abs(self.warp) < 1.0 or (len(self.a) > 1 and not np.all(np.abs(self.poles()) < 1.0)):
            raise NotImplementedError("a warped IIR filter with a pole on or outside the unit circle is unstable: the "
                                      "time-parallel carry of the device recursion is exact only for a stable one")
        b = np.zeros(self.N)
        b[:len(self.b)] = self.b
        return (backend.SFILT_WARPED_IIR, np.concatenate([[float(self.warp)], b, self.sigmas]), self.N, len(self.a))


# ---- Kautz -----------------------------------------------------------------------------------------------------------
class KautzFilter(RealtimeFilter):
    """A Kautz filter over a set of poles that defines its orthonormal basis, for real signals (B. Bank: Warped, Kautz,
    and Fixed-Pole Parallel Filters: A Review, JAES 2022; the Kautz toolbox of Aalto university).  Complex poles are
    given with a positive imaginary part; their conjugates are implied.

    The cascade of all-pass sections, first the real poles, then the pairs: a real pole p is the direct-form-II value
    w[n] = x[n] + p w[n-1] with the tap sqrt(1 - p^2) w[n] and the all-pass output w[n-1] - p w[n]; a pair (q, r) =
    (-2 Re p, |p|^2) is w[n] = x[n] - q w[n-1] - r w[n-2] with the taps g (w[n] -+ w[n-1]) and the all-pass output
    r w[n] + q w[n-1] + w[n-2].  The tap filters and the all-pass of one pole share that state (the reference runs one
    lfilter for each; the difference is rounding)."""

    def __init__(self, poles, sampling_rate_hz: int):
        assert not np.any(poles.imag < 0.0), "No poles with negative imaginary part should be passed"
        assert not np.any(np.abs(poles) >= 1.0), "No poles should lie outside the unit circle"
        self.sampling_rate_hz = sampling_rate_hz
        self._set_poles(poles)
        self.set_filter_coefficients(np.ones(self.n_real_poles), np.ones(self.n_complex_poles))

    @staticmethod
    def from_ir(ir: ImpulseResponse, order: int, iterations: int):
        """Approximate the IR with an optimal pole basis (Brandenstein / Unbehauen 1998) and its coefficients."""
        f = KautzFilter(np.ones(2) * 0.5, ir.sampling_rate_hz)
        f.fit_poles_and_coefficients_to_ir(ir, order, iterations)
        return f

    def _set_poles(self, poles):
        poles = np.asarray(poles)
        real = poles.imag == 0.0
        self.poles_real = np.real(poles[real])
        self.poles_complex = poles[~real]
        self.n_complex_poles = len(self.poles_complex) * 2
        self.n_real_poles = len(self.poles_real)
        self.total_n_poles = self.n_complex_poles + self.n_real_poles
        p = self.poles_real
        self._q = -2.0 * np.real(self.poles_complex)
        self._r = np.abs(self.poles_complex) ** 2.0
        self._g_real = (1.0 - p ** 2.0) ** 0.5
        self._g_complex = np.stack([((1.0 - self._r) * (1.0 + self._r - self._q) / 2.0) ** 0.5,
                                    ((1.0 - self._r) * (1.0 + self._r + self._q) / 2.0) ** 0.5], axis=1).reshape(-1, 2)
        self.set_n_channels(1)

    def set_filter_coefficients(self, c_real, c_complex):
        """The weights of the taps: c_real per real pole, c_complex per complex pole, adjacent pairs (a + jb, a - jb)."""
        assert self.n_complex_poles == len(c_complex)
        assert self.n_real_poles == len(c_real)
        self.coefficients_real_poles = c_real
        self.coefficients_complex_poles = c_complex
        return self

    def set_n_channels(self, n_channels: int):
        self._state = np.zeros((self.total_n_poles, n_channels))

    def reset_state(self):
        self._state.fill(0.0)

    def process_sample(self, x: float, channel: int):
        st, y = self._state, 0.0
        n_real = self.n_real_poles
        for i, p in enumerate(self.poles_real):
            w1 = st[i, channel]
            w = x + p * w1
            y += self._g_real[i] * w * self.coefficients_real_poles[i]
            x = -p * w + w1
            st[i, channel] = w
        for j in range(len(self.poles_complex)):
            q, r = self._q[j], self._r[j]
            w1, w2 = st[n_real + 2 * j, channel], st[n_real + 2 * j + 1, channel]
            w = x - q * w1 - r * w2
            y += (self._g_complex[j, 0] * (w - w1) * self.coefficients_complex_poles[2 * j]
                  + self._g_complex[j, 1] * (w + w1) * self.coefficients_complex_poles[2 * j + 1])
            x = r * w + q * w1 + w2
            st[n_real + 2 * j + 1, channel] = w1
            st[n_real + 2 * j, channel] = w
        return y

    def _structure(self, c_real, c_complex):
        c_real = np.asarray(c_real, dtype=np.float64)
        c_complex = np.asarray(c_complex, dtype=np.float64).reshape(-1, 2)
        real = np.stack([self.poles_real, self._g_real, c_real], axis=1)
        pairs = np.concatenate([self._q[:, None], self._r[:, None], self._g_complex, c_complex], axis=1)
        return backend.SFILT_KAUTZ, np.concatenate([real.ravel(), pairs.ravel()]), self.total_n_poles, self.n_real_poles

    def fit_coefficients_to_ir(self, ir: ImpulseResponse):
        """The least-squares weights for a single-channel impulse response: the taps at the last sample of the
        time-reversed IR.  One device run: every tap is a combination of the final state."""
        assert ir.number_of_channels == 1, "Only a single-channel IR is supported"
        _refuse_complex(ir)
        ones = np.ones(self.n_real_poles), np.ones(self.n_complex_poles)
        self.set_filter_coefficients(*ones)
        reversed_ir = ImpulseResponse(None, ir.time_data[::-1].copy(), ir.sampling_rate_hz, constrain_amplitude=False)
        _, zf = _run(reversed_ir, self._structure(*ones), want_zf=True)
        n_real = self.n_real_poles
        w, w1 = zf[n_real::2, 0], zf[n_real + 1::2, 0]
        taps = np.stack([self._g_complex[:, 0] * (w - w1), self._g_complex[:, 1] * (w + w1)], axis=1)
        self.set_filter_coefficients(self._g_real * zf[:n_real, 0], taps.ravel())
        self.sampling_rate_hz = ir.sampling_rate_hz
        return self

    def filter_signal(self, signal: Signal) -> Signal:
        assert signal.sampling_rate_hz == self.sampling_rate_hz, "Sampling rates do not match"
        _refuse_complex(signal, self.coefficients_real_poles, self.coefficients_complex_poles)
        return _run(signal, self._structure(self.coefficients_real_poles, self.coefficients_complex_poles))[0]

    def get_ir(self, length_samples: int) -> ImpulseResponse:
        d = np.zeros((length_samples, 1))
        d[0] = 1.0
        return self.filter_signal(ImpulseResponse(None, d, self.sampling_rate_hz))

    def fit_poles_and_coefficients_to_ir(self, ir: ImpulseResponse, order: int, iterations: int):
        """Poles by the iteration of Brandenstein and Unbehauen (Least-squares approximation of FIR by IIR filters,
        IEEE Trans. SP 46, 1998), as the Kautz toolbox runs it, then the weights.  The pole search is design code:
        its intermediate denominators may be unstable, and it stays scipy on the host; the weights' fit runs on the
        device."""
        assert ir.number_of_channels == 1, "Only a single-channel IR is supported"
        self._set_poles(_optimal_poles(order, iterations, ir.time_data.squeeze().copy()))
        self.fit_coefficients_to_ir(ir)
        return self


def _optimal_poles(order: int, iterations: int, target):
    """Each pass filters the time-reversed target by 1 / D_i, solves the linear least-squares problem for the next
    denominator D_{i+1} and records the energy left after the all-pass z^-order D(1/z) / D(z); the denominator of the
    smallest energy gives the poles (those with non-negative imaginary part are returned)."""
    from scipy.linalg import lstsq
    from scipy.signal import lfilter
    assert target.ndim == 1, "This is only valid for 1D time series"
    n = len(target)
    target = target[::-1]
    den = np.zeros(order + 1)
    den[0] = 1.0
    tried = np.zeros((iterations, order + 1))
    energy = np.zeros(iterations)
    for it in range(iterations):
        v = lfilter([1.0], den, target)
        rhs = np.concatenate([np.zeros(order), -v[:n - order]])
        cols = np.zeros((n, order))
        for j in range(order):
            cols[j:, j] = v[:n - j]
        den = np.concatenate([[1.0], lstsq(cols, rhs)[0][::-1]])
        tried[it] = den
        energy[it] = np.sum(lfilter(den[::-1], den, target) ** 2)
    ok = ~np.isnan(energy)
    poles = np.roots(tried[ok][np.argmin(energy[ok])])
    return poles[poles.imag >= 0.0]
