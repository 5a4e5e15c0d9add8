"""Host shim: the reference's private numeric backends, same
names and argument meaning, executed by the HIP library through ctypes.

    _welch        <- dsptoolbox/standard/_spectral_methods.py:10-173
    _stft         <- dsptoolbox/standard/_spectral_methods.py:176-282
    _csm_welch    <- dsptoolbox/standard/_spectral_methods.py:285-371
    _lfilter_fir  <- dsptoolbox/classes/filter_helpers.py:454-503
    welch_transfer_function  <- the per-channel _welch loop of
                     transfer_functions/transfer_functions.py:476-534, fused
    rfft_spectrum <- scipy.fft.rfft call of classes/signal.py:899-911
    spectral_division <- transfer_functions/_transfer_functions.py:19-42

Arrays cross the boundary as (samples, channels) float64 like in the reference; the shim transposes to planar fp32,
the device computes in fp32/complex64 (finish() in fp64) and results are cast back to float64/complex128.  Anything
the device path does not implement raises NotImplementedError -- nothing is silently computed on the CPU.

A call builds ONE plan from its parameters and the shape of its samples (_WelchPlan by _welch_plan, _StftPlan by
_stft_plan: checks, window, framing, and `tail()`, the one place an entry family's argument order is written), asks
ONE route (_welch_route for a Welch estimate, _host_route for every other host function), casts by that route
(_host_input) and makes one call; device buffers of a call live in a device_scope.
"""

from __future__ import annotations

import ctypes as C
import math
import os
from contextlib import contextmanager
from typing import NamedTuple
from warnings import warn

import numpy as np
from scipy.signal import check_COLA
from scipy.signal.windows import get_window

from ._lib import DeviceBuffer, DevicePlanar, get_context, load_library
from .standard.enums import SpectrumScaling, Window

DS_TF = {"H1": 1, "H2": 2, "H3": 3}
DS_AVG = {"mean": 0, "median": 1}
DS_FB_PARALLEL, DS_FB_SEQUENTIAL, DS_FB_SUMMED = 1, 2, 3


def _planar_f32(x: np.ndarray) -> np.ndarray:
    """(N, C) float64 -> (C, N) float32 C-contiguous.  Large C-order float64 arrays go through the
    library's threaded cast + transpose (numpy's strided cast takes 0.2 s for the 537 MB of the
    headline shape); everything else through numpy."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim == 2 and x.dtype == np.float64 and x.flags.c_contiguous and x.size >= (1 << 20):
        lib = load_library()
        out = np.empty((x.shape[1], x.shape[0]), dtype=np.float32)
        if lib.ds_host_planar_f32(_ptr(x), x.shape[0], x.shape[1], _ptr(out), x.shape[0], 0) == 0:
            return out
    return np.ascontiguousarray(x.T, dtype=np.float32)


def _interleaved_f64(planar: np.ndarray, dst: np.ndarray | None = None) -> np.ndarray:
    """(C, N) float32 C-contiguous -> (N, C) float64 (the reverse of _planar_f32), into dst if given."""
    n_ch, n = planar.shape
    if dst is None:
        dst = np.empty((n, n_ch), dtype=np.float64)
    if planar.dtype == np.float32 and planar.flags.c_contiguous and dst.flags.c_contiguous \
            and planar.size >= (1 << 20):
        if load_library().ds_host_interleave_f64(_ptr(planar), n, n_ch, n, _ptr(dst), 0) == 0:
            return dst
    dst[...] = planar.T
    return dst


def _widen(a: np.ndarray) -> np.ndarray:
    """float32 -> float64 / complex64 -> complex128 of a C-contiguous array (threaded for large ones)."""
    wide = np.complex128 if a.dtype == np.complex64 else np.float64
    if a.dtype in (np.float32, np.complex64) and a.flags.c_contiguous and a.size >= (1 << 14):
        out = np.empty(a.shape, dtype=wide)
        n = a.size * (2 if a.dtype == np.complex64 else 1)
        # (mid-size arrays -- the spectra of a device-resident estimate -- in the calling thread: numpy's astype
        # takes 80 us for 2049 x 64 complex values, this loop 25)
        if load_library().ds_host_widen_f64(_ptr(a), n, _ptr(out), 0 if a.size >= (1 << 20) else 1) == 0:
            return out
    return a.astype(wide)


def _fusable(a) -> bool:
    """Large (N, C) float64 C-order array: crosses the boundary as it is (the *_f64 entry points cast
    + transpose it in host threads straight into pinned upload chunks)."""
    return isinstance(a, np.ndarray) and a.ndim == 2 and a.dtype == np.float64 and a.flags.c_contiguous \
        and a.size >= (1 << 20)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


_WINDOWS: dict = {}


def _window_array(window_type, length: int) -> np.ndarray:
    """scipy.signal.get_window(spec, length, fftbins=True), computed once per (spec, length): the array is handed out
    read-only (55 us for 4096 Hann samples is a quarter of a device-resident transfer-function call)."""
    spec = window_type.to_scipy_format() if isinstance(window_type, Window) else window_type
    try:
        key = (spec if not isinstance(spec, list) else tuple(spec), int(length))
        hash(key)
    except TypeError:
        return get_window(spec, length, fftbins=True)
    w = _WINDOWS.get(key)
    if w is None:
        if len(_WINDOWS) >= 64:
            _WINDOWS.pop(next(iter(_WINDOWS)))
        w = _WINDOWS[key] = np.array(get_window(spec, length, fftbins=True))  # (scipy hands out a view: own the data)
        w.setflags(write=False)
    return w


def _finish_params(scaling: SpectrumScaling, W: int, fs_hz: int, window: np.ndarray):
    """(amp_sqrt, norm_scale, factor, halve_edges) of _welch's tail (:141-171)."""
    norm = scaling.fft_norm()
    norm_scale = 1.0 if norm == "backward" else (1.0 / W**2 if norm == "forward" else 1.0 / W)
    phys = scaling.has_physical_units()
    factor = float(np.asarray(scaling.get_scaling_factor(W, fs_hz, window)).ravel()[0]) if phys else 1.0
    return int(scaling.is_amplitude_scaling()), float(norm_scale), factor, int(phys)


def _welch_checks(window_length_samples, overlap_percent, average):
    assert window_length_samples in [2**k for k in range(3, 19)], (
        "Window length should be a power of 2 between [8, 262_144] or [2**3, 2**18]")
    assert overlap_percent >= 0 and overlap_percent < 100, \
        "overlap_percent should be between 0 and 100"
    assert average in ("mean", "median"), f"{average} is not valid. Use either mean or median"


_COLA: dict = {}


def _window_key(window: np.ndarray):
    """Identity of one of _window_array's read-only arrays (they live as long as the cache), content hash otherwise."""
    if not window.flags.writeable and window.base is None:
        return ("id", id(window), window.size)
    return ("bytes", window.size, hash(np.ascontiguousarray(window).tobytes()))


def _cola_ok(window: np.ndarray, overlap: int) -> bool:
    """scipy.signal.check_COLA, remembered per (window, overlap)."""
    key = (int(overlap), _window_key(window))
    ok = _COLA.get(key)
    if ok is None:
        if len(_COLA) >= 256:
            _COLA.clear()
        ok = _COLA[key] = bool(check_COLA(window, nperseg=len(window), noverlap=overlap))
    return ok


def _welch_framing(n_samples: int, W: int, overlap_percent: float, window: np.ndarray):
    overlap = int(overlap_percent / 100 * W)  # truncation, _spectral_methods.py:106
    hop = W - overlap
    if not _cola_ok(window, overlap):
        warn("Selected window type and overlap do not meet the constant "
             "overlap and add constraint! Results might be distorted")
    n_frames = int(np.ceil(n_samples / hop))  # helpers/other.py:206
    return hop, n_frames


class _WelchPlan(NamedTuple):
    """Everything a Welch call derives from its parameters before it looks at the samples' layout: built once per call by
    _welch_plan, handed to _welch_route and to the one call the function makes."""
    W: int
    B: int            # W // 2 + 1 bins
    hop: int
    n_frames: int
    window: np.ndarray  # float64, read-only (one of _window_array's)
    detrend: int      # detrend and avg as the ints the C entries take
    avg: int
    average: str      # "mean" / "median": what the precision rules ask
    amp: int          # _finish_params
    norm_scale: float
    factor: float
    phys: int

    def window_for(self, route: str) -> np.ndarray:
        """The window in the precision of the route's kernels."""
        return np.ascontiguousarray(self.window, dtype=np.float64) if route == ROUTE_X64 else self.window.astype(np.float32)

    def tail(self, window_ptr, mode: str | None = None, with_avg: bool = True) -> tuple:
        """The arguments every Welch entry ends with, after its inputs and before its outputs: W, hop, n_frames, window,
        detrend, avg, [transfer-function mode], amp, norm_scale, factor, phys.  THE place where their order is written
        (ds_csm_bins_dev averages by the mean only and takes no avg)."""
        return ((self.W, self.hop, self.n_frames, window_ptr, self.detrend) + ((self.avg,) if with_avg else ())
                + (() if mode is None else (DS_TF[mode],)) + (self.amp, self.norm_scale, self.factor, self.phys))


def _welch_plan(n_samples: int, fs_hz: int, window_type, window_length_samples: int, overlap_percent: float, detrend: bool,
                average: str, scaling: SpectrumScaling) -> _WelchPlan:
    """The reference's assertions (window length, then overlap, then average), the cached window, the framing (with its
    COLA warning) and the finish parameters."""
    _welch_checks(window_length_samples, overlap_percent, average)
    W = int(window_length_samples)
    window = _window_array(window_type, W)
    hop, n_frames = _welch_framing(n_samples, W, overlap_percent, window)
    return _WelchPlan(W, W // 2 + 1, hop, n_frames, window, int(bool(detrend)), DS_AVG[average], average,
                      *_finish_params(scaling, W, fs_hz, window))


# Arithmetic of the transfer-function estimate behind the reference-shaped API
# (transfer_functions.compute_transfer_function): "auto" takes the float64 route
# (ds_welch_tf_x64: float64 transforms, sums and finish, the reference's own precision) when the
# problem is small -- frame spectra of all channels <= 64 MB, window <= 262144 (median averaging: at
# most 4096 frames) -- or when it is SHORT: fewer than 128 frames (and <= 1.25 GB of frame spectra), where
# an fp32 estimate has too few frames to average its transform rounding down (the two sweep cases of
# round 2 that reached 1.1e-6 / 1.8e-6 in the coherence had 98 and 110 frames of 8192 samples: they are
# tests now) --
# and the fp32 kernels otherwise; "f32" / "f64" force one.  Environment:
# DSPTOOLBOX_AMD_TF_PRECISION.  backend.welch_transfer_function itself defaults to "f32".
TF_PRECISION = os.environ.get("DSPTOOLBOX_AMD_TF_PRECISION", "auto")
_X64_AUTO_BYTES = 64 << 20
_X64_MAX_WINDOW = 262144  # (16384 until round 4: k_frames_cls / k_split of kernels_welch_f64.hpp carry it to the reference's limit)
_X64_SHORT_BYTES = 1280 << 20  # frame spectra of a short estimate (transfer functions, auto / cross spectra): see _short_bytes
_X64_MATRIX_BYTES = 256 << 20  # ... of a short cross-spectral matrix (float64 pair sums grow with channels^2), and of the matrix itself


# The same for the Welch spectra themselves (get_spectrum with the Welch method: ds_welch_psd / ds_welch_csd) and
# the cross-spectral matrix (get_csm: ds_csm): "auto" sends SHORT estimates -- fewer than 128 frames, frame
# spectra <= 1.25 GB, window <= 262144; the matrix: up to 1024 channels, <= 256 MB of frame spectra and of matrices -- through
# ds_welch_spec_x64 / ds_csm_x64; "f32" keeps the fp32 kernels for every shape.  Environment:
# DSPTOOLBOX_AMD_SPEC_PRECISION.  (tests/sweeps/edge_welch.py, round 4: fp32 cross spectra and matrices of
# one to five frames reach 2-3e-6 of the largest element under the amplitude scalings.)
SPEC_PRECISION = os.environ.get("DSPTOOLBOX_AMD_SPEC_PRECISION", "auto")


def _short_bytes(W: int) -> int:
    """Byte cap of a short estimate's frame spectra on the float64 route: 1.25 GB for every window (at 50 % overlap the frame
    spectra of a signal are 16 bytes per sample whatever the window, so this is 64 + 1 channels x 2^20 samples).  It was 256 MB up
    to 16384-sample windows until round 5 (the float64 KERNELS are 5-8 x slower than the fp32 ones: 3.5 against 0.4 ms at
    1 GB); measured end to end through this host API with the reference's float64 arrays (tools/x64_cap_time.py,
    profiles/r05_sweeps.txt) the float64 route costs the same or less -- 13.4 against 12.6 ms at 1 GB of 8192-sample frames, 8.8
    against 22.6 ms and 3.7 against 6.2 ms at 0.5 / 0.3 GB of 16384-sample frames: the arrays cross PCIe as they are instead of
    through a host cast -- and the estimates of 45 ... 61 frames of 8192 / 16384 samples that the randomized sweeps found at
    1.0-1.7e-6 in the coherence on the fp32 kernels (20 + 20 and 33 + 33 channels: 320-530 MB) now take it."""
    return _X64_SHORT_BYTES


def _x64_short(precision, n_spectra: int, n_frames: int, W: int, average: str, cap: int | None = None) -> bool:
    """Does a SHORT estimate of `n_spectra` channel spectra take the float64 route?"""
    assert precision in ("auto", "f32"), "DSPTOOLBOX_AMD_SPEC_PRECISION: 'auto' or 'f32'"
    if precision != "auto" or W > _X64_MAX_WINDOW or n_frames >= 128:
        return False
    if average != "mean" and n_frames > 4096:
        return False
    return n_spectra * n_frames * (W // 2 + 1) * 16 <= (_short_bytes(W) if cap is None else cap)


def _tf_x64_applies(precision, n_cx: int, n_cy: int, n_frames: int, W: int, average: str) -> bool:
    ok = W <= _X64_MAX_WINDOW and (average == "mean" or n_frames <= 4096)
    if precision == "f64":
        if not ok:
            raise NotImplementedError("the float64 route covers windows up to 262144 (median: up to 4096 frames)")
        return True
    if precision == "auto":
        nbytes = (n_cx + n_cy) * n_frames * (W // 2 + 1) * 16
        return ok and (nbytes <= _X64_AUTO_BYTES or (n_frames < 128 and nbytes <= _short_bytes(W)))
    assert precision in (None, "f32"), "precision: 'f32', 'f64' or 'auto'"
    return False


ROUTE_X64, ROUTE_FUSED, ROUTE_PLANAR, ROUTE_RESIDENT = "x64", "fused", "planar", "resident"


def _welch_route(plan: _WelchPlan, kind: str, channels, holds: str = "host", precision: str | None = None) -> str:
    """Transport and precision of one Welch call -- THE place that chooses between
        ROUTE_X64       float64 kernels fed from host float64 arrays (a caller with resident samples hands in its host copy),
        ROUTE_FUSED     fp32 kernels, the caller's large float64 array cast + transposed by the library on its way up,
        ROUTE_PLANAR    fp32 kernels, planar float32 made here and uploaded,
        ROUTE_RESIDENT  fp32 kernels over samples that are in HBM already.
    kind: "spectra" (channels = spectra estimated: C auto, 2 C cross), "tf" (channels = (inputs, outputs); precision as
    welch_transfer_function's) or "matrix" (channels = C).  holds: "host", "fusable" (every array _fusable) or "resident".
    SPEC_PRECISION is read here, at call time."""
    if kind == "tf":
        x64 = _tf_x64_applies(precision, channels[0], channels[1], plan.n_frames, plan.W, plan.average)
    elif kind == "matrix":
        x64 = (channels <= 1024 and _x64_short(SPEC_PRECISION, channels, plan.n_frames, plan.W, plan.average, cap=_X64_MATRIX_BYTES)
               and plan.B * channels * channels * 16 <= _X64_MATRIX_BYTES)  # (the matrix itself, complex128, crosses PCIe too)
    else:
        x64 = _x64_short(SPEC_PRECISION, channels, plan.n_frames, plan.W, plan.average)
    if x64:
        return ROUTE_X64
    return ROUTE_RESIDENT if holds == "resident" else ROUTE_FUSED if holds == "fusable" else ROUTE_PLANAR


def _host_route(a, fuses: bool = True) -> str:
    """Transport of a host function that is no Welch estimate (STFT, rFFT, deconvolution, FIR) -- THE place that chooses
    between ROUTE_FUSED (the `*_f64` entry: float64 on both sides through the pinned chunk pipelines) and ROUTE_PLANAR (planar
    float32 made here, the result widened here).  fuses: the function's own condition beside the array being _fusable."""
    return ROUTE_FUSED if fuses and _fusable(a) else ROUTE_PLANAR


def _host_input(a, route: str) -> np.ndarray:
    """A flat or (N, C) array as the host entries of `route` read it: float64 for the float64 kernels, as it is for the
    fused transport, planar (C, N) float32 otherwise."""
    if route == ROUTE_X64:
        return np.ascontiguousarray(a, dtype=np.float64)
    return a if route == ROUTE_FUSED else _planar_f32(a)


def _samples_shape(x) -> tuple:
    """(samples, channels) of a flat or (N, C) array or of a DevicePlanar."""
    if isinstance(x, DevicePlanar):
        return x.n_samples, x.n_ch
    n, n_ch = x.shape if x.ndim != 1 else (x.shape[0], 1)
    return n, n_ch


class _DeviceScope:
    """Device buffers of one call (see device_scope)."""
    __slots__ = ("ctx", "_temps", "_results")

    def __init__(self, ctx):
        self.ctx, self._temps, self._results = ctx, [], []

    def alloc(self, nbytes: int, result: bool = False) -> DeviceBuffer:
        """A buffer of the call; result=True: the one that leaves with what the call returns."""
        buf = DeviceBuffer(self.ctx, nbytes)
        (self._results if result else self._temps).append(buf)
        return buf

    def upload(self, arr: np.ndarray) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        buf = self.alloc(arr.nbytes)
        self.ctx.upload(buf.ptr, arr)
        return buf


@contextmanager
def device_scope(ctx):
    """with device_scope(ctx) as dev: the temporaries of dev.alloc / dev.upload are freed on the way out, a result buffer
    (alloc(..., result=True)) survives a clean exit and is freed when the body raises.  Context-owned or borrowed memory
    (_window_dev, _result_scratch, a DevicePlanar) is simply not registered.  A kernel that may still read a temporary
    when the body ends needs its ctx.sync() inside the body."""
    dev = _DeviceScope(ctx)
    try:
        yield dev
    except BaseException:
        for buf in dev._results:
            buf.free()
        raise
    finally:
        for buf in dev._temps:
            buf.free()


def _welch(x, y, fs_hz: int, window_type, window_length_samples: int, overlap_percent: float,
           detrend: bool, average: str, scaling: SpectrumScaling):
    """Welch auto (y None) or cross spectrum; shapes as in the reference."""
    auto = y is None
    x = np.asarray(x).squeeze()
    if not auto:
        y = np.asarray(y).squeeze()
        assert x.shape == y.shape, "Shapes of data do not match"
    assert x.ndim <= 2, f"{x.shape} are too many dimensions. Use flat arrays or 2D-Arrays instead"
    return _spectra_host(_welch_plan(x.shape[0], fs_hz, window_type, window_length_samples, overlap_percent, detrend, average,
                                     scaling), x, y)


def _spectra_host(plan: _WelchPlan, x: np.ndarray, y: np.ndarray | None):
    """The host routes of the auto (y None) or cross spectra of flat or (N, C) arrays, for a plan of their length."""
    auto = y is None
    multi = x.ndim == 2
    n, n_ch = x.shape[0], (x.shape[1] if multi else 1)
    # a short estimate takes the reference's own float64 arithmetic on the device (ds_welch_spec_x64)
    route = _welch_route(plan, "spectra", (1 if auto else 2) * n_ch,
                         "fusable" if _fusable(x) and (auto or _fusable(y)) else "host")
    arrays = [_host_input(a.reshape(n, n_ch), route) for a in ((x,) if auto else (x, y))]
    inputs = [_ptr(a) for a in arrays]
    w = plan.window_for(route)
    ctx = get_context()
    if route == ROUTE_X64:
        out = np.empty((plan.B, n_ch), dtype=np.complex128)
        ctx.check(ctx.lib.ds_welch_spec_x64(ctx.handle, inputs[0], None if auto else inputs[1], n_ch, n, *plan.tail(_ptr(w)),
                                            _ptr(out)), "ds_welch_spec_x64")
        res = out if (not auto or plan.avg) else np.ascontiguousarray(out.real)
    else:
        name = ("ds_welch_psd" if auto else "ds_welch_csd") + ("_f64" if route == ROUTE_FUSED else "")
        out = np.empty((plan.B, n_ch), dtype=np.float32 if auto else np.complex64)
        ctx.check(getattr(ctx.lib, name)(ctx.handle, *inputs, n_ch, n, *plan.tail(_ptr(w)), _ptr(out)), name)
        # median averaging makes the reference's autospectrum complex128 (median_re + 1j*median_im)
        res = out.astype(np.complex128 if plan.avg else np.float64) if auto else _widen(out)
    return res if multi else res[:, 0]


_TF_ENTRY = {ROUTE_X64: "ds_welch_tf_x64", ROUTE_FUSED: "ds_welch_tf_f64", ROUTE_PLANAR: "ds_welch_tf"}


def welch_transfer_function(output_td, input_td, fs_hz: int, window_length_samples: int, mode: str,
                            window_type=Window.Hann, overlap_percent: float = 50.0,
                            detrend: bool = True, average: str = "mean",
                            scaling: SpectrumScaling = SpectrumScaling.FFTBackward,
                            precision: str | None = None):
    """H1/H2/H3 + coherence for every output channel in one device call.
    output_td (N, Cy); input_td (N, 1) or (N, Cy).  -> (tf complex128 (B, Cy),
    coherence float64 (B, Cy)).  precision: "f32" (default), "f64" or "auto" (see TF_PRECISION)."""
    yo, xi = np.asarray(output_td), np.asarray(input_td)
    if yo.ndim == 1:
        yo = yo[:, None]
    if xi.ndim == 1:
        xi = xi[:, None]
    return _tf_host(_welch_plan(yo.shape[0], fs_hz, window_type, window_length_samples, overlap_percent, detrend, average,
                                scaling), yo, xi, mode, precision)


def _tf_host(plan: _WelchPlan, yo: np.ndarray, xi: np.ndarray, mode: str, precision: str | None):
    """The host routes of the transfer function of (N, Cy) outputs and (N, Cx) inputs, for a plan of N samples."""
    n, n_cy, n_cx = yo.shape[0], yo.shape[1], xi.shape[1]
    if mode not in DS_TF:
        raise ValueError("Unsupported transfer function type")
    assert xi.shape[0] == n, "Signal lengths do not match"
    # large float64 C-order arrays (the reference's own layout) cross the boundary as they are: the
    # library casts + transposes them in threads straight into pinned upload chunks
    fused = _fusable(yo) and xi.ndim == 2 and xi.dtype == np.float64 and xi.flags.c_contiguous
    route = _welch_route(plan, "tf", (n_cx, n_cy), "fusable" if fused else "host", precision)
    x_in, y_in, w = _host_input(xi, route), _host_input(yo, route), plan.window_for(route)
    x64 = route == ROUTE_X64
    tf = np.empty((plan.B, n_cy), dtype=np.complex128 if x64 else np.complex64)
    coh = np.empty((plan.B, n_cy), dtype=np.float64 if x64 else np.float32)
    ctx = get_context()
    ctx.check(getattr(ctx.lib, _TF_ENTRY[route])(ctx.handle, _ptr(x_in), n_cx, _ptr(y_in), n_cy, n, *plan.tail(_ptr(w), mode),
                                                 _ptr(tf), _ptr(coh)), _TF_ENTRY[route])
    return (tf, coh) if x64 else (tf.astype(np.complex128), coh.astype(np.float64))


# ---- the same calls over samples that are ALREADY in HBM (Signal.to_device / from_planar_f32) -------------------------
# No cast, no transpose, no upload of the signal; small results come down through the context's page-locked staging
# buffer, results that are signals stay on the device (DevicePlanar).  Windows and taps are a few KB: uploaded per call.
# The window and the result scratch below belong to the context: a call borrows them and frees nothing.
def _window_dev(ctx, window: np.ndarray) -> DeviceBuffer:
    """The float32 window on the device, kept per context (a handful of KB each, keyed by content): a resident call
    neither allocates nor uploads one (hipMalloc + hipFree cost more than the 0.12 ms of kernels they surround)."""
    cache = ctx.__dict__.setdefault("_window_cache", {})
    key = _window_key(window)
    hit = cache.get(key)
    if hit is None:
        if len(cache) >= 32:
            cache.pop(next(iter(cache)))[0].free()
        # (the window object rides along: an id is only a key while its object lives)
        hit = cache[key] = (DeviceBuffer.from_array(ctx, np.ascontiguousarray(window, dtype=np.float32)), window)
    return hit[0]


def _result_scratch(ctx, nbytes: int) -> DeviceBuffer:
    """Context-owned device buffer for SMALL results that are downloaded before the call returns (transfer functions,
    spectra): reused by every call of the thread, grown when needed."""
    cur = ctx.__dict__.get("_result_scratch")
    if cur is None or cur.nbytes < nbytes:
        if cur is not None:
            cur.free()
        cur = ctx.__dict__["_result_scratch"] = DeviceBuffer(ctx, max(int(nbytes), 1 << 22))
    return cur


def _tf_resident(plan: _WelchPlan, y_dev: DevicePlanar, x_dev: DevicePlanar, mode: str, narrow: bool):
    """ROUTE_RESIDENT of the transfer function (ds_welch_tf_dev) for a plan of y_dev.n_samples samples."""
    if mode not in DS_TF:
        raise ValueError("Unsupported transfer function type")
    n, n_cy = y_dev.n_samples, y_dev.n_ch
    assert x_dev.n_samples == n, "Signal lengths do not match"
    ctx = y_dev.ctx
    n_tf = plan.B * n_cy * 8
    d_w, d_res = _window_dev(ctx, plan.window), _result_scratch(ctx, n_tf + n_tf // 2)
    ctx.check(ctx.lib.ds_welch_tf_dev(ctx.handle, C.c_void_p(x_dev.ptr), x_dev.n_ch, x_dev.ld, C.c_void_p(y_dev.ptr), n_cy,
                                      y_dev.ld, n, *plan.tail(C.c_void_p(d_w.ptr), mode), C.c_void_p(d_res.ptr),
                                      C.c_void_p(d_res.ptr + n_tf)), "ds_welch_tf_dev")
    raw = ctx.download_result(d_res.ptr, (n_tf + n_tf // 2,), np.uint8)
    tf = raw[:n_tf].view(np.complex64).reshape(plan.B, n_cy)
    coh = raw[n_tf:].view(np.float32).reshape(plan.B, n_cy)
    return (tf, coh) if narrow else (_widen(tf), _widen(coh))


def welch_transfer_function_device(y_dev: DevicePlanar, x_dev: DevicePlanar, fs_hz: int, window_length_samples: int,
                                   mode: str, window_type=Window.Hann, overlap_percent: float = 50.0,
                                   detrend: bool = True, average: str = "mean",
                                   scaling: SpectrumScaling = SpectrumScaling.FFTBackward, narrow: bool = False):
    """welch_transfer_function on device-resident planar float32 samples (fp32 kernels, ds_welch_tf_dev): the resident
    route whatever _welch_route would say -- a caller that wants the precision rule asks it first, as
    compute_transfer_function does.
    -> (tf complex128 (B, Cy), coherence float64 (B, Cy)); narrow=True: the complex64 / float32 arrays as they came
    off the device (page-locked, owned by the caller) -- what Spectrum widens on first access."""
    plan = _welch_plan(y_dev.n_samples, fs_hz, window_type, window_length_samples, overlap_percent, detrend, average, scaling)
    return _tf_resident(plan, y_dev, x_dev, mode, narrow)


def _psd_resident(plan: _WelchPlan, x_dev: DevicePlanar):
    """ROUTE_RESIDENT of the auto spectra (ds_welch_psd_dev) for a plan of x_dev.n_samples samples."""
    ctx = x_dev.ctx
    d_w, d_o = _window_dev(ctx, plan.window), _result_scratch(ctx, plan.B * x_dev.n_ch * 4)
    ctx.check(ctx.lib.ds_welch_psd_dev(ctx.handle, C.c_void_p(x_dev.ptr), x_dev.n_ch, x_dev.ld, x_dev.n_samples,
                                       *plan.tail(C.c_void_p(d_w.ptr)), C.c_void_p(d_o.ptr)), "ds_welch_psd_dev")
    out = ctx.download_staged(d_o.ptr, (plan.B, x_dev.n_ch), np.float32)
    return out.astype(np.complex128 if plan.avg else np.float64)


def _welch_psd_device(x_dev: DevicePlanar, fs_hz: int, window_type, window_length_samples: int, overlap_percent: float,
                      detrend: bool, average: str, scaling: SpectrumScaling):
    """Welch auto spectra of every channel of a device-resident signal (ds_welch_psd_dev) -> (B, C) as _welch.  The
    resident route whatever _welch_route would say (Signal.get_spectrum asks it first)."""
    return _psd_resident(_welch_plan(x_dev.n_samples, fs_hz, window_type, window_length_samples, overlap_percent, detrend,
                                     average, scaling), x_dev)


class DeviceSTFT:
    """A spectrogram that stays in HBM: (bins, frames, channels) complex64 in `buf` -- the layout ds_stft_r2c writes,
    ds_istft and ds_band_power read.  What `Signal.get_spectrogram(on_device=True)` returns in place of the array;
    `to_host()` gives the reference's complex128 array."""

    def __init__(self, buf: DeviceBuffer, shape, power: bool):
        self.buf, self.shape, self.power = buf, tuple(int(v) for v in shape), bool(power)

    def to_host(self) -> np.ndarray:
        n = int(np.prod(self.shape))
        if self.power or n < (1 << 20):
            out = self.buf.to_array(self.shape, np.complex64)
            return out.real.astype(np.float64) if self.power else _widen(out)
        # a large spectrogram: page-locked chunks (the link's rate), each widened by the host threads while it is hot
        ctx, lib = self.buf.ctx, load_library()
        res = np.empty(self.shape, dtype=np.complex128)
        flat = res.reshape(-1)
        chunk = 4 << 20  # complex values: 32 MB down, 64 MB out
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            part = ctx.download_staged(self.buf.ptr + 8 * i0, (m,), np.complex64)
            if lib.ds_host_widen_f64(_ptr(part), 2 * m, C.c_void_p(flat.ctypes.data + 16 * i0), 0) != 0:
                flat[i0:i0 + m] = part
        return res

    def __deepcopy__(self, memo):
        return self


def _stft_device(x_dev: DevicePlanar, fs_hz: int, window_length_samples: int, window_type, overlap_percent: float,
                 fft_length_samples, detrend: bool, padding: bool, scaling: SpectrumScaling, keep_on_device: bool):
    """_stft of a device-resident signal -> (time_s, freqs_hz, stft): stft the (B', F, C) complex128 array, or a
    DeviceSTFT when keep_on_device."""
    plan = _stft_plan(x_dev.n_samples, x_dev.n_ch, fs_hz, window_length_samples, window_type, overlap_percent,
                      fft_length_samples, detrend, padding, scaling)
    ctx = x_dev.ctx
    d_w = _window_dev(ctx, plan.window32)
    with device_scope(ctx) as dev:
        d_s = dev.alloc(int(np.prod(plan.shape)) * 8, result=keep_on_device)
        ctx.check(ctx.lib.ds_stft_r2c_dev(ctx.handle, C.c_void_p(x_dev.ptr), *plan.tail(C.c_void_p(d_w.ptr), x_dev.ld),
                                          C.c_void_p(d_s.ptr)), "ds_stft_r2c_dev")
        stft = DeviceSTFT(d_s, plan.shape, plan.power)
        if keep_on_device:
            ctx.sync()
        else:
            stft = stft.to_host()
    return plan.time_s, plan.freqs_hz, stft


def _bank_outputs(d_y: DeviceBuffer, n_ch: int, n: int, n_out: int, mode: int):
    """The n_out outputs of a device filter bank, slices of its ONE band-major buffer: the list of them for a Parallel
    bank, the single one otherwise."""
    outs = [DevicePlanar(d_y, n_ch, n, n, 4 * i * n_ch * n) for i in range(n_out)]
    return outs if mode == DS_FB_PARALLEL else outs[0]


def fir_filter_bank_device(x_dev: DevicePlanar, taps_list, mode: int):
    """fir_filter_bank over device-resident samples (ds_fir_ola_dev): Parallel -> a list of K DevicePlanar (slices of ONE
    output buffer, band-major as the kernel writes it), Sequential / Summed -> one DevicePlanar.  Nothing comes down."""
    taps = np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.float64) for t in taps_list]), dtype=np.float32)
    k, t = taps.shape
    ctx = x_dev.ctx
    n, n_ch = x_dev.n_samples, x_dev.n_ch
    n_out = k if mode == DS_FB_PARALLEL else 1
    with device_scope(ctx) as dev:
        d_t = dev.upload(taps)
        d_y = dev.alloc(n_out * n_ch * n * 4, result=True)
        ctx.check(ctx.lib.ds_fir_ola_dev(ctx.handle, C.c_void_p(x_dev.ptr), n_ch, x_dev.ld, n, C.c_void_p(d_t.ptr), k, t,
                                         int(mode), C.c_void_p(d_y.ptr), n), "ds_fir_ola_dev")
        ctx.sync()  # (the taps buffer is freed on the way out)
    return _bank_outputs(d_y, n_ch, n, n_out, mode)


def _istft_device(stft: DeviceSTFT, nfft: int, W: int, step: int, window, scale: float, frame_offset: int,
                  n_frames_total: int) -> DevicePlanar:
    """_istft of a device-resident spectrogram -> device-resident planar samples (ds_istft_dev)."""
    if nfft < 2:
        raise ValueError("fft_length_samples must be at least 2")
    assert not stft.power, "a power spectrogram has no phase to invert"
    n_bins, n_frames, n_ch = stft.shape
    if W > nfft:
        raise ValueError(f"operands could not be broadcast together with shapes ({nfft},{n_frames},{n_ch}) ({W},1,1)")
    total_length = int(step * n_frames_total + W * (1 - step / W))
    ctx = stft.buf.ctx
    d_w = _window_dev(ctx, window)
    with device_scope(ctx) as dev:
        d_o = dev.alloc(n_ch * total_length * 4, result=True)
        ctx.check(ctx.lib.ds_istft_dev(ctx.handle, C.c_void_p(stft.buf.ptr), n_bins, n_frames, n_ch, nfft, W, step,
                                       frame_offset, n_frames_total, C.c_void_p(d_w.ptr), float(scale), total_length,
                                       C.c_void_p(d_o.ptr), total_length), "ds_istft_dev")
        ctx.sync()
    return DevicePlanar(d_o, n_ch, total_length)


def spectral_division_device(y_dev: DevicePlanar, x_dev: DevicePlanar, n_fft: int, n_out: int, eps_from_spectrum=None):
    """irfft(rfft(y, n_fft) * R, n_fft)[:n_out] with R = conj(X) / (|X|^2 + eps) (or 1 / X) built from the spectrum of the
    device-resident x (one channel for every channel of y, or one per channel), all on the device: ds_rfft_dev ->
    ds_deconv_inverse_dev -> ds_deconv_dev.  eps_from_spectrum(denum_fft (B, Cx) complex128) -> eps (B,) is the host's
    band detection (the reference's find_frequencies_above_threshold on channel 0); None: plain division.
    -> DevicePlanar (Cy, n_out)."""
    ctx = y_dev.ctx
    n, n_cy, n_cx = y_dev.n_samples, y_dev.n_ch, x_dev.n_ch
    assert x_dev.n_samples == n and n <= n_fft and n_out <= n_fft
    B = n_fft // 2 + 1
    with device_scope(ctx) as dev:
        d_xs = dev.alloc(B * n_cx * 8)
        d_r = dev.alloc(B * n_cx * 8)
        d_o = dev.alloc(n_cy * int(n_out) * 4, result=True)
        d_e = None
        ctx.check(ctx.lib.ds_rfft_dev(ctx.handle, C.c_void_p(x_dev.ptr), n_cx, x_dev.ld, n, int(n_fft), 1.0,
                                      C.c_void_p(d_xs.ptr)), "ds_rfft_dev")
        if eps_from_spectrum is not None:
            den = ctx.download_staged(d_xs.ptr, (B, n_cx), np.complex64).astype(np.complex128)
            d_e = dev.upload(np.ascontiguousarray(eps_from_spectrum(den), dtype=np.float32))
        ctx.check(ctx.lib.ds_deconv_inverse_dev(ctx.handle, C.c_void_p(d_xs.ptr), n_cx, B, C.c_void_p(d_e.ptr) if d_e else None,
                                                C.c_void_p(d_r.ptr)), "ds_deconv_inverse")
        ctx.check(ctx.lib.ds_deconv_dev(ctx.handle, C.c_void_p(y_dev.ptr), 1, n_cy, y_dev.ld, n, int(n_fft), C.c_void_p(d_r.ptr),
                                        int(n_cx > 1), int(n_out), int(n_out), C.c_void_p(d_o.ptr)), "ds_deconv_dev")
        ctx.sync()
    return DevicePlanar(d_o, n_cy, int(n_out))


class _StftPlan(NamedTuple):
    """Everything an STFT derives from its parameters and the SHAPE of the samples, before it looks at the samples: built
    once per call by _stft_plan, handed to the one call the function makes."""
    n: int
    n_ch: int
    W: int
    hop: int
    nfft: int
    B: int            # nfft // 2 + 1 bins
    pad_front: int
    n_frames: int
    window: np.ndarray  # float64, read-only when it is one of _window_array's
    detrend: int
    scale: float
    edge: float
    power: int
    time_s: np.ndarray
    freqs_hz: np.ndarray

    @property
    def shape(self) -> tuple:
        """Of the spectrogram: (bins, frames, channels)."""
        return (self.B, self.n_frames, self.n_ch)

    @property
    def window32(self) -> np.ndarray:
        """The window as the kernels read it (a fresh array: _window_dev keys it by content)."""
        return self.window.astype(np.float32)

    def tail(self, window_ptr, ld: int | None = None) -> tuple:
        """The arguments of every ds_stft_r2c* entry between its input and its output: n, n_ch, [leading dimension of
        resident samples], W, hop, nfft, pad_front, n_frames, window, detrend, scale, edge, power.  THE place where their
        order is written."""
        return ((self.n, self.n_ch) + (() if ld is None else (ld,)) + (self.W, self.hop, self.nfft, self.pad_front,
                self.n_frames, window_ptr, self.detrend, self.scale, self.edge, self.power))


def _stft_plan(n_samples: int, n_ch: int, fs_hz: int, window_length_samples: int, window_type, overlap_percent: float,
               fft_length_samples, detrend: bool, padding: bool, scaling: SpectrumScaling) -> _StftPlan:
    """Argument checks (the reference's assertions, in its order) and launch parameters of the STFT of n_samples x n_ch
    samples, wherever they are."""
    assert window_length_samples in [2**k for k in range(4, 17)], (
        "Window length should be a power of 2 between [16, 65536] or [2**4, 2**16]")
    assert overlap_percent >= 0 and overlap_percent < 100, "overlap_percent should be between 0 and 100"
    W = int(window_length_samples)
    nfft = W if fft_length_samples is None else int(fft_length_samples)
    # any positive length, as numpy's rfft(n=...) (_spectral_methods.py:268): frames are cropped to
    # nfft or zero-padded; powers of two >= 8 take the fused kernels, everything else the general
    # route of the library (kernels_stft_any.hpp)
    assert nfft >= 2, "fft_length_samples must be at least 2"
    window = _window_array(window_type, W)
    overlap = int(overlap_percent / 100 * W + 0.5)  # rounding, _spectral_methods.py:247
    hop = W - overlap
    if not _cola_ok(window, overlap):
        warn("Selected window type and overlap do not meet the constant overlap and add constraint! Results might be distorted")
    n, n_ch = int(n_samples), int(n_ch)
    pad_front = overlap if padding else 0
    n_padded = n + 2 * pad_front
    n_frames = int(np.ceil(n_padded / hop))
    if scaling.has_physical_units():
        scale = float(np.asarray(scaling.get_scaling_factor(nfft, fs_hz, window)).ravel()[0])
        edge = 2**-0.5
        power = int(not scaling.is_amplitude_scaling())
    else:
        norm = scaling.fft_norm()
        scale = 1.0 if norm == "backward" else (1.0 / nfft if norm == "forward" else nfft**-0.5)
        edge, power = 1.0, 0
    return _StftPlan(n, n_ch, W, hop, nfft, nfft // 2 + 1, pad_front, n_frames, window, int(bool(detrend)), scale, edge, power,
                     np.linspace(0, n_padded / fs_hz, n_frames), np.fft.rfftfreq(W, 1 / fs_hz))


def _stft(x, fs_hz: int, window_length_samples: int, window_type, overlap_percent: float,
          fft_length_samples, detrend: bool, padding: bool, scaling: SpectrumScaling):
    """-> (time_s (F,), freqs_hz (B,), stft (B', F, C))."""
    xa = np.asarray(x)
    plan = _stft_plan(*_samples_shape(xa), fs_hz, window_length_samples, window_type, overlap_percent, fft_length_samples,
                      detrend, padding, scaling)
    # the fused entry hands back complex128; a power scaling keeps only the real part, taken here from the complex64 array
    route = _host_route(xa, fuses=not plan.power)
    fused = route == ROUTE_FUSED
    x_in, w32 = _host_input(xa, route), plan.window32
    out = np.empty(plan.shape, dtype=np.complex128 if fused else np.complex64)
    name = "ds_stft_r2c_f64" if fused else "ds_stft_r2c"
    ctx = get_context()
    ctx.check(getattr(ctx.lib, name)(ctx.handle, _ptr(x_in), *plan.tail(_ptr(w32)), _ptr(out)), name)
    if not fused:
        out = out.real.astype(np.float64) if plan.power else _widen(out)
    return plan.time_s, plan.freqs_hz, out


def _spectrogram_band_power(x, fs_hz: int, window_length_samples: int, window_type, overlap_percent: float, fft_length_samples,
                            detrend: bool, padding: bool, scaling: SpectrumScaling, band_filters, to_db: bool, dct_abs: bool):
    """STFT -> sum_b filters[band, b] |stft[b]|^2 (-> dB -> |DCT-II| over bands), everything on the
    device: the spectrogram never travels to the host.  band_filters (bands, B').
    -> (time_s, freqs_hz, out (bands, F, C) float64)."""
    resident = isinstance(x, DevicePlanar)  # a device-resident signal: its samples are read in place
    if not resident:
        x = np.asarray(x)
    plan = _stft_plan(*_samples_shape(x), fs_hz, window_length_samples, window_type, overlap_percent, fft_length_samples,
                      detrend, padding, scaling)
    filt = np.ascontiguousarray(band_filters, dtype=np.float32)
    assert filt.ndim == 2 and filt.shape[1] == plan.B, (
        f"Shape of the mel filter matrix {filt.shape} does not match the STFT {plan.shape}")
    n_bands = filt.shape[0]
    nz = filt != 0
    b0 = np.where(nz.any(axis=1), nz.argmax(axis=1), 0).astype(np.int32)
    b1 = np.where(nz.any(axis=1), filt.shape[1] - nz[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    ctx = x.ctx if resident else get_context()
    n_fc = plan.n_frames * plan.n_ch
    with device_scope(ctx) as dev:
        d_x = x if resident else dev.upload(_planar_f32(x))
        d_w = dev.upload(plan.window32)
        d_s = dev.alloc(plan.B * n_fc * 8)
        d_f = dev.upload(filt)
        d_b0, d_b1 = dev.upload(b0), dev.upload(b1)
        d_o = dev.alloc(n_bands * n_fc * 4)
        ctx.check(ctx.lib.ds_stft_r2c_dev(ctx.handle, C.c_void_p(d_x.ptr),
                                          *plan.tail(C.c_void_p(d_w.ptr), x.ld if resident else plan.n), C.c_void_p(d_s.ptr)),
                  "ds_stft_r2c_dev")
        ctx.check(ctx.lib.ds_band_power_dev(ctx.handle, C.c_void_p(d_s.ptr), plan.B, n_fc, C.c_void_p(d_f.ptr),
                                            C.c_void_p(d_b0.ptr), C.c_void_p(d_b1.ptr), n_bands, int(bool(to_db)),
                                            int(bool(dct_abs)), C.c_void_p(d_o.ptr)), "ds_band_power_dev")
        out = d_o.to_array((n_bands, plan.n_frames, plan.n_ch), np.float32)
    return plan.time_s, plan.freqs_hz, out.astype(np.float64)


BF_METHODS = {"mvdr": 0, "functional": 1, "orthogonal": 2}  # ds_bf_eig_map's method codes


def _bf_inputs(csm, h, dtype=np.complex128):
    cs = np.ascontiguousarray(csm, dtype=dtype)
    hs = np.ascontiguousarray(h, dtype=dtype)
    assert cs.ndim == 3 and hs.ndim == 3 and cs.shape[1] == cs.shape[2], "csm must be (bins, C, C)"
    assert hs.shape[0] == cs.shape[0] and hs.shape[1] == cs.shape[1], "steering vector must be (bins, C, grid points)"
    return cs, hs


def _bf_map(entry: str, cs: np.ndarray, hs: np.ndarray, *params) -> np.ndarray:
    """One beamformer map entry (csm, h, bins, C, grid points, *params, out) over _bf_inputs' arrays -> (G, F), real."""
    n_bins, n_ch, n_grid = hs.shape
    out = np.empty((n_grid, n_bins), dtype=hs.real.dtype)
    ctx = get_context()
    ctx.check(getattr(ctx.lib, entry)(ctx.handle, _ptr(cs), _ptr(hs), n_bins, n_ch, n_grid, *params, _ptr(out)), entry)
    return out


def _das_map(csm, h):
    """Re(h^H csm h) per grid point and bin: csm (F, C, C), h (F, C, G) -> (G, F) float64."""
    return _bf_map("ds_das_map", *_bf_inputs(csm, h, np.complex64)).astype(np.float64)


def hermitian_eigh(a):
    """numpy.linalg.eigh of a stack of Hermitian matrices on the device (ds_bf_eigh; the lower triangle is read):
    a (F, C, C) -> w (F, C) ascending float64, v (F, C, C) complex128 with v[f][:, k] the eigenvector of w[f][k]."""
    a = np.ascontiguousarray(a, dtype=np.complex128)
    assert a.ndim == 3 and a.shape[1] == a.shape[2], "a must be (matrices, C, C)"
    n_mat, n_ch = a.shape[0], a.shape[1]
    w = np.empty((n_mat, n_ch), dtype=np.float64)
    v = np.empty_like(a)
    ctx = get_context()
    ctx.check(ctx.lib.ds_bf_eigh(ctx.handle, _ptr(a), n_mat, n_ch, _ptr(w), _ptr(v)), "ds_bf_eigh")
    return w, v


def beamformer_eig_map(csm, h, method: str, gamma: float = 10.0, n_eig: int = 0) -> np.ndarray:
    """MVDR, Functional or Orthogonal map per grid point and bin from one eigendecomposition of every bin's CSM
    (ds_bf_eig_map, float64): csm (F, C, C) the selected bins, h (F, C, G) -> (G, F) float64."""
    cs, hs = _bf_inputs(csm, h)
    return _bf_map("ds_bf_eig_map", cs, hs, BF_METHODS[method], float(gamma), int(n_eig))


def beamformer_cleansc_map(csm, h, maximum_iterations: int, safety_factor: float, remove_csm_diagonal: bool) -> np.ndarray:
    """CLEAN-SC clean map per grid point and bin (ds_bf_cleansc, float64): csm (F, C, C) the selected bins,
    h (F, C, G) -> (G, F) float64."""
    cs, hs = _bf_inputs(csm, h)
    return _bf_map("ds_bf_cleansc", cs, hs, int(maximum_iterations), float(safety_factor), int(bool(remove_csm_diagonal)))


def _istft(stft, nfft: int, W: int, step: int, window, scale: float, frame_offset: int, n_frames_total: int):
    """Frame-wise irfft (length nfft, cropped to W) * scale * window, overlap-added at
    (frame + frame_offset) * step and divided by the squared-window envelope clipped at 1e-4
    (standard/_framed_signal_representation.py:70-137).  stft (B, F, C) -> (total_length, C)."""
    if nfft < 2:
        raise ValueError("fft_length_samples must be at least 2")
    if np.isrealobj(stft):
        stft = stft.astype(np.complex128)
    n_bins, n_frames, n_ch = stft.shape
    if W > nfft:  # the reference's `td_framed *= window[:, None, None]` cannot broadcast either
        raise ValueError(f"operands could not be broadcast together with shapes ({nfft},{n_frames},{n_ch}) ({W},1,1)")
    # length of the reference's reconstruction buffer (same float expression, :112-115)
    total_length = int(step * n_frames_total + W * (1 - step / W))
    # a large complex128 spectrogram is narrowed in host threads into pinned upload chunks, float64 (N, C) comes back
    # (its own condition: _host_route speaks of (N, C) float64 samples); anything else goes up as complex64, planar comes back
    fused = stft.dtype == np.complex128 and stft.flags.c_contiguous and stft.size >= (1 << 19)
    sp = stft if fused else np.ascontiguousarray(stft, dtype=np.complex64)
    out = np.empty((total_length, n_ch), dtype=np.float64) if fused else np.empty((n_ch, total_length), dtype=np.float32)
    w32 = np.ascontiguousarray(window, dtype=np.float32)
    name = "ds_istft_f64" if fused else "ds_istft"
    ctx = get_context()
    ctx.check(getattr(ctx.lib, name)(ctx.handle, _ptr(sp), n_bins, n_frames, n_ch, nfft, W, step, frame_offset, n_frames_total,
                                     _ptr(w32), float(scale), total_length, _ptr(out)), name)
    return out if fused else _interleaved_f64(out)


_STAGED_RESULT_BYTES = 512 << 20  # largest result that goes through the context's page-locked staging buffer (which stays allocated)


_CSM_ENTRY = {ROUTE_X64: "ds_csm_x64", ROUTE_FUSED: "ds_csm_f64", ROUTE_PLANAR: "ds_csm"}


def _csm_welch(time_data, sampling_rate_hz: int, window_length_samples: int, window_type,
               overlap_percent, detrend: bool, average: str, scaling: SpectrumScaling):
    """-> (f (B,), csm (B, C, C) complex128)."""
    td = np.asarray(time_data)
    if td.ndim == 1:
        td = td[:, None]
    n, n_ch = td.shape
    plan = _welch_plan(n, sampling_rate_hz, window_type, window_length_samples, overlap_percent, detrend, average, scaling)
    # a short estimate runs in float64 end to end on the device (ds_csm_x64)
    route = _welch_route(plan, "matrix", n_ch, "fusable" if _fusable(td) else "host")
    x, w = _host_input(td, route), plan.window_for(route)
    ctx = get_context()
    shape = (plan.B, n_ch, n_ch)
    nbytes = plan.B * n_ch * n_ch * 8
    if route == ROUTE_X64:
        out = np.empty(shape, dtype=np.complex128)
    elif nbytes <= _STAGED_RESULT_BYTES:
        # the complex64 matrices land in the context's page-locked staging buffer (the link's full rate, no first-touch faults
        # of a fresh array) and are widened out of it into the complex128 array the caller gets
        out = ctx.staging(nbytes).view(np.complex64).reshape(shape)
    else:  # (up to 512 MB; a larger result -- hundreds of channels -- comes back into an ordinary array)
        out = np.empty(shape, dtype=np.complex64)
    ctx.check(getattr(ctx.lib, _CSM_ENTRY[route])(ctx.handle, _ptr(x), n_ch, n, *plan.tail(_ptr(w)), _ptr(out)),
              _CSM_ENTRY[route])
    return np.fft.rfftfreq(plan.W, 1 / sampling_rate_hz), out if route == ROUTE_X64 else _widen(out)


class DeviceCSM:
    """A Welch cross-spectral matrix that stays in HBM: (bins, C, C) complex64 in `buf`, the frequency
    vector on the host.  What `Signal.get_csm(on_device=True)` returns and the device delay-and-sum map
    consumes (the reference's beamformers take `self.signal.get_csm()` and keep going,
    beamforming/beamforming.py:838-876)."""

    def __init__(self, ctx, buf, freqs_hz, n_ch: int):
        self.ctx, self.buf, self.freqs_hz, self.n_ch = ctx, buf, freqs_hz, int(n_ch)
        self.n_bins = len(freqs_hz)

    def to_host(self) -> np.ndarray:
        shape = (self.n_bins, self.n_ch, self.n_ch)
        if self.n_bins * self.n_ch * self.n_ch * 8 > _STAGED_RESULT_BYTES:
            return _widen(self.buf.to_array(shape, np.complex64))
        return _widen(self.ctx.download_staged(self.buf.ptr, shape, np.complex64))

    def free(self):
        self.buf.free()


def _csm_welch_device(time_data, sampling_rate_hz: int, window_length_samples: int, window_type,
                      overlap_percent, detrend: bool, average: str, scaling: SpectrumScaling) -> DeviceCSM:
    """_csm_welch whose result stays on the device (ds_csm_dev, the fp32 kernels for every shape) -> DeviceCSM.
    time_data: the (N, C) array, or the DevicePlanar of a device-resident signal (read in place)."""
    resident = isinstance(time_data, DevicePlanar)
    td = time_data if resident else np.asarray(time_data)
    n = td.n_samples if resident else td.shape[0]
    plan = _welch_plan(n, sampling_rate_hz, window_type, window_length_samples, overlap_percent, detrend, average, scaling)
    ctx = td.ctx if resident else get_context()
    with device_scope(ctx) as dev:
        x = td if resident else DevicePlanar(dev.upload(_planar_f32(td)), 1 if td.ndim == 1 else td.shape[1], n)
        d_w = dev.upload(plan.window_for(ROUTE_PLANAR))
        d_c = dev.alloc(plan.B * x.n_ch * x.n_ch * 8, result=True)  # (the matrix only leaves this function inside a DeviceCSM)
        ctx.check(ctx.lib.ds_csm_dev(ctx.handle, C.c_void_p(x.ptr), x.n_ch, x.ld, n, *plan.tail(C.c_void_p(d_w.ptr)),
                                     C.c_void_p(d_c.ptr)), "ds_csm_dev")
        ctx.sync()
    return DeviceCSM(ctx, d_c, np.fft.rfftfreq(plan.W, 1 / sampling_rate_hz), x.n_ch)


def _das_map_device(csm: DeviceCSM, id1: int, id2: int, h, remove_csm_diagonal: bool):
    """Delay-and-sum map of the bins [id1, id2) of a device-resident CSM: the diagonal treatment
    (beamforming.py:840-845) and Re(h^H csm h) (:853-858) on the device; only the steering vectors go up and
    the (grid points, bins) map comes down.  h (bins, C, G) complex -> (G, bins) float64."""
    hs = np.ascontiguousarray(h, dtype=np.complex64)
    nb = id2 - id1
    assert hs.ndim == 3 and hs.shape[0] == nb and hs.shape[1] == csm.n_ch, "steering vector must be (bins, C, grid points)"
    n_grid = hs.shape[2]
    ctx = csm.ctx
    with device_scope(ctx) as dev:
        d_h = dev.upload(hs)
        d_s = dev.alloc(nb * csm.n_ch * csm.n_ch * 8)
        d_m = dev.alloc(n_grid * nb * 4)
        src = csm.buf.ptr + id1 * csm.n_ch * csm.n_ch * 8
        scale = csm.n_ch / (csm.n_ch - 1) if remove_csm_diagonal else 1.0
        ctx.check(ctx.lib.ds_csm_das_prepare_dev(ctx.handle, C.c_void_p(src), nb, csm.n_ch, float(scale),
                                                 int(bool(remove_csm_diagonal)), C.c_void_p(d_s.ptr)), "ds_csm_das_prepare_dev")
        ctx.check(ctx.lib.ds_das_map_dev(ctx.handle, C.c_void_p(d_s.ptr), C.c_void_p(d_h.ptr), nb, csm.n_ch, n_grid,
                                         C.c_void_p(d_m.ptr)), "ds_das_map_dev")
        out = d_m.to_array((n_grid, nb), np.float32)
    return out.astype(np.float64)


def _csm_welch_bins(time_data, sampling_rate_hz: int, window_length_samples: int, window_type,
                    overlap_percent, detrend: bool, scaling: SpectrumScaling, bin_start: int,
                    bin_stop: int):
    """Rows [bin_start, bin_stop) of the Welch CSM (mean averaging): one rank's share when the
    matrix is split by frequency bins.  -> (bin_stop - bin_start, C, C) complex128."""
    td = np.asarray(time_data)
    n, n_ch = td.shape[0], (1 if td.ndim == 1 else td.shape[1])
    plan = _welch_plan(n, sampling_rate_hz, window_type, window_length_samples, overlap_percent, detrend, "mean", scaling)
    count = int(bin_stop) - int(bin_start)
    if count <= 0:
        return np.zeros((0, n_ch, n_ch), dtype=np.complex128)
    ctx = get_context()
    with device_scope(ctx) as dev:
        d_x = dev.upload(_planar_f32(td))
        d_w = dev.upload(plan.window_for(ROUTE_PLANAR))
        d_c = dev.alloc(count * n_ch * n_ch * 8)
        ctx.check(ctx.lib.ds_csm_bins_dev(ctx.handle, C.c_void_p(d_x.ptr), n_ch, n, n, *plan.tail(C.c_void_p(d_w.ptr), with_avg=False),
                                          int(bin_start), count, C.c_void_p(d_c.ptr)), "ds_csm_bins_dev")
        out = d_c.to_array((count, n_ch, n_ch), np.complex64)
    return out.astype(np.complex128)


def _csm_fft(spectrum, scaling: SpectrumScaling, window, sampling_rate_hz: int):
    """Cross-spectral matrix of ONE whole-signal spectrum (B, C) (FFTBackward-normalised),
    dsptoolbox/standard/_spectral_methods.py:374-443.  -> (B, C, C) complex128."""
    if window is not None:
        raise NotImplementedError("time-windowed signals are outside the GPU hot path")
    xs = np.ascontiguousarray(spectrum, dtype=np.complex64)
    nb, n_ch = xs.shape
    if scaling == SpectrumScaling.FFTBackward:
        amp, factor, halve = 0, 1.0, 0
    else:
        # the reference passes `spectrum.shape[0] // 2 + 1` as the length (:436)
        factor = float(np.asarray(SpectrumScaling.FFTBackward.conversion_factor(
            scaling, nb // 2 + 1, sampling_rate_hz, None)).ravel()[0])
        amp, halve = int(scaling.is_amplitude_scaling()), 1
    out = np.empty((nb, n_ch, n_ch), dtype=np.complex64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_csm_spec(ctx.handle, _ptr(xs), nb, 1, n_ch, amp, 1.0, factor, halve,
                                  _ptr(out)), "ds_csm_spec")
    return out.astype(np.complex128)


def rfft_spectrum(time_data, n_fft: int, scale: float = 1.0):
    """rfft(time_data, n=n_fft, axis=0) * scale -> (n_fft/2+1, C) complex128."""
    route = _host_route(time_data)
    fused = route == ROUTE_FUSED
    x_in = _host_input(time_data, route)
    n, n_ch = x_in.shape if fused else x_in.shape[::-1]
    out = np.empty((n_fft // 2 + 1, n_ch), dtype=np.complex128 if fused else np.complex64)
    name = "ds_rfft_f64" if fused else "ds_rfft"
    ctx = get_context()
    ctx.check(getattr(ctx.lib, name)(ctx.handle, _ptr(x_in), n_ch, n, int(n_fft), float(scale), _ptr(out)), name)
    return out if fused else out.astype(np.complex128)


def spectral_division(num_td, n_fft: int, inverse_spectrum, n_out: int):
    """irfft(rfft(num_td, n_fft) * inverse_spectrum, n_fft)[:n_out] per channel.
    num_td (N, C) or (M, N, C) for a batch of M items; inverse_spectrum (B,)
    shared or (B, C) per channel.  -> same leading shape, float64."""
    num_td = np.asarray(num_td)
    batched = num_td.ndim == 3
    fused = _host_route(num_td) == ROUTE_FUSED  # one large item only: a batch is 3-D, which _fusable is not
    items = num_td if batched else num_td[None]
    m, n, n_ch = items.shape
    r = np.asarray(inverse_spectrum)
    per_channel = r.ndim == 2
    rp = np.ascontiguousarray(r.T if per_channel else r, dtype=np.complex64)  # (C, B) or (B,)
    assert rp.shape[-1] == n_fft // 2 + 1, "Frequency vector does not match"
    if fused:
        y_in, out = num_td, np.empty((int(n_out), n_ch), dtype=np.float64)
    else:
        y_in = np.empty((m, n_ch, n), dtype=np.float32)  # (M, C, N)
        if n * n_ch >= (1 << 20):
            for i in range(m):
                y_in[i] = _planar_f32(items[i])
        else:
            y_in[...] = np.transpose(items, (0, 2, 1))
        out = np.empty((m, n_ch, n_out), dtype=np.float32)
    name = "ds_deconv_f64" if fused else "ds_deconv"
    ctx = get_context()
    ctx.check(getattr(ctx.lib, name)(ctx.handle, _ptr(y_in), *(() if fused else (m,)), n_ch, n, int(n_fft), _ptr(rp),
                                     int(per_channel), int(n_out), _ptr(out)), name)
    if fused:
        return out
    res = np.empty((m, n_out, n_ch), dtype=np.float64)
    if n_out * n_ch >= (1 << 20):
        for i in range(m):
            _interleaved_f64(out[i], res[i])
    else:
        res[...] = np.transpose(out, (0, 2, 1))
    return res if batched else res[0]


def regularized_inverse(denum_spectrum, eps=None):
    """conj(X)/(|X|^2+eps) (regularised) or 1/X, on the device.  denum_spectrum
    (B, C) complex; eps (B,) or None.  -> (B, C) complex128."""
    xs = np.ascontiguousarray(denum_spectrum, dtype=np.complex64)
    nb, n_ch = xs.shape
    ctx = get_context()
    with device_scope(ctx) as dev:
        d_x = dev.upload(xs)
        d_e = dev.upload(np.ascontiguousarray(eps, dtype=np.float32)) if eps is not None else None
        d_r = dev.alloc(xs.nbytes)
        ctx.check(ctx.lib.ds_deconv_inverse_dev(ctx.handle, C.c_void_p(d_x.ptr), n_ch, nb,
                                                C.c_void_p(d_e.ptr) if d_e else None,
                                                C.c_void_p(d_r.ptr)), "ds_deconv_inverse")
        r = d_r.to_array((n_ch, nb), np.complex64)
    return r.T.astype(np.complex128)


def fir_filter_bank(x, taps_list, mode: int):
    """x (N, C); taps_list K arrays of equal length T.  Parallel -> (K, N, C);
    Sequential / Summed -> (N, C).  float64."""
    taps = np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.float64) for t in taps_list]), dtype=np.float32)
    k, t = taps.shape
    xa = np.asarray(x)
    route = _host_route(xa)
    fused = route == ROUTE_FUSED
    x_in = _host_input(xa, route)
    n, n_ch = x_in.shape if fused else x_in.shape[::-1]
    n_out = k if mode == DS_FB_PARALLEL else 1
    out = np.empty((n_out, n, n_ch), dtype=np.float64) if fused else np.empty((n_out, n_ch, n), dtype=np.float32)
    name = "ds_fir_ola_f64" if fused else "ds_fir_ola"
    ctx = get_context()
    ctx.check(getattr(ctx.lib, name)(ctx.handle, _ptr(x_in), n_ch, n, _ptr(taps), k, t, int(mode), _ptr(out)), name)
    if not fused:
        planar, out = out, np.empty((n_out, n, n_ch), dtype=np.float64)
        for i in range(n_out):
            _interleaved_f64(planar[i], out[i])
    return out if mode == DS_FB_PARALLEL else out[0]


def _lfilter_fir(b, a, x, zi=None, axis: int = 0):
    """Causal FIR filtering y = (x * b)[:N] along axis 0 (dsptoolbox/classes/filter_helpers.py:
    454-503).  With zi (T-1, C): the full convolution (N + T - 1 samples, device) gets zi added
    to its head, the new state is its tail; returns (y, zf)."""
    a = np.atleast_1d(a)
    assert len(a) == 1, f"{a} is not valid. It has to be 1 in order to be a valid FIR filter"
    b = np.asarray(b)
    if b.ndim != 1:
        b = np.squeeze(b)
        assert b.ndim == 1, "FIR Filters for audio must be 1D-arrays"
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise NotImplementedError("complex input signals are outside the GPU hot path (Signal.time_data is real)")
    if np.iscomplexobj(b):
        # complex taps on a real signal (filter_helpers.py:364-371 stores the imaginary part of the output in
        # Signal.time_data_imaginary): two real convolutions, x * Re b + i x * Im b, one device call
        return _lfilter_fir_complex(b, x, zi)
    if zi is not None:
        zi = np.asarray(zi)
        assert zi.ndim == x.ndim, \
            "Vector to filter and initial values should have the same number of dimensions!"
    if x.ndim < 2:
        x = x[..., None]
        if zi is not None:
            zi = zi[..., None]
    assert x.ndim == 2, "Filtering only works on 2D-arrays"
    if zi is None:
        return fir_filter_bank(x, [b], DS_FB_PARALLEL)[0]
    # mode="full": run the device convolution over the signal followed by T - 1 zeros
    xfull = np.concatenate([x, np.zeros((len(b) - 1, x.shape[1]))], axis=0)
    y = fir_filter_bank(xfull, [b], DS_FB_PARALLEL)[0]
    y[: zi.shape[0], :] += zi
    zf = y[-zi.shape[0]:, :]
    return y[: x.shape[0], :], zf


def fir_transfer_function(taps_list, frequency_vector_hz, sampling_rate_hz: int) -> np.ndarray:
    """H_k(f) = sum_n b_k[n] exp(-2 pi i f n / fs) for every filter of the list at every frequency, float64 on
    the device (ds_fir_freqz) -- scipy.signal.freqz(b, 1, worN=f, fs=fs)[1] of the reference's
    Filter.get_transfer_function (classes/filter.py:893-900).  -> (frequencies, filters) complex128."""
    f = np.ascontiguousarray(frequency_vector_hz, dtype=np.float64)
    assert f.ndim == 1, "Frequency vector can only have one dimension"
    n_taps = max(len(t) for t in taps_list)
    taps = np.zeros((len(taps_list), n_taps), dtype=np.complex128)
    for k, t in enumerate(taps_list):
        taps[k, :len(t)] = t
    out = np.empty((len(taps_list), len(f)), dtype=np.complex128)
    ctx = get_context()
    ctx.check(ctx.lib.ds_fir_freqz(ctx.handle, _ptr(taps), taps.shape[0], n_taps, _ptr(f), len(f),
                                   float(sampling_rate_hz), _ptr(out)), "ds_fir_freqz")
    return np.ascontiguousarray(out.T)


def _pad_trim(vector: np.ndarray, desired_length: int) -> np.ndarray:
    """Zero-pad or trim the END of axis 0 (helpers/other.py:216-259 with its defaults)."""
    v = np.asarray(vector)
    n = v.shape[0]
    if n == desired_length:
        return v.copy()
    if n > desired_length:
        return v[:desired_length].copy()
    return np.concatenate([v, np.zeros((desired_length - n,) + v.shape[1:], dtype=v.dtype)], axis=0)


def _lfilter_fir_complex(b, x, zi=None):
    """_lfilter_fir for complex taps b on a real x: the real and the imaginary part of b are two band
    filters of one parallel bank; state (complex) as in the real case."""
    if zi is not None:
        zi = np.asarray(zi)
    if x.ndim < 2:
        x = x[..., None]
        if zi is not None:
            zi = zi[..., None]
    assert x.ndim == 2, "Filtering only works on 2D-arrays"
    br, bi = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
    if zi is None:
        out = fir_filter_bank(x, [br, bi], DS_FB_PARALLEL)
        return out[0] + 1j * out[1]
    xfull = np.concatenate([x, np.zeros((len(b) - 1, x.shape[1]))], axis=0)
    out = fir_filter_bank(xfull, [br, bi], DS_FB_PARALLEL)
    y = out[0] + 1j * out[1]
    y[: zi.shape[0], :] += zi
    zf = y[-zi.shape[0]:, :]
    return y[: x.shape[0], :], zf


def _lfilter_zi_fir(b):
    """scipy.signal.lfilter_zi(b, [1.0]) in closed form (the reference's Filter.initialize_zi,
    classes/filter.py:331-353): steady-state step-response state of a transposed direct-form
    FIR filter, zi[i] = sum_{j > i} b[j].  Host-side parameter preparation."""
    b = np.asarray(b)
    b = b.astype(np.complex128 if np.iscomplexobj(b) else np.float64)
    return np.cumsum(b[::-1])[::-1][1:].copy()


def _filtfilt_fir(b, x):
    """Zero-phase FIR filtering = scipy.signal.filtfilt(b, [1.0], x, axis=0) with its defaults
    (odd extension by 3*len(b) samples, steady-state initial conditions), the zero_phase branch
    of the reference (filter_helpers.py:362-363).  Both convolutions run on the device; the
    extension, the time reversals and the state terms are host-side array plumbing."""
    b = np.asarray(b, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim < 2:
        x = x[..., None]
    edge = 3 * len(b)
    if x.shape[0] <= edge:
        raise ValueError(
            "The length of the input vector x must be greater than padlen, which is %d." % edge)
    ext = np.concatenate([2 * x[:1] - x[edge:0:-1], x, 2 * x[-1:] - x[-2:-(edge + 2):-1]], axis=0)
    zi = _lfilter_zi_fir(b)[:, None]
    y, _ = _lfilter_fir(b, [1.0], ext, zi * ext[:1])
    y, _ = _lfilter_fir(b, [1.0], y[::-1], zi * y[-1:])
    return y[::-1][edge:-edge]


# ---- IIR filtering: cascades of second-order sections (ds_iir_sos, csrc/kernels_iir.hpp) ----------------------------
IIR_MAX_SECTIONS = 32  # one cascade on the device (DS_ERR_UNSUP above)
_IDENTITY_SECTION = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def _sos_stack(sos_list) -> np.ndarray:
    """K filters' (n_k, 6) sections -> [K][max n_k][6] float64; shorter cascades are padded with the identity section,
    which passes its input through exactly and keeps a zero state."""
    n_max = max(np.atleast_2d(s).shape[0] for s in sos_list)
    out = np.tile(_IDENTITY_SECTION, (len(sos_list), n_max, 1))
    for k, s in enumerate(sos_list):
        s = np.atleast_2d(np.asarray(s, dtype=np.float64))
        out[k, :s.shape[0]] = s
    return out


def _sequential_cascades(sos_list) -> list:
    """The sections of a Sequential bank, in order, as consecutive cascades of at most IIR_MAX_SECTIONS (one device call
    each): a list of one for a bank that fits."""
    sections = np.concatenate([np.atleast_2d(np.asarray(s, dtype=np.float64)) for s in sos_list])
    return [sections[i0:i0 + IIR_MAX_SECTIONS] for i0 in range(0, len(sections), IIR_MAX_SECTIONS)]


def iir_sos_filter(x, sos_list, mode: int, zi=None):
    """sosfilt of x (N, C) float64 through K cascades of second-order sections (the recursion in float64 on the
    device).  Parallel -> (K, N, C); Sequential / Summed -> (N, C).  zi (K, n_max, 2, C) (sosfilt's per-filter
    layout, identity-padded sections included) gives the initial state; then (y, zf) is returned, zf in the same
    layout.  A Sequential bank longer than one device cascade runs as consecutive cascades."""
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if xa.ndim == 1:
        xa = xa[:, None]
    if mode == DS_FB_SEQUENTIAL:
        cascades = _sequential_cascades(sos_list)
        if zi is None and len(cascades) > 1:
            y = xa
            for sections in cascades:
                y = iir_sos_filter(y, [sections], DS_FB_PARALLEL)[0]
            return y
        sos_list = cascades if zi is None else sos_list
    sos = _sos_stack(sos_list)
    k, n_sec = sos.shape[0], sos.shape[1]
    n, n_ch = xa.shape
    y = np.empty(((k if mode == DS_FB_PARALLEL else 1), n, n_ch), dtype=np.float64)
    zf = None
    if zi is not None:
        zi = np.ascontiguousarray(zi, dtype=np.float64)
        assert zi.shape == (k, n_sec, 2, n_ch), "zi must be (filters, sections, 2, channels)"
        zf = np.empty_like(zi)
    ctx = get_context()
    ctx.check(ctx.lib.ds_iir_sos(ctx.handle, _ptr(xa), n_ch, n, _ptr(sos), k, n_sec,
                                 None if zi is None else _ptr(zi), int(mode), _ptr(y),
                                 None if zf is None else _ptr(zf)), "ds_iir_sos")
    y = y if mode == DS_FB_PARALLEL else y[0]
    return y if zi is None else (y, zf)


def iir_sos_filter_device(x_dev: DevicePlanar, sos_list, mode: int):
    """iir_sos_filter over device-resident samples (ds_iir_sos_dev, no state): Parallel -> a list of K DevicePlanar
    (slices of ONE output buffer), Sequential / Summed -> one DevicePlanar.  Nothing comes down."""
    if mode == DS_FB_SEQUENTIAL:
        sos_list = _sequential_cascades(sos_list)
        if len(sos_list) > 1:
            y = x_dev
            for sections in sos_list:
                y = iir_sos_filter_device(y, [sections], DS_FB_PARALLEL)[0]
            return y
    sos = _sos_stack(sos_list)
    k, n_sec = sos.shape[0], sos.shape[1]
    ctx = x_dev.ctx
    n, n_ch = x_dev.n_samples, x_dev.n_ch
    n_out = k if mode == DS_FB_PARALLEL else 1
    with device_scope(ctx) as dev:
        d_y = dev.alloc(n_out * n_ch * n * 4, result=True)
        ctx.check(ctx.lib.ds_iir_sos_dev(ctx.handle, C.c_void_p(x_dev.ptr), n_ch, x_dev.ld, n, _ptr(sos), k, n_sec, None,
                                         int(mode), C.c_void_p(d_y.ptr), n, None), "ds_iir_sos_dev")
    return _bank_outputs(d_y, n_ch, n, n_out, mode)


# ---- IIR filtering with complex coefficients (ds_iir_sos_c128, csrc/kernels_ciir.hpp) -------------------------------
CIIR_MAX_SEC = 16  # sections of one complex cascade on the device (CIIR_MAX_SEC of the kernels; DS_ERR_UNSUP above)


def iir_sos_filter_complex(x, sos_list, zi=None, real_only: bool = False):
    """sosfilt of REAL x (N, C) through K cascades of second-order sections with complex coefficients, every filter on
    every channel (the recursion in complex float64 on the device) -> (K, N, C) complex128, or float64 (the real part;
    the imaginary plane is then never written) with real_only.  zi (K, n_max, 2, C) complex gives the initial state;
    then (y, zf) is returned, zf in the same layout."""
    if np.iscomplexobj(x):
        raise NotImplementedError("complex input samples are not run through the device recursion (its input is real)")
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if xa.ndim == 1:
        xa = xa[:, None]
    n_max = max(np.atleast_2d(s).shape[0] for s in sos_list)
    if n_max > CIIR_MAX_SEC:
        raise NotImplementedError(f"cascades of more than {CIIR_MAX_SEC} complex second-order sections are not run on "
                                  f"the device (got {n_max}); split the filter")
    sos = _complex_sos_stack(sos_list)
    k = sos.shape[0]
    n, n_ch = xa.shape
    y_re = np.empty((k, n, n_ch), dtype=np.float64)
    y_im = None if real_only else np.empty((k, n, n_ch), dtype=np.float64)
    zf = None
    if zi is not None:
        zi = np.ascontiguousarray(zi, dtype=np.complex128)
        assert zi.shape == (k, n_max, 2, n_ch), "zi must be (filters, sections, 2, channels)"
        zf = np.empty_like(zi)
    ctx = get_context()
    ctx.check(ctx.lib.ds_iir_sos_c128(ctx.handle, _ptr(xa), n_ch, n, _ptr(sos), k, n_max,
                                      None if zi is None else _ptr(zi), _ptr(y_re),
                                      None if y_im is None else _ptr(y_im), None if zf is None else _ptr(zf)),
              "ds_iir_sos_c128")
    y = y_re if real_only else y_re + 1j * y_im
    return y if zi is None else (y, zf)


# ---- structure filters: lattice-ladder, warped and Kautz recursions (ds_sfilt, csrc/kernels_sfilt.hpp) ----------------
SFILT_MAX_STATES = 64  # state values of one structure on the device (MAX_D of the kernels; DS_ERR_UNSUP above)
SFILT_FIR_LATTICE, SFILT_IIR_LATTICE, SFILT_SOS_LATTICE, SFILT_WARPED_FIR, SFILT_WARPED_IIR, SFILT_KAUTZ = range(6)


def sfilt_coef_count(kind: int, d: int, aux: int) -> int:
    """Values in the packed coefficient array of a structure (coef_count of the kernels; include/dsptoolbox_amd.h)."""
    return {SFILT_FIR_LATTICE: d, SFILT_IIR_LATTICE: 2 * d + 1, SFILT_SOS_LATTICE: 5 * (d // 2), SFILT_WARPED_FIR: 1 + d,
            SFILT_WARPED_IIR: 1 + d + aux + 1, SFILT_KAUTZ: 3 * aux + 6 * ((d - aux) // 2)}[kind]


def _sfilt_args(kind: int, coef, d: int, aux: int, n_ch: int, zi, want_zf: bool):
    """NotImplementedError beyond the kernels' bounds, before anything reaches the device; the packed coefficients
    (their count held against what kind, d and aux imply: the entry reads that many), zi and the zf to fill as
    contiguous float64."""
    if np.iscomplexobj(coef):
        raise NotImplementedError("structure filters with complex coefficients are not run on the device (its "
                                  "recursions are real)")
    if d > SFILT_MAX_STATES:
        raise NotImplementedError(f"structure filters with more than {SFILT_MAX_STATES} states are not run on the device "
                                  f"(got {d}): the carry's state vector is one value per lane of a wave")
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    assert kind in range(6) and d >= 1 and 0 <= aux <= d, "unknown structure kind or state counts out of range"
    assert coef.shape == (sfilt_coef_count(kind, d, aux),), \
        f"the structure needs {sfilt_coef_count(kind, d, aux)} packed coefficients, got an array of shape {coef.shape}"
    if zi is not None:
        zi = np.ascontiguousarray(zi, dtype=np.float64)
        assert zi.shape == (d, n_ch), "zi must be (states, channels)"
    zf = np.empty((d, n_ch), dtype=np.float64) if want_zf else None
    return coef, zi, zf


def sfilt_filter(x, kind: int, coef, d: int, aux: int = 0, zi=None, want_zf: bool = False):
    """x (N, C) float64 through one structure filter (the recursion in float64 on the device): kind, the packed
    coefficients, the state count d and aux as include/dsptoolbox_amd.h lays them out.  zi (d, C) gives the initial state
    (None: zero).  -> y (N, C), or (y, zf) with want_zf."""
    if np.iscomplexobj(x):
        raise NotImplementedError("complex input samples are not run through the device recursion (its input is real)")
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if xa.ndim == 1:
        xa = xa[:, None]
    n, n_ch = xa.shape
    coef, zi, zf = _sfilt_args(kind, coef, d, aux, n_ch, zi, want_zf)
    y = np.empty((n, n_ch), dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_sfilt(ctx.handle, _ptr(xa), n_ch, n, int(kind), _ptr(coef), int(d), int(aux),
                               None if zi is None else _ptr(zi), _ptr(y), None if zf is None else _ptr(zf)), "ds_sfilt")
    return (y, zf) if want_zf else y


def sfilt_filter_device(x_dev: DevicePlanar, kind: int, coef, d: int, aux: int = 0, zi=None, want_zf: bool = False):
    """sfilt_filter over device-resident samples (ds_sfilt_dev): -> a DevicePlanar, or (DevicePlanar, zf); only the
    states (zi up, zf down) cross."""
    ctx = x_dev.ctx
    n, n_ch = x_dev.n_samples, x_dev.n_ch
    coef, zi, zf = _sfilt_args(kind, coef, d, aux, n_ch, zi, want_zf)
    with device_scope(ctx) as dev:
        d_y = dev.alloc(n_ch * n * 4, result=True)
        ctx.check(ctx.lib.ds_sfilt_dev(ctx.handle, C.c_void_p(x_dev.ptr), n_ch, x_dev.ld, n, int(kind), _ptr(coef), int(d),
                                       int(aux), None if zi is None else _ptr(zi), C.c_void_p(d_y.ptr), n,
                                       None if zf is None else _ptr(zf)), "ds_sfilt_dev")
    y = DevicePlanar(d_y, n_ch, n, n, 0)
    return (y, zf) if want_zf else y


# ---- realtime filters: state-variable, direct form, parallel, state space; the direct FIR sum (ds_rtfilt, ds_rtfir,
# csrc/kernels_rtfilt.hpp) ---------------------------------------------------------------------------------------------
RTFILT_MAX_STATES = 64  # state values of one filter on the device (MAX_D of the kernels; DS_ERR_UNSUP above)
RTFILT_SVF, RTFILT_TDF2, RTFILT_PARALLEL, RTFILT_STATE_SPACE = range(4)
RTFIR_MAX_TAPS = 4096  # taps of the direct FIR sum (FIR_MAX_TAPS of the kernels)
RTFIR_MAX_WORK = 2 ** 40  # multiply-adds (samples x channels x taps) of one call of it


def rtfilt_coef_count(kind: int, d: int, aux: int) -> int:
    """Values in the packed coefficient array of a filter (coef_count of the kernels; include/dsptoolbox_amd.h)."""
    return {RTFILT_SVF: 3, RTFILT_TDF2: 2 * d + 2, RTFILT_PARALLEL: 5 * aux, RTFILT_STATE_SPACE: d * d + 2 * d + 1}[kind]


def rtfilt_bands(kind: int) -> int:
    return 4 if kind == RTFILT_SVF else 1


def _rtfir_taps(b, n: int, n_ch: int):
    """NotImplementedError beyond the FIR sum's bounds; the taps as contiguous float64."""
    if np.iscomplexobj(b):
        raise NotImplementedError("structure filters with complex coefficients are not run on the device (its "
                                  "recursions are real)")
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert b.ndim == 1 and len(b) >= 1, "the FIR sum needs a vector of at least one tap"
    if len(b) > RTFIR_MAX_TAPS:
        raise NotImplementedError(f"the direct FIR sum holds at most {RTFIR_MAX_TAPS} taps (got {len(b)})")
    if n * n_ch * len(b) > RTFIR_MAX_WORK:
        raise NotImplementedError(f"the direct FIR sum runs at most 2^40 multiply-adds (samples x channels x taps) in one "
                                  f"call (got {n * n_ch * len(b)})")
    return b


def _rtfilt_args(kind: int, coef, d: int, aux: int, delay: int, fir, n: int, n_ch: int, zi, want_zf: bool):
    """As _sfilt_args: NotImplementedError beyond the kernels' bounds before anything reaches the device; the packed
    coefficients, the FIR part, zi and the zf to fill as contiguous float64."""
    if np.iscomplexobj(coef):
        raise NotImplementedError("structure filters with complex coefficients are not run on the device (its "
                                  "recursions are real)")
    if d > RTFILT_MAX_STATES:
        raise NotImplementedError(f"realtime filters with more than {RTFILT_MAX_STATES} states are not run on the device "
                                  f"(got {d}): the carry's state vector is one value per lane of a wave")
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    assert kind in range(4) and d >= 1 and aux >= 0 and delay >= 0, "unknown filter kind or counts out of range"
    assert coef.shape == (rtfilt_coef_count(kind, d, aux),), \
        f"the filter needs {rtfilt_coef_count(kind, d, aux)} packed coefficients, got an array of shape {coef.shape}"
    if fir is not None:
        fir = _rtfir_taps(fir, n, n_ch)
    if zi is not None:
        zi = np.ascontiguousarray(zi, dtype=np.float64)
        assert zi.shape == (d, n_ch), "zi must be (states, channels)"
    zf = np.empty((d, n_ch), dtype=np.float64) if want_zf else None
    return coef, fir, zi, zf


def _host_samples(x):
    if np.iscomplexobj(x):
        raise NotImplementedError("complex input samples are not run through the device recursion (its input is real)")
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    return xa[:, None] if xa.ndim == 1 else xa


def rtfilt_filter(x, kind: int, coef, d: int, aux: int = 0, delay: int = 0, fir=None, zi=None, want_zf: bool = False):
    """x (N, C) float64 through one realtime filter (the recursion in float64 on the device): kind, the packed
    coefficients, d, aux, the parallel filter's delay and FIR part as include/dsptoolbox_amd.h lays them out.  zi (d, C)
    gives the initial state (None: zero).  -> y (N, C), for the state-variable filter (4, N, C); or (y, zf) with
    want_zf."""
    xa = _host_samples(x)
    n, n_ch = xa.shape
    coef, fir, zi, zf = _rtfilt_args(kind, coef, d, aux, delay, fir, n, n_ch, zi, want_zf)
    nb = rtfilt_bands(kind)
    y = np.empty((nb, n, n_ch), dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_rtfilt(ctx.handle, _ptr(xa), n_ch, n, int(kind), _ptr(coef), int(d), int(aux), int(delay),
                                None if fir is None else _ptr(fir), 0 if fir is None else len(fir),
                                None if zi is None else _ptr(zi), _ptr(y), None if zf is None else _ptr(zf)), "ds_rtfilt")
    y = y if nb > 1 else y[0]
    return (y, zf) if want_zf else y


def rtfilt_filter_device(x_dev: DevicePlanar, kind: int, coef, d: int, aux: int = 0, delay: int = 0, fir=None, zi=None,
                         want_zf: bool = False):
    """rtfilt_filter over device-resident samples (ds_rtfilt_dev): -> a DevicePlanar (a list of four for the
    state-variable filter), or (that, zf); only the coefficients and the states (zi up, zf down) cross."""
    ctx = x_dev.ctx
    n, n_ch = x_dev.n_samples, x_dev.n_ch
    coef, fir, zi, zf = _rtfilt_args(kind, coef, d, aux, delay, fir, n, n_ch, zi, want_zf)
    nb = rtfilt_bands(kind)
    with device_scope(ctx) as dev:
        d_y = dev.alloc(nb * n_ch * n * 4, result=True)
        ctx.check(ctx.lib.ds_rtfilt_dev(ctx.handle, C.c_void_p(x_dev.ptr), n_ch, x_dev.ld, n, int(kind), _ptr(coef), int(d),
                                        int(aux), int(delay), None if fir is None else _ptr(fir),
                                        0 if fir is None else len(fir), None if zi is None else _ptr(zi),
                                        C.c_void_p(d_y.ptr), n, None if zf is None else _ptr(zf)), "ds_rtfilt_dev")
    y = [DevicePlanar(d_y, n_ch, n, n, b * n_ch * n * 4) for b in range(nb)] if nb > 1 else DevicePlanar(d_y, n_ch, n, n, 0)
    return (y, zf) if want_zf else y


def rtfir_filter(x, b, hist=None):
    """x (N, C) float64 through the direct float64 FIR sum y[n] = b[0] x[n] + sum b[i + 1] x[n - 1 - i] on the device.
    hist (C, order): the samples before the first one, oldest first (None: zeros).  -> y (N, C)."""
    xa = _host_samples(x)
    n, n_ch = xa.shape
    b = _rtfir_taps(b, n, n_ch)
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.float64)
        assert hist.shape == (n_ch, len(b) - 1), "hist must be (channels, order)"
    y = np.empty((n, n_ch), dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_rtfir(ctx.handle, _ptr(xa), n_ch, n, _ptr(b), len(b), None if hist is None else _ptr(hist),
                               _ptr(y)), "ds_rtfir")
    return y


def rtfir_filter_device(x_dev: DevicePlanar, b, hist=None):
    """rtfir_filter over device-resident samples (ds_rtfir_dev) -> a DevicePlanar; only the taps and the history cross."""
    ctx = x_dev.ctx
    n, n_ch = x_dev.n_samples, x_dev.n_ch
    b = _rtfir_taps(b, n, n_ch)
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.float64)
        assert hist.shape == (n_ch, len(b) - 1), "hist must be (channels, order)"
    with device_scope(ctx) as dev:
        d_y = dev.alloc(n_ch * n * 4, result=True)
        ctx.check(ctx.lib.ds_rtfir_dev(ctx.handle, C.c_void_p(x_dev.ptr), n_ch, x_dev.ld, n, _ptr(b), len(b),
                                       None if hist is None else _ptr(hist), C.c_void_p(d_y.ptr), n), "ds_rtfir_dev")
    return DevicePlanar(d_y, n_ch, n, n, 0)


# ---- sums over a pair of signals (ds_pair_moments, csrc/kernels_dist.hpp) -------------------------------------------
PAIR_SPAN = 4096  # samples one workgroup of the reduction sums (SPAN of the kernels)


def pair_moments(a, b, par=None) -> np.ndarray:
    """Per channel of a (N, Ca) and b (N, Cb) float64 (one side may have a single channel, paired with every channel of
    the other): sum (a - mu_a)^2, sum (b - mu_b)^2, sum a b, sum a, sum b, sum (alpha a - b)^2 as (C, 6) float64, in
    float64 and a fixed order on the device.  par (C, 3) holds alpha, mu_a, mu_b per channel (None: zeros)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    a = a[:, None] if a.ndim == 1 else a
    b = b[:, None] if b.ndim == 1 else b
    assert a.shape[0] == b.shape[0], "Length of signals do not match"
    n_ch = max(a.shape[1], b.shape[1])
    out = np.empty((n_ch, 6), dtype=np.float64)
    if par is not None:
        par = np.ascontiguousarray(par, dtype=np.float64)
        assert par.shape == (n_ch, 3), "par must be (channels, 3)"
    ctx = get_context()
    ctx.check(ctx.lib.ds_pair_moments(ctx.handle, _ptr(a), a.shape[1], _ptr(b), b.shape[1], a.shape[0],
                                      None if par is None else _ptr(par), _ptr(out)), "ds_pair_moments")
    return out


def pair_moments_device(a_dev: DevicePlanar, b_dev: DevicePlanar, par=None) -> np.ndarray:
    """pair_moments over device-resident fp32 planar signals (ds_pair_moments_dev): only the sums come down."""
    assert a_dev.n_samples == b_dev.n_samples, "Length of signals do not match"
    n_ch = max(a_dev.n_ch, b_dev.n_ch)
    out = np.empty((n_ch, 6), dtype=np.float64)
    if par is not None:
        par = np.ascontiguousarray(par, dtype=np.float64)
        assert par.shape == (n_ch, 3), "par must be (channels, 3)"
    ctx = a_dev.ctx
    ctx.check(ctx.lib.ds_pair_moments_dev(ctx.handle, C.c_void_p(a_dev.ptr), a_dev.n_ch, a_dev.ld, C.c_void_p(b_dev.ptr),
                                          b_dev.n_ch, b_dev.ld, a_dev.n_samples, None if par is None else _ptr(par),
                                          _ptr(out)), "ds_pair_moments_dev")
    return out


# ---- frequency-weighted segmental SNR (ds_fw_snr_seg, csrc/kernels_dist.hpp) ----------------------------------------
FW_SNR_CHUNK_FRAMES = 32  # frames transformed and reduced per pass over the workspace (a test lowers it)


def _complex_sos_stack(sos_list) -> np.ndarray:
    n_max = max(np.atleast_2d(s).shape[0] for s in sos_list)
    sos = np.tile(_IDENTITY_SECTION.astype(np.complex128), (len(sos_list), n_max, 1))
    for k, s in enumerate(sos_list):
        s = np.atleast_2d(np.asarray(s, dtype=np.complex128))
        sos[k, :s.shape[0]] = s
    return sos


def fw_snr_seg(x, xhat, sos_list, window, snr_range_db, gamma: float) -> np.ndarray:
    """The frequency-weighted segmental SNR of xhat (N, C) against x (N, C) or (N, 1), per channel of xhat, in one
    device call: both through the bank of complex sos filters (real parts), frames of len(window) samples at half
    overlap, one float64 transform per (frame, band, channel), the weighted log ratio reduced per frame, clipped
    and averaged.  x and xhat are float64 arrays or, both, DevicePlanar (fp32, resident)."""
    sos = _complex_sos_stack(sos_list)
    window = np.ascontiguousarray(window, dtype=np.float64)
    lo, hi = float(snr_range_db[0]), float(snr_range_db[1])
    tail = (_ptr(sos), sos.shape[0], sos.shape[1], _ptr(window), len(window), lo, hi, float(gamma), int(FW_SNR_CHUNK_FRAMES))
    if isinstance(x, DevicePlanar):
        assert isinstance(xhat, DevicePlanar) and x.n_samples == xhat.n_samples, "Signal lengths do not match"
        out = np.empty(xhat.n_ch, dtype=np.float64)
        ctx = x.ctx
        ctx.check(ctx.lib.ds_fw_snr_seg_dev(ctx.handle, C.c_void_p(x.ptr), x.n_ch, x.ld, C.c_void_p(xhat.ptr), xhat.n_ch,
                                            xhat.ld, x.n_samples, *tail, _ptr(out)), "ds_fw_snr_seg_dev")
        return out
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    xhat = np.ascontiguousarray(np.asarray(xhat, dtype=np.float64))
    x = x[:, None] if x.ndim == 1 else x
    xhat = xhat[:, None] if xhat.ndim == 1 else xhat
    assert x.shape[0] == xhat.shape[0], "Signal lengths do not match"
    out = np.empty(xhat.shape[1], dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_fw_snr_seg(ctx.handle, _ptr(x), x.shape[1], _ptr(xhat), xhat.shape[1], x.shape[0], *tail,
                                    _ptr(out)), "ds_fw_snr_seg")
    return out


def _ba_section(b, a) -> np.ndarray:
    """A ba filter of order <= 2 as one second-order section (lfilter normalises by a[0] as the section does)."""
    b = np.asarray(b, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    if max(len(b), len(a)) > 3:
        raise NotImplementedError("IIR ba filters of order > 2 are not run on the device (one second-order section "
                                  "at most); use FilterCoefficientsType.Sos or Zpk for higher orders")
    sec = np.zeros(6)
    sec[:len(b)] = b
    sec[3:3 + len(a)] = a
    return sec[None, :]


def _sosfilt(sos, x, zi=None):
    """scipy.signal.sosfilt(sos, x, axis=0[, zi]) for x (N, C) real on the device; zi (K, 2, C)."""
    if zi is None:
        return iir_sos_filter(x, [sos], DS_FB_PARALLEL)[0]
    y, zf = iir_sos_filter(x, [sos], DS_FB_PARALLEL, zi=np.asarray(zi)[None])
    return y[0], zf[0]


def _lfilter_iir(b, a, x, zi=None):
    """scipy.signal.lfilter(b, a, x, axis=0[, zi]) of an IIR filter of order <= 2 on the device; zi (order, C)."""
    sec = _ba_section(b, a)
    if zi is None:
        return _sosfilt(sec, x)
    zi = np.asarray(zi, dtype=np.float64)
    order = zi.shape[0]
    z2 = np.zeros((1, 2, zi.shape[1]))
    z2[0, :order] = zi
    y, zf = _sosfilt(sec, x, z2)
    return y, zf[0, :order]


def _odd_extension(x, padlen: int):
    if padlen == 0:
        return x
    left = 2 * x[:1] - x[padlen:0:-1]
    right = 2 * x[-1:] - x[-2:-(padlen + 2):-1]
    return np.concatenate([left, x, right])


def _filtfilt_sections(sos, x, padlen: int):
    """Forward-backward filtering as scipy's sosfiltfilt / filtfilt (padtype 'odd'): the odd extension by padlen
    samples, the steady-state initial state scaled by the first sample of each pass, two device calls -- the second
    over the reversed signal."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.shape[0] <= padlen:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {padlen}.")
    from scipy.signal import sosfilt_zi
    zi = sosfilt_zi(sos)[:, :, None]  # (K, 2, 1)
    ext = _odd_extension(x, padlen)
    y, _ = _sosfilt(sos, ext, zi * ext[0][None, None, :])
    yr = np.ascontiguousarray(y[::-1])
    y, _ = _sosfilt(sos, yr, zi * yr[0][None, None, :])
    y = y[::-1]
    return np.ascontiguousarray(y[padlen:y.shape[0] - padlen] if padlen > 0 else y)


def _sosfiltfilt(sos, x):
    """scipy.signal.sosfiltfilt(sos, x, axis=0) on the device."""
    sos = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    n_first = min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return _filtfilt_sections(sos, x, 3 * (2 * len(sos) + 1 - n_first))


def _filtfilt_iir(b, a, x):
    """scipy.signal.filtfilt(b, a, x, axis=0) of an IIR filter of order <= 2 on the device."""
    return _filtfilt_sections(_ba_section(b, a), x, 3 * max(len(a), len(b)))


# ---- fractional delays and their weighted sums (ds_delay_sum, csrc/kernels_delay.hpp) ------------------------------
DELAY_MAX_ORDER = 255  # the kernel's limit (DS_ERR_UNSUP above)


def _kaiser_window_beta(side_lobe_suppression_db: float) -> float:
    """standard/_standard_backend.py:259-287 (pyfar's Eq. 7.75 of Oppenheim & Schafer)."""
    a = np.abs(side_lobe_suppression_db)
    if a > 50:
        return 0.1102 * (a - 8.7)
    if a >= 21:
        return 0.5842 * (a - 21) ** 0.4 + 0.07886 * (a - 21)
    return 0.0


def _delay_split(delay_samples, order: int):
    """(integer_delay, fraction) of _fractional_delay_filter (standard/_standard_backend.py:430-492) for one delay in
    samples or an array of them: int() truncation, the fraction as delay - int(delay), and M_opt with np.round's
    half-to-even (a fraction of exactly 0.5 does not shift).  The same float64 operations as the reference, so an
    integer part never flips against it."""
    d = np.asarray(delay_samples, dtype=np.float64)
    d_int = np.trunc(d)
    frac = d - d_int
    if order % 2:
        m_opt = np.trunc(frac) - (order - 1) / 2
    else:
        m_opt = np.round(frac) - order / 2
    integer_delay = np.trunc(d_int + m_opt).astype(np.int64)
    if np.ndim(delay_samples) == 0:
        return int(integer_delay), float(frac)
    return integer_delay, frac


def _delay_terms(n_rows: int, n_terms: int, src, shift, frac, weight):
    src = np.ascontiguousarray(np.broadcast_to(np.asarray(src, dtype=np.int32), (n_rows, n_terms)))
    shift = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.int64), (n_rows, n_terms)))
    frac = np.ascontiguousarray(np.broadcast_to(np.asarray(frac, dtype=np.float64), (n_rows, n_terms)))
    weight = np.ascontiguousarray(np.broadcast_to(np.asarray(weight, dtype=np.float64), (n_rows, n_terms)))
    return src, shift, frac, weight


def delay_sum(x, src_len, src, shift, frac, weight, order: int, side_lobe_suppression_db: float, out_len: int,
              want_samples: bool = True, want_peaks: bool = False):
    """y[g, t] = sum_j weight[g,j] (h(frac[g,j]) * x_{src[g,j]})[t - shift[g,j]] for 0 <= t < out_len on the device
    (ds_delay_sum, float64).  x (N, sources) float64, source c read over its first src_len[c] samples; src is a
    (rows, terms) array, shift, frac and weight broadcast to it; frac < 0 marks a pass-through (a delay of exactly 0).  Returns
    (y (out_len, rows) float64 or None, peaks (rows,) float64 or None): peaks[g] = max_t |y[g, t]|."""
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if xa.ndim == 1:
        xa = xa[:, None]
    n_x, n_src = xa.shape
    n_rows, n_terms = np.shape(src)
    src, shift, frac, weight = _delay_terms(n_rows, n_terms, src, shift, frac, weight)
    lens = np.ascontiguousarray(np.broadcast_to(np.asarray(src_len, dtype=np.int64), (n_src,)))
    y = np.empty((int(out_len), n_rows), dtype=np.float64) if want_samples else None
    pk = np.zeros(n_rows, dtype=np.float64) if want_peaks else None
    ctx = get_context()
    ctx.check(ctx.lib.ds_delay_sum(ctx.handle, _ptr(xa), n_src, n_x, _ptr(lens), n_rows, n_terms, _ptr(src),
                                   _ptr(shift), _ptr(frac), _ptr(weight), int(order),
                                   float(_kaiser_window_beta(side_lobe_suppression_db)), int(out_len),
                                   None if y is None else _ptr(y), None if pk is None else _ptr(pk)), "ds_delay_sum")
    return y, pk


def delay_sum_device(x_dev: DevicePlanar, src_len, src, shift, frac, weight, order: int,
                     side_lobe_suppression_db: float, out_len: int) -> DevicePlanar:
    """delay_sum over device-resident planar float32 sources (ds_delay_sum_dev, float64 arithmetic) -> a DevicePlanar
    of the rows (rows, out_len).  Nothing comes down."""
    n_rows, n_terms = np.shape(src)
    src, shift, frac, weight = _delay_terms(n_rows, n_terms, src, shift, frac, weight)
    lens = np.ascontiguousarray(np.broadcast_to(np.asarray(src_len, dtype=np.int64), (x_dev.n_ch,)))
    ctx = x_dev.ctx
    out_len = int(out_len)
    with device_scope(ctx) as dev:
        d_y = dev.alloc(n_rows * out_len * 4, result=True)
        ctx.check(ctx.lib.ds_delay_sum_dev(ctx.handle, C.c_void_p(x_dev.ptr), x_dev.n_ch, x_dev.ld, _ptr(lens), n_rows,
                                           n_terms, _ptr(src), _ptr(shift), _ptr(frac), _ptr(weight), int(order),
                                           float(_kaiser_window_beta(side_lobe_suppression_db)), out_len,
                                           C.c_void_p(d_y.ptr), out_len, None), "ds_delay_sum_dev")
    return DevicePlanar(d_y, n_rows, out_len, out_len)


def stack_device(planars, lengths) -> DevicePlanar:
    """One-channel device signals -> one DevicePlanar (sources, max length): row j holds the first lengths[j] samples
    of planars[j], zeros after them.  Each row is a pass-through of ds_delay_sum_dev (a unit tap: exact)."""
    ctx = planars[0].ctx
    n_max = int(max(lengths))
    one = np.zeros((1, 1), dtype=np.int32)
    zero = np.zeros((1, 1), dtype=np.int64)
    through = np.full((1, 1), -1.0)
    w = np.ones((1, 1))
    with device_scope(ctx) as dev:
        buf = dev.alloc(len(planars) * n_max * 4, result=True)
        for j, (p, n) in enumerate(zip(planars, lengths)):
            lens = np.array([int(n)], dtype=np.int64)
            ctx.check(ctx.lib.ds_delay_sum_dev(ctx.handle, C.c_void_p(p.ptr), 1, p.ld, _ptr(lens), 1, 1, _ptr(one),
                                               _ptr(zero), _ptr(through), _ptr(w), 1, 0.0, n_max,
                                               C.c_void_p(buf.ptr + 4 * j * n_max), n_max, None), "ds_delay_sum_dev")
    return DevicePlanar(buf, len(planars), n_max, n_max)


# ---- continuous wavelet transform (ds_cwt, ds_cwt_dev, ds_cwt_squeeze_dev; csrc/kernels_cwt.hpp) ------------------
CWT_MAX_TAPS = 1 << 18  # the kernels' limit (DS_ERR_UNSUP above)


class DeviceScalogram:
    """A scalogram that stays in HBM: (frequencies, samples, channels) in `buf`, complex64 as ds_cwt_dev writes it or
    complex128 after ds_cwt_squeeze_dev.  What `transforms.cwt(on_device=True)` returns; `to_host()` gives the
    reference's complex128 array."""

    def __init__(self, buf: DeviceBuffer, shape, dtype):
        self.buf, self.shape, self.dtype = buf, tuple(int(v) for v in shape), np.dtype(dtype)

    def to_host(self) -> np.ndarray:
        if self.dtype == np.complex128:
            return self.buf.to_array(self.shape, np.complex128)
        return DeviceSTFT(self.buf, self.shape, False).to_host()

    def __deepcopy__(self, memo):
        return self


def _cwt_taps(waves):
    """The normalised float64 wavelets -> (tap lengths int64, all taps back to back as complex64).  Raises
    NotImplementedError for a wavelet beyond CWT_MAX_TAPS before anything reaches the device."""
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    if lens.size and lens.max() > CWT_MAX_TAPS:
        raise NotImplementedError(f"cwt: wavelets longer than {CWT_MAX_TAPS} taps are not built "
                                  f"(the longest here has {int(lens.max())})")
    if lens.size and lens.min() < 1:
        raise ValueError("cwt: a wavelet has no taps")
    taps = np.ascontiguousarray(np.concatenate([np.asarray(w).ravel() for w in waves]).astype(np.complex64))
    return lens, taps


def cwt_host(td: np.ndarray, waves) -> np.ndarray:
    """The scalogram (F, N, C) complex128 of td (N, C) float64 with the normalised wavelets (ds_cwt: fp32 kernels,
    the result widened on the way down)."""
    lens, taps = _cwt_taps(waves)
    xa = np.ascontiguousarray(np.asarray(td, dtype=np.float64))
    n, n_ch = xa.shape
    out = np.empty((len(waves), n, n_ch), dtype=np.complex128)
    ctx = get_context()
    ctx.check(ctx.lib.ds_cwt(ctx.handle, _ptr(xa), n_ch, n, len(waves), _ptr(lens), _ptr(taps), 1, _ptr(out)),
              "ds_cwt")
    return out


def cwt_device(x_dev: DevicePlanar, channels, waves) -> DeviceScalogram:
    """The scalogram of the channels `channels` of device-resident planar float32 samples (ds_cwt_dev), left in HBM
    as complex64 (F, N, len(channels))."""
    lens, taps = _cwt_taps(waves)
    ch = np.ascontiguousarray(np.asarray(channels, dtype=np.int32).ravel())
    n = x_dev.n_samples
    ctx = x_dev.ctx
    with device_scope(ctx) as dev:
        buf = dev.alloc(max(8 * len(waves) * n * len(ch), 8), result=True)
        ctx.check(ctx.lib.ds_cwt_dev(ctx.handle, C.c_void_p(x_dev.ptr), x_dev.n_ch, x_dev.ld, n, _ptr(ch), len(ch),
                                     len(waves), _ptr(lens), _ptr(taps), C.c_void_p(buf.ptr)), "ds_cwt_dev")
    return DeviceScalogram(buf, (len(waves), n, len(ch)), np.complex64)


def cwt_squeeze_device(scal: DeviceScalogram, freqs, fs, delta_w: float = 0.05,
                       apply_frequency_normalization: bool = False) -> DeviceScalogram:
    """_squeeze_scalogram (transforms/_transforms.py:227-301) of a complex64 device scalogram (ds_cwt_squeeze_dev,
    float64 arithmetic) -> a complex128 DeviceScalogram.  The thresholds and normalisations are the reference's numpy
    expressions."""
    assert scal.dtype == np.complex64
    n_f, n, n_ch = scal.shape
    freqs = np.ascontiguousarray(np.asarray(freqs, dtype=np.float64))
    delta_f = np.ascontiguousarray(delta_w * freqs)
    norm = None
    if apply_frequency_normalization:
        norm = 1 / (freqs / fs)
        norm **= -3 / 2
        norm = np.ascontiguousarray(norm)
    ctx = scal.buf.ctx
    with device_scope(ctx) as dev:
        buf = dev.alloc(max(16 * n_f * n * n_ch, 16), result=True)
        ctx.check(ctx.lib.ds_cwt_squeeze_dev(ctx.handle, C.c_void_p(scal.buf.ptr), n_f, n, n_ch, _ptr(freqs),
                                             _ptr(delta_f), None if norm is None else _ptr(norm), float(fs),
                                             C.c_void_p(buf.ptr)), "ds_cwt_squeeze_dev")
    return DeviceScalogram(buf, scal.shape, np.complex128)


# ---- fractional-octave smoothing (ds_octave_smooth, ds_octave_smooth_complex; csrc/kernels_smooth.hpp) ------------
SMOOTH_MAX_WORK = 1e13  # bins x window x channels of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)


def _smooth_guard(n_bins: int, n_window: int, n_ch: int) -> None:
    """NotImplementedError for a call beyond the direct summation's work bound, before anything reaches the device."""
    if float(n_bins) * float(n_window) * float(n_ch) > SMOOTH_MAX_WORK:
        raise NotImplementedError(f"fractional-octave smoothing of {n_bins} bins x {n_ch} channels with a window of "
                                  f"{n_window} taps is beyond the device kernel's work bound ({SMOOTH_MAX_WORK:.0e} "
                                  "multiply-adds per call)")


def _smooth_axis(n_bins: int, bin_spacing_octaves):
    """(k_log or None, beta) of helpers/smoothing.py:55-67: numpy's own values of N ** (arange(N) / (N - 1)) -- the
    last one is exactly N, which keeps the last linear bin an interpolation."""
    if bin_spacing_octaves is not None:
        return None, bin_spacing_octaves
    if n_bins < 2:
        raise ValueError("fractional-octave smoothing of linearly spaced bins needs at least two bins")
    k_log = n_bins ** (np.arange(n_bins, dtype=np.float64) / (n_bins - 1))
    return k_log, np.log2(k_log[1])


def _smooth_window_length(num_fractions, beta) -> int:
    n_window = int(1 / (num_fractions * beta) + 0.5)  # round
    return n_window + 1 - n_window % 2                # odd: the delay is a whole number of bins


def _smooth_window(n_window: int, window_type, window_vec) -> np.ndarray:
    """The window of helpers/smoothing.py:74-98 (scipy on the host: n_window values) with the reference's two
    assertions and its gaussian alpha -> sigma rule.  A caller's vector is copied, not normalised in place."""
    if window_type is not None:
        assert window_vec is None, "When window type is passed, no window vector should be added"
        if "gauss" in window_type[0]:
            window_type = ("gaussian", (n_window - 1) / (2 * window_type[1]))
        return np.ascontiguousarray(get_window(window_type, n_window, fftbins=False), dtype=np.float64)
    assert window_vec is not None, "When using a window as a vector, window type should be None"
    return np.array(window_vec, dtype=np.float64).ravel()


def fractional_octave_smoothing(vector, bin_spacing_octaves=None, num_fractions=3, window_type="hann",
                                window_vec=None, clip_values: bool = False):
    """_fractional_octave_smoothing (helpers/smoothing.py:9-129) along the first axis of a real (N,) or (N, C) array,
    on the device in float64: PCHIP to a logarithmic axis (linear bins, bin_spacing_octaves None), an edge-padded
    convolution with the unit-sum window, linear interpolation back, optional clip at 0.

    The reference pads by the odd window length it derives from the spacing even when the caller hands in a window
    vector of another length L, and so returns N + n_window - L points for logarithmic bins (and fails to interpolate
    back for linear ones): reproduced, the padding of that corner made on the host."""
    vector = np.asarray(vector, dtype=np.float64)
    assert vector.ndim in (1, 2), "the vector to smooth is (bins,) or (bins, channels)"
    one_dim = vector.ndim == 1
    v = np.ascontiguousarray(vector[:, None] if one_dim else vector)
    n_bins, n_ch = v.shape
    k_log, beta = _smooth_axis(n_bins, bin_spacing_octaves)
    n_window = _smooth_window_length(num_fractions, beta)
    window = _smooth_window(n_window, window_type, window_vec)
    crop = None
    if len(window) != n_window:
        if k_log is not None:
            raise ValueError(f"a window vector of {len(window)} values on linearly spaced bins: the reference pads for "
                             f"{n_window} and cannot interpolate its {n_bins + n_window - len(window)} points back")
        if n_bins + n_window - len(window) < 1:
            raise ValueError("the window vector is longer than the padded data")
        # pad for n_window as the reference does; the entry's own (clamped) padding then never shows in the crop
        v = np.ascontiguousarray(np.pad(v, ((n_window // 2, n_window // 2), (0, 0)), mode="edge"))
        crop = (len(window) // 2, n_bins + n_window - len(window))
        n_bins = v.shape[0]
    _smooth_guard(n_bins, len(window), n_ch)
    out = np.empty_like(v)
    ctx = get_context()
    ctx.check(ctx.lib.ds_octave_smooth(ctx.handle, _ptr(v), n_bins, n_ch, None if k_log is None else _ptr(k_log),
                                       _ptr(window), len(window), int(bool(clip_values)), _ptr(out)), "ds_octave_smooth")
    if crop is not None:
        out = out[crop[0]:crop[0] + crop[1]].copy()
    return out.squeeze() if one_dim else out


def smooth_complex_spectrum(spectrum, num_fractions, bin_spacing_octaves=None, window_type="hann",
                            clip_magnitude: bool = False):
    """A complex (N, C) spectrum smoothed as the reference's callers do it (classes/signal.py:913-928, classes/
    spectrum.py:859-868): |z| (clipped at 0 if clip_magnitude) and np.unwrap(np.angle(z), axis=0) through
    fractional_octave_smoothing, recombined as mag * exp(1j * phase) -- one upload, one download
    (ds_octave_smooth_complex), float64 / complex128."""
    z = np.ascontiguousarray(spectrum, dtype=np.complex128)
    assert z.ndim == 2, "the spectrum is (bins, channels)"
    n_bins, n_ch = z.shape
    k_log, beta = _smooth_axis(n_bins, bin_spacing_octaves)
    n_window = _smooth_window_length(num_fractions, beta)
    window = _smooth_window(n_window, window_type, None)
    _smooth_guard(n_bins, n_window, 2 * n_ch)
    out = np.empty_like(z)
    ctx = get_context()
    ctx.check(ctx.lib.ds_octave_smooth_complex(ctx.handle, _ptr(z), n_bins, n_ch, None if k_log is None else _ptr(k_log),
                                               _ptr(window), n_window, int(bool(clip_magnitude)), _ptr(out)),
              "ds_octave_smooth_complex")
    return out


# ---- direct sums (ds_dft, ds_dft_dev, ds_complex_smooth; csrc/kernels_direct.hpp) ---------------------------------
# terms of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
DFT_MAX_WORK = 1e12           # frequencies x samples x channels of the plain DFT
DFT_WINDOWED_MAX_WORK = 2e10  # kept window terms of the windowed DFT
CSMOOTH_MAX_WORK = 2e11       # band lengths x channels of complex smoothing
DFT_MIN_WEIGHT_LOG2 = -70.0   # window terms below 2^-70 are skipped
SMOOTHING_DOMAINS = ("RealImaginary", "PowerPhase", "MagnitudePhase", "Power", "Magnitude", "EquivalentComplex")


def _dft_guard(terms: float, windowed: bool = False) -> None:
    """NotImplementedError for a direct DFT beyond the work bound, before anything reaches the device."""
    bound = DFT_WINDOWED_MAX_WORK if windowed else DFT_MAX_WORK
    if float(terms) > bound:
        raise NotImplementedError(f"a direct DFT of {float(terms):.3g} terms is beyond the device kernel's work bound "
                                  f"({bound:.0e} terms per call)")


def _csmooth_guard(terms: float) -> None:
    if float(terms) > CSMOOTH_MAX_WORK:
        raise NotImplementedError(f"complex smoothing of {float(terms):.3g} band terms is beyond the device kernel's "
                                  f"work bound ({CSMOOTH_MAX_WORK:.0e} terms per call)")


def _windowed_kept_distance(alpha, half: float, n_samples: int, min_weight_log2: float = DFT_MIN_WEIGHT_LOG2):
    """Per bin, the largest distance from the peak whose weight exp(-alpha (d / half)^2 / 2) reaches
    2^min_weight_log2 (the rule of ds_dft), at most n_samples."""
    with np.errstate(divide="ignore", invalid="ignore"):
        d = half * np.sqrt(-2.0 * np.log(2.0) * min_weight_log2 / np.asarray(alpha, dtype=np.float64))
    return np.where(d < n_samples, d, n_samples).astype(np.int64)


def _windowed_kept_terms(alpha, peak, half: float, n_samples: int,
                         min_weight_log2: float = DFT_MIN_WEIGHT_LOG2) -> float:
    d = _windowed_kept_distance(alpha, half, n_samples, min_weight_log2)[:, None]
    pk = np.asarray(peak, dtype=np.int64)[None, :]
    return float((np.minimum(n_samples, pk + d + 1) - np.maximum(0, pk - d)).sum())


def _dft_call(samples, freqs_hz, fs, alpha, peak, half, min_weight_log2):
    freqs = np.ascontiguousarray(freqs_hz, dtype=np.float64).ravel()
    resident = isinstance(samples, DevicePlanar)
    if resident:
        n, n_ch = samples.n_samples, samples.n_ch
    else:
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        assert samples.ndim == 2, "the samples are (samples, channels)"
        n, n_ch = samples.shape
    windowed = alpha is not None
    if windowed:
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).ravel()
        peak = np.ascontiguousarray(peak, dtype=np.int64).ravel()
        assert len(alpha) == len(freqs) and len(peak) == n_ch, "alpha is per frequency, peak per channel"
        _dft_guard(_windowed_kept_terms(alpha, peak, half, n, min_weight_log2), True)
    else:
        _dft_guard(float(len(freqs)) * n * n_ch)
    out = np.empty((len(freqs), n_ch), dtype=np.complex128)
    tail = (_ptr(freqs), len(freqs), float(fs), _ptr(alpha) if windowed else None, _ptr(peak) if windowed else None,
            float(half), float(min_weight_log2), _ptr(out))
    if resident:
        ctx = samples.ctx
        ctx.check(ctx.lib.ds_dft_dev(ctx.handle, C.c_void_p(samples.ptr), n_ch, samples.ld, n, *tail), "ds_dft_dev")
    else:
        ctx = get_context()
        ctx.check(ctx.lib.ds_dft(ctx.handle, _ptr(samples), n, n_ch, *tail), "ds_dft")
    return out


def dft(time_data, freqs_hz, fs):
    """X[k, c] = sum_n x[n, c] exp(-2 pi i f_k n / fs) at any frequencies (transforms/_transforms.py:_dft_backend),
    float64 on the device.  time_data: (samples, channels) float64 on the host or a `DevicePlanar`."""
    return _dft_call(time_data, freqs_hz, fs, None, None, 1.0, DFT_MIN_WEIGHT_LOG2)


def windowed_dft(time_data, freqs_hz, fs, alpha, peak, half, min_weight_log2: float = DFT_MIN_WEIGHT_LOG2):
    """The same sum under the Gaussian window exp(alpha_k * -0.5 ((n - peak_c) / half)^2) per bin and channel
    (transfer_functions/_transfer_functions.py:_fdw_backend).  Terms whose weight is below 2^min_weight_log2 are
    skipped; -inf keeps all of them."""
    return _dft_call(time_data, freqs_hz, fs, alpha, peak, half, min_weight_log2)


def _csmooth_indices(freqs_hz, octave_fraction):
    """(ind_low, ind_high, window_length, pass) per bin in the statements of _complex_smoothing_backend
    (transfer_functions/_transfer_functions.py:519-541), int32: the band clipped to the spectrum, its unclipped
    length, and the bins the reference copies."""
    f = np.asarray(freqs_hz, dtype=np.float64)
    delta_f = f[1] - f[0]
    factor = 2.0 ** (1.0 / octave_fraction / 2.0)
    i = np.arange(len(f), dtype=np.int64)
    ind_low = i - ((f - f / factor) / delta_f + 0.5).astype(np.int64)        # int(x + 0.5) of x >= 0
    ind_high = i + ((f * factor - f) / delta_f + 0.5).astype(np.int64) + 1
    window_length = ind_high - ind_low
    ind_low = np.maximum(ind_low, 0)
    ind_high = np.minimum(ind_high, len(f))
    passed = ind_low + 2 >= ind_high
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (ind_low, ind_high, window_length, passed))


def complex_smoothing(spectrum, freqs_hz, octave_fraction, domain, window_values):
    """_complex_smoothing_backend and the domain transforms of transfer_functions.complex_smoothing
    (transfer_functions.py:1827-1875) on a float64 / complex128 (bins, channels) spectrum over linearly spaced
    frequencies: one upload, one download (ds_complex_smooth).  domain: a name of SMOOTHING_DOMAINS (or an enum
    member carrying one); window_values: the window prototype on linspace(-1, 1, len(window_values))."""
    name = getattr(domain, "name", domain)
    if name not in SMOOTHING_DOMAINS:
        raise ValueError("Invalid smoothing domain")
    assert octave_fraction > 0.0, "Octave fraction must be greater than 0"
    z = np.ascontiguousarray(spectrum, dtype=np.complex128)
    assert z.ndim == 2, "the spectrum is (bins, channels)"
    n_bins, n_ch = z.shape
    freqs = np.asarray(freqs_hz, dtype=np.float64)
    assert len(freqs) == n_bins and n_bins >= 2, "one frequency per bin, at least two bins"
    lo, hi, wlen, passed = _csmooth_indices(freqs, octave_fraction)
    _csmooth_guard(float((hi - lo)[passed == 0].sum()) * n_ch)
    wy = np.ascontiguousarray(window_values, dtype=np.float64)
    wx = np.linspace(-1.0, 1.0, len(wy), endpoint=True)
    out = np.empty_like(z)
    ctx = get_context()
    ctx.check(ctx.lib.ds_complex_smooth(ctx.handle, _ptr(z), n_bins, n_ch, _ptr(lo), _ptr(hi), _ptr(wlen), _ptr(passed),
                                        _ptr(wx), _ptr(wy), len(wy), SMOOTHING_DOMAINS.index(name), _ptr(out)),
              "ds_complex_smooth")
    return out


# ---- complex128 transforms of any length and what is built on them (csrc/kernels_fft64.hpp) -----------------------
# transform lengths of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
FFT64_MAX_POW2 = 1 << 22  # powers of two: the four-step route
FFT64_MAX_ANY = 1 << 21   # every other length: Bluestein on a power of two >= 2 n - 1
MIN_PHASE_OUTPUTS = ("spectrum", "phase", "ir", "group_delay")  # DS_MIN_PHASE_* of the header


def _fft64_guard(n: int) -> None:
    """NotImplementedError for a transform length beyond the kernels' bounds, before anything reaches the device."""
    n = int(n)
    pow2 = n > 0 and n & (n - 1) == 0
    if n > (FFT64_MAX_POW2 if pow2 else FFT64_MAX_ANY):
        raise NotImplementedError(f"a float64 transform of {n} points is beyond the device kernels' bounds "
                                  f"(powers of two up to {FFT64_MAX_POW2}, other lengths up to {FFT64_MAX_ANY})")


def _host_columns(a, dtype):
    if isinstance(a, DevicePlanar):
        raise NotImplementedError("device-resident (fp32 planar) inputs are not built for the float64 transforms: "
                                  "pass the host float64 array")
    a = np.ascontiguousarray(a, dtype=dtype)
    assert a.ndim == 2, "the array is (rows, channels)"
    return a


def fft_c128(data, n: int | None = None, inverse: bool = False):
    """numpy.fft.fft / ifft(data, n, axis=0) of a real or complex (rows, channels) host array on the device, complex128.
    Any n >= 1 within the bounds; the input is zero-padded or cropped to n rows."""
    cplx = np.iscomplexobj(data)
    a = _host_columns(data, np.complex128 if cplx else np.float64)
    n = a.shape[0] if n is None else int(n)
    if n < 1 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("fft_c128: empty input or n < 1")
    _fft64_guard(n)
    out = np.empty((n, a.shape[1]), dtype=np.complex128)
    ctx = get_context()
    ctx.check(ctx.lib.ds_fft_c128(ctx.handle, _ptr(a), int(cplx), a.shape[0], a.shape[1], n, int(bool(inverse)),
                                  _ptr(out)), "ds_fft_c128")
    return out


def hilbert(time_data):
    """The analytic signal of a real (samples, channels) array (transforms.hilbert), complex128."""
    a = _host_columns(time_data, np.float64)
    _fft64_guard(a.shape[0])
    out = np.empty(a.shape, dtype=np.complex128)
    ctx = get_context()
    ctx.check(ctx.lib.ds_hilbert(ctx.handle, _ptr(a), a.shape[0], a.shape[1], _ptr(out)), "ds_hilbert")
    return out


def cepstrum(time_data, complex: bool = True):
    """ifft(log(fft(x))) -- the principal logarithm -- or, complex False, ifft(log|fft(x)|); complex128 either way, as
    numpy returns it (transforms.cepstrum)."""
    a = _host_columns(time_data, np.float64)
    _fft64_guard(a.shape[0])
    out = np.empty(a.shape, dtype=np.complex128)
    ctx = get_context()
    ctx.check(ctx.lib.ds_cepstrum(ctx.handle, _ptr(a), a.shape[0], a.shape[1], int(bool(complex)), _ptr(out)),
              "ds_cepstrum")
    return out


def from_complex_cepstrum(cepstrum):
    """real(ifft(exp(fft(cepstrum)))) of a (quefrency, channels) array (transforms.from_complex_cepstrum), float64."""
    a = _host_columns(cepstrum, np.complex128)
    _fft64_guard(a.shape[0])
    out = np.empty(a.shape, dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_from_cepstrum(ctx.handle, _ptr(a), a.shape[0], a.shape[1], _ptr(out)), "ds_from_cepstrum")
    return out


def min_phase_fft_length(n_samples: int, padding_factor: int) -> int:
    """The transform length of helpers/minimum_phase.py:30-32."""
    from scipy.fft import next_fast_len
    return int(next_fast_len(max(int(n_samples) * int(padding_factor), int(n_samples))))


def min_phase(time_data, n_fft: int, output: str, n_out: int = 0, delta_f: float = 1.0):
    """The real-cepstrum minimum-phase equivalent of a real (samples, channels) array zero-padded to n_fft rows
    (helpers/minimum_phase.py:8-79), one upload and one download.  output: "spectrum" (n_fft, C) complex128; "phase"
    of the bins 0 .. n_fft // 2; "ir", the first n_out rows; "group_delay", -gradient(unwrap(phase)) / (2 pi delta_f)."""
    a = _host_columns(time_data, np.float64)
    n_fft = int(n_fft)
    _fft64_guard(n_fft)
    kind = MIN_PHASE_OUTPUTS.index(output)
    rows = {"spectrum": n_fft, "ir": int(n_out)}.get(output, n_fft // 2 + 1)
    out = np.empty((rows, a.shape[1]), dtype=np.complex128 if output == "spectrum" else np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_min_phase(ctx.handle, _ptr(a), a.shape[0], a.shape[1], n_fft, kind, int(n_out), float(delta_f),
                                   _ptr(out)), "ds_min_phase")
    return out


def group_delay_phase(time_data, delta_f: float, latency_samples=None, fs: float = 0.0):
    """-gradient(unwrap(angle(rfft(x)))) / (2 pi delta_f) on the n // 2 + 1 bins of a real (samples, channels) array
    (_group_delay_direct of the reference on the spectrum's phase), float64.  With latency_samples (one per channel)
    the phase is wrap(angle + 2 pi f latency / fs) before the unwrap (_remove_ir_latency_from_phase,
    helpers/latency.py:152-181)."""
    a = _host_columns(time_data, np.float64)
    _fft64_guard(a.shape[0])
    out = np.empty((a.shape[0] // 2 + 1, a.shape[1]), dtype=np.float64)
    ctx = get_context()
    if latency_samples is None:
        ctx.check(ctx.lib.ds_group_delay_phase(ctx.handle, _ptr(a), a.shape[0], a.shape[1], float(delta_f), _ptr(out)),
                  "ds_group_delay_phase")
        return out
    lat = np.ascontiguousarray(latency_samples, dtype=np.float64)
    assert lat.shape == (a.shape[1],), "one latency per channel"
    ctx.check(ctx.lib.ds_group_delay_phase_lat(ctx.handle, _ptr(a), a.shape[0], a.shape[1], float(delta_f), _ptr(lat),
                                               float(fs), _ptr(out)), "ds_group_delay_phase_lat")
    return out


# ---- latency estimation by cross-correlation (csrc/kernels_latency.hpp) ---------------------------------------------
# bounds of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
LATENCY_MAX_ROWS = FFT64_MAX_POW2  # rows of the full correlation, len(td1) + len(td2) - 1
LATENCY_MAX_COLUMNS = 65535        # channels of both signals together
LATENCY_MAX_POINTS = 16            # polynomial_points
LATENCY_WINDOW_MARGIN = 200        # rows kept before the first and after the last peak (helpers/latency.py:34-38)


def _finite_columns(a, name: str) -> np.ndarray:
    a = _host_columns(a, np.float64)
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name}: empty array")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds non-finite samples: the peak of a correlation with NaN or infinity in it is not "
                         "defined here (numpy's argmax returns the first NaN)")
    return a


def latency_peaks(td1, td2, polynomial_points: int, pearson: bool = False, reverse_pairs: bool = False):
    """The peaks of scipy's full-mode correlate(td2[:, c], td1[:, c]) per channel c of td1 (samples, channels); td2 has
    as many channels or one, which then serves every pair.  The correlation is formed and searched on the device and
    never comes down.  td2 None: the peaks of |td1| itself.  Returns (peaks, window, near, r):
      peaks   (C,) int64, the row of the largest magnitude, the first among equal ones; the lag is len(td1) - 1 - peak
      window  (lo, M), the rows [lo, lo + M) shared by all channels that the Hilbert transform was taken of, and
      near    (C, 2 p + 2), imag(hilbert(window))[d - p .. d + p + 1] around each channel's row d = peak - lo, NaN for
              rows outside the window -- both None with polynomial_points p = 0
      r       with pearson: (C, 3) Pearson's r of the pair (td2 channel, td1 channel) at the integer lags
              len(td1) - 1 - peak + (-1, 0, 1), (C, 1) at the lag itself when p = 0; reverse_pairs takes the peak of
              channel C - 1 - c for pair c (the reference's order with in2 None, standard.latency).
    Non-finite samples raise ValueError before anything is uploaded."""
    p = int(polynomial_points)
    if p < 0:
        raise ValueError("polynomial_points must be at least 0")
    a = _finite_columns(td1, "td1")
    b = None if td2 is None else _finite_columns(td2, "td2")
    if b is not None and b.shape[1] not in (1, a.shape[1]):
        raise ValueError("td2 needs as many channels as td1, or one")
    if b is None and pearson:
        raise ValueError("correlation coefficients need a second signal")
    rows = a.shape[0] + (b.shape[0] - 1 if b is not None else 0)
    cols = a.shape[1] + (b.shape[1] if b is not None else 0)
    if rows > LATENCY_MAX_ROWS or cols > LATENCY_MAX_COLUMNS or p > LATENCY_MAX_POINTS:
        raise NotImplementedError(f"a correlation of {rows} rows, {cols} channels and {p} polynomial points is beyond the "
                                  f"device kernels' bounds ({LATENCY_MAX_ROWS} rows, {LATENCY_MAX_COLUMNS} channels of both "
                                  f"signals together, {LATENCY_MAX_POINTS} points)")
    n_ch = a.shape[1]
    peaks = np.empty(n_ch, dtype=np.int64)
    window = np.zeros(2, dtype=np.int64)
    near = np.empty((n_ch, 2 * p + 2), dtype=np.float64) if p > 0 else None
    r = np.empty((n_ch, 3 if p > 0 else 1), dtype=np.float64) if pearson else None
    ctx = get_context()
    ctx.check(ctx.lib.ds_latency(ctx.handle, _ptr(a), a.shape[0], n_ch, None if b is None else _ptr(b),
                                 0 if b is None else b.shape[0], 0 if b is None else b.shape[1], p, int(bool(reverse_pairs)),
                                 _ptr(peaks), _ptr(window) if p > 0 else None, None if near is None else _ptr(near),
                                 None if r is None else _ptr(r)), "ds_latency")
    return peaks, ((int(window[0]), int(window[1])) if p > 0 else None), near, r


def lag_pearson(time_data, other_time_data, lags, columns=None, other_columns=None) -> np.ndarray:
    """Pearson's r per entry j between column columns[j] of time_data and column other_columns[j] of other_time_data
    (default: j, or 0 for a one-channel time_data) at the integer lag lags[j], as _get_correlation_of_latencies forms it
    (helpers/latency.py:218-265): a lag > 0 drops the first lag samples of the other signal, otherwise the first -lag
    of time_data; both are cut to the shorter.  NaN where fewer than two samples are left or a channel is constant."""
    t = _finite_columns(time_data, "time_data")
    o = _finite_columns(other_time_data, "other_time_data")
    lags = np.atleast_1d(np.asarray(lags)).astype(np.int64)
    n = len(lags)
    ct = (np.zeros(n, dtype=np.int64) if t.shape[1] == 1 else np.arange(n)) if columns is None else np.asarray(columns)
    co = np.arange(n) if other_columns is None else np.asarray(other_columns)
    rows = np.ascontiguousarray(np.stack([ct, co, lags], axis=1), dtype=np.int64)
    out = np.empty(n, dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_lag_pearson(ctx.handle, _ptr(t), t.shape[0], t.shape[1], _ptr(o), o.shape[0], o.shape[1], _ptr(rows),
                                     n, _ptr(out)), "ds_lag_pearson")
    return out


_LATENCY_FAILED = "Fractional latency detection failed for channel {}. Integer latency is returned"


def _fractional_index(h_near, p: int, d: int, ch: int = 0) -> float:
    """The sub-sample peak row of one channel from the 2 p + 2 values h_near = imag(hilbert)[d - p .. d + p + 1] the
    device returned, in the branches of _get_fractional_impulse_peak_index (helpers/latency.py:46-97): move the row one
    back when the two values at d and d + 1 have the same sign; if they still have, warn and return the integer row;
    otherwise fit 2 p points with a polynomial of degree 2 p - 1 and take its first real root in [0, 1]; without one,
    warn and return the integer row.  A value that is needed but NaN lies outside the array (the peak is within p + 1
    rows of one of its ends): ValueError, no guess."""
    from warnings import warn
    h = np.asarray(h_near, dtype=np.float64)
    assert h.shape == (2 * p + 2,), "2 p + 2 values around the peak"

    def rows(first: int, count: int) -> np.ndarray:  # the values at rows d + first .. d + first + count - 1
        v = h[first + p:first + p + count]
        if first + p < 0 or len(v) != count or np.isnan(v).any():
            raise ValueError(f"channel {ch}: the peak lies within {p + 1} rows of an end of the array; its neighbourhood "
                             "is not there to fit")
        return v

    selection = rows(0, 2)
    move_back = int(selection[0] * selection[1] > 0)
    d = int(d) - move_back
    selection = rows(-move_back, 2)
    if selection[0] * selection[1] > 0:
        warn(_LATENCY_FAILED.format(ch))
        return float(d + move_back)
    pol = np.polyfit(np.arange(-p + 1, p + 1), rows(-move_back - p + 1, 2 * p), deg=2 * p - 1)
    roots = np.roots(pol)
    roots = roots[(roots == roots.real) & (roots <= 1) & (roots >= 0)].real
    if len(roots) == 0:
        warn(_LATENCY_FAILED.format(ch))
        return float(d + move_back)
    return d + roots[0]


def fractional_peak_rows(peaks, window, near, p: int) -> np.ndarray:
    """latency_peaks' results as the rows _get_fractional_impulse_peak_index returns, (C,) float64."""
    lo = window[0]
    return np.array([_fractional_index(near[c], p, int(peaks[c]) - lo, c) for c in range(len(peaks))], dtype=np.float64) + lo


# ---- linear prediction per (frame, channel) pair (csrc/kernels_lpc.hpp) ---------------------------------------------
# bounds of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
LPC_MAX_WINDOW = 8192   # a pair's frame (Burg: its two error rows) lives in the LDS of one workgroup
LPC_MAX_ORDER = 255     # order + 1 coefficients, a lane of the workgroup each
LPC_MAX_PAIRS = (1 << 31) - 1  # one workgroup per (frame, channel) pair
LPC_MAX_WORK = 1e11     # frames x channels x window x (order + 1)
LPC_METHODS = ("yule_walker", "burg")  # DS_LPC_* of the header


def _lpc_frames(n_samples: int, hop: int) -> int:
    """ceil(N / hop): _get_framed_signal(..., keep_last_frames=True) of the reference, the rule of _welch_framing."""
    return -(-int(n_samples) // int(hop))


def _lpc_guard(n_frames: int, n_ch: int, window_length: int, order: int) -> None:
    """ValueError for an order or a window the estimators cannot take, NotImplementedError beyond the kernels' bounds;
    before anything reaches the device."""
    L, order, pairs = int(window_length), int(order), int(n_frames) * int(n_ch)
    if order < 1:
        raise ValueError("lpc: the order must be at least 1")
    if order >= L:
        raise ValueError(f"lpc: the order ({order}) must be below the window length ({L})")
    if L > LPC_MAX_WINDOW or order > LPC_MAX_ORDER or pairs > LPC_MAX_PAIRS:
        raise NotImplementedError(f"linear prediction with a window of {L} samples, order {order} and {pairs} (frame, "
                                  f"channel) pairs is beyond the device kernels' bounds (windows up to {LPC_MAX_WINDOW}, "
                                  f"orders up to {LPC_MAX_ORDER}, {LPC_MAX_PAIRS} pairs)")
    work = float(pairs) * L * (order + 1)
    if work > LPC_MAX_WORK:
        raise NotImplementedError(f"linear prediction of {work:.3g} lag products is beyond the device kernels' work "
                                  f"bound ({LPC_MAX_WORK:.0e} = frames x channels x window x (order + 1) per call)")


def lpc(time_data, order: int, window, hop: int, method: str = "yule_walker"):
    """The AR coefficients a (order + 1, frames, channels), a[0] = 1, and the variances (frames, channels) of every
    windowed frame of (samples, channels) data -- float64 on the host or a `DevicePlanar` -- by Yule-Walker (biased
    autocorrelation, Levinson-Durbin; var = the final prediction error) or by Burg's method (var = the running
    denominator `den` of helpers/ar_estimation.py:200, as the reference returns it).  Frame f covers the samples
    f hop .. f hop + len(window) - 1, zeros past the end; there are ceil(samples / hop) frames.  A frame of zeros gives
    NaN (Yule-Walker) or [1, 0, ...] and 0 (Burg).  ValueError("Invalid prediction error: Singular Matrix") when the
    prediction error of any pair is <= 0 after any order, as in the reference."""
    window = np.ascontiguousarray(window, dtype=np.float64).ravel()
    L, hop, order, kind = len(window), int(hop), int(order), LPC_METHODS.index(method)
    if hop < 1:
        raise ValueError("lpc: the hop size must be at least 1")
    resident = isinstance(time_data, DevicePlanar)
    if resident:
        n, n_ch = time_data.n_samples, time_data.n_ch
    else:
        if np.iscomplexobj(time_data):
            raise ValueError("lpc: the samples must be real")
        assert np.ndim(time_data) == 2, "the samples are (samples, channels)"
        n, n_ch = np.shape(time_data)
    if n < 1 or n_ch < 1:
        raise ValueError("lpc: empty input")
    n_frames = _lpc_frames(n, hop)
    _lpc_guard(n_frames, n_ch, L, order)
    a = np.empty((order + 1, n_frames, n_ch), dtype=np.float64)
    var = np.empty((n_frames, n_ch), dtype=np.float64)
    singular = C.c_int(0)
    tail = (_ptr(window), L, hop, order, kind, _ptr(a), _ptr(var), C.byref(singular))
    if resident:
        ctx = time_data.ctx
        ctx.check(ctx.lib.ds_lpc_dev(ctx.handle, C.c_void_p(time_data.ptr), n_ch, time_data.ld, n, *tail), "ds_lpc_dev")
    else:
        x = np.ascontiguousarray(time_data, dtype=np.float64)
        ctx = get_context()
        ctx.check(ctx.lib.ds_lpc(ctx.handle, _ptr(x), n, n_ch, *tail), "ds_lpc")
    if singular.value:
        raise ValueError("Invalid prediction error: Singular Matrix")
    return a, var


def levinson_durbin(r):
    """_levison_durbin_recursion (helpers/ar_estimation.py:6-68) along axis 0 of an (order + 1, ...) autocorrelation, on
    the device: (a with a[0] = 1 in r's shape, the prediction errors in r.shape[1:]).  ValueError where the reference
    raises it: a prediction error <= 0 after any order."""
    r = np.asarray(r, dtype=np.float64)
    if r.ndim < 1 or r.shape[0] < 2 or r.size == 0:
        raise ValueError("levinson_durbin: needs the lags 0 .. order, order >= 1, along axis 0")
    order = r.shape[0] - 1
    if order > LPC_MAX_ORDER or r.size // r.shape[0] > LPC_MAX_PAIRS:
        raise NotImplementedError(f"a Levinson-Durbin recursion of order {order} is beyond the device kernel's bound "
                                  f"({LPC_MAX_ORDER})")
    cols = np.ascontiguousarray(r.reshape(order + 1, -1))
    a = np.empty_like(cols)
    var = np.empty(cols.shape[1], dtype=np.float64)
    singular = C.c_int(0)
    ctx = get_context()
    ctx.check(ctx.lib.ds_levinson(ctx.handle, _ptr(cols), order, cols.shape[1], _ptr(a), _ptr(var), C.byref(singular)),
              "ds_levinson")
    if singular.value:
        raise ValueError("Invalid prediction error: Singular Matrix")
    return a.reshape(r.shape), var.reshape(r.shape[1:])


def lpc_synthesize(a, sources, window, hop: int, n_out: int):
    """scipy's lfilter([1], a[:, f, c], sources[:, f, c]) from zero state for every frame and channel, then the
    overlap-add of _reconstruct_framed_signal (standard/_framed_signal_representation.py:70-137): frames times the
    window, added at hop spacing, over the envelope sum window^2 clipped below at 1e-4, padded or trimmed to n_out
    samples.  a: (order + 1, frames, channels); sources: (len(window), frames, channels); returns (n_out, channels)."""
    window = np.ascontiguousarray(window, dtype=np.float64).ravel()
    a = np.ascontiguousarray(a, dtype=np.float64)
    sources = np.ascontiguousarray(sources, dtype=np.float64)
    L, hop, n_out = len(window), int(hop), int(n_out)
    assert a.ndim == 3 and sources.ndim == 3, "a is (order + 1, frames, channels), sources (window, frames, channels)"
    order, n_frames, n_ch = a.shape[0] - 1, a.shape[1], a.shape[2]
    assert sources.shape == (L, n_frames, n_ch), "sources must be (len(window), frames, channels)"
    if hop < 1 or n_out < 1 or n_frames < 1 or n_ch < 1:
        raise ValueError("lpc_synthesize: needs hop >= 1, frames, channels and output samples")
    _lpc_guard(n_frames, n_ch, L, order)
    if n_out * n_ch > LPC_MAX_PAIRS * 256:
        raise NotImplementedError("lpc_synthesize: more output samples than one launch covers")
    y = np.empty((n_out, n_ch), dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_lpc_synth(ctx.handle, _ptr(a), _ptr(sources), _ptr(window), L, n_frames, n_ch, hop, order, n_out,
                                   _ptr(y)), "ds_lpc_synth")
    return y


# ---- the all-pass table of frequency warping and the Laguerre transform (csrc/kernels_warp.hpp) --------------------
# bounds of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
WARP_MAX_SIDE = 1 << 17      # input and output samples: the longest responses in practice
WARP_MAX_CHANNELS = 65536    # channel groups are the grid's second dimension
WARP_MAX_WORK = 1e12         # input samples x output samples x channel groups: two seconds at the measured rate
WARP_GROUP = 4               # channels a workgroup accumulates (G of csrc/warp_plan.hpp)


def _warp_check(n_in: int, n_out: int, n_ch: int) -> None:
    """ValueError for an empty table, NotImplementedError beyond the kernel's bounds; before anything reaches the device."""
    n_in, n_out, n_ch = int(n_in), int(n_out), int(n_ch)
    if n_in < 1 or n_out < 1 or n_ch < 1:
        raise ValueError("allpass_table: needs input samples, output samples and channels")
    if n_in > WARP_MAX_SIDE or n_out > WARP_MAX_SIDE or n_ch > WARP_MAX_CHANNELS:
        raise NotImplementedError(f"an all-pass table of {n_in} x {n_out} samples and {n_ch} channels is beyond the device "
                                  f"kernel's bounds ({WARP_MAX_SIDE} samples a side, {WARP_MAX_CHANNELS} channels)")
    work = float(n_in) * n_out * (-(-n_ch // WARP_GROUP))
    if work > WARP_MAX_WORK:
        raise NotImplementedError(f"an all-pass table of {work:.3g} cells is beyond the device kernel's work bound "
                                  f"({WARP_MAX_WORK:.0e} = input samples x output samples x groups of {WARP_GROUP} channels)")


def allpass_table(time_data, p: float, q: float, row0, col0):
    """out[j, ch] = sum_i c[i, j] x[i, ch] for the table c[i, j] = p c[i-1, j] + c[i-1, j-1] + q c[i, j-1] (i, j >= 1)
    with the first row `row0` (its length is the number of output samples) and the first column `col0` (one value per
    input sample; c[0, 0] = col0[0]).  x is (samples, channels) float64 on the host or a `DevicePlanar`; the table and
    the sums are float64 on the device, in a fixed order."""
    row0 = np.ascontiguousarray(row0, dtype=np.float64).ravel()
    col0 = np.ascontiguousarray(col0, dtype=np.float64).ravel()
    p, q = float(p), float(q)
    if not (np.isfinite(p) and np.isfinite(q)):
        raise ValueError("allpass_table: p and q must be finite")
    resident = isinstance(time_data, DevicePlanar)
    if resident:
        n_in, n_ch = time_data.n_samples, time_data.n_ch
    else:
        if np.iscomplexobj(time_data):
            raise ValueError("allpass_table: the samples must be real")
        assert np.ndim(time_data) == 2, "the samples are (samples, channels)"
        n_in, n_ch = np.shape(time_data)
    n_out = len(row0)
    _warp_check(n_in, n_out, n_ch)
    assert len(col0) == n_in, "col0 has a value per input sample"
    out = np.empty((n_out, n_ch), dtype=np.float64)
    tail = (p, q, _ptr(row0), _ptr(col0), n_out, _ptr(out))
    if resident:
        ctx = time_data.ctx
        ctx.check(ctx.lib.ds_allpass_table_dev(ctx.handle, C.c_void_p(time_data.ptr), n_ch, time_data.ld, n_in, *tail),
                  "ds_allpass_table_dev")
    else:
        x = np.ascontiguousarray(time_data, dtype=np.float64)
        ctx = get_context()
        ctx.check(ctx.lib.ds_allpass_table(ctx.handle, _ptr(x), n_in, n_ch, *tail), "ds_allpass_table")
    return out


def _running_powers(first: float, ratio: float, n: int) -> np.ndarray:
    """first, first ratio, first ratio^2, ...: running float64 products, as a first-order recursion makes them"""
    v = np.full(n, float(ratio))
    v[0] = float(first)
    return np.multiply.accumulate(v)


def _table_length(time_data) -> int:
    return time_data.n_samples if isinstance(time_data, DevicePlanar) else np.shape(time_data)[0]


def warp_time_series(time_data, warping_factor: float):
    """_warp_time_series of the reference (transforms/_transforms.py:386-428): sample i of every channel times the
    all-pass (z^-1 - lambda) / (1 - lambda z^-1) applied i times to a unit pulse, summed over i.  (samples, channels)
    float64 on the host or a `DevicePlanar` -> (samples, channels) float64."""
    lam, n = float(warping_factor), _table_length(time_data)
    row0 = np.zeros(n)
    row0[:1] = 1.0
    return allpass_table(time_data, -lam, lam, row0, _running_powers(1.0, -lam, n))


def laguerre_transform(time_data, warping_factor: float):
    """The discrete Laguerre transform of the reference (transforms/transforms.py:955-1016): output j is the last
    sample of the time-reversed input after sqrt(1 - f^2) / (1 + f z^-1) and j all-passes (f + z^-1) / (1 + f z^-1)."""
    f, n = float(warping_factor), _table_length(time_data)
    s = (1.0 - f ** 2.0) ** 0.5
    return allpass_table(time_data, -f, f, _running_powers(s, f, n), _running_powers(s, -f, n))


# ---- shoebox room simulation: image sources and modes (ds_room_ism, ds_room_modal_tf; csrc/kernels_room.hpp) --------
# bounds of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
ISM_MAX_CELLS = 1 << 27       # (2 LIMIT + 1)^3 lattice cells of eight image sources each
ISM_MAX_LIST_BYTES = 1 << 30  # the 4-byte ids of one slab of l planes; a larger call is walked slab by slab
ISM_MAX_OUT = 1 << 24         # output samples per band
ISM_MAX_BANDS = 8             # the reference's octave bands
MODAL_MAX_WORK = 1e11         # modes x frequencies
# the reference's u_vectors: the eight sources of a cell, (ux, uy, uz)
_ISM_U = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0], [1, 1, 1]])


def ism_limit(room_dim, t60_s: float, max_order, c: float = 343) -> int:
    """LIMIT of _generate_rir (room_acoustics/_room_acoustics.py:208-213): the lattice runs from -LIMIT to LIMIT."""
    l_max = c * (t60_s * 1.1) / 2 / np.asarray(room_dim, dtype=np.float64)
    limit = int(np.ceil(np.sqrt(l_max @ l_max)))
    if max_order is not None:
        limit = limit if max_order > limit else int(max_order)
    return limit


def _ism_cell_indices(lvec, room_dim, s_pos, r_pos, sr, c):
    """The eight sample indices of cell lvec in the reference's statements (:247-251, :218-219)."""
    pos = ((1 - 2 * _ISM_U) * s_pos) + (2 * np.asarray(lvec) * room_dim) - r_pos
    sq = pos ** 2
    d = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) ** 0.5
    return np.asarray(d / c * sr + 0.5).astype(np.int64)


def _ism_wall_powers(alpha, limit: int) -> np.ndarray:
    """beta^k, k = 0 .. limit + 1, of the walls south, west, floor, north, east, ceiling: (6, limit + 2).  alpha: one
    mean coefficient or six in the reference's order north, south, east, west, floor, ceiling (:196-204)."""
    beta = np.atleast_1d(np.sqrt(1 - np.asarray(alpha, dtype=np.float64)))
    if len(beta) == 1:
        walls = np.ones(6) * beta
    elif len(beta) == 6:
        walls = np.array([beta[1], beta[3], beta[4], beta[0], beta[2], beta[5]])
    else:
        raise ValueError("Wrong length for absorption coefficients")
    return walls[:, None] ** np.arange(limit + 2)[None, :]


def _ism_guard(limit: int, n_out: int, n_band: int) -> None:
    cells = (2 * limit + 1) ** 3
    if cells > ISM_MAX_CELLS:
        raise NotImplementedError(f"an image-source sum over {cells:.3g} lattice cells (LIMIT = {limit}) is beyond the "
                                  f"device kernels' work bound ({ISM_MAX_CELLS} cells per call); pass max_order")
    if n_out > ISM_MAX_OUT or n_band > ISM_MAX_BANDS:
        raise NotImplementedError(f"an image-source response of {n_out} samples in {n_band} bands is beyond the device "
                                  f"kernels' bounds ({ISM_MAX_OUT} samples, {ISM_MAX_BANDS} bands)")


def image_source_rir(room_dim, alphas, s_pos, r_pos, t60_s: float, max_order, sr: int, n_out: int, c: float = 343,
                     max_list_bytes: int | None = None) -> np.ndarray:
    """_generate_rir of the reference (room_acoustics/_room_acoustics.py:162-269) for every row of `alphas` at once,
    padded or trimmed to n_out samples: (bands, n_out) float64 from the device.  alphas: (bands, 1) or (bands, 6)
    absorption coefficients (a scalar or a vector is one band); the bands share the lattice, as they share the room's
    T60 in the reference.  Raises the reference's IndexError when a source falls beyond its int(1.1 T60 5 sr) buffer,
    ValueError when source and receiver coincide (the reference divides by zero there) and NotImplementedError beyond
    the bounds above.  max_list_bytes lowers the memory of the source list (a test does); the result does not depend
    on it."""
    room_dim, s_pos, r_pos = (np.ascontiguousarray(np.squeeze(v), dtype=np.float64) for v in (room_dim, s_pos, r_pos))
    assert room_dim.shape == s_pos.shape == r_pos.shape == (3,), "dimensions and positions are (x, y, z)"
    alphas = np.asarray(alphas, dtype=np.float64)
    alphas = alphas.reshape(1, -1) if alphas.ndim < 2 else alphas
    n_band, n_out, sr = alphas.shape[0], int(n_out), int(sr)
    if n_out < 1 or n_band < 1:
        raise ValueError("image_source_rir: needs output samples and a band")
    if np.array_equal(s_pos, r_pos):
        raise ValueError("Source and receiver positions coincide: the direct sound would be infinite")
    limit = ism_limit(room_dim, t60_s, max_order, c)
    _ism_guard(limit, n_out, n_band)
    if max_list_bytes is not None and int(max_list_bytes) < (2 * limit + 1) ** 2 * 32:
        raise NotImplementedError(f"a source list of {int(max_list_bytes)} bytes does not hold one plane of the lattice "
                                  f"({(2 * limit + 1) ** 2 * 32} bytes)")
    # the largest index belongs to a corner cell: every axis' |pos| peaks at l = -LIMIT or LIMIT
    buffer_length = int(t60_s * 1.1 * 5 * sr)
    corners = [(a, b, d) for a in (-limit, limit) for b in (-limit, limit) for d in (-limit, limit)]
    largest = max(int(_ism_cell_indices(lv, room_dim, s_pos, r_pos, sr, c).max()) for lv in corners)
    if largest >= buffer_length:
        raise IndexError(f"index {largest} is out of bounds for axis 0 with size {buffer_length}")
    pw = np.ascontiguousarray(np.stack([_ism_wall_powers(a, limit) for a in alphas]))
    out = np.empty((n_band, n_out), dtype=np.float64)
    ctx = get_context()
    ctx.check(ctx.lib.ds_room_ism(ctx.handle, _ptr(room_dim), _ptr(s_pos), _ptr(r_pos), float(sr), float(c), limit,
                                  _ptr(pw), n_band, n_out, int(max_list_bytes or 0), _ptr(out)), "ds_room_ism")
    return out


def room_modal_response(omega_n, eta, weight, omega2) -> np.ndarray:
    """p[f] = sum_n weight[n] / (omega_n[n]^2 + 2j eta[n] omega_n[n] - omega2[f]), the modes added in the table's order
    (the loop of get_analytical_transfer_function, room_acoustics/_room_acoustics.py:633-670): complex128 (frequencies,)
    from the device."""
    omega_n, eta, weight, omega2 = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (omega_n, eta, weight, omega2))
    assert len(omega_n) == len(eta) == len(weight), "omega_n, eta and weight are per mode"
    if len(omega_n) < 1 or len(omega2) < 1:
        raise ValueError("room_modal_response: needs a mode and a frequency")
    work = float(len(omega_n)) * len(omega2)
    if work > MODAL_MAX_WORK:
        raise NotImplementedError(f"a modal sum of {work:.3g} terms is beyond the device kernel's work bound "
                                  f"({MODAL_MAX_WORK:.0e} = modes x frequencies per call)")
    p = np.empty(len(omega2), dtype=np.complex128)
    ctx = get_context()
    ctx.check(ctx.lib.ds_room_modal_tf(ctx.handle, _ptr(omega_n), _ptr(eta), _ptr(weight), len(omega_n), _ptr(omega2),
                                       len(omega2), _ptr(p)), "ds_room_modal_tf")
    return p


# ---- variable-Q transform (ds_vqt, ds_resample_int; csrc/kernels_vqt.hpp) ---------------------------------------------
VQT_MAX_OUTPUT_BYTES = 1 << 34  # the complex128 result (csrc/size_guards.hpp; DS_ERR_UNSUP above)
VQT_MAX_DECIMATION = 48         # d: the decimator stages 83 d + 1 samples of four channels in LDS
VQT_MAX_OCTAVES = 7             # the first interpolation stage goes up by 2^octave, at most 64
VQT_MAX_KERNEL = 2048           # taps of one kernel, staged in LDS beside the samples it meets
VQT_MAX_ROWS = 65535            # octaves x bins, and the channel groups of four
VQT_SAMPLE_TILE = {1: 256, 2: 128}  # samples per workgroup of k_vqt_decimate and k_vqt_bank by channel count; else 64


def _vqt_interp_tile(up: int, n_ch: int) -> int:
    """Output samples of one row a workgroup of k_vqt_interp takes (interp_span of the kernels, times `up`)."""
    cg = 1 if n_ch == 1 else 2 if n_ch == 2 else 4
    return 4 * min(max(4 * 256 // (up * cg), 1), 128) * up


def _resample_taps(up: int, down: int) -> np.ndarray:
    """The filter scipy.signal.resample_poly designs by default for an integer ratio: up * firwin(20 r + 1, 1 / r,
    window=("kaiser", 5.0)) with r = max(up, down); the single tap 1.0 for r = 1, where scipy returns a copy."""
    from scipy.signal import firwin
    r = max(int(up), int(down))
    if r == 1:
        return np.ones(1)
    h = firwin(20 * r + 1, 1.0 / r, window=("kaiser", 5.0))
    h *= up
    return h


class _VqtPlan(NamedTuple):
    d: int              # the first decimation
    mid_fs: int         # fs // d: an integer, not the true rate (kept from the reference)
    n_oct: int
    bins: int
    kernel_len: np.ndarray   # int64 [bins]
    kernel_taps: np.ndarray  # complex128, the kernels back to back
    taps_dec: np.ndarray
    taps_half: np.ndarray
    taps_up: np.ndarray      # 2^o firwin(20 2^o + 1) for o = 1 .. n_oct - 1, then d firwin(20 d + 1)


def _vqt_kernels(q: float, highest_f: float, bins: int, mid_fs: int, window, gamma: float) -> list:
    """transforms/_transforms.py:327-383: the complex kernels of one octave, the highest frequency first."""
    freqs = highest_f * 2 ** (-1 / bins * np.arange(bins))
    factor = 2 ** (1 / bins) - 1
    lengths = np.round(q * mid_fs / ((freqs * factor) + gamma)).astype(int)
    kernels = []
    for ind in range(len(lengths)):
        w = get_window(window, lengths[ind], fftbins=False)
        w /= w.sum()
        kernels.append(w * np.exp(1j * freqs[ind] * 2 * np.pi / mid_fs * np.arange(-lengths[ind] // 2, lengths[ind] // 2)))
    return kernels


def _vqt_guard(n_samples: int, n_ch: int, d: int, n_oct: int, bins: int, longest_kernel: int) -> None:
    """NotImplementedError for a transform beyond the kernels' bounds, each named, before anything reaches the device."""
    rows = n_oct * bins
    if d > VQT_MAX_DECIMATION:
        raise NotImplementedError(f"vqt: a decimation of {d} is beyond VQT_MAX_DECIMATION = {VQT_MAX_DECIMATION} "
                                  "(the sampling rate is too far above the highest octave)")
    if n_oct > VQT_MAX_OCTAVES:
        raise NotImplementedError(f"vqt: {n_oct} octaves are beyond VQT_MAX_OCTAVES = {VQT_MAX_OCTAVES}")
    if longest_kernel > VQT_MAX_KERNEL:
        raise NotImplementedError(f"vqt: a kernel of {longest_kernel} taps is beyond VQT_MAX_KERNEL = {VQT_MAX_KERNEL}")
    if rows > VQT_MAX_ROWS or (n_ch + 3) // 4 > VQT_MAX_ROWS:
        raise NotImplementedError(f"vqt: {rows} rows or {n_ch} channels are beyond VQT_MAX_ROWS = {VQT_MAX_ROWS} "
                                  "(rows, and channel groups of four)")
    if 16.0 * rows * n_samples * n_ch > VQT_MAX_OUTPUT_BYTES:
        raise NotImplementedError(f"vqt: a result of {16.0 * rows * n_samples * n_ch:.3g} bytes is beyond "
                                  f"VQT_MAX_OUTPUT_BYTES = 2^34")


def _vqt_plan(n_samples: int, n_ch: int, fs: int, q: float, gamma: float, octaves, bins_per_octave: int, a4_tuning,
              window) -> _VqtPlan:
    """The reference's setup (transforms/transforms.py:876-890) and the tap tables, on the host in float64.
    ZeroDivisionError when the top octave lies above Nyquist / 1.1 (d = 0), as in the reference."""
    fs = int(fs)  # (a numpy integer would divide by zero silently)
    highest_f = a4_tuning * 2 ** (octaves[1] - 4 + 2 / 12)
    d = int((fs // 2) / (highest_f * 1.1))
    mid_fs = fs // d
    n_oct = int(octaves[1] - octaves[0] + 1)
    bins = int(bins_per_octave)
    if n_oct < 1 or bins < 1:
        raise ValueError("vqt: needs at least one octave and one bin per octave")
    gamma = gamma / fs * mid_fs
    freqs = highest_f * 2 ** (-1 / bins * np.arange(bins))
    lengths = np.round(q * mid_fs / ((freqs * (2 ** (1 / bins) - 1)) + gamma)).astype(int)
    if lengths.min() < 1:
        raise ValueError("vqt: a kernel has no taps")
    _vqt_guard(n_samples, n_ch, d, n_oct, bins, int(lengths.max()))
    kernels = _vqt_kernels(q, highest_f, bins, mid_fs, window, gamma)
    ups = [_resample_taps(1 << o, 1) for o in range(1, n_oct)] + [_resample_taps(d, 1)]
    return _VqtPlan(d, mid_fs, n_oct, bins, np.array([len(k) for k in kernels], dtype=np.int64),
                    np.ascontiguousarray(np.concatenate(kernels), dtype=np.complex128), _resample_taps(1, d),
                    _resample_taps(1, 2), np.ascontiguousarray(np.concatenate(ups)))


def vqt(samples, fs: int, q: float = 1, gamma: float = 50, octaves=(1, 5), bins_per_octave: int = 24, a4_tuning=440,
        window="hann", on_device: bool = False):
    """The variable-Q coefficients (octaves x bins, samples, channels) complex128 of `samples`: (N, C) float64 on the
    host, or a `DevicePlanar` whose float32 samples are read where they lie.  The decimators, the kernel bank and the
    polyphase interpolators run on the device in float64 (ds_vqt).  Returns the array, or with `on_device` a
    `DeviceScalogram` left in HBM."""
    resident = isinstance(samples, DevicePlanar)
    if resident:
        n, n_ch = samples.n_samples, samples.n_ch
    else:
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        assert samples.ndim == 2, "the samples are (samples, channels)"
        n, n_ch = samples.shape
    if n < 1 or n_ch < 1:
        raise ValueError("vqt: needs at least one sample and one channel")
    p = _vqt_plan(n, n_ch, fs, q, gamma, octaves, bins_per_octave, a4_tuning, window)
    shape = (p.n_oct * p.bins, n, n_ch)
    ctx = samples.ctx if resident else get_context()
    head = (C.c_void_p(samples.ptr), 1, n_ch, samples.ld, n) if resident else (_ptr(samples), 0, n_ch, n, n)
    tables = (p.d, p.n_oct, p.bins, _ptr(p.kernel_len), _ptr(p.kernel_taps), _ptr(p.taps_dec), _ptr(p.taps_half),
              _ptr(p.taps_up))
    if not on_device:
        out = np.empty(shape, dtype=np.complex128)
        ctx.check(ctx.lib.ds_vqt(ctx.handle, *head, *tables, _ptr(out), 0), "ds_vqt")
        return out
    with device_scope(ctx) as dev:
        buf = dev.alloc(16 * shape[0] * n * n_ch, result=True)
        ctx.check(ctx.lib.ds_vqt(ctx.handle, *head, *tables, C.c_void_p(buf.ptr), 1), "ds_vqt")
        ctx.sync()
    return DeviceScalogram(buf, shape, np.complex128)


def resample_int(td, up: int, down: int) -> np.ndarray:
    """scipy.signal.resample_poly(td, up, down, axis=0) with its default filter for real (n, C) float64 data and an
    integer ratio (one of `up` and `down` is 1), on the device in float64 (ds_resample_int): the stage the variable-Q
    transform is built from, here by itself."""
    up, down = int(up), int(down)
    if up < 1 or down < 1 or (up != 1 and down != 1):
        raise ValueError("resample_int: one of up and down must be 1, the other a positive integer")
    if down > VQT_MAX_DECIMATION or up > 1 << (VQT_MAX_OCTAVES - 1):
        raise NotImplementedError(f"resample_int: down beyond VQT_MAX_DECIMATION = {VQT_MAX_DECIMATION} or up beyond "
                                  f"{1 << (VQT_MAX_OCTAVES - 1)}")
    x = np.ascontiguousarray(td, dtype=np.float64)
    assert x.ndim == 2, "the samples are (samples, channels)"
    n, n_ch = x.shape
    if n < 1 or n_ch < 1:
        raise ValueError("resample_int: needs at least one sample and one channel")
    out = np.empty((-(-n * up // down), n_ch))
    taps = _resample_taps(up, down)
    ctx = get_context()
    ctx.check(ctx.lib.ds_resample_int(ctx.handle, _ptr(x), n, n_ch, up, down, _ptr(taps), _ptr(out)), "ds_resample_int")
    return out


# ---- rational-ratio resampling (ds_resample_poly, ds_resample_poly_dev; csrc/kernels_resample.hpp) ---------------------
RESAMPLE_MAX_RATE = 640           # max(up, down) of the reduced ratio (csrc/size_guards.hpp; DS_ERR_UNSUP above)
RESAMPLE_MAX_SAMPLES = 1 << 31    # the longer of input and output, times the channels
RESAMPLE_MAX_CHANNELS = 65535     # grid.y carries the channel groups
RESAMPLE_NT, RESAMPLE_PASSES, RESAMPLE_LDS_DOUBLES = 256, 4, 20480  # csrc/resample_plan.hpp


def _resample_tile(up: int, down: int, n_ch: int) -> tuple:
    """(tile, chunks, span, LDS bytes) of make_plan in csrc/resample_plan.hpp for a reduced ratio: the output samples a
    workgroup takes, the pieces its sums run in, the input samples per channel it stages for each, and what it declares."""
    cg = 1 if n_ch == 1 else 2 if n_ch == 2 else 4
    terms = -(-(20 * max(up, down) + 1) // up)
    table = up * (terms | 1)
    w = (RESAMPLE_LDS_DOUBLES - table) // cg

    def adv(tile):
        return -(-(tile - 1) * down // up)

    tile = RESAMPLE_PASSES * RESAMPLE_NT // cg
    while tile > 1 and adv(tile) + terms > w and adv(tile) > w // 2:
        tile >>= 1
    jc = min(terms, w - adv(tile))
    return tile, -(-terms // jc), adv(tile) + jc, 8 * (table + (adv(tile) + jc) * cg)


def _resample_ratio(who: str, up, down, n: int, n_ch: int) -> tuple:
    """The reduced (up, down) and the output length; ValueError for a bad ratio or no samples, NotImplementedError beyond
    the kernel's bounds, each named, before anything reaches the device."""
    if int(up) != up or int(down) != down or up < 1 or down < 1:
        raise ValueError(f"{who}: up and down are positive integers")
    if n < 1 or n_ch < 1:
        raise ValueError(f"{who}: needs at least one sample and one channel")
    up, down = int(up), int(down)
    g = math.gcd(up, down)
    up, down = up // g, down // g
    n_out = -(-n * up // down)
    if max(up, down) > RESAMPLE_MAX_RATE:
        raise NotImplementedError(f"{who}: the ratio {up} / {down} is beyond RESAMPLE_MAX_RATE = {RESAMPLE_MAX_RATE} "
                                  "(the larger of up and down once reduced: its taps would not fit a workgroup's LDS)")
    if max(n, n_out) * n_ch > RESAMPLE_MAX_SAMPLES:
        raise NotImplementedError(f"{who}: {max(n, n_out)} samples of {n_ch} channels are beyond RESAMPLE_MAX_SAMPLES = 2^31")
    if n_ch > RESAMPLE_MAX_CHANNELS:
        raise NotImplementedError(f"{who}: {n_ch} channels are beyond RESAMPLE_MAX_CHANNELS = {RESAMPLE_MAX_CHANNELS}")
    return up, down, n_out


def resample_poly(td, up: int, down: int, scale: float = 1.0) -> np.ndarray:
    """scale * scipy.signal.resample_poly(td, up, down, axis=0) with its default filter for real (n, C) float64 data and
    any ratio whose reduced form stays within RESAMPLE_MAX_RATE, on the device in float64 (ds_resample_poly).  `scale` is
    folded into the taps.  A ratio of 1 / 1 returns a copy (times `scale`) without touching the device."""
    if np.iscomplexobj(td):
        raise NotImplementedError("resample_poly: complex samples are not run on the device")
    x = np.ascontiguousarray(td, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    assert x.ndim == 2, "the samples are (samples, channels)"
    n, n_ch = x.shape
    up, down, n_out = _resample_ratio("resample_poly", up, down, n, n_ch)
    if up == down:
        return x.copy() if scale == 1.0 else x * scale
    taps = _resample_taps(up, down)
    if scale != 1.0:
        taps *= scale
    out = np.empty((n_out, n_ch))
    ctx = get_context()
    ctx.check(ctx.lib.ds_resample_poly(ctx.handle, _ptr(x), n, n_ch, up, down, _ptr(taps), _ptr(out)), "ds_resample_poly")
    return out


def resample_poly_device(x_dev: DevicePlanar, up: int, down: int, scale: float = 1.0) -> DevicePlanar:
    """resample_poly of planar float32 samples in HBM, read where they lie and summed in float64, into a new planar
    float32 buffer of ceil(n up / down) samples per channel (ds_resample_poly_dev); nothing comes down to the host.  A
    ratio of 1 / 1 without a scale returns the (immutable) samples themselves."""
    assert isinstance(x_dev, DevicePlanar), "the samples are a DevicePlanar"
    n, n_ch = x_dev.n_samples, x_dev.n_ch
    up, down, n_out = _resample_ratio("resample_poly_device", up, down, n, n_ch)
    if up == down:
        return x_dev if scale == 1.0 else level_apply(x_dev, gain=scale)
    taps = _resample_taps(up, down)
    if scale != 1.0:
        taps *= scale
    ctx = x_dev.ctx
    with device_scope(ctx) as dev:
        d_y = dev.alloc(4 * n_ch * n_out, result=True)
        ctx.check(ctx.lib.ds_resample_poly_dev(ctx.handle, C.c_void_p(x_dev.ptr), x_dev.ld, n, n_ch, up, down, _ptr(taps),
                                               C.c_void_p(d_y.ptr), n_out), "ds_resample_poly_dev")
    return DevicePlanar(d_y, n_ch, n_out, n_out, 0)


# ---- audio effects (ds_fx_*, csrc/kernels_fx.hpp) ---------------------------------------------------------------------
FX_MAX_STREAMS = 65535        # bands x channels of one call (csrc/size_guards.hpp; DS_ERR_UNSUP above)
FX_MAX_SAMPLES = 1 << 28      # padded samples of one stream
FX_MAX_ELEMENTS = 1 << 30     # streams x padded samples
FX_MAX_CURVES = 8             # distortion curves of one call
FX_MAX_VOICES = 64            # chorus voices of one call
FX_FOLLOW_TILE = 512          # samples of one round of the follower (FOLLOW_TILE of the kernels)
FX_THREADS = 256              # threads of the sample-parallel kernels and reductions (NT of the kernels)
FX_CURVES = {"Arctan": 0, "HardClip": 1, "SoftClip": 2, "NoDistortion": 3}  # DS_FX_CURVE_* of the header
FX_SATURATIONS = {"digital": 0, "arctan": 1}                                # DS_FX_SAT_*


def _fx_guard(n_streams: int, n_padded: int, voices: int = 0, curves: int = 0) -> None:
    """NotImplementedError for an effect beyond the kernels' bounds, each named, before anything reaches the device."""
    if n_streams > FX_MAX_STREAMS:
        raise NotImplementedError(f"effects: {n_streams} streams (bands x channels) are beyond FX_MAX_STREAMS = {FX_MAX_STREAMS}")
    if n_padded > FX_MAX_SAMPLES:
        raise NotImplementedError(f"effects: {n_padded} padded samples are beyond FX_MAX_SAMPLES = 2^28")
    if n_streams * n_padded > FX_MAX_ELEMENTS:
        raise NotImplementedError(f"effects: {n_streams} streams x {n_padded} samples are beyond FX_MAX_ELEMENTS = 2^30")
    if voices > FX_MAX_VOICES:
        raise NotImplementedError(f"effects: {voices} chorus voices are beyond FX_MAX_VOICES = {FX_MAX_VOICES}")
    if curves > FX_MAX_CURVES:
        raise NotImplementedError(f"effects: {curves} distortion curves are beyond FX_MAX_CURVES = {FX_MAX_CURVES}")


def _fx_samples(x):
    """x as the entries take it: a DevicePlanar as it is, anything else as a C-order (samples, streams) float64 array."""
    if isinstance(x, DevicePlanar):
        return x
    if np.iscomplexobj(x):
        raise NotImplementedError("effects: complex samples are not run on the device (the recursions are real)")
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    assert x.ndim == 2 and x.shape[0] >= 1 and x.shape[1] >= 1, "the samples are (samples, streams)"
    return x


def _fx_run(entry: str, x, n_out: int, *middle, voices: int = 0, curves: int = 0):
    """One ds_fx_* call whose result is samples: x (N, S) float64 -> (n_out, S) float64, or a DevicePlanar read where it
    lies -> a DevicePlanar of n_out samples.  `middle`: the entry's arguments between n and y."""
    x = _fx_samples(x)
    n, n_str = _samples_shape(x)
    _fx_guard(n_str, n_out, voices, curves)
    if isinstance(x, DevicePlanar):
        ctx = x.ctx
        with device_scope(ctx) as dev:
            d_y = dev.alloc(4 * n_str * n_out, result=True)
            ctx.check(getattr(ctx.lib, entry)(ctx.handle, C.c_void_p(x.ptr), 1, n_str, x.ld, n, *middle,
                                              C.c_void_p(d_y.ptr), n_out), entry)
        return DevicePlanar(d_y, n_str, n_out, n_out, 0)
    y = np.empty((n_out, n_str), dtype=np.float64)
    ctx = get_context()
    ctx.check(getattr(ctx.lib, entry)(ctx.handle, _ptr(x), 0, n_str, n, n, *middle, _ptr(y), n_out), entry)
    return y


def fx_follower_coefficient(samples) -> float:
    """1 - exp(ln 0.05 / samples): the one-pole coefficient that reaches 95 % after `samples` steps; 1 for 0 samples."""
    with np.errstate(divide="ignore"):
        return float(1 - np.exp(np.log(1 - 0.95) / np.float64(samples)))


def fx_compress(x, threshold_db: float, ratio: float, knee_db: float, attack_samples: int, release_samples: int,
                pre_gain: float = 1.0, final_gain: float = 1.0, downward: bool = True, relative: bool = True,
                make_up: bool = True):
    """The compressor's sample loop and the stages around it (ds_fx_compress): gains are linear factors."""
    par = np.array([pre_gain, threshold_db, ratio, knee_db, fx_follower_coefficient(attack_samples),
                    fx_follower_coefficient(release_samples), 10 ** (-300.0 / 10), final_gain], dtype=np.float64)
    n = _samples_shape(_fx_samples(x))[0]
    return _fx_run("ds_fx_compress", x, n, _ptr(par), int(bool(downward)), int(bool(relative)), int(bool(make_up)))


def fx_detect(x, threshold_db: float, c_release: float, relative: bool = True) -> np.ndarray:
    """The activity detector's gate (ds_fx_detect): -> (N, S) bool, True where the smoothed power is above the threshold."""
    x = _fx_samples(x)
    n, n_str = _samples_shape(x)
    _fx_guard(n_str, n)
    mask = np.empty((n_str, n), dtype=np.uint8)
    if isinstance(x, DevicePlanar):
        ctx, head = x.ctx, (C.c_void_p(x.ptr), 1, n_str, x.ld, n)
    else:
        ctx, head = get_context(), (_ptr(x), 0, n_str, n, n)
    ctx.check(ctx.lib.ds_fx_detect(ctx.handle, *head, float(c_release), float(threshold_db), int(bool(relative)), _ptr(mask)),
              "ds_fx_detect")
    return mask.T.astype(bool)


def fx_delay(x, delay_samples: int, padding: int, feedback: float, saturation: str = "digital"):
    """The feedback delay line over the samples and `padding` zeros behind them, peak restored (ds_fx_delay)."""
    n = _samples_shape(_fx_samples(x))[0]
    return _fx_run("ds_fx_delay", x, n + int(padding), int(delay_samples), int(padding), float(feedback),
                   FX_SATURATIONS[saturation])


def fx_chorus(x, delays, mix: float):
    """The chorus gather (ds_fx_chorus): delays (N, V) integer samples per voice, the reference's index table."""
    n = _samples_shape(_fx_samples(x))[0]
    delays = np.asarray(delays)
    assert delays.ndim == 2 and delays.shape[0] == n and delays.shape[1] >= 1, "the delays are (samples, voices)"
    max_delay = int(np.abs(delays).max())
    _fx_guard(1, n + max_delay, voices=delays.shape[1])
    m = np.ascontiguousarray(delays, dtype=np.int32)
    return _fx_run("ds_fx_chorus", x, n, _ptr(m), m.shape[1], max_delay, float(mix), voices=m.shape[1])


def fx_distort(x, kinds, levels, offsets, mixes, gain: float = 1.0):
    """The sum of the peak-restored distortion curves (ds_fx_distort): kinds are FX_CURVES values, levels and offsets
    linear; curves with a mix weight of 0 are left out as the reference skips them."""
    keep = [i for i, w in enumerate(mixes) if w != 0.0]
    _fx_guard(1, 1, curves=len(keep))
    kind = np.array([kinds[i] for i in keep], dtype=np.int32)
    par = np.ascontiguousarray([[levels[i], offsets[i], mixes[i]] for i in keep], dtype=np.float64)
    n = _samples_shape(_fx_samples(x))[0]
    return _fx_run("ds_fx_distort", x, n, len(keep), _ptr(kind), _ptr(par), float(gain), curves=len(keep))


def fx_tremolo(x, modulator):
    """Every stream times the per-sample modulator (ds_fx_tremolo)."""
    n = _samples_shape(_fx_samples(x))[0]
    mod = np.ascontiguousarray(modulator, dtype=np.float64)
    assert mod.shape == (n,), "the modulator has one value per sample"
    return _fx_run("ds_fx_tremolo", x, n, _ptr(mod))


# ---- spectral subtraction (ds_fx_specsub, csrc/kernels_specsub.hpp) --------------------------------------------------------
SS_MIN_WINDOW = 4                 # the packed transform has at least two points (csrc/size_guards.hpp)
SS_MAX_WINDOW = 16384             # W / 2 complex points in LDS: 128 KiB (DS_ERR_UNSUP above)
SS_MAX_WORKSPACE_BYTES = 1 << 32  # 8 (W + 2) bytes x frames x streams
SS_MAX_OLA_TERMS = 1 << 29        # samples x streams x ceil(W / step)
SS_TRACK_TILE = 8                 # frames a lane of k_ss_track loads ahead (TRACK_TILE of the kernels)
SS_OLA_TILE = 256                 # kept output samples of one workgroup of k_ss_ola (OLA_TILE)
SS_WINDOW_FLOOR = 1e-6            # the reference clips its window from below here
SS_MODES = {"adaptive": 0, "static": 1}  # DS_FX_SPECSUB_* of the header


def specsub_frames(n: int, window: int, step: int) -> int:
    """ceil((n + 2 W) / step): the frames of a signal padded by W zeros at both ends, the last ones zero-padded."""
    return -(-(int(n) + 2 * int(window)) // int(step))


def specsub_window(window_type, window: int) -> np.ndarray:
    """The reference's window: scipy's periodic one, clipped from below at 1e-6."""
    spec = window_type.to_scipy_format() if isinstance(window_type, Window) else window_type
    return np.clip(get_window(spec, int(window)), a_min=SS_WINDOW_FLOOR, a_max=None).astype(np.float64)


def _specsub_guard(n_streams: int, n: int, window: int, step: int) -> None:
    """ValueError for a window or step the frames cannot take, NotImplementedError beyond the kernels' bounds, each named;
    before anything reaches the device."""
    if window < 1 or window & (window - 1):
        raise ValueError(f"spectral subtraction: the window, {window} samples, is not a power of two")
    if window < SS_MIN_WINDOW:
        raise NotImplementedError(f"spectral subtraction: a window of {window} samples is below SS_MIN_WINDOW = {SS_MIN_WINDOW}")
    if window > SS_MAX_WINDOW:
        raise NotImplementedError(f"spectral subtraction: a window of {window} samples is beyond SS_MAX_WINDOW = {SS_MAX_WINDOW}")
    if not 1 <= step <= window:
        raise ValueError(f"spectral subtraction: a step of {step} samples is not in 1 .. {window} (the overlap is too large)")
    frames = specsub_frames(n, window, step)
    if frames >= 1 << 31 or 8 * (window + 2) * frames * n_streams > SS_MAX_WORKSPACE_BYTES:
        raise NotImplementedError(f"spectral subtraction: a frame workspace of {8 * (window + 2) * frames * n_streams:.3g} bytes "
                                  f"({frames} frames x {n_streams} streams) is beyond SS_MAX_WORKSPACE_BYTES = 2^32")
    if n * n_streams * -(-window // step) > SS_MAX_OLA_TERMS:
        raise NotImplementedError(f"spectral subtraction: {n * n_streams * -(-window // step):.3g} overlap-add terms are beyond "
                                  f"SS_MAX_OLA_TERMS = 2^29")


def fx_specsub(x, window_type, window: int, step: int, mode: str = "adaptive", threshold_db: float = -40.0,
               forgetting: float = 0.9, factor: float = 2.0, exponent: float = 2.0, noise_table=None, env_floor=None):
    """Spectral subtraction of every stream (ds_fx_specsub): frames of `window` samples `step` apart of the zero-padded
    samples, magnitudes max(|X|^e - t, 0)^(1 / e), weighted overlap-add, the peak restored.  mode "adaptive": t follows the
    gated frames' amplitudes; "static": t = factor noise_table, (bins,) for every stream or (streams, bins), already
    |PSD|^(e / 2).  env_floor: where the overlap-added squared window is clipped from below; None for no clipping."""
    x = _fx_samples(x)
    n, n_str = _samples_shape(x)
    window, step = int(window), int(step)
    _fx_guard(n_str, n)
    _specsub_guard(n_str, n, window, step)
    win = specsub_window(window_type, window)
    table = None
    if SS_MODES[mode] == SS_MODES["static"]:
        table = np.asarray(noise_table, dtype=np.float64)
        table = np.ascontiguousarray(np.broadcast_to(table, (n_str, window // 2 + 1)))
    return _fx_run("ds_fx_specsub", x, n, _ptr(win), _ptr(win), window, step, SS_MODES[mode], float(threshold_db),
                   float(forgetting), float(factor), float(exponent), _ptr(table) if table is not None else None,
                   -1.0 if env_floor is None else float(env_floor))


# ---- levels and loudness (ds_level_*, ds_moving_rms, ds_loudness_blocks, ds_envelope_analytic; csrc/kernels_level.hpp) ----
LEVEL_NT = 256                # lanes per workgroup (NT of the kernels)
LEVEL_PER_LANE = 16           # samples a lane of a reduction adds in turn (PER_LANE)
LEVEL_SPAN = LEVEL_NT * LEVEL_PER_LANE  # samples per workgroup of a reduction (SPAN)
LEVEL_TILE = 1024             # outputs per workgroup of the moving window (TILE)
LEVEL_VEC_BYTES = 16          # bytes a lane of the apply kernels loads and stores at once (VEC_BYTES)
LEVEL_MAX_ORDER = 8           # polynomial order of a trend (MAX_ORDER)
LEVEL_MAX_CHANNELS = 65535    # csrc/size_guards.hpp; DS_ERR_UNSUP above
LEVEL_MAX_SAMPLES = (1 << 31) - 1
LEVEL_MAX_ELEMENTS = 1 << 33
LEVEL_MOVING_MAX_WORK = 1e12  # channels x samples x (2 + min(window, samples) / 1024)
LEVEL_NORMS = {"none": 0, "peak_each": 1, "peak_all": 2, "rms_each": 3, "rms_all": 4}  # DS_LEVEL_NORM_* of the header


def level_basis(n: int, order: int) -> np.ndarray:
    """The recurrence of the discrete Chebyshev (Gram) polynomials orthonormal on 0 .. n - 1, as the entries take it:
    [(n - 1) / 2, 1 / sqrt(n), a_0 .. a_7, b_0 .. b_7] with P_{k+1} = a_k t P_k - b_k P_{k-1}, a_k = 1 / beta_{k+1},
    b_k = beta_k / beta_{k+1}, beta_k^2 = k^2 (n^2 - k^2) / (4 (4 k^2 - 1)); formed in long double, filled up to `order`."""
    n, order = int(n), int(order)
    assert 0 <= order <= LEVEL_MAX_ORDER and order < n, "the order is at most 8 and below the length"
    ld = np.longdouble
    out = np.zeros(2 + 2 * LEVEL_MAX_ORDER, dtype=np.float64)
    out[0] = float((ld(n) - 1) / 2)
    out[1] = float(1 / np.sqrt(ld(n)))
    k = np.arange(0, order + 1, dtype=ld)
    beta = np.sqrt(k * k * (ld(n) * ld(n) - k * k) / (4 * (4 * k * k - 1)))
    for i in range(order):
        out[2 + i] = float(1 / beta[i + 1])
        out[2 + LEVEL_MAX_ORDER + i] = float(beta[i] / beta[i + 1])
    return out


def _level_guard(n_ch: int, n: int) -> None:
    """NotImplementedError for a shape beyond the kernels' bounds, before anything reaches the device."""
    if n_ch > LEVEL_MAX_CHANNELS or n > LEVEL_MAX_SAMPLES or n_ch * n > LEVEL_MAX_ELEMENTS:
        raise NotImplementedError(f"levels: {n_ch} channels x {n} samples are beyond the device kernels' bounds "
                                  f"({LEVEL_MAX_CHANNELS} channels, 2^31 - 1 samples a channel, 2^33 samples in all)")


def _level_samples(x):
    """x as the entries take it, and the arguments that describe it: (x, pointer, on_device, n_ch, ld, n).  No context is
    opened: the callers' guards come first."""
    if not isinstance(x, DevicePlanar):
        if np.iscomplexobj(x):
            raise NotImplementedError("levels: complex samples are not run on the device")
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x[:, None] if x.ndim == 1 else x
        assert x.ndim == 2 and x.shape[0] >= 1 and x.shape[1] >= 1, "the samples are (samples, channels)"
    n, n_ch = _samples_shape(x)
    _level_guard(n_ch, n)
    if isinstance(x, DevicePlanar):
        return x, C.c_void_p(x.ptr), 1, n_ch, x.ld, n
    return x, _ptr(x), 0, n_ch, n, n


def _level_ctx(x):
    return x.ctx if isinstance(x, DevicePlanar) else get_context()


def _level_order(n: int, order: int) -> int:
    """The order that is fitted: a polynomial through every sample (order >= n) leaves the same zero residual as n - 1."""
    return min(int(order), n - 1)


def level_project(x, order: int = 0) -> np.ndarray:
    """Per channel of x ((N, C) float64, or a DevicePlanar read where it lies): the coefficients c_k = sum_n x[n] P_k(n),
    k = 0 .. 8 (zero past the order) in the basis of level_basis, and max |x|, as (C, 10) float64 (ds_level_project)."""
    x, px, on_dev, n_ch, ld, n = _level_samples(x)
    order = _level_order(n, order)
    basis = level_basis(n, order)
    out = np.empty((n_ch, 10), dtype=np.float64)
    ctx = _level_ctx(x)
    ctx.check(ctx.lib.ds_level_project(ctx.handle, px, on_dev, n_ch, ld, n, order, _ptr(basis), _ptr(out)), "ds_level_project")
    return out


def level_stats(x, order: int = 0, common: bool = False) -> np.ndarray:
    """Per channel: sum (x - p)^2 term by term, max |x - p|, max |x| as (C, 3) float64, p the least-squares polynomial
    of `order` (0: the mean) of the channel; common: the mean of all channels together (ds_level_stats)."""
    x, px, on_dev, n_ch, ld, n = _level_samples(x)
    order = _level_order(n, order)
    basis = level_basis(n, order)
    out = np.empty((n_ch, 3), dtype=np.float64)
    ctx = _level_ctx(x)
    ctx.check(ctx.lib.ds_level_stats(ctx.handle, px, on_dev, n_ch, ld, n, order, _ptr(basis), int(bool(common)), _ptr(out)),
              "ds_level_stats")
    return out


def level_apply(x, order: int = -1, norm: str = "none", norm_factor: float = 1.0, gain=None, fade=None,
                at_start: bool = False, at_end: bool = False):
    """y[n] = (x[n] - p(n)) g fade[n] fade[N - 1 - n] in one pass (ds_level_apply), every factor optional: order >= 0
    removes the channel's least-squares polynomial; gain (C,) or, with norm one of LEVEL_NORMS, norm_factor over the
    peak or the centred rms found on the device; fade (L,) on the first L samples (at_start) and mirrored on the last
    (at_end).  x (N, C) float64 -> (N, C) float64; a DevicePlanar is read where it lies -> a DevicePlanar."""
    x, px, on_dev, n_ch, ld, n = _level_samples(x)
    order = _level_order(n, order) if order >= 0 else -1
    basis = level_basis(n, max(order, 0))
    if gain is not None:
        gain = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float64), (n_ch,)))
    l_fade = 0
    if fade is not None:
        fade = np.ascontiguousarray(fade, dtype=np.float64)
        assert fade.ndim == 1 and 1 <= fade.shape[0] <= n and (at_start or at_end), "a fade has 1 .. N samples and an end"
        l_fade = fade.shape[0]
    middle = (order, _ptr(basis), LEVEL_NORMS[norm], float(norm_factor), None if gain is None else _ptr(gain),
              None if fade is None else _ptr(fade), l_fade, int(bool(at_start)), int(bool(at_end)))
    ctx = _level_ctx(x)
    if on_dev:
        with device_scope(ctx) as dev:
            d_y = dev.alloc(4 * n_ch * n, result=True)
            ctx.check(ctx.lib.ds_level_apply(ctx.handle, px, 1, n_ch, ld, n, *middle, C.c_void_p(d_y.ptr), n), "ds_level_apply")
        return DevicePlanar(d_y, n_ch, n, n, 0)
    y = np.empty((n, n_ch), dtype=np.float64)
    ctx.check(ctx.lib.ds_level_apply(ctx.handle, px, 0, n_ch, n, n, *middle, _ptr(y), n), "ds_level_apply")
    return y


def moving_rms(x, window_length: int) -> np.ndarray:
    """sqrt(max(0, mean of the last `window_length` squares of x minus its least-squares line)), samples before the first
    counted as zero, as (N, C) float64 (ds_moving_rms)."""
    x, px, on_dev, n_ch, ld, n = _level_samples(x)
    w = int(window_length)
    assert w >= 1, "the window has at least one sample"
    if n_ch * n * (2 + min(w, n) / 1024) > LEVEL_MOVING_MAX_WORK:
        raise NotImplementedError(f"levels: a window of {w} samples over {n_ch} x {n} samples is beyond "
                                  f"LEVEL_MOVING_MAX_WORK = {LEVEL_MOVING_MAX_WORK:g} squares")
    basis = level_basis(n, _level_order(n, 1))
    out = np.empty((n, n_ch), dtype=np.float64)
    ctx = _level_ctx(x)
    ctx.check(ctx.lib.ds_moving_rms(ctx.handle, px, on_dev, n_ch, ld, n, _ptr(basis), w, _ptr(out)), "ds_moving_rms")
    return out


def loudness_block_count(n: int, tg: int, step: int) -> int:
    """ceil((n - tg) / step), never below 0: the frames the reference cuts without padding."""
    return max(0, -(-(int(n) - int(tg)) // int(step)))


def loudness_blocks(x, sos, tg: int, step: int) -> np.ndarray:
    """The mean squares of the blocks of tg samples every `step` of x filtered by the cascade sos (K, 6) from rest, as
    (blocks, C) float64 (ds_loudness_blocks); (0, C) when the signal holds no block."""
    x, px, on_dev, n_ch, ld, n = _level_samples(x)
    sos = np.ascontiguousarray(np.atleast_2d(sos), dtype=np.float64)
    assert sos.ndim == 2 and sos.shape[1] == 6 and sos.shape[0] >= 1, "sos is (sections, 6) with at least one section"
    if sos.shape[0] > IIR_MAX_SECTIONS:
        raise NotImplementedError(f"levels: a cascade of {sos.shape[0]} sections is beyond the {IIR_MAX_SECTIONS} of the section runner")
    n_blocks = loudness_block_count(n, tg, step)
    z = np.empty((n_blocks, n_ch), dtype=np.float64)
    if n_blocks == 0:
        return z
    ctx = _level_ctx(x)
    ctx.check(ctx.lib.ds_loudness_blocks(ctx.handle, px, on_dev, n_ch, ld, n, _ptr(sos), sos.shape[0], int(tg), int(step),
                                         n_blocks, _ptr(z)), "ds_loudness_blocks")
    return z


def envelope_analytic(x) -> np.ndarray:
    """|hilbert(x minus its least-squares line)| as (N, C) float64 (ds_envelope_analytic), within the bounds of the
    float64 transform."""
    n = _samples_shape(x if isinstance(x, DevicePlanar) else np.asarray(x))[0]
    _fft64_guard(n)
    x, px, on_dev, n_ch, ld, n = _level_samples(x)
    basis = level_basis(n, _level_order(n, 1))
    out = np.empty((n, n_ch), dtype=np.float64)
    ctx = _level_ctx(x)
    ctx.check(ctx.lib.ds_envelope_analytic(ctx.handle, px, on_dev, n_ch, ld, n, _ptr(basis), _ptr(out)), "ds_envelope_analytic")
    return out
