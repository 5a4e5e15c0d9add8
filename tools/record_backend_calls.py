"""Call transcript of the host shim (dsptoolbox_amd/backend.py) against a recording stand-in for Context: no GPU, no
ds_init.  Every `ctx.lib.ds_*` call returns 0 and is logged as (entry, scalar arguments by value, pointers as
"null" / "host" / "dev<allocation>+<offset>"); malloc, upload, free, download*, staging and sync are logged with their
sizes and are otherwise inert.  Numeric results are uninitialised and are described by type, dtype and shape only.

    python tools/record_backend_calls.py welch      # rewrites tests/golden/backend_calls.json        (cases)
    python tools/record_backend_calls.py xform      # rewrites tests/golden/backend_calls_xform.json  (xform_cases)
tests/test_backend_calls_host.py compares `record()` with those files: a refactor of the shim must leave them unchanged,
so a fixture is rewritten only BEFORE the refactor it is to judge.  `cases` (the Welch functions and everything that
holds device buffers) was recorded before the Welch half of the shim was rebuilt; `xform_cases` (STFT, iSTFT, rFFT,
deconvolution, FIR, beamformer maps, IIR: their host-pointer paths above all) before the other half was.
Only names that the shim has had since the Welch routes were settled are touched.  Arrays of 2^20 elements and more
go through the library's threaded host casts: those cases need the built library (no GPU)."""
import bisect
import contextlib
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import dsptoolbox_amd as dsp  # noqa: E402
from dsptoolbox_amd import _lib, backend  # noqa: E402
from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar  # noqa: E402
from dsptoolbox_amd.standard.enums import SpectrumScaling, Window  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "backend_calls.json")
WELCH_ENTRIES = ("ds_welch_psd", "ds_welch_psd_f64", "ds_welch_psd_dev", "ds_welch_csd", "ds_welch_csd_f64",
                 "ds_welch_spec_x64", "ds_welch_tf", "ds_welch_tf_f64", "ds_welch_tf_dev", "ds_welch_tf_x64", "ds_csm",
                 "ds_csm_f64", "ds_csm_x64", "ds_csm_dev", "ds_csm_bins_dev")
FIXTURE_XFORM = os.path.join(ROOT, "tests", "golden", "backend_calls_xform.json")
XFORM_ENTRIES = ("ds_stft_r2c", "ds_stft_r2c_f64", "ds_stft_r2c_dev", "ds_istft", "ds_istft_f64", "ds_istft_dev",
                 "ds_band_power_dev", "ds_rfft", "ds_rfft_f64", "ds_rfft_dev", "ds_deconv", "ds_deconv_f64", "ds_deconv_dev",
                 "ds_deconv_inverse_dev", "ds_fir_ola", "ds_fir_ola_f64", "ds_fir_ola_dev", "ds_fir_freqz", "ds_das_map",
                 "ds_csm_spec", "ds_bf_eigh", "ds_bf_eig_map", "ds_bf_cleansc", "ds_iir_sos", "ds_iir_sos_dev")
_DEV_BASE = 0x500000000000


class _RecordingLib:
    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        if not name.startswith("ds_"):
            raise AttributeError(name)

        def entry(handle, *args):
            self._ctx.log.append(["call", name, [self._ctx.describe(a) for a in args]])
            return 0
        return entry


class RecordingContext:
    """Stands in for _lib.Context: `log` is the transcript, `live` the allocations not freed yet."""

    def __init__(self):
        self.lib, self.handle, self.device = _RecordingLib(self), 1, 0
        self.log, self.live, self.free_count = [], set(), {}
        self._bases, self._sizes = [], []

    # ---- what the transcript says about one argument
    def _label(self, addr):
        i = bisect.bisect_right(self._bases, addr) - 1
        if i >= 0 and addr < self._bases[i] + max(self._sizes[i], 1) + 4096:
            return f"dev{i}+{addr - self._bases[i]}"
        return "host"

    def describe(self, a):
        if a is None:
            return "null"
        if isinstance(a, C.c_void_p):
            return "null" if a.value is None else self._label(a.value)
        if isinstance(a, (bool, np.bool_)):
            return int(a)
        if isinstance(a, (int, np.integer)):
            return int(a)
        if isinstance(a, (float, np.floating)):
            return float(a)
        raise TypeError(f"argument {a!r} of type {type(a).__name__} in a C call")

    # ---- Context's surface
    def check(self, rc, what=""):
        assert rc == 0, what

    def malloc(self, nbytes):
        nbytes = int(nbytes)
        base = (self._bases[-1] + self._sizes[-1] + (1 << 16)) & ~0xFFF if self._bases else _DEV_BASE
        self._bases.append(base)
        self._sizes.append(nbytes)
        self.live.add(len(self._bases) - 1)
        self.log.append(["malloc", nbytes])
        return base

    def free(self, dptr):
        i = self._bases.index(dptr)
        self.free_count[i] = self.free_count.get(i, 0) + 1
        self.live.discard(i)
        if self.log and self.log[-1][0] == "free":  # (a run of frees is one event: their order is not behaviour)
            self.log[-1][1] = sorted(self.log[-1][1] + [i])
        else:
            self.log.append(["free", [i]])

    def upload(self, dptr, arr):
        self.log.append(["upload", self._label(dptr), int(np.ascontiguousarray(arr).nbytes)])

    def download(self, dptr, arr):
        arr[...] = 0
        self.log.append(["download", self._label(dptr), int(arr.nbytes)])

    def staging(self, nbytes):
        self.log.append(["staging", int(nbytes)])
        return np.zeros(int(nbytes), dtype=np.uint8)

    def _down(self, kind, dptr, shape, dtype):
        shape = tuple(int(v) for v in np.atleast_1d(shape))
        self.log.append([kind, self._label(dptr), list(shape), np.dtype(dtype).name])
        return np.zeros(shape, dtype=dtype)

    def download_result(self, dptr, shape, dtype):
        return self._down("download_result", dptr, shape, dtype)

    def download_staged(self, dptr, shape, dtype):
        return self._down("download_staged", dptr, shape, dtype)

    def sync(self):
        self.log.append(["sync"])


def describe_result(r):
    if isinstance(r, np.ndarray):
        return ["ndarray", r.dtype.name, list(r.shape)]
    if isinstance(r, (tuple, list)):
        return [type(r).__name__, [describe_result(v) for v in r]]
    if isinstance(r, DevicePlanar):
        return ["DevicePlanar", r.n_ch, r.n_samples, r.ld, r.offset_bytes]
    if isinstance(r, backend.DeviceCSM):
        return ["DeviceCSM", r.n_bins, r.n_ch, int(r.buf.nbytes)]
    if isinstance(r, backend.DeviceSTFT):
        return ["DeviceSTFT", list(r.shape), r.power, int(r.buf.nbytes)]
    if isinstance(r, backend.DeviceScalogram):
        return ["DeviceScalogram", list(r.shape), r.dtype.name, int(r.buf.nbytes)]
    if isinstance(r, dsp.Spectrum):
        return ["Spectrum", r.number_of_channels, len(r.frequency_vector_hz)]
    return [type(r).__name__]


@contextlib.contextmanager
def patched(**values):
    """Module attributes of backend (thresholds, precisions) for the length of one case."""
    old = {k: getattr(backend, k) for k in values}
    try:
        for k, v in values.items():
            setattr(backend, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(backend, k, v)


def run_case(fn, **patch):
    """One case on a fresh stand-in -> {"log", "result" | "error", "warnings", "live"}."""
    ctx = RecordingContext()
    saved = backend.get_context, _lib.get_context
    backend.get_context = _lib.get_context = lambda: ctx
    out = {}
    try:
        with warnings.catch_warnings(record=True) as caught, patched(**patch):
            warnings.simplefilter("always")
            try:
                res = fn(ctx)
                out["result"] = describe_result(res)
            except Exception as e:  # noqa: BLE001
                res = None
                out["error"] = [type(e).__name__, str(e)]
            out["log"] = json.loads(json.dumps(ctx.log))  # (before `res` goes: its buffers are still alive)
            out["live"] = sorted(ctx.live)
            # every warning of the shim's own (a framing done twice warns twice); numpy's RuntimeWarnings about casting the
            # uninitialised results are not behaviour
            out["warnings"] = sorted(str(w.message) for w in caught if w.category is UserWarning)
            del res
    finally:
        backend.get_context, _lib.get_context = saved
    return out


def resident(ctx, n, n_ch, ld=None):
    """Device-resident planar samples of the stand-in (an allocation, nothing uploaded)."""
    ld = n if ld is None else ld
    return DevicePlanar(DeviceBuffer(ctx, 4 * n_ch * ld), n_ch, n, ld)


def cases():
    """name -> (function of the stand-in context, backend attributes patched for the case)."""
    fs, hann, bw = 48000, Window.Hann, SpectrumScaling.FFTBackward
    z = np.zeros
    c = {}

    def add(name, fn, **patch):
        assert name not in c, name
        c[name] = (fn, patch)

    def welch(x, y=None, W=16, ov=50.0, det=True, avg="mean", sc=bw, win=hann):
        return lambda ctx: backend._welch(x, y, fs, win, W, ov, det, avg, sc)

    def tf(y, x, W=16, mode="H1", **kw):
        return lambda ctx: backend.welch_transfer_function(y, x, fs, W, mode, **kw)

    def tf_dev(n, n_cy, n_cx, W=16, mode="H1", **kw):
        return lambda ctx: backend.welch_transfer_function_device(resident(ctx, n, n_cy), resident(ctx, n, n_cx, n + 3), fs,
                                                                   W, mode, **kw)

    def psd_dev(n, n_ch, W=16, ov=50.0, det=True, avg="mean", sc=bw, win=hann):
        return lambda ctx: backend._welch_psd_device(resident(ctx, n, n_ch), fs, win, W, ov, det, avg, sc)

    def csm(x, W=16, ov=50.0, det=True, avg="mean", sc=bw, win=hann):
        return lambda ctx: backend._csm_welch(x, fs, W, win, ov, det, avg, sc)

    def csm_dev(x, W=16, ov=50.0, det=True, avg="mean", sc=bw):
        return lambda ctx: backend._csm_welch_device(x(ctx) if callable(x) else x, fs, W, hann, ov, det, avg, sc)

    def csm_bins(x, b0, b1, W=16, ov=50.0, det=True, sc=bw):
        return lambda ctx: backend._csm_welch_bins(x, fs, W, hann, ov, det, sc, b0, b1)

    # ---- the smallest shape with several frames and a ragged last one: 100 samples, W = 16, 50 % overlap
    add("welch/flat", welch(z(100)))
    add("welch/2d", welch(z((100, 2))))
    add("welch/cross_flat", welch(z(100), z(100)))
    add("welch/cross_2d", welch(z((100, 3)), z((100, 3))))
    add("welch/median_auto", welch(z((100, 2)), avg="median"))
    add("welch/median_cross", welch(z((100, 2)), z((100, 2)), avg="median"))
    add("welch/no_detrend", welch(z((100, 2)), det=False))
    add("welch/non_cola", welch(z((100, 2)), ov=33.0))
    add("welch/overlap_0", welch(z((100, 2)), ov=0.0))
    add("welch/window_tuple", welch(z((100, 2)), win=("kaiser", 5.0)))
    for s in SpectrumScaling:
        add(f"welch/scaling_{s.name}", welch(z((100, 2)), sc=s))
        add(f"welch/f32_scaling_{s.name}", welch(z((100, 2)), sc=s), SPEC_PRECISION="f32")
    add("welch/f32_flat", welch(z(100)), SPEC_PRECISION="f32")
    add("welch/f32_cross", welch(z((100, 2)), z((100, 2))), SPEC_PRECISION="f32")
    add("welch/f32_cross_flat", welch(z(100), z(100), avg="median"), SPEC_PRECISION="f32")
    add("welch/f32_median_auto", welch(z((100, 2)), avg="median", det=False), SPEC_PRECISION="f32")
    add("welch/precision_illegal", welch(z((100, 2))), SPEC_PRECISION="f64")
    add("welch/frames_127", welch(z((508, 2)), W=8))
    add("welch/frames_128", welch(z((512, 2)), W=8))
    add("welch/cross_frames_127", welch(z((508, 2)), z((508, 2)), W=8))
    add("welch/cross_frames_128", welch(z((512, 2)), z((512, 2)), W=8))
    add("welch/short_bytes_at", welch(z((40, 2)), W=8), _X64_SHORT_BYTES=1600)       # 2 x 10 frames x 5 bins x 16
    add("welch/short_bytes_over", welch(z((40, 3)), W=8), _X64_SHORT_BYTES=1600)
    add("welch/cross_short_bytes_over", welch(z((40, 1)), z((40, 1)), W=8), _X64_SHORT_BYTES=1599)
    add("welch/fusable_at", welch(z((1 << 19, 2)), W=8))
    add("welch/fusable_under", welch(z(((1 << 19) - 1, 2)), W=8))
    add("welch/fusable_median", welch(z((1 << 19, 2)), W=8, avg="median"))
    add("welch/cross_fusable_at", welch(z((1 << 19, 2)), z((1 << 19, 2)), W=8))
    add("welch/cross_fusable_one_side", welch(z((1 << 19, 2)), z((1 << 19, 2), dtype=np.float32), W=8))
    add("welch/fusable_short", welch(z((1 << 17, 8)), W=1 << 16))  # a fusable array whose estimate is short
    add("welch/reject_window", welch(z((100, 2)), W=100))
    add("welch/reject_window_small", welch(z((100, 2)), W=4))
    add("welch/reject_overlap", welch(z((100, 2)), ov=100.0))
    add("welch/reject_overlap_negative", welch(z((100, 2)), ov=-1.0))
    add("welch/reject_average", welch(z((100, 2)), avg="max"))
    add("welch/reject_window_before_overlap", welch(z((100, 2)), W=100, ov=100.0, avg="max"))
    add("welch/reject_shapes", welch(z((100, 2)), z((100, 3))))
    add("welch/reject_ndim", welch(z((100, 2, 2))))

    # ---- transfer functions
    for mode in ("H1", "H2", "H3"):
        add(f"tf/{mode}", tf(z((100, 2)), z((100, 1)), mode=mode))
        add(f"tf/{mode}_auto", tf(z((100, 2)), z((100, 1)), mode=mode, precision="auto"))
        add(f"tf_dev/{mode}", tf_dev(100, 2, 1, mode=mode))
    add("tf/flat", tf(z(100), z(100)))
    add("tf/per_channel", tf(z((100, 3)), z((100, 3))))
    add("tf/per_channel_f64", tf(z((100, 3)), z((100, 3)), precision="f64"))
    add("tf/median", tf(z((100, 2)), z((100, 1)), average="median", detrend=False))
    add("tf/median_f64", tf(z((100, 2)), z((100, 1)), average="median", detrend=False, precision="f64"))
    add("tf/non_cola", tf(z((100, 2)), z((100, 1)), overlap_percent=33.0))
    add("tf/non_cola_auto", tf(z((100, 2)), z((100, 1)), overlap_percent=33.0, precision="auto"))
    for s in SpectrumScaling:
        add(f"tf/scaling_{s.name}", tf(z((100, 2)), z((100, 1)), scaling=s))
        add(f"tf/f64_scaling_{s.name}", tf(z((100, 2)), z((100, 1)), scaling=s, precision="f64"))
    add("tf/precision_f32", tf(z((100, 2)), z((100, 1)), precision="f32"))
    add("tf/precision_illegal", tf(z((100, 2)), z((100, 1)), precision="bad"))
    add("tf/auto_bytes_at", tf(z((800, 1)), z((800, 1)), W=8, precision="auto"), _X64_AUTO_BYTES=32000)  # 2 x 200 x 5 x 16
    add("tf/auto_bytes_over", tf(z((800, 2)), z((800, 1)), W=8, precision="auto"), _X64_AUTO_BYTES=32000)
    add("tf/frames_127", tf(z((508, 1)), z((508, 1)), W=8, precision="auto"), _X64_AUTO_BYTES=0)
    add("tf/frames_128", tf(z((512, 1)), z((512, 1)), W=8, precision="auto"), _X64_AUTO_BYTES=0)
    add("tf/short_bytes_at", tf(z((40, 1)), z((40, 1)), W=8, precision="auto"), _X64_AUTO_BYTES=0, _X64_SHORT_BYTES=1600)
    add("tf/short_bytes_over", tf(z((40, 2)), z((40, 1)), W=8, precision="auto"), _X64_AUTO_BYTES=0, _X64_SHORT_BYTES=1600)
    add("tf/median_4096", tf(z((16384, 1)), z((16384, 1)), W=8, average="median", precision="auto"))
    add("tf/median_4097", tf(z((16388, 1)), z((16388, 1)), W=8, average="median", precision="auto"))
    add("tf/median_4097_f64", tf(z((16388, 1)), z((16388, 1)), W=8, average="median", precision="f64"))
    add("tf/window_over_f64", tf(z((100, 1)), z((100, 1)), W=1 << 18, precision="f64"), _X64_MAX_WINDOW=1 << 17)
    add("tf/fusable_at", tf(z((1 << 19, 2)), z((1 << 19, 1)), W=8))
    add("tf/fusable_under", tf(z(((1 << 19) - 1, 2)), z(((1 << 19) - 1, 1)), W=8))
    add("tf/fusable_auto", tf(z((1 << 19, 2)), z((1 << 19, 1)), W=8, precision="auto"))
    add("tf/fusable_auto_large", tf(z((1 << 19, 2)), z((1 << 19, 1)), W=8, precision="auto", mode="H3"), _X64_AUTO_BYTES=0)
    add("tf/fusable_f64", tf(z((1 << 19, 2)), z((1 << 19, 2)), W=8, precision="f64"))
    add("tf/fusable_input_f32", tf(z((1 << 19, 2)), z((1 << 19, 1), dtype=np.float32), W=8))
    add("tf/reject_mode", tf(z((100, 2)), z((100, 1)), mode="H4"))
    add("tf/reject_window_before_mode", tf(z((100, 2)), z((100, 1)), W=100, mode="H4"))
    add("tf/reject_overlap", tf(z((100, 2)), z((100, 1)), overlap_percent=100.0))
    add("tf/reject_average", tf(z((100, 2)), z((100, 1)), average="max", mode="H4"))
    add("tf/reject_lengths", tf(z((100, 2)), z((90, 1))))
    add("tf/reject_lengths_f64", tf(z((100, 2)), z((90, 1)), precision="f64"))
    add("tf/reject_lengths_fused", tf(z((1 << 19, 2)), z((90, 1)), W=8))
    add("tf_dev/per_channel_median", tf_dev(100, 3, 3, average="median", detrend=False))
    add("tf_dev/narrow", tf_dev(100, 2, 1, narrow=True))
    add("tf_dev/non_cola", tf_dev(100, 2, 1, overlap_percent=33.0))
    add("tf_dev/scaling", tf_dev(100, 2, 1, scaling=SpectrumScaling.AmplitudeSpectralDensity))
    add("tf_dev/large_result", tf_dev(1 << 15, 40, 1, W=1 << 15))  # the result scratch grows beyond 4 MB
    add("tf_dev/reject_mode", tf_dev(100, 2, 1, mode="H4"))
    add("tf_dev/reject_window", tf_dev(100, 2, 1, W=100, mode="H4"))
    add("tf_dev/reject_overlap", tf_dev(100, 2, 1, overlap_percent=-2.0))
    add("tf_dev/reject_average", tf_dev(100, 2, 1, average="max"))
    add("tf_dev/reject_lengths", lambda ctx: backend.welch_transfer_function_device(
        resident(ctx, 100, 2), resident(ctx, 90, 1), fs, 16, "H1"))

    def tf_dev_twice(ctx):  # the second call finds the window and the result scratch in the context
        y, x = resident(ctx, 100, 2), resident(ctx, 100, 1)
        backend.welch_transfer_function_device(y, x, fs, 16, "H1")
        return backend.welch_transfer_function_device(y, x, fs, 16, "H2")
    add("tf_dev/twice", tf_dev_twice)

    # ---- auto spectra of resident samples
    add("psd_dev/mean", psd_dev(100, 2))
    add("psd_dev/median", psd_dev(100, 2, avg="median", det=False))
    add("psd_dev/non_cola", psd_dev(100, 2, ov=33.0))
    for s in SpectrumScaling:
        add(f"psd_dev/scaling_{s.name}", psd_dev(100, 2, sc=s))
    add("psd_dev/reject_window", psd_dev(100, 2, W=4))
    add("psd_dev/reject_overlap", psd_dev(100, 2, ov=100.0))
    add("psd_dev/reject_average", psd_dev(100, 2, avg="max"))

    # ---- cross-spectral matrices
    add("csm/2d", csm(z((100, 2))))
    add("csm/flat", csm(z(100)))
    add("csm/median", csm(z((100, 3)), avg="median", det=False))
    add("csm/non_cola", csm(z((100, 2)), ov=33.0))
    for s in SpectrumScaling:
        add(f"csm/scaling_{s.name}", csm(z((100, 2)), sc=s))
        add(f"csm/f32_scaling_{s.name}", csm(z((100, 2)), sc=s), SPEC_PRECISION="f32")
    add("csm/f32_median", csm(z((100, 3)), avg="median"), SPEC_PRECISION="f32")
    add("csm/precision_illegal", csm(z((100, 2))), SPEC_PRECISION="f64")
    add("csm/frames_127", csm(z((508, 2)), W=8))
    add("csm/frames_128", csm(z((512, 2)), W=8))
    add("csm/channels_1024", csm(z((16, 1024)), W=8))
    add("csm/channels_1025", csm(z((16, 1025)), W=8))
    add("csm/frame_bytes_at", csm(z((40, 2)), W=8), _X64_MATRIX_BYTES=1600)     # 2 x 10 frames x 5 bins x 16
    add("csm/frame_bytes_over", csm(z((40, 3)), W=8), _X64_MATRIX_BYTES=1600)
    add("csm/matrix_bytes_at", csm(z((8, 8)), W=8), _X64_MATRIX_BYTES=5120)     # 5 bins x 8 x 8 x 16
    add("csm/matrix_bytes_over", csm(z((8, 9)), W=8), _X64_MATRIX_BYTES=5120)
    add("csm/short_bytes_not_the_cap", csm(z((40, 2)), W=8), _X64_SHORT_BYTES=16)
    add("csm/fusable_at", csm(z((1 << 19, 2)), W=8))
    add("csm/fusable_under", csm(z(((1 << 19) - 1, 2)), W=8))
    add("csm/fusable_short", csm(z((1 << 17, 8)), W=1 << 16))
    add("csm/staged_at", csm(z((100, 2)), W=16), SPEC_PRECISION="f32", _STAGED_RESULT_BYTES=9 * 4 * 8)
    add("csm/staged_over", csm(z((100, 2)), W=16), SPEC_PRECISION="f32", _STAGED_RESULT_BYTES=9 * 4 * 8 - 1)
    add("csm/reject_window", csm(z((100, 2)), W=100))
    add("csm/reject_overlap", csm(z((100, 2)), ov=100.0))
    add("csm/reject_average", csm(z((100, 2)), avg="max"))
    add("csm_dev/host", csm_dev(z((100, 2))))
    add("csm_dev/host_flat", csm_dev(z(100)))
    add("csm_dev/resident", csm_dev(lambda ctx: resident(ctx, 100, 3, 104)))
    add("csm_dev/median_non_cola", csm_dev(z((100, 2)), ov=33.0, avg="median", det=False))
    add("csm_dev/scaling", csm_dev(z((100, 2)), sc=SpectrumScaling.PowerSpectralDensity))
    add("csm_dev/reject_window", csm_dev(z((100, 2)), W=100))
    add("csm_dev/reject_overlap", csm_dev(z((100, 2)), ov=100.0))
    add("csm_dev/reject_average", csm_dev(z((100, 2)), avg="max"))
    add("csm_bins/some", csm_bins(z((100, 2)), 2, 7))
    add("csm_bins/flat_no_detrend", csm_bins(z(100), 0, 9, det=False))
    add("csm_bins/non_cola_scaling", csm_bins(z((100, 2)), 1, 2, ov=33.0, sc=SpectrumScaling.AmplitudeSpectrum))
    add("csm_bins/empty", csm_bins(z((100, 2)), 5, 5))
    add("csm_bins/reversed", csm_bins(z((100, 2)), 5, 3))
    add("csm_bins/reject_window", csm_bins(z((100, 2)), 2, 7, W=100))
    add("csm_bins/reject_overlap", csm_bins(z((100, 2)), 2, 7, ov=100.0))

    # ---- the reference-shaped API: Signal.get_spectrum / get_csm and compute_transfer_function
    def signal(ctx, n, n_ch, on_device, W=16, **par):
        s = (dsp.Signal.from_planar_f32(resident(ctx, n, n_ch), fs) if on_device
             else dsp.Signal(None, np.zeros((n, n_ch)), fs))
        s.set_spectrum_parameters(window_length_samples=W, **par)
        return s

    def spectrum(n, n_ch, on_device, W=16, **par):
        return lambda ctx: signal(ctx, n, n_ch, on_device, W, **par).get_spectrum()

    def get_csm(n, n_ch, sig_on_device, on_device, W=16, **par):
        return lambda ctx: signal(ctx, n, n_ch, sig_on_device, W, **par).get_csm(on_device=on_device)

    def ctf(n, n_cy, n_cx, on_device, W=16, mode="H1", **par):
        def fn(ctx):
            x = signal(ctx, n, n_cx, on_device, W, **par)
            y = signal(ctx, n, n_cy, on_device, W)
            mode_ = dsp.transfer_functions.TransferFunctionType[mode] if isinstance(mode, str) and mode in ("H1", "H2", "H3") else mode
            return dsp.transfer_functions.compute_transfer_function(y, x, W, mode_)
        return fn

    add("signal/spectrum_host", spectrum(100, 2, False))
    add("signal/spectrum_resident_short", spectrum(100, 2, True))
    add("signal/spectrum_resident_short_f32", spectrum(100, 2, True), SPEC_PRECISION="f32")
    add("signal/spectrum_resident_frames_127", spectrum(508, 2, True, W=8))
    add("signal/spectrum_resident_frames_128", spectrum(512, 2, True, W=8))
    add("signal/spectrum_resident_median_non_cola", spectrum(512, 2, True, W=8, average="median", overlap_percent=33.0))
    add("signal/spectrum_resident_short_bytes_over", spectrum(40, 3, True, W=8), _X64_SHORT_BYTES=1600)
    add("signal/spectrum_resident_reject_window", spectrum(512, 2, True, W=100))
    add("signal/spectrum_resident_reject_overlap", spectrum(512, 2, True, W=8, overlap_percent=100.0))
    add("signal/spectrum_resident_precision_illegal", spectrum(512, 2, True, W=8), SPEC_PRECISION="f64")
    add("signal/csm_host", get_csm(100, 2, False, False))
    add("signal/csm_host_long", get_csm(512, 2, False, False, W=8))
    add("signal/csm_resident_signal", get_csm(100, 2, True, False))
    add("signal/csm_on_device", get_csm(100, 2, False, True))
    add("signal/csm_on_device_resident", get_csm(100, 2, True, True))
    add("signal/csm_one_channel", get_csm(100, 1, False, False))
    for mode in ("H1", "H2", "H3"):
        add(f"ctf/host_{mode}", ctf(100, 2, 1, False, mode=mode))
        add(f"ctf/resident_{mode}", ctf(100, 2, 1, True, mode=mode), TF_PRECISION="f32")
    add("ctf/resident_auto_small", ctf(100, 2, 1, True))
    add("ctf/resident_f64", ctf(100, 2, 1, True), TF_PRECISION="f64")
    add("ctf/resident_precision_illegal", ctf(100, 2, 1, True), TF_PRECISION="bad")
    add("ctf/host_precision_illegal", ctf(100, 2, 1, False), TF_PRECISION="bad")
    add("ctf/host_f32", ctf(100, 2, 2, False), TF_PRECISION="f32")
    add("ctf/host_f64", ctf(100, 2, 2, False, average="median"), TF_PRECISION="f64")
    add("ctf/resident_auto_bytes_at", ctf(800, 1, 1, True, W=8), _X64_AUTO_BYTES=32000)
    add("ctf/resident_auto_bytes_over", ctf(800, 2, 1, True, W=8), _X64_AUTO_BYTES=32000)
    add("ctf/resident_frames_127", ctf(508, 1, 1, True, W=8), _X64_AUTO_BYTES=0)
    add("ctf/resident_frames_128", ctf(512, 1, 1, True, W=8), _X64_AUTO_BYTES=0)
    add("ctf/resident_median_4096", ctf(16384, 1, 1, True, W=8, average="median"))
    add("ctf/resident_median_4097", ctf(16388, 1, 1, True, W=8, average="median"))
    add("ctf/resident_median_4097_f64", ctf(16388, 1, 1, True, W=8, average="median"), TF_PRECISION="f64")
    add("ctf/resident_non_cola", ctf(512, 2, 1, True, W=8, overlap_percent=33.0), TF_PRECISION="f32")
    add("ctf/resident_non_cola_f64", ctf(100, 2, 1, True, overlap_percent=33.0))
    add("ctf/resident_per_channel", ctf(512, 2, 2, True, W=8, detrend=False), TF_PRECISION="f32")
    add("ctf/resident_reject_window", ctf(512, 2, 1, True, W=100))
    add("ctf/resident_reject_overlap", ctf(512, 2, 1, True, W=8, overlap_percent=100.0))
    add("ctf/reject_mode", ctf(100, 2, 1, True, mode="H1 please"))
    add("ctf/reject_channels", ctf(100, 2, 3, False))

    # ---- the other functions that hold device buffers
    def stft_dev(keep, **kw):
        return lambda ctx: backend._stft_device(resident(ctx, 100, 2), fs, 16, hann, kw.get("ov", 50.0), kw.get("nfft"),
                                                True, kw.get("pad", True), kw.get("sc", bw), keep)
    add("stft_dev/array", stft_dev(False))
    add("stft_dev/keep", stft_dev(True))
    add("stft_dev/keep_power_nfft", stft_dev(True, nfft=32, sc=SpectrumScaling.PowerSpectrum, pad=False))
    add("stft_dev/reject_window", lambda ctx: backend._stft_device(resident(ctx, 100, 2), fs, 8, hann, 50.0, None, True, True,
                                                                   bw, True))
    add("stft_dev/non_cola", stft_dev(False, ov=33.0))

    def istft_dev(nfft=16, W=16, power=False):
        def fn(ctx):
            st = backend.DeviceSTFT(DeviceBuffer(ctx, 9 * 13 * 2 * 8), (9, 13, 2), power)
            return backend._istft_device(st, nfft, W, 8, np.ones(W), 0.5, 1, 15)
        return fn
    add("istft_dev/plain", istft_dev())
    add("istft_dev/reject_nfft", istft_dev(nfft=1))
    add("istft_dev/reject_power", istft_dev(power=True))
    add("istft_dev/reject_window", istft_dev(nfft=16, W=32))

    filt = np.zeros((4, 9))
    filt[0, 1:4], filt[1, 3:6], filt[3, 5:9] = 1.0, 0.5, 0.25

    def band_power(on_device, filters=filt, to_db=True, dct_abs=False):
        return lambda ctx: backend._spectrogram_band_power(
            resident(ctx, 100, 2, 112) if on_device else np.zeros((100, 2)), fs, 16, hann, 50.0, None, True, True, bw, filters,
            to_db, dct_abs)
    add("band_power/host", band_power(False))
    add("band_power/resident", band_power(True, to_db=False, dct_abs=True))
    add("band_power/reject_filters", band_power(False, filters=np.zeros((4, 8))))

    taps = [np.ones(5), np.ones(5) * 0.5, np.ones(5) * 0.25]
    for name, mode in (("parallel", backend.DS_FB_PARALLEL), ("sequential", backend.DS_FB_SEQUENTIAL),
                       ("summed", backend.DS_FB_SUMMED)):
        add(f"fir_bank_dev/{name}", lambda ctx, m=mode: backend.fir_filter_bank_device(resident(ctx, 100, 2, 104), taps, m))
        add(f"iir_dev/{name}", lambda ctx, m=mode: backend.iir_sos_filter_device(
            resident(ctx, 100, 2, 104), [np.array([[1.0, 0, 0, 1, 0, 0]]), np.array([[1.0, 0, 0, 1, 0, 0]] * 2)], m))
    add("iir_dev/sequential_long", lambda ctx: backend.iir_sos_filter_device(
        resident(ctx, 100, 2), [np.array([[1.0, 0, 0, 1, 0, 0]] * 20)] * 2, backend.DS_FB_SEQUENTIAL))

    def division(n_cx, eps):
        return lambda ctx: backend.spectral_division_device(resident(ctx, 100, 2), resident(ctx, 100, n_cx, 101), 128, 120,
                                                            (lambda den: np.ones(den.shape[0])) if eps else None)
    add("division_dev/plain", division(1, False))
    add("division_dev/regularized_per_channel", division(2, True))
    add("division_dev/reject_lengths", lambda ctx: backend.spectral_division_device(
        resident(ctx, 100, 2), resident(ctx, 90, 1), 128, 120))
    add("regularized_inverse/eps", lambda ctx: backend.regularized_inverse(np.ones((9, 2), dtype=complex), np.ones(9)))
    add("regularized_inverse/plain", lambda ctx: backend.regularized_inverse(np.ones((9, 2), dtype=complex)))

    def das_dev(diag, n_grid=5):
        def fn(ctx):
            m = backend.DeviceCSM(ctx, DeviceBuffer(ctx, 9 * 3 * 3 * 8), np.fft.rfftfreq(16, 1 / fs), 3)
            return backend._das_map_device(m, 2, 6, np.ones((4, 3, n_grid), dtype=complex), diag)
        return fn
    add("das_dev/plain", das_dev(False))
    add("das_dev/no_diagonal", das_dev(True))

    def delay_dev(ctx):
        return backend.delay_sum_device(resident(ctx, 100, 3), [100, 90, 80], np.array([[0, 1], [2, 0]]), [[3, 4], [5, 6]],
                                        [[0.25, -1.0], [0.5, 0.75]], 1.0, 11, 60.0, 120)
    add("delay_dev/sum", delay_dev)
    add("delay_dev/stack", lambda ctx: backend.stack_device([resident(ctx, 100, 1), resident(ctx, 80, 1, 96)], [100, 80]))
    waves = [np.ones(5, dtype=complex), np.ones(9, dtype=complex)]
    add("cwt_dev/transform", lambda ctx: backend.cwt_device(resident(ctx, 100, 3), [0, 2], waves))
    add("cwt_dev/reject_empty_wavelet", lambda ctx: backend.cwt_device(resident(ctx, 100, 3), [0], [np.ones(0)]))

    def squeeze(norm):
        def fn(ctx):
            sc = backend.DeviceScalogram(DeviceBuffer(ctx, 2 * 100 * 2 * 8), (2, 100, 2), np.complex64)
            return backend.cwt_squeeze_device(sc, [1000.0, 2000.0], fs, apply_frequency_normalization=norm)
        return fn
    add("cwt_dev/squeeze", squeeze(False))
    add("cwt_dev/squeeze_normalized", squeeze(True))
    return c


def xform_cases():
    """The same for the functions that are no Welch estimate: name -> (function of the stand-in context, patches)."""
    fs, hann, bw = 48000, Window.Hann, SpectrumScaling.FFTBackward
    z = np.zeros
    big = z((1 << 19, 2))  # _fusable: float64, C order, 2^20 values (never written: shared by the cases)
    c = {}

    def add(name, fn, **patch):
        assert name not in c, name
        c[name] = (fn, patch)

    # ---- _stft: 100 samples x 2 channels, W = 16, 50 % overlap
    def stft(x, W=16, ov=50.0, nfft=None, det=True, pad=True, sc=bw, win=hann):
        return lambda ctx: backend._stft(x, fs, W, win, ov, nfft, det, pad, sc)
    add("stft/planar", stft(z((100, 2))))
    add("stft/flat", stft(z(100)))
    add("stft/list", stft([[0.0, 0.0]] * 100))
    add("stft/fusable", stft(big))
    add("stft/fusable_under", stft(z(((1 << 19) - 1, 2))))
    add("stft/large_float32", stft(z((1 << 19, 2), dtype=np.float32)))
    add("stft/fusable_power", stft(big, sc=SpectrumScaling.PowerSpectrum))  # (the plan used to be built twice)
    add("stft/fusable_power_non_cola", stft(big, sc=SpectrumScaling.PowerSpectrum, ov=33.0))
    add("stft/fusable_non_cola", stft(big, ov=33.0))
    add("stft/fusable_nfft_24_no_padding", stft(big, nfft=24, pad=False, det=False))
    for s in SpectrumScaling:
        add(f"stft/scaling_{s.name}", stft(z((100, 2)), sc=s))
    add("stft/nfft_12", stft(z((100, 2)), nfft=12))
    add("stft/nfft_32", stft(z((100, 2)), nfft=32))
    add("stft/nfft_24", stft(z((100, 2)), nfft=24))
    add("stft/nfft_32_power_density", stft(z((100, 2)), nfft=32, sc=SpectrumScaling.PowerSpectralDensity))
    add("stft/no_padding", stft(z((100, 2)), pad=False))
    add("stft/no_detrend", stft(z((100, 2)), det=False))
    add("stft/non_cola", stft(z((100, 2)), ov=33.0))
    add("stft/overlap_0", stft(z((100, 2)), ov=0.0))
    add("stft/window_tuple", stft(z((100, 2)), win=("kaiser", 5.0)))
    add("stft/reject_window_8", stft(z((100, 2)), W=8))
    add("stft/reject_window_2_17", stft(z((100, 2)), W=1 << 17))
    add("stft/reject_overlap_100", stft(z((100, 2)), ov=100.0))
    add("stft/reject_overlap_negative", stft(z((100, 2)), ov=-1.0))
    add("stft/reject_nfft_1", stft(z((100, 2)), nfft=1))
    add("stft/reject_window_before_overlap", stft(z((100, 2)), W=8, ov=100.0, nfft=1))
    add("stft/reject_overlap_before_nfft", stft(z((100, 2)), ov=100.0, nfft=1))
    add("stft/reject_ndim", stft(z((100, 2, 2))))
    add("stft/fusable_reject_window", stft(big, W=8))
    add("stft/fusable_reject_nfft_1", stft(big, nfft=1, sc=SpectrumScaling.PowerSpectrum))

    def stft_dev(keep, n=100, n_ch=2, ld=None, **kw):
        return lambda ctx: backend._stft_device(resident(ctx, n, n_ch, ld), fs, kw.get("W", 16), hann, kw.get("ov", 50.0),
                                                kw.get("nfft"), kw.get("det", True), kw.get("pad", True), kw.get("sc", bw), keep)
    add("stft_dev/array_ld", stft_dev(False, ld=104))
    add("stft_dev/keep_no_detrend_nfft_12", stft_dev(True, nfft=12, det=False))
    add("stft_dev/array_power", stft_dev(False, sc=SpectrumScaling.PowerSpectralDensity))
    add("stft_dev/array_large", stft_dev(False, n=1 << 17, n_ch=2))  # 2^20 values and more come down in chunks
    add("stft_dev/reject_overlap", stft_dev(True, ov=100.0))
    add("stft_dev/reject_nfft", stft_dev(True, nfft=1))

    def stft_dev_twice(ctx):  # the second call finds the window in the context
        x = resident(ctx, 100, 2)
        backend._stft_device(x, fs, 16, hann, 50.0, None, True, True, bw, True)
        return backend._stft_device(x, fs, 16, hann, 50.0, 32, False, True, SpectrumScaling.AmplitudeSpectrum, False)
    add("stft_dev/twice", stft_dev_twice)

    filt = np.zeros((4, 9))
    filt[0, 1:4], filt[1, 3:6], filt[3, 5:9] = 1.0, 0.5, 0.25

    def band_power(on_device, filters=filt, to_db=True, dct_abs=False, **kw):
        return lambda ctx: backend._spectrogram_band_power(
            resident(ctx, 100, 2, 112) if on_device else kw.get("x", np.zeros((100, 2))), fs, kw.get("W", 16), hann,
            kw.get("ov", 50.0), kw.get("nfft"), kw.get("det", True), kw.get("pad", True), kw.get("sc", bw), filters, to_db, dct_abs)
    add("band_power/host", band_power(False))
    add("band_power/host_flat", band_power(False, x=np.zeros(100)))
    add("band_power/host_no_detrend_no_padding", band_power(False, det=False, pad=False, to_db=False))
    add("band_power/host_nfft_24", band_power(False, filters=np.ones((2, 13)), nfft=24))
    add("band_power/resident", band_power(True, to_db=False, dct_abs=True))
    add("band_power/resident_non_cola_power", band_power(True, ov=33.0, sc=SpectrumScaling.PowerSpectrum))
    add("band_power/reject_filters", band_power(False, filters=np.zeros((4, 8))))
    add("band_power/reject_filters_resident", band_power(True, filters=np.zeros(9)))
    add("band_power/reject_window", band_power(False, W=8))
    add("band_power/reject_window_resident", band_power(True, W=8))

    # ---- _istft
    def istft(spec, nfft=16, W=16, step=8, offset=1, total=None):
        return lambda ctx: backend._istft(spec, nfft, W, step, np.ones(W), 0.5, offset,
                                          np.shape(spec)[1] + 2 if total is None else total)
    add("istft/small", istft(z((9, 13, 2), dtype=np.complex128)))
    add("istft/small_complex64", istft(z((9, 13, 2), dtype=np.complex64), offset=0, total=13))
    add("istft/real", istft(z((9, 13, 2))))
    add("istft/nfft_24_window_16", istft(z((13, 13, 2), dtype=np.complex128), nfft=24))
    add("istft/fused_at", istft(z((8, 1 << 15, 2), dtype=np.complex128), nfft=14, W=8, step=4))        # 2^19 values
    add("istft/fused_under", istft(z((1, (1 << 19) - 1, 1), dtype=np.complex128), nfft=2, W=2, step=1))  # (2^19 - 1 is prime)
    add("istft/large_real", istft(z((8, 1 << 15, 2)), nfft=14, W=8, step=4))
    add("istft/large_complex64", istft(z((8, 1 << 15, 2), dtype=np.complex64), nfft=14, W=8, step=4))
    add("istft/large_not_contiguous", istft(z((2, 1 << 15, 8), dtype=np.complex128).transpose(2, 1, 0), nfft=14, W=8, step=4))
    add("istft/reject_nfft", istft(z((9, 13, 2), dtype=np.complex128), nfft=1))
    add("istft/reject_window", istft(z((9, 13, 2), dtype=np.complex128), nfft=16, W=32))
    add("istft/fused_reject_window", istft(z((8, 1 << 15, 2), dtype=np.complex128), nfft=14, W=16))

    def istft_dev(nfft=16, W=16, power=False):
        def fn(ctx):
            st = backend.DeviceSTFT(DeviceBuffer(ctx, 9 * 13 * 2 * 8), (9, 13, 2), power)
            return backend._istft_device(st, nfft, W, 8, np.ones(W), 0.5, 1, 15)
        return fn
    add("istft_dev/plain", istft_dev())

    # ---- rfft_spectrum
    add("rfft/planar", lambda ctx: backend.rfft_spectrum(z((100, 2)), 128))
    add("rfft/flat", lambda ctx: backend.rfft_spectrum(z(100), 128))
    add("rfft/list", lambda ctx: backend.rfft_spectrum([[0.0, 0.0]] * 100, 128))
    add("rfft/scale", lambda ctx: backend.rfft_spectrum(z((100, 2)), 100, 0.5))
    add("rfft/fusable", lambda ctx: backend.rfft_spectrum(big, 1 << 19))
    add("rfft/fusable_scale", lambda ctx: backend.rfft_spectrum(big, 1 << 20, 0.25))
    add("rfft/fusable_under", lambda ctx: backend.rfft_spectrum(z(((1 << 19) - 1, 2)), 1 << 19))
    add("rfft/large_float32", lambda ctx: backend.rfft_spectrum(z((1 << 19, 2), dtype=np.float32), 1 << 19))

    # ---- spectral_division
    def division(num, n_fft, inv, n_out):
        return lambda ctx: backend.spectral_division(num, n_fft, inv, n_out)
    one = np.ones(65, dtype=complex)
    add("division/one_shared", division(z((100, 2)), 128, one, 120))
    add("division/one_per_channel", division(z((100, 2)), 128, np.ones((65, 2), dtype=complex), 120))
    add("division/batch_3", division(z((3, 100, 2)), 128, one, 120))
    add("division/batch_3_per_channel", division(z((3, 100, 2)), 128, np.ones((65, 2), dtype=complex), 100))
    inv_big = np.ones((1 << 18) + 1, dtype=complex)
    add("division/fusable_shared", division(big, 1 << 19, inv_big, 100))
    add("division/fusable_per_channel", division(big, 1 << 19, np.ones(((1 << 18) + 1, 2), dtype=complex), 1 << 19))
    add("division/batch_of_fusable_items", division(z((2, 1 << 19, 2)), 1 << 19, inv_big, 100))
    add("division/large_float32", division(z((1 << 19, 2), dtype=np.float32), 1 << 19, inv_big, 100))
    inv_20 = np.ones((1 << 19) + 1, dtype=complex)
    add("division/transposes_at", division(z((1, 1 << 20, 1)), 1 << 20, inv_20, 1 << 20))  # n * n_ch and n_out * n_ch = 2^20
    add("division/transposes_under", division(z((1, (1 << 20) - 1, 1)), 1 << 20, inv_20, (1 << 20) - 1))
    add("division/transpose_in_at_out_under", division(z((1, 1 << 19, 2)), 1 << 20, inv_20, (1 << 19) - 1))
    add("division/reject_inverse_length", division(z((100, 2)), 128, np.ones(64, dtype=complex), 120))
    add("division/reject_inverse_length_per_channel", division(z((100, 2)), 128, np.ones((2, 65), dtype=complex), 120))
    add("division/fusable_reject_inverse_length", division(big, 1 << 19, np.ones(64, dtype=complex), 100))

    def division_dev(n_cx, eps):
        return lambda ctx: backend.spectral_division_device(resident(ctx, 100, 2), resident(ctx, 100, n_cx, 101), 128, 120,
                                                            (lambda den: np.ones(den.shape[0])) if eps else None)
    add("division_dev/plain", division_dev(1, False))
    add("division_dev/regularized_per_channel", division_dev(2, True))

    # ---- FIR filter banks
    taps = [np.ones(5), np.ones(5) * 0.5, np.ones(5) * 0.25]
    modes = (("parallel", backend.DS_FB_PARALLEL), ("sequential", backend.DS_FB_SEQUENTIAL), ("summed", backend.DS_FB_SUMMED))
    for name, mode in modes:
        add(f"fir_bank/{name}", lambda ctx, m=mode: backend.fir_filter_bank(z((100, 2)), taps, m))
        add(f"fir_bank/{name}_fusable", lambda ctx, m=mode: backend.fir_filter_bank(big, taps, m))
        add(f"fir_bank_dev/{name}", lambda ctx, m=mode: backend.fir_filter_bank_device(resident(ctx, 100, 2, 104), taps, m))
    add("fir_bank/flat", lambda ctx: backend.fir_filter_bank(z(100), taps[:1], backend.DS_FB_PARALLEL))
    add("fir_bank/fusable_under", lambda ctx: backend.fir_filter_bank(z(((1 << 19) - 1, 2)), taps[:1], backend.DS_FB_SUMMED))
    add("fir_bank/unequal_taps", lambda ctx: backend.fir_filter_bank(z((100, 2)), [np.ones(5), np.ones(4)], backend.DS_FB_PARALLEL))
    add("fir_bank/unequal_taps_fusable", lambda ctx: backend.fir_filter_bank(big, [np.ones(5), np.ones(4)], backend.DS_FB_PARALLEL))
    add("fir_bank_dev/unequal_taps", lambda ctx: backend.fir_filter_bank_device(resident(ctx, 100, 2), [np.ones(5), np.ones(4)],
                                                                                 backend.DS_FB_PARALLEL))

    def lfilter(b, x, zi=None, a=(1.0,)):
        return lambda ctx: backend._lfilter_fir(b, a, x, zi)
    add("lfilter_fir/plain", lfilter(np.ones(5), z((100, 2))))
    add("lfilter_fir/column_taps", lfilter(np.ones((5, 1)), z((100, 2))))
    add("lfilter_fir/zi", lfilter(np.ones(5), z((100, 2)), z((4, 2))))
    add("lfilter_fir/flat", lfilter(np.ones(5), z(100)))
    add("lfilter_fir/flat_zi", lfilter(np.ones(5), z(100), z(4)))
    add("lfilter_fir/complex_taps", lfilter(np.ones(5) * (1 + 1j), z((100, 2))))
    add("lfilter_fir/complex_taps_zi", lfilter(np.ones(5) * (1 + 1j), z((100, 2)), z((4, 2), dtype=complex)))
    add("lfilter_fir/complex_taps_flat_zi", lfilter(np.ones(5) * (1 + 1j), z(100), z(4, dtype=complex)))
    add("lfilter_fir/fusable", lfilter(np.ones(5), big))
    add("lfilter_fir/reject_a", lfilter(np.ones(5), z((100, 2)), a=(1.0, 0.5)))
    add("lfilter_fir/reject_taps_2d", lfilter(np.ones((2, 5)), z((100, 2))))
    add("lfilter_fir/reject_complex_signal", lfilter(np.ones(5), z((100, 2), dtype=complex)))
    add("lfilter_fir/reject_zi_ndim", lfilter(np.ones(5), z((100, 2)), z(4)))
    add("lfilter_fir/reject_ndim", lfilter(np.ones(5), z((100, 2, 2))))
    add("lfilter_fir/reject_ndim_complex_taps", lfilter(np.ones(5) * 1j, z((100, 2, 2))))
    add("lfilter_fir/reject_a_before_complex_signal", lfilter(np.ones((2, 5)), z((100, 2), dtype=complex), a=(1.0, 0.5)))

    add("fir_freqz/two", lambda ctx: backend.fir_transfer_function([np.ones(5), np.ones(3)], np.linspace(0, 24000, 9), fs))
    add("fir_freqz/reject_frequencies", lambda ctx: backend.fir_transfer_function([np.ones(5)], z((9, 2)), fs))

    # ---- beamformer maps and their spectra
    def bf(fn, csm_shape=(4, 3, 3), h_shape=(4, 3, 5), *args):
        return lambda ctx: fn(np.zeros(csm_shape, dtype=complex), np.ones(h_shape, dtype=complex), *args)
    for name, fn, args in (("das", backend._das_map, ()), ("eig_map", backend.beamformer_eig_map, ("mvdr",)),
                           ("cleansc", backend.beamformer_cleansc_map, (10, 0.5, True))):
        add(f"{name}/plain", bf(fn, (4, 3, 3), (4, 3, 5), *args))
        add(f"{name}/reject_csm", bf(fn, (4, 3, 2), (4, 3, 5), *args))
        add(f"{name}/reject_csm_ndim", bf(fn, (3, 3), (4, 3, 5), *args))
        add(f"{name}/reject_steering_bins", bf(fn, (4, 3, 3), (3, 3, 5), *args))
        add(f"{name}/reject_steering_channels", bf(fn, (4, 3, 3), (4, 2, 5), *args))
    add("das/float32_inputs", lambda ctx: backend._das_map(np.zeros((4, 3, 3), dtype=np.float32), np.ones((4, 3, 1))))
    add("eig_map/functional", bf(backend.beamformer_eig_map, (4, 3, 3), (4, 3, 5), "functional", 4.0))
    add("eig_map/orthogonal", bf(backend.beamformer_eig_map, (4, 3, 3), (4, 3, 5), "orthogonal", 10.0, 2))
    add("eig_map/reject_method", bf(backend.beamformer_eig_map, (4, 3, 3), (4, 3, 5), "music"))
    add("cleansc/keep_diagonal", bf(backend.beamformer_cleansc_map, (4, 3, 3), (4, 3, 5), 3, 0.25, False))
    add("eigh/plain", lambda ctx: backend.hermitian_eigh(np.zeros((4, 3, 3), dtype=complex)))
    add("eigh/real", lambda ctx: backend.hermitian_eigh(np.zeros((4, 3, 3))))
    add("eigh/reject_shape", lambda ctx: backend.hermitian_eigh(np.zeros((4, 3, 2), dtype=complex)))
    for s in SpectrumScaling:
        add(f"csm_fft/scaling_{s.name}", lambda ctx, s=s: backend._csm_fft(np.zeros((9, 2), dtype=complex), s, None, fs))
    add("csm_fft/window", lambda ctx: backend._csm_fft(np.zeros((9, 2), dtype=complex), bw, np.ones(16), fs))

    # ---- IIR cascades
    ident = [1.0, 0, 0, 1, 0, 0]
    sos2 = [np.array([ident]), np.array([ident] * 2)]
    for name, mode in modes:
        add(f"iir/{name}", lambda ctx, m=mode: backend.iir_sos_filter(z((100, 2)), sos2, m))
        add(f"iir/{name}_zi", lambda ctx, m=mode: backend.iir_sos_filter(z((100, 2)), sos2, m, zi=z((2, 2, 2, 2))))
        add(f"iir_dev/{name}", lambda ctx, m=mode: backend.iir_sos_filter_device(resident(ctx, 100, 2, 104), sos2, m))
    add("iir/flat", lambda ctx: backend.iir_sos_filter(z(100), sos2, backend.DS_FB_PARALLEL))
    add("iir/one_section_flat", lambda ctx: backend.iir_sos_filter(z((100, 2)), [np.array(ident)], backend.DS_FB_SUMMED))
    add("iir/sequential_32", lambda ctx: backend.iir_sos_filter(z((100, 2)), [np.array([ident] * 16)] * 2, backend.DS_FB_SEQUENTIAL))
    add("iir/sequential_40", lambda ctx: backend.iir_sos_filter(z((100, 2)), [np.array([ident] * 20)] * 2, backend.DS_FB_SEQUENTIAL))
    add("iir/sequential_3x15", lambda ctx: backend.iir_sos_filter(z((100, 2)), [np.array([ident] * 15)] * 3, backend.DS_FB_SEQUENTIAL))
    add("iir/sequential_40_zi", lambda ctx: backend.iir_sos_filter(z((100, 2)), [np.array([ident] * 20)] * 2,
                                                                   backend.DS_FB_SEQUENTIAL, zi=z((2, 20, 2, 2))))
    add("iir/parallel_40", lambda ctx: backend.iir_sos_filter(z((100, 2)), [np.array([ident] * 40)], backend.DS_FB_PARALLEL))
    add("iir/reject_zi_shape", lambda ctx: backend.iir_sos_filter(z((100, 2)), sos2, backend.DS_FB_PARALLEL, zi=z((2, 2, 2, 3))))
    add("iir/reject_zi_shape_sequential", lambda ctx: backend.iir_sos_filter(z((100, 2)), sos2, backend.DS_FB_SEQUENTIAL,
                                                                             zi=z((1, 3, 2, 2))))
    add("iir_dev/sequential_32", lambda ctx: backend.iir_sos_filter_device(
        resident(ctx, 100, 2), [np.array([ident] * 16)] * 2, backend.DS_FB_SEQUENTIAL))
    add("iir_dev/sequential_long", lambda ctx: backend.iir_sos_filter_device(
        resident(ctx, 100, 2), [np.array([ident] * 20)] * 2, backend.DS_FB_SEQUENTIAL))
    add("iir_dev/sequential_3x15", lambda ctx: backend.iir_sos_filter_device(
        resident(ctx, 100, 2, 104), [np.array([ident] * 15)] * 3, backend.DS_FB_SEQUENTIAL))

    # ---- the reference-shaped callers that build an STFT plan
    def signal(ctx, on_device, n=100, n_ch=2, **par):
        s = (dsp.Signal.from_planar_f32(resident(ctx, n, n_ch), fs) if on_device else dsp.Signal(None, np.zeros((n, n_ch)), fs))
        s.set_spectrogram_parameters(**{"window_length_samples": 16, **par})
        return s

    def spectrogram(sig_on_device, on_device=False, **par):
        return lambda ctx: signal(ctx, sig_on_device, **par).get_spectrogram(on_device=on_device)

    def round_trip(sig_on_device, on_device, **par):
        def fn(ctx):
            s = signal(ctx, sig_on_device, **par)
            return dsp.transforms.istft(s.get_spectrogram(on_device=on_device)[2], original_signal=s)
        return fn
    for where, dev in (("host", False), ("resident", True)):
        add(f"signal/spectrogram_{where}", spectrogram(dev))
        add(f"signal/spectrogram_{where}_on_device", spectrogram(dev, True))
        add(f"signal/spectrogram_{where}_non_cola_power", spectrogram(dev, overlap_percent=33.0, detrend=True,
                                                                      scaling=SpectrumScaling.PowerSpectrum))
        add(f"signal/spectrogram_{where}_reject_window", spectrogram(dev, window_length_samples=8))
        add(f"signal/istft_{where}", round_trip(dev, False))
        add(f"signal/istft_{where}_on_device", round_trip(dev, True))
        add(f"signal/istft_{where}_on_device_no_padding", round_trip(dev, True, padding=False, fft_length_samples=32))
        add(f"signal/log_mel_{where}", lambda ctx, dev=dev: dsp.transforms.log_mel_spectrogram(
            signal(ctx, dev, n=300, window_length_samples=64), n_bands=4, generate_plot=False))
        add(f"signal/mfcc_{where}", lambda ctx, dev=dev: dsp.transforms.mfcc(
            signal(ctx, dev, n=300, window_length_samples=64), mel_filters=np.ones((3, 33)), generate_plot=False))
        add(f"signal/chroma_{where}", lambda ctx, dev=dev: dsp.transforms.chroma_stft(
            signal(ctx, dev, n=300, window_length_samples=64)))
        add(f"signal/axes_{where}", lambda ctx, dev=dev: dsp.transforms._spectrogram_axes(signal(ctx, dev)))
        add(f"signal/axes_{where}_nfft_24_non_cola", lambda ctx, dev=dev: dsp.transforms._spectrogram_axes(
            signal(ctx, dev, fft_length_samples=24, overlap_percent=33.0, padding=False)))
        add(f"signal/axes_{where}_reject_overlap", lambda ctx, dev=dev: dsp.transforms._spectrogram_axes(
            signal(ctx, dev, overlap_percent=100.0)))
    add("signal/log_mel_bin_mismatch", lambda ctx: dsp.transforms.log_mel_spectrogram(
        signal(ctx, False, n=300, window_length_samples=64, fft_length_samples=32), n_bands=4, generate_plot=False))
    return c


def record(case_list=cases):
    """name -> transcript of every case of `cases` or `xform_cases`."""
    return {name: run_case(fn, **patch) for name, (fn, patch) in case_list().items()}


def entries_reached(transcript):
    return {e[1] for case in transcript.values() for e in case["log"] if e[0] == "call"}


if __name__ == "__main__":
    which = {"welch": (cases, FIXTURE, WELCH_ENTRIES), "xform": (xform_cases, FIXTURE_XFORM, XFORM_ENTRIES)}
    if len(sys.argv) != 2 or sys.argv[1] not in which:
        sys.exit("usage: record_backend_calls.py welch|xform   (rewrites that fixture from the shim as it is NOW)")
    case_list, fixture, entries = which[sys.argv[1]]
    t = record(case_list)
    missing = sorted(set(entries) - entries_reached(t))
    assert not missing, f"no case reaches {missing}"
    with open(fixture, "w") as f:
        json.dump(t, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{len(t)} cases, {sum(len(c['log']) for c in t.values())} events, entries: {sorted(entries_reached(t))}")
