"""Resident entries on poisoned, pitched, offset views against dense uploads.

A. Every case of view_cases.ENTRIES (and of what the library builds on them) runs once on a dense upload and on three
   views x two poisons of the same samples; every result must have the dense result's shape and dtype, be finite where
   it is, and equal it bit for bit: the kernels index by sample number, sum in a fixed order, and their address-dependent
   variants change how values are moved, not how they are summed.
B. The views the library itself builds (a trimmed inverse STFT, a padded or trimmed signal, a warped response cut to
   total_length) fed to its public calls, against the same call on a dense re-upload of the view's samples.
C. Output pitch through the C ABI: rows of pitch n_out + 3 from a base one float into a poisoned buffer; the valid
   samples equal the dense call's, every other byte keeps its poison."""

import ctypes as C

import numpy as np
import pytest

import view_cases as vc
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DeviceBuffer, DeviceError, DevicePlanar, get_context

pytestmark = pytest.mark.gpu

CASES = vc.all_cases()


def bits(a):
    """the values of a real or complex array as unsigned integers (complex: real and imaginary parts side by side)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    a = a.view(a.real.dtype) if np.iscomplexobj(a) else a
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def parts(a):
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype) if np.iscomplexobj(a) else a


def same_bits(what, got, want):
    """shape and dtype; finite wherever `want` is; bit for bit equal there, equal (NaN as NaN) elsewhere"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape, g.dtype, w.dtype)
        diff = bits(g) != bits(w)
        if w.dtype != np.bool_:
            gp, wp = parts(g), parts(w)
            fin = np.isfinite(wp)
            bad = fin & ~np.isfinite(gp)
            assert not bad.any(), (what, i, "poison reached a result: not finite at", np.argwhere(bad)[:8].tolist())
            assert np.array_equal(gp[~fin], wp[~fin], equal_nan=True), (what, i, "differs where the dense result is not finite")
            diff &= fin
        at = np.argwhere(diff)[:4]
        assert not diff.any(), (what, i, f"{int(diff.sum())} of {diff.size} values differ from the dense result, first at",
                                at.tolist(), [parts(g)[tuple(j)] if w.dtype != np.bool_ else g[tuple(j)] for j in at],
                                [parts(w)[tuple(j)] if w.dtype != np.bool_ else w[tuple(j)] for j in at])


def upload_view(ctx, plane, front, gap, fill):
    owner, ld, off = vc.layout(plane, front, gap, fill)
    return DevicePlanar(DeviceBuffer.from_array(ctx, owner), plane.shape[0], plane.shape[1], ld, off)


def run_on(ctx, run, devs):
    ctx.routes()
    try:
        out = run(ctx, devs)
        ctx.sync()
    except DeviceError as e:
        if "illegal" in str(e) or "launch failure" in str(e):  # a faulted device runs nothing more of this session
            pytest.exit(f"device fault: {e}", returncode=3)
        raise
    finally:
        routes = sorted(ctx.routes())
        for d in devs:
            d.owner.free()
    return tuple(np.array(o) for o in out), routes


@pytest.mark.parametrize("case", CASES, ids=[vc.case_id(c) for c in CASES])
def test_views_give_the_dense_result(case):
    built = case.build()
    planes, run = built[:2]
    ctx = get_context()
    dense, dense_routes = run_on(ctx, run, [DevicePlanar.from_planar(ctx, p) for p in planes])
    print(f"{vc.case_id(case)}: dense launches {' '.join(dense_routes) or '-'}")
    changed, failed = set(), []
    if len(built) > 2:
        try:
            print(f"  dense result against the family's oracle: {built[2](dense):.3f} of its bound")
        except AssertionError as e:  # (the views are still run: the log shows what else the mistake reaches)
            failed.append(f"dense result against the family's oracle: {str(e)[:600]}")
    for v, view in enumerate(vc.VIEW_NAMES):
        for fill in vc.FILLS:
            # plane j lies in view v + j: two operands never share a layout
            devs = [upload_view(ctx, p, *vc.VIEWS(p.shape[1])[(v + j) % 3], fill) for j, p in enumerate(planes)]
            got, routes = run_on(ctx, run, devs)
            if routes != dense_routes:
                changed.add((view, " ".join(routes)))
            try:
                same_bits(f"{vc.case_id(case)} {view} {fill}", got, dense)
            except AssertionError as e:  # every view and poison is run: the log shows which of them a mistake reaches
                failed.append(str(e)[:600])
    for view, routes in sorted(changed):
        print(f"  {view}: launches {routes}")
    if not changed:
        print("  views: the same launches")
    assert not failed, "\n".join(failed)


# ---- B. the chains the library itself builds --------------------------------------------------------------------------------
FS = 48000


def dense_copy(sig):
    """The same samples on a dense, aligned upload of their own."""
    return type(sig).from_planar_f32(sig.device_samples.to_planar(), sig.sampling_rate_hz)


def equal_results(what, got, want):
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    same_bits(what, [np.asarray(g) for g in got], [np.asarray(w) for w in want])


@pytest.fixture(scope="module")
def trimmed():
    """A resident inverse STFT trimmed to its original's length: a view 4 x 513 bytes into its owner (the overlap of
    50.1 % of 1024 samples), ld > n_samples, live overlap-added samples in front of every row and behind it.
    -> (the view, its dense copy)"""
    import dsptoolbox_amd as dsp
    x = np.random.default_rng(77).standard_normal((6000, 3)) * 0.3
    sd = dsp.Signal.from_planar_f32(backend._planar_f32(x), FS)
    sd.set_spectrogram_parameters(window_length_samples=1024, overlap_percent=50.1, padding=True)
    _, _, handle = sd.get_spectrogram(on_device=True)
    view = dsp.transforms.istft(handle, original_signal=sd)
    d = view.device_samples
    assert view.on_device and d.n_samples == 6000 and d.ld > d.n_samples and d.offset_bytes == 4 * 513
    assert d.offset_bytes % 16 != 0
    return view, dense_copy(view)


def _psd(s):
    from dsptoolbox_amd.standard.enums import SpectrumScaling
    s.set_spectrum_parameters(window_length_samples=512, scaling=SpectrumScaling.PowerSpectralDensity)
    return s.get_spectrum()


def _tf(s):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd.transfer_functions.enums import TransferFunctionType
    x = np.random.default_rng(78).standard_normal((len(s), 1)) * 0.3
    si = dsp.Signal.from_planar_f32(backend._planar_f32(x), FS)
    for q in (s, si):
        q.set_spectrum_parameters(window_length_samples=1024)
    tf = dsp.transfer_functions.compute_transfer_function(s, si, 1024, TransferFunctionType.H1)
    return tf.spectral_data, tf.coherence


def _spectrogram(s):
    s.set_spectrogram_parameters(window_length_samples=1024, padding=True)
    return s.get_spectrogram()


def _fir_bank(s):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd.standard.enums import FilterBankMode, FilterPassType
    fb = dsp.FilterBank([dsp.Filter.fir_filter(300, [300.0 * (k + 1), 900.0 * (k + 1)], FilterPassType.Bandpass, FS)
                         for k in range(2)])
    return fb.filter_signal(s, FilterBankMode.Parallel).get_all_time_data()[0]


def _iir(s):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd.standard.enums import FilterPassType
    return dsp.Filter.iir_filter(6, [500.0, 1000.0], FilterPassType.Bandpass, FS).filter_signal(s).time_data


def _resample(s):
    import dsptoolbox_amd as dsp
    return dsp.resample(s, 44100).time_data


def _normalize(s):
    import dsptoolbox_amd as dsp
    return dsp.normalize(s, -6.0, peak_normalization=False, each_channel=False).time_data


def _compress(s):
    import dsptoolbox_amd as dsp
    return dsp.effects.Compressor(-14, 1.0, 30, 4).apply(s).time_data


def _vqt(s):
    import dsptoolbox_amd as dsp
    return dsp.transforms.vqt(s, octaves=[5, 6], bins_per_octave=6)


CONSUMERS = {"welch_psd": _psd, "welch_tf": _tf, "spectrogram": _spectrogram, "fir_bank": _fir_bank, "iir": _iir,
             "resample": _resample, "normalize": _normalize, "compressor": _compress, "vqt": _vqt}


@pytest.mark.parametrize("consumer", list(CONSUMERS))
def test_trimmed_reconstruction_feeds_the_library(trimmed, consumer, monkeypatch):
    monkeypatch.setattr(backend, "TF_PRECISION", "f32")  # the resident fp32 entries, whatever the precision rule would pick
    monkeypatch.setattr(backend, "SPEC_PRECISION", "f32")
    view, dense = trimmed
    ctx = get_context()
    ctx.routes()
    got = CONSUMERS[consumer](view)
    print(f"{consumer} on the trimmed view: {' '.join(sorted(ctx.routes()))}")
    assert view.on_device and not view._has_host_copy, "the view was brought to the host: the resident entry did not run"
    equal_results(consumer, got, CONSUMERS[consumer](dense))


def test_trimmed_signal_rms_and_fade():
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd.beamforming import _pad_trim_signal
    from dsptoolbox_amd.standard.enums import FadeType
    x = np.random.default_rng(79).standard_normal((5003, 3)) * 0.3 + 0.1
    sd = dsp.Signal.from_planar_f32(backend._planar_f32(x), FS)
    view = _pad_trim_signal(sd, 4097)
    d = view.device_samples
    assert view.on_device and d.n_samples == 4097 and d.ld == 5003
    dense = dense_copy(view)
    equal_results("rms", dsp.rms(view), dsp.rms(dense))
    equal_results("fade", dsp.fade(view, FadeType.Logarithmic, 0.01).time_data, dsp.fade(dense, FadeType.Logarithmic, 0.01).time_data)
    assert not view._has_host_copy


@pytest.mark.parametrize("fill", vc.FILLS)
def test_warp_of_a_truncated_view_with_a_poisoned_gap(fill):
    import dsptoolbox_amd as dsp
    ctx = get_context()
    n, keep = 300, 257
    x = vc._noise(80, n, 5, 0.3)
    outs = []
    for v in range(3):
        sig = dsp.Signal.from_planar_f32(upload_view(ctx, x, *vc.VIEWS(n)[v], fill), FS)
        outs.append(dsp.transforms.warp(sig, -0.6, False, total_length=keep).time_data)
    dense = dsp.Signal.from_planar_f32(np.ascontiguousarray(x[:, :keep]), FS)
    want = dsp.transforms.warp(dense, -0.6, False).time_data
    for v, got in enumerate(outs):
        equal_results(f"warp {vc.VIEW_NAMES[v]} {fill}", got, want)


# ---- C. output pitch -----------------------------------------------------------------------------------------------------
_ptr = backend._ptr


_held = []  # the device buffers of the running case: the test frees them whatever happens


def hold(buf):
    _held.append(buf)
    return buf


def into_pitched_rows(ctx, n_rows, n_out, call):
    """call(y pointer, ld_y) once on dense rows and once on rows of pitch n_out + 3 from a base one float into a buffer
    of "big" poison: the valid samples equal, every other element still poison."""
    dense = hold(DeviceBuffer(ctx, 4 * n_rows * n_out))
    call(dense.ptr, n_out)
    ctx.sync()
    want = dense.to_array((n_rows, n_out), np.float32)
    ld_y = n_out + 3
    size = 1 + n_rows * ld_y + 64
    host = vc.poison(size, "big")
    buf = hold(DeviceBuffer.from_array(ctx, host))
    call(buf.ptr + 4, ld_y)
    ctx.sync()
    got = buf.to_array((size,), np.float32)
    valid = vc.valid_mask(size, n_rows, n_out, ld_y, 1)
    same_bits("valid samples", [got[valid].reshape(n_rows, n_out)], [want])
    touched = np.argwhere(bits(got[~valid]) != bits(host[~valid]))
    assert touched.size == 0, ("written outside the output rows at (index among the poison)", touched[:8].ravel().tolist())
    return want


def _x(ctx, seed, n, n_ch):
    plane = vc._noise(seed, n, n_ch, 0.3, 0.05)
    x = DevicePlanar.from_planar(ctx, plane)
    hold(x.owner)
    return plane, x


def _c_iir(ctx):
    from scipy.signal import butter
    plane, x = _x(ctx, 500, vc.N_RECURSIVE, 3)
    sos = backend._sos_stack([butter(4, 0.2, output="sos"), butter(3, 0.6, "high", output="sos")])
    k, n_sec = sos.shape[:2]
    return 2 * 3, x.n_samples, lambda y, ld: ctx.check(ctx.lib.ds_iir_sos_dev(
        ctx.handle, C.c_void_p(x.ptr), 3, x.ld, x.n_samples, _ptr(sos), k, n_sec, None, backend.DS_FB_PARALLEL,
        C.c_void_p(y), ld, None), "ds_iir_sos_dev")


def _c_sfilt(ctx):
    import sfilt_cases as sc
    plane, x = _x(ctx, 501, vc.N_RECURSIVE, 3)
    kid, coef, d, aux = sc.pack(sc.structure("kautz", 5))
    coef, _, _ = backend._sfilt_args(kid, coef, d, aux, 3, None, False)
    return 3, x.n_samples, lambda y, ld: ctx.check(ctx.lib.ds_sfilt_dev(
        ctx.handle, C.c_void_p(x.ptr), 3, x.ld, x.n_samples, int(kid), _ptr(coef), d, aux, None, C.c_void_p(y), ld, None),
        "ds_sfilt_dev")


def _c_rtfilt(ctx):
    import rtfilt_cases as rc
    plane, x = _x(ctx, 502, vc.N_RECURSIVE, 3)
    kid, coef, d, aux, delay, fir = rc.pack(rc.structure("svf", 2))
    coef, fir, _, _ = backend._rtfilt_args(kid, coef, d, aux, delay, fir, x.n_samples, 3, None, False)
    # four bands, band b's rows at y + b * n_ch * ld_y: twelve rows of one pitch
    return 4 * 3, x.n_samples, lambda y, ld: ctx.check(ctx.lib.ds_rtfilt_dev(
        ctx.handle, C.c_void_p(x.ptr), 3, x.ld, x.n_samples, int(kid), _ptr(coef), d, aux, delay, None, 0, None,
        C.c_void_p(y), ld, None), "ds_rtfilt_dev")


def _c_rtfir(ctx):
    import rtfilt_cases as rc
    plane, x = _x(ctx, 503, rc.FIR_TILE + 1, 3)
    b = backend._rtfir_taps(np.random.default_rng(504).standard_normal(64), x.n_samples, 3)
    return 3, x.n_samples, lambda y, ld: ctx.check(ctx.lib.ds_rtfir_dev(
        ctx.handle, C.c_void_p(x.ptr), 3, x.ld, x.n_samples, _ptr(b), len(b), None, C.c_void_p(y), ld), "ds_rtfir_dev")


def _c_resample(ctx):
    import resample_cases as rsc
    n = rsc.edge_lengths(160, 147, 3)[-1]
    plane, x = _x(ctx, 505, n, 3)
    taps = backend._resample_taps(160, 147)
    return 3, rsc.n_out(n, 160, 147), lambda y, ld: ctx.check(ctx.lib.ds_resample_poly_dev(
        ctx.handle, C.c_void_p(x.ptr), x.ld, n, 3, 160, 147, _ptr(taps), C.c_void_p(y), ld), "ds_resample_poly_dev")


def _c_delay_sum(ctx):
    plane, x = _x(ctx, 506, 700, 3)
    src, shift, frac, weight = backend._delay_terms(4, 2, [[0, 1], [2, 0], [1, 2], [2, 2]], [[0, 5], [-3, 100], [250, -1], [7, 400]],
                                                    [[0.25, -1.0], [0.5, 0.0], [0.75, 0.125], [-1.0, 0.9]],
                                                    [[1.0, 0.5], [-0.5, 0.25], [0.3, 0.7], [1.0, -1.0]])
    lens = np.array([700, 699, 333], dtype=np.int64)
    beta = float(backend._kaiser_window_beta(60.0))
    return 4, 900, lambda y, ld: ctx.check(ctx.lib.ds_delay_sum_dev(
        ctx.handle, C.c_void_p(x.ptr), 3, x.ld, _ptr(lens), 4, 2, _ptr(src), _ptr(shift), _ptr(frac), _ptr(weight), 11, beta,
        900, C.c_void_p(y), ld, None), "ds_delay_sum_dev")


def _c_fx_delay(ctx):
    plane, x = _x(ctx, 507, 700, 2)
    return 2, 700 + 515, lambda y, ld: ctx.check(ctx.lib.ds_fx_delay(
        ctx.handle, C.c_void_p(x.ptr), 1, 2, x.ld, 700, 256, 515, 0.4, backend.FX_SATURATIONS["digital"], C.c_void_p(y), ld),
        "ds_fx_delay")


def _c_fx_tremolo(ctx):
    plane, x = _x(ctx, 508, 257, 3)
    mod = np.ascontiguousarray(1.0 - 0.4 * (0.5 + 0.5 * np.sin(0.02 * np.arange(257))))
    return 3, 257, lambda y, ld: ctx.check(ctx.lib.ds_fx_tremolo(
        ctx.handle, C.c_void_p(x.ptr), 1, 3, x.ld, 257, _ptr(mod), C.c_void_p(y), ld), "ds_fx_tremolo")


def _c_level_apply(ctx):
    # input and output rows of one pitch, n + 3, the input rows two floats past a 16-byte boundary where the output rows
    # are one float past it: no row pair shares an alignment, so the scalar-row path runs
    n = 1003
    x = upload_view(ctx, vc._noise(509, n, 3, 0.3, 0.05), vc.MARGIN + 2, 3, "big")
    hold(x.owner)
    basis = backend.level_basis(n, 0)
    gain = np.array([0.5, -1.25, 2.0])
    fade = np.ascontiguousarray(np.linspace(0.0, 1.0, 301)[1:] ** 2)
    return 3, n, lambda y, ld: ctx.check(ctx.lib.ds_level_apply(
        ctx.handle, C.c_void_p(x.ptr), 1, 3, x.ld, n, -1, _ptr(basis), backend.LEVEL_NORMS["none"], 1.0, _ptr(gain), _ptr(fade),
        len(fade), 1, 1, C.c_void_p(y), ld), "ds_level_apply")


def _c_fir_ola(ctx):
    import route_cases as rcs
    q = rcs.fir_problem(1025, 5000, 3, "parallel")
    x = DevicePlanar.from_planar(ctx, q["xp"])
    taps = hold(DeviceBuffer.from_array(ctx, q["taps"]))
    hold(x.owner)
    return 3 * 3, 5000, lambda y, ld: ctx.check(ctx.lib.ds_fir_ola_dev(
        ctx.handle, C.c_void_p(x.ptr), 3, x.ld, 5000, C.c_void_p(taps.ptr), 3, 1025, rcs.DS_FB["parallel"], C.c_void_p(y), ld),
        "ds_fir_ola_dev")


OUTPUTS = {"ds_iir_sos_dev": _c_iir, "ds_sfilt_dev": _c_sfilt, "ds_rtfilt_dev": _c_rtfilt, "ds_rtfir_dev": _c_rtfir,
           "ds_resample_poly_dev": _c_resample, "ds_delay_sum_dev": _c_delay_sum, "ds_fx_delay": _c_fx_delay,
           "ds_fx_tremolo": _c_fx_tremolo, "ds_level_apply": _c_level_apply, "ds_fir_ola_dev": _c_fir_ola}


@pytest.mark.parametrize("entry", list(OUTPUTS))
def test_output_pitch_and_untouched_gaps(entry):
    ctx = get_context()
    try:
        n_rows, n_out, call = OUTPUTS[entry](ctx)
        want = into_pitched_rows(ctx, n_rows, n_out, call)
        assert np.all(np.isfinite(want)) and np.any(want != 0)
    finally:
        ctx.sync()
        while _held:
            _held.pop().free()
