"""The float64 any-length transform and what is built on it, on the device: ds_fft_c128 against numpy.fft across the
route edges (one workgroup in LDS up to 8192, four-step above, Bluestein for every other length; 4097 sends Bluestein to
a 16384-point four-step, at 50000 k^2 passes 2^31, 384000 needs the 64-bit k^2), every public function against the
reference's results of tests/golden/phase/cases.npz, the group delays on every bin, the guards, and run-to-run identity.
Bounds: 1e-9 of each channel's largest magnitude (phases as exp(i phi)); group delays 1e-9 N / fs per bin; the analytic
group delay 1e-9 (N / fs) max|B| / |B(w)| per bin, the conditioning of its quotient."""

import ctypes as C

import numpy as np
import pytest
from scipy.fft import next_fast_len

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DeviceError, get_context
from test_phase_host import analytic_spectra, cases, golden, phase_error
from test_smoothing_host import channel_error

pytestmark = pytest.mark.gpu
TOL = 1e-9
tf, tr = dsp.transfer_functions, dsp.transforms


def ir_of(x, fs):
    return dsp.ImpulseResponse(None, x.copy(), fs, constrain_amplitude=False)


# ---- the transform itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8, 255, 256, 1000, 4097, 8192, 16384, 50000, 131072, 384000])
def test_fft_c128_against_numpy(n):
    rng = np.random.default_rng(n)
    worst = 0.0
    for n_ch in ((1, 3) if n >= 131072 else (1, 3, 5)):
        for n_in in sorted({max(1, n - 7), n, n + 5}):  # pad, exact, crop
            real = rng.standard_normal((n_in, n_ch))
            real[:, -1] *= 1e-3
            for x in (real, real + 1j * rng.standard_normal((n_in, n_ch))):
                for inverse in (False, True):
                    out = backend.fft_c128(x, n, inverse=inverse)
                    ref = (np.fft.ifft if inverse else np.fft.fft)(x, n, axis=0)
                    assert out.shape == ref.shape and out.dtype == np.complex128
                    e = channel_error(out, ref)
                    worst = max(worst, e)
                    assert e <= TOL, (n, n_ch, n_in, x.dtype, inverse, e)
    print(f"fft_c128 n = {n}: {worst:.2e} of the column maximum")


def test_fft_c128_round_trip_at_384000():
    x = np.random.default_rng(384000).standard_normal((384000, 3))
    back = backend.fft_c128(backend.fft_c128(x), inverse=True)
    e = channel_error(back, x.astype(np.complex128))
    print(f"round trip at 384000: {e:.2e}")
    assert e <= TOL, e


# ---- the public functions against the reference's results ----------------------------------------------------------
def test_golden_hilbert():
    _, meta = golden()
    for case, x, ref, _ in cases("hilbert"):
        out = tr.hilbert(ir_of(x, meta["fs"]))
        assert type(out) is dsp.ImpulseResponse and out.time_data_imaginary is not None
        e = channel_error(out.time_data + 1j * out.time_data_imaginary, ref)
        print(f"hilbert {case['sig']}: {e:.2e}")
        assert e <= TOL, (case, e)
    sig = dsp.Signal(None, x.copy(), meta["fs"], constrain_amplitude=False)
    assert type(tr.hilbert(sig)) is dsp.Signal
    mb = tr.hilbert(dsp.MultiBandSignal([sig, sig.copy()]))
    assert type(mb) is dsp.MultiBandSignal and len(mb.bands) == 2
    assert channel_error(mb.bands[1].time_data + 1j * mb.bands[1].time_data_imaginary, ref) <= TOL


def test_golden_cepstrum_and_back():
    z, meta = golden()
    for case, x, ref, _ in cases("cepstrum"):
        out = tr.cepstrum(ir_of(x, meta["fs"]), complex=case["complex"])
        assert out.shape == ref.shape and out.dtype == np.complex128
        e = channel_error(out, ref)
        print(f"cepstrum {case['sig']} complex={case['complex']}: {e:.2e}")
        assert e <= TOL, (case, e)
        if case["complex"]:
            back = tr.from_complex_cepstrum(out, meta["fs"])
            assert type(back) is dsp.Signal and back.sampling_rate_hz == meta["fs"]
            e = channel_error(back.time_data, x)
            print(f"from_complex_cepstrum {case['sig']}: {e:.2e}")
            assert e <= TOL, (case, e)


def test_golden_min_phase_ir():
    _, meta = golden()
    seen = set()
    for case, x, ref, _ in cases("min_phase_ir"):
        out = tf.min_phase_ir(ir_of(x, meta["fs"]), padding_factor=case["padding_factor"], alpha=case["alpha"])
        assert type(out) is dsp.ImpulseResponse and out.time_data.shape == ref.shape
        e = channel_error(out.time_data, ref)
        print(f"min_phase_ir {case['sig']} alpha={case['alpha']} padding={case['padding_factor']}: {e:.2e}")
        assert e <= TOL, (case, e)
        seen.add((len(x), case["padding_factor"], case["alpha"] == 1.0))
    assert {(n, 8, a) for n in (255, 256, 1000, 6000) for a in (True, False)} | {(4097, 2, True)} == seen


def test_golden_minimum_phase():
    _, meta = golden()
    for case, x, ref, f_ref in cases("minimum_phase"):
        f, out = tf.minimum_phase(ir_of(x, meta["fs"]), padding_factor=case["padding_factor"])
        assert out.shape == ref.shape and out.dtype == np.float64
        assert np.allclose(f, f_ref, rtol=1e-12, atol=0.0)
        e = phase_error(out, ref)
        print(f"minimum_phase {case['sig']} padding={case['padding_factor']}: {e:.2e}")
        assert e <= TOL, (case, e)


# ---- group delays: every bin ----------------------------------------------------------------------------------------
def gd_check(what, case, out, ref, n_transform, fs):
    """1e-9 N / fs per bin: a gradient of phases good to 1e-9, divided by 2 pi delta_f with delta_f = fs / N.  At a
    step of exactly 1 Hz the reference does not divide by 2 pi (radians per bin): the same gradient gives 2 pi 1e-9."""
    assert out.shape == ref.shape and out.dtype == np.float64, (what, case)
    bound = TOL * n_transform / fs * (2 * np.pi if n_transform == fs else 1.0)
    e = float(np.abs(out - ref).max())
    print(f"{what} {case['sig']}: {e:.2e} s (bound {bound:.2e} s)")
    assert e <= bound, (what, case, e, bound)


def test_golden_minimum_group_delay():
    _, meta = golden()
    for case, x, ref, f_ref in cases("minimum_group_delay", smoothing=0):
        fs = case.get("fs", meta["fs"])
        f, out = tf.minimum_group_delay(ir_of(x, fs), padding_factor=case["padding_factor"])
        assert np.allclose(f, f_ref, rtol=1e-12, atol=0.0)
        gd_check("minimum_group_delay", case, out, ref, backend.min_phase_fft_length(len(x), case["padding_factor"]), fs)


def test_golden_group_delay_numerical():
    _, meta = golden()
    for case, x, ref, f_ref in cases("group_delay", analytic_computation=False, smoothing=0):
        fs = case.get("fs", meta["fs"])
        f, out = tf.group_delay(ir_of(x, fs), analytic_computation=False)
        np.testing.assert_array_equal(f, f_ref)
        gd_check("group_delay", case, out, ref, len(x), fs)


def test_golden_excess_group_delay():
    _, meta = golden()
    for case, x, ref, f_ref in cases("excess_group_delay", smoothing=0):
        fs = case.get("fs", meta["fs"])
        f, out = tf.excess_group_delay(ir_of(x, fs))
        assert np.allclose(f, f_ref, rtol=1e-12, atol=0.0)
        gd_check("excess_group_delay", case, out, ref, backend.min_phase_fft_length(len(x), 1), fs)


def test_golden_group_delay_analytic():
    _, meta = golden()
    fs = meta["fs"]
    seen = set()
    for case, x, ref, f_ref in cases("group_delay", analytic_computation=True):
        latency = case["remove_ir_latency"]
        f, out = tf.group_delay(ir_of(x, fs), analytic_computation=True, remove_ir_latency=latency)
        np.testing.assert_array_equal(f, f_ref)
        assert out.shape == ref.shape
        for c in range(x.shape[1]):
            b = np.concatenate([x[:, c], np.zeros(next_fast_len(8 * len(x), True) - len(x))]) if latency else x[:, c]
            if latency:
                b = b[max(int(np.argmax(np.abs(b))) - 1, 0):]
            _, den = analytic_spectra(b, len(f))
            bound = TOL * (len(b) / fs) * np.abs(den).max() / np.abs(den)
            assert bound.max() <= 1e-6 * len(b) / fs  # (the generator's 60 dB)
            err = np.abs(out[:, c] - ref[:, c])
            print(f"analytic group delay {case['sig']} latency={latency} channel {c}: worst {(err / bound).max():.2e} of the bound")
            assert (err <= bound).all(), (case, c, float((err / bound).max()))
        seen.add((len(x) % 2, latency))
    assert seen == {(0, False), (0, True), (1, False), (1, True)}


def test_analytic_group_delay_of_a_zero_channel_is_zero():
    x = np.zeros((255, 2))
    x[4, 0] = 1.0
    f, gd = tf.group_delay(dsp.Signal(None, x, 48000, constrain_amplitude=False))
    assert gd.shape == (128, 2) and np.array_equal(gd[:, 1], np.zeros(128))
    assert np.abs(gd[:, 0] - 4 / 48000).max() <= TOL * 255 / 48000


def test_smoothed_group_delays():
    _, meta = golden()
    fs = meta["fs"]
    n_seen = 0
    for fn in ("group_delay", "minimum_group_delay", "excess_group_delay"):
        for case, x, ref, _ in cases(fn, smoothing=3):
            if fn == "group_delay":
                _, out = tf.group_delay(ir_of(x, fs), analytic_computation=False, smoothing=3)
            else:
                _, out = getattr(tf, fn)(ir_of(x, fs), smoothing=3)
            e = channel_error(out, ref)
            print(f"{fn} smoothing=3: {e:.2e} of the channel maximum")
            assert e <= TOL, (case, e)
            n_seen += 1
    assert n_seen == 3


# ---- guards and identity ------------------------------------------------------------------------------------------
def test_length_bounds_raise_before_anything_is_uploaded():
    ctx = get_context()
    x = np.ones((4, 1))
    out = np.empty((4, 1), dtype=np.complex128)  # never written: the entry answers before it stages anything
    for n_fft in ((1 << 21) + 1, 3 << 20, 1 << 23):
        with pytest.raises(NotImplementedError, match="not built"):
            ctx.check(ctx.lib.ds_fft_c128(ctx.handle, backend._ptr(x), 0, 4, 1, n_fft, 0, backend._ptr(out)), "ds_fft_c128")
        with pytest.raises(NotImplementedError, match="not built"):
            ctx.check(ctx.lib.ds_min_phase(ctx.handle, backend._ptr(x), 4, 1, n_fft, 2, 4, 1.0, backend._ptr(out)), "ds_min_phase")
        with pytest.raises(NotImplementedError, match="beyond the device kernels' bounds"):
            backend.fft_c128(x, n_fft)


def test_a_call_beyond_the_free_memory_is_refused_before_anything_is_uploaded():
    """65535 channels of 2^22 points are 8.8 TB of planar buffers: DS_ERR_NOMEM from the estimate, with nothing allocated
    (the free memory is what it was) and the one input row never read past."""
    ctx = get_context()
    n_ch = 65535
    x = np.ones((1, n_ch))
    out = np.empty((1, 1), dtype=np.complex128)  # never written
    free0, free1, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
    ctx.check(ctx.lib.ds_mem_info(ctx.handle, C.byref(free0), C.byref(total)), "ds_mem_info")
    with pytest.raises(DeviceError, match="more device memory than is free"):
        ctx.check(ctx.lib.ds_fft_c128(ctx.handle, backend._ptr(x), 0, 1, n_ch, 1 << 22, 0, backend._ptr(out)), "ds_fft_c128")
    ctx.check(ctx.lib.ds_mem_info(ctx.handle, C.byref(free1), C.byref(total)), "ds_mem_info")
    assert free1.value == free0.value


def test_the_same_call_returns_the_same_bits():
    z, meta = golden()
    x = np.random.default_rng(7).standard_normal((384000, 1))
    assert np.array_equal(backend.fft_c128(x), backend.fft_c128(x))
    x = np.random.default_rng(8).standard_normal((16384, 3))
    assert np.array_equal(backend.fft_c128(x, inverse=True), backend.fft_c128(x, inverse=True))
    ir = ir_of(z["ir1000"], meta["fs"])
    assert np.array_equal(tf.min_phase_ir(ir).time_data, tf.min_phase_ir(ir).time_data)
    assert np.array_equal(tf.minimum_group_delay(ir)[1], tf.minimum_group_delay(ir)[1])
    assert np.array_equal(backend.hilbert(z["ir255"]), backend.hilbert(z["ir255"]))
