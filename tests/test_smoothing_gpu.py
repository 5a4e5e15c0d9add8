"""Fractional-octave smoothing on the device: every golden case of the reference and the tile / halo edges of
k_smooth against the float64 restatement of tests/test_smoothing_host.py within 1e-9 of the channel's largest value
(the bound of the project's float64 routes); the complex path through Signal.get_spectrum, spectral_deconvolve and
Spectrum.apply_octave_smoothing within the fp32 bound 1e-6, and within 1e-9 when the float64 entry is fed the float64
spectrum itself."""

import numpy as np
import pytest
from scipy.fft import next_fast_len, rfft

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd.standard.enums import SpectrumMethod, SpectrumScaling, Window
from test_smoothing_host import channel_error, fos_cases, golden, ref_smoothing

pytestmark = pytest.mark.gpu
TOL64, TOL32 = 1e-9, 1e-6
FS = 48000


def test_golden_cases():
    worst = 0.0
    for i, case, v, window, wvec, ref in fos_cases():
        out = dsp.tools.fractional_octave_smoothing(v, case["spacing"], case["fractions"], window, wvec, case["clip"])
        assert out.shape == ref.shape and out.dtype == np.float64, (i, out.shape, ref.shape)
        e = channel_error(out, ref)
        worst = max(worst, e)
        assert e <= TOL64, (i, case, e)
        if case["clip"]:
            assert out.min() >= 0.0
    print(f"golden smoothing cases: worst {worst:.2e} of the channel maximum")


@pytest.mark.parametrize("n_bins", [2048, 2049, 2050, 4097])
def test_tile_and_halo_edges(n_bins):
    # k_smooth owns 128 bins x 16 channels (2048 x 1 for one channel) and walks the window in chunks of 129 taps
    # (2049): 1, 3 channels are partial groups, 64 and 65 fill four groups and start a fifth
    rng = np.random.default_rng(n_bins)
    worst = 0.0
    for n_ch in (1, 3, 64, 65):
        v = rng.standard_normal((n_bins, n_ch)) + 0.2
        for fractions in (1, 3):
            out = backend.fractional_octave_smoothing(v, None, fractions)
            e = channel_error(out, ref_smoothing(v, None, fractions))
            worst = max(worst, e)
            assert e <= TOL64, (n_bins, n_ch, fractions, e)
    print(f"{n_bins} bins: worst {worst:.2e} of the channel maximum")


def test_window_walked_in_chunks():
    n = 65537
    v = np.random.default_rng(7).standard_normal((n, 2)) + 0.1
    k_log, beta = backend._smooth_axis(n, None)
    assert backend._smooth_window_length(1, beta) == 4097
    out = backend.fractional_octave_smoothing(v, None, 1)
    e = channel_error(out, ref_smoothing(v, None, 1))
    print(f"65537 bins x 2, 4097 taps: {e:.2e} of the channel maximum")
    assert e <= TOL64


def test_even_window_on_logarithmic_bins():
    # the entry's own rule for an even window: n_window / 2 in front, n_window / 2 - 1 behind
    ctx = backend.get_context()
    rng = np.random.default_rng(3)
    v = np.ascontiguousarray(rng.standard_normal((300, 5)))
    w = rng.random(8) + 0.1
    out = np.empty_like(v)
    ctx.check(ctx.lib.ds_octave_smooth(ctx.handle, backend._ptr(v), 300, 5, None, backend._ptr(w), 8, 0,
                                       backend._ptr(out)), "ds_octave_smooth")
    padded = np.pad(v, ((4, 3), (0, 0)), mode="edge")
    ref = np.stack([np.convolve(padded[:, c], w / w.sum(), mode="valid") for c in range(5)], axis=1)
    assert channel_error(out, ref) <= TOL64


def test_constant_stays_constant():
    for n_bins, spacing in ((1000, None), (4097, None), (500, 1 / 96)):
        v = np.full((n_bins, 3), 2.5) * np.array([1.0, -1.0, 1e-3])
        out = backend.fractional_octave_smoothing(v, spacing, 3)
        assert np.abs(out / v - 1.0).max() <= 1e-14


def test_clip_never_returns_a_negative_value():
    v = np.random.default_rng(11).standard_normal((3000, 4))
    for spacing in (None, 1 / 200):
        plain = backend.fractional_octave_smoothing(v, spacing, 12)
        clipped = backend.fractional_octave_smoothing(v, spacing, 12, clip_values=True)
        assert plain.min() < 0.0 and clipped.min() >= 0.0
        np.testing.assert_array_equal(clipped, np.clip(plain, 0, None))


def signal_of(case, z):
    s = dsp.Signal(None, z[case["sig"]].copy(), FS)
    s.set_spectrum_parameters(method=SpectrumMethod.FFT, smoothing=case["smoothing"],
                              pad_to_fast_length=case["pad"], scaling=SpectrumScaling[case["scaling"]])
    return s


def test_get_spectrum_smoothed():
    z, meta = golden()
    worst = 0.0
    for i, case in enumerate(meta["spec"]):
        f, sp = signal_of(case, z).get_spectrum()
        ref = z[f"spec_{i}_out"]
        assert sp.shape == ref.shape and sp.dtype == ref.dtype, (i, sp.shape, sp.dtype)
        e = channel_error(sp, ref)
        worst = max(worst, e)
        assert e <= TOL32, (i, case, e)
    print(f"get_spectrum with smoothing: worst {worst:.2e} of the channel's largest magnitude")


def test_complex_entry_on_the_float64_spectrum():
    z, meta = golden()
    worst = 0.0
    for i, case in enumerate(meta["spec"]):
        if case["scaling"] != "FFTBackward":
            continue
        x = z[case["sig"]]
        sp = rfft(x, axis=0, n=next_fast_len(len(x), True) if case["pad"] else len(x))
        out = backend.smooth_complex_spectrum(sp, case["smoothing"], clip_magnitude=True)
        e = channel_error(out, z[f"spec_{i}_out"])
        worst = max(worst, e)
        assert e <= TOL64, (i, case, e)
    print(f"ds_octave_smooth_complex on the float64 spectrum: worst {worst:.2e}")


def test_spectral_deconvolve_with_a_smoothed_input():
    z, meta = golden()
    case = meta["deconv"][0]
    x = z[case["sig"]]
    out_sig = dsp.Signal(None, x.copy(), FS)
    in_sig = dsp.Signal(None, x[:, ::-1].copy(), FS)
    in_sig.set_spectrum_parameters(method=SpectrumMethod.FFT, smoothing=case["smoothing"], pad_to_fast_length=True,
                                   scaling=SpectrumScaling.FFTBackward)
    ir = dsp.transfer_functions.spectral_deconvolve(out_sig, in_sig, apply_regularization=True,
                                                    start_stop_hz=case["start_stop_hz"])
    ref = z["deconv_0_out"]
    assert ir.time_data.shape == ref.shape
    e = channel_error(ir.time_data, ref)
    print(f"spectral_deconvolve with a smoothed input: {e:.2e} of the channel maximum")
    assert e <= TOL32


def test_spectrum_apply_octave_smoothing():
    z, meta = golden()
    for i, case in enumerate(meta["spectrum"]):
        spec = dsp.Spectrum(z[f"spectrum_{i}_freqs"], z[f"spectrum_{i}_in"])
        assert spec.apply_octave_smoothing(case["fraction"], Window[case["window"]]) is spec
        ref = z[f"spectrum_{i}_out"]
        assert spec.spectral_data.dtype == ref.dtype and spec.spectral_data.shape == ref.shape
        e = channel_error(spec.spectral_data, ref)
        print(f"Spectrum.apply_octave_smoothing case {i}: {e:.2e}")
        assert e <= TOL64  # float64 in, float64 arithmetic


def test_no_smoothing_is_unchanged():
    z, _ = golden()
    x = z["sig3001"]
    s = dsp.Signal(None, x.copy(), FS)
    s.set_spectrum_parameters(method=SpectrumMethod.FFT, smoothing=0, pad_to_fast_length=True,
                              scaling=SpectrumScaling.FFTBackward)
    f, sp = s.get_spectrum()
    np.testing.assert_array_equal(sp, backend.rfft_spectrum(x, next_fast_len(len(x), True), 1.0))


def test_welch_ignores_smoothing():
    z, _ = golden()
    a = dsp.Signal(None, z["sig4096"].copy(), FS)
    b = dsp.Signal(None, z["sig4096"].copy(), FS)
    a.set_spectrum_parameters(method=SpectrumMethod.WelchPeriodogram, smoothing=0, window_length_samples=512)
    b.set_spectrum_parameters(method=SpectrumMethod.WelchPeriodogram, smoothing=3, window_length_samples=512)
    np.testing.assert_array_equal(a.get_spectrum()[1], b.get_spectrum()[1])


def test_size_guard_raises():
    with pytest.raises(NotImplementedError, match="work bound"):
        backend._smooth_guard(1 << 22, 1 << 18, 64)
    # the entry answers before anything is uploaded or launched: 2^42 bins x 8 taps is 3.5e13 multiply-adds
    ctx = backend.get_context()
    v = np.zeros((4, 1))
    w = np.ones(8)
    rc = ctx.lib.ds_octave_smooth(ctx.handle, backend._ptr(v), 1 << 42, 1, None, backend._ptr(w), 8, 0, backend._ptr(v))
    assert rc == -2 and "work bound" in ctx.last_error()
