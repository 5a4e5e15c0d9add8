"""The direct sums on the device: every case of tests/golden/direct/cases.npz through the public functions, the tile
and chunk edges of k_dft and k_csmooth against the restatements of tests/test_direct_host.py, a 2^20-sample signal
against a long-double evaluation, and the guards.  Bounds: 1e-9 (float64) and 1e-6 (through the fp32 transform) of each
channel's largest output magnitude."""

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from test_direct_host import (FS, golden, longdouble_dft, ref_csmooth, ref_dft, ref_windowed_sum, window_values)
from test_smoothing_host import channel_error

pytestmark = pytest.mark.gpu
TOL64, TOL32 = 1e-9, 1e-6
tf = dsp.transfer_functions


# ---- the reference's cases ------------------------------------------------------------------------------------------
def test_golden_dft():
    z, meta = golden()
    for i, case in enumerate(meta["dft"]):
        ref = z[f"dft_{i}_out"]
        out = dsp.transforms.dft(dsp.Signal(None, z[case["sig"]].copy(), FS, constrain_amplitude=False), z["dft_freqs"])
        assert out.shape == ref.shape and out.dtype == np.complex128
        e = channel_error(out, ref)
        print(f"dft {case['sig']}: {e:.2e} of the channel maximum")
        assert e <= TOL64, (case, e)


def test_golden_window_frequency_dependent():
    z, meta = golden()
    worst = 0.0
    for i, case in enumerate(meta["fdw"]):
        x, ref = z[case["sig"]], z[f"fdw_{i}_out"]
        sp = tf.window_frequency_dependent(dsp.ImpulseResponse(None, x.copy(), FS, constrain_amplitude=False),
                                           case["cycles"], case["end_db"])
        assert isinstance(sp, dsp.Spectrum)
        np.testing.assert_array_equal(sp.frequency_vector_hz, np.fft.rfftfreq(len(x), 1 / FS))
        assert sp.spectral_data.shape == ref.shape and sp.spectral_data.dtype == np.complex128
        assert np.all(sp.spectral_data[0] == 0.0)
        e = channel_error(sp.spectral_data, ref)
        worst = max(worst, e)
        assert e <= TOL64, (case, e)
    print(f"window_frequency_dependent: worst {worst:.2e} of the channel maximum")


def test_golden_complex_smoothing():
    z, meta = golden()
    worst32 = worst64 = 0.0
    for i, case in enumerate(meta["smooth"]):
        name, ref = case["sig"], z[f"smooth_{i}_out"]
        domain = tf.SmoothingDomain[case["domain"]]
        ir = dsp.ImpulseResponse(None, z[name].copy(), FS, constrain_amplitude=False)
        sp = tf.complex_smoothing(ir, case["fraction"], domain, dsp.Window[case["window"]])
        np.testing.assert_allclose(sp.frequency_vector_hz, z[f"{name}_freqs"], rtol=1e-12)
        assert sp.spectral_data.shape == ref.shape and sp.spectral_data.dtype == np.complex128
        e32 = channel_error(sp.spectral_data, ref)
        out = backend.complex_smoothing(z[f"{name}_spectrum"], z[f"{name}_freqs"], case["fraction"], domain,
                                        window_values(case["window"]))
        e64 = channel_error(out, ref)
        worst32, worst64 = max(worst32, e32), max(worst64, e64)
        assert e32 <= TOL32, (case, e32)
        assert e64 <= TOL64, (case, e64)
    assert {c["domain"] for c in meta["smooth"]} == set(backend.SMOOTHING_DOMAINS)
    print(f"complex_smoothing: worst {worst32:.2e} through the API, {worst64:.2e} on the float64 spectrum")


# ---- k_dft ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [1023, 1024, 1025, 2047, 2048, 2049])
def test_dft_tile_and_chunk_edges(n_samples):
    # k_dft owns 16 frequencies x 4 channels x one sample chunk; with so few frequency tiles the chunks are 1024
    # samples (their unit), so 1024 and 2048 fill one and two chunks exactly.  15 / 16 / 17 frequencies and 3 / 5
    # channels are partial tiles, a full one and the start of a second.
    rng = np.random.default_rng(n_samples)
    worst = 0.0
    for n_ch in (1, 3, 5):
        x = rng.standard_normal((n_samples, n_ch))
        for n_freq in (1, 15, 16, 17):
            freqs = rng.uniform(-1000.0, 30000.0, n_freq)
            e = channel_error(backend.dft(x, freqs, FS), ref_dft(x, freqs, FS))
            worst = max(worst, e)
            assert e <= TOL64, (n_samples, n_ch, n_freq, e)
    print(f"{n_samples} samples: worst {worst:.2e} of the channel maximum")


def test_long_signal_phase_and_device_resident_samples():
    n = 1 << 20
    rng = np.random.default_rng(20)
    x = (rng.standard_normal((n, 1)) * np.exp(-np.arange(n) / 4e5)[:, None]).astype(np.float32).astype(np.float64)
    freqs = np.array([0.37, 1000.0, 7777.7, FS / 2 - 0.37, FS / 2, FS - 1.0, 1234.5678, 19999.99])
    ref = longdouble_dft(x, freqs, FS)
    host = dsp.transforms.dft(dsp.Signal(None, x.copy(), FS, constrain_amplitude=False), freqs)
    e = channel_error(host, ref)
    print(f"2^20 samples against long double: {e:.2e} of the channel maximum")
    assert e <= TOL64
    resident = dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), FS)
    assert resident.on_device and not resident._has_host_copy
    dev = dsp.transforms.dft(resident, freqs)
    assert not resident._has_host_copy  # the samples were not downloaded
    e = channel_error(dev, host)
    print(f"ds_dft_dev against ds_dft: {e:.2e}")
    assert e <= TOL64


def ir_with_peaks(n, peaks, seed):
    rng = np.random.default_rng(seed)
    x = 0.05 * rng.standard_normal((n, len(peaks)))
    x[list(peaks), np.arange(len(peaks))] = 1.0
    return x


@pytest.mark.parametrize("cycles", [1, 100000])
def test_windowed_peaks_at_both_ends(cycles):
    # peaks at sample 0 and at N - 1: two channels of one workgroup whose kept ranges lie as far apart as they can;
    # 100000 cycles keep every term, 1 cycle leaves the top bins a few samples
    n = 3000
    x = ir_with_peaks(n, (0, n - 1), 1)
    f, alpha, peak, half = tf._fdw_parameters(x, FS, cycles, -50.0)
    kept = backend._windowed_kept_terms(alpha, peak, half, n) / (len(f) * x.size)
    assert kept == 1.0 if cycles > 1 else kept < 0.05
    assert list(peak) == [0, n - 1]
    sp = tf.window_frequency_dependent(dsp.ImpulseResponse(None, x.copy(), FS, constrain_amplitude=False), cycles)
    ref = np.pad(ref_windowed_sum(x, f, FS, alpha, peak, half), ((1, 0), (0, 0)))
    e = channel_error(sp.spectral_data, ref)
    print(f"cycles {cycles}: {100 * kept:.1f} % of the terms kept, {e:.2e} of the channel maximum")
    assert e <= TOL64


def test_windowed_range_on_a_chunk_edge():
    # 3000 samples x 64 frequencies: four frequency tiles, chunks of 1024 samples.  With the peak at 1500 a kept
    # distance of 476 starts the range on sample 1024, one of 547 ends it with sample 2047; 475 / 477 and 546 / 548
    # lie one sample to either side.
    n, half = 3000, 1499.5
    x = ir_with_peaks(n, (1500, 1500), 2)
    x[:, 1] = np.random.default_rng(3).standard_normal(n)  # a channel that is not small away from the peak
    dists = np.array([475, 476, 477, 546, 547, 548] * 11)[:64]
    alpha = 140.0 * np.log(2.0) * (half / (dists + 0.5)) ** 2
    np.testing.assert_array_equal(backend._windowed_kept_distance(alpha, half, n), dists)
    freqs = np.linspace(100.0, 20000.0, 64)
    peak = np.array([1500, 1500])
    out = backend.windowed_dft(x, freqs, FS, alpha, peak, half)
    e = channel_error(out, ref_windowed_sum(x, freqs, FS, alpha, peak, half))
    print(f"kept ranges on chunk edges: {e:.2e}")
    assert e <= TOL64
    everything = backend.windowed_dft(x, freqs, FS, alpha, peak, half, -np.inf)
    # the skipped terms are below N 2^-70; what is left is the rounding of two summation orders, at most N eps
    assert channel_error(everything, out) <= n * 2.0 ** -52


# ---- k_csmooth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [2, 3, 4, 5, 8, 9, 257])
def test_smoothing_tile_edges(n_bins):
    # k_csmooth gives each of a workgroup's four waves one bin and each wave eight real columns: 4 / 5 and 8 / 9 bins
    # fill workgroups and start the next, 1 / 3 / 5 channels are 2 / 6 / 10 columns
    rng = np.random.default_rng(n_bins)
    f = np.linspace(0.0, FS / 2, n_bins)
    wy = window_values("Hann")
    for n_ch in (1, 3, 5):
        sp = 1.0 + 0.2 * (rng.standard_normal((n_bins, n_ch)) + 1j * rng.standard_normal((n_bins, n_ch)))
        for domain in ("RealImaginary", "Magnitude", "EquivalentComplex"):
            for fraction in (0.5, 3):
                out = backend.complex_smoothing(sp, f, fraction, domain, wy)
                e = channel_error(out, ref_csmooth(sp, f, fraction, domain, wy))
                assert e <= TOL64, (n_bins, n_ch, domain, fraction, e)


def test_smoothing_widest_bands_and_passed_bins():
    n_bins = 4097
    rng = np.random.default_rng(4)
    f = np.fft.rfftfreq(2 * (n_bins - 1), 1 / FS)
    sp = 1.0 + 0.2 * (rng.standard_normal((n_bins, 2)) + 1j * rng.standard_normal((n_bins, 2)))
    wy = window_values("Hann")
    lo, hi, wlen, passed = backend._csmooth_indices(f, 0.5)
    assert passed[0] and not passed[-1] and hi[-1] == n_bins
    assert (hi - lo).max() > 2000 and (wlen > hi - lo).any()  # bands clipped at the last bin
    for domain in ("RealImaginary", "Power"):
        out = backend.complex_smoothing(sp, f, 0.5, domain, wy)
        e = channel_error(out, ref_csmooth(sp, f, 0.5, domain, wy))
        print(f"4097 bins at half an octave, {domain}: {e:.2e}")
        assert e <= TOL64
    out = backend.complex_smoothing(sp, f, 0.5, "RealImaginary", wy)
    np.testing.assert_array_equal(out[passed.astype(bool)], sp[passed.astype(bool)])
    # 1/12 octave: the 18 lowest bins are copied
    lo, hi, wlen, passed = backend._csmooth_indices(f, 12)
    assert passed[:18].all() and passed.sum() == 18
    out = backend.complex_smoothing(sp, f, 12, "RealImaginary", wy)
    np.testing.assert_array_equal(out[:18], sp[:18])
    assert channel_error(out, ref_csmooth(sp, f, 12, "RealImaginary", wy)) <= TOL64
    # a frequency vector that starts above 0: the lowest bands reach below the first bin and are clipped there
    f_up = f[:1025] + 6000.0
    lo, hi, wlen, passed = backend._csmooth_indices(f_up, 3)
    assert ((lo == 0) & (wlen > hi - lo) & (hi < 1025) & (passed == 0)).any()
    out = backend.complex_smoothing(sp[:1025], f_up, 3, "MagnitudePhase", wy)
    e = channel_error(out, ref_csmooth(sp[:1025], f_up, 3, "MagnitudePhase", wy))
    print(f"bands clipped at bin 0: {e:.2e}")
    assert e <= TOL64


# ---- properties -----------------------------------------------------------------------------------------------------
def test_dft_at_the_rfft_bins_is_the_rfft():
    x = np.random.default_rng(5).standard_normal((1000, 3))
    out = backend.dft(x, np.fft.rfftfreq(1000, 1 / FS), FS)
    assert channel_error(out, np.fft.rfft(x, axis=0)) <= TOL64


def test_constant_spectrum_stays_constant():
    sp = np.full((1000, 2), 2.5 - 1.5j) * np.array([1.0, 1e-3])
    out = backend.complex_smoothing(sp, np.linspace(0, FS / 2, 1000), 3, "RealImaginary", window_values("Hann"))
    assert np.abs(out / sp - 1.0).max() <= 1e-14


def test_identical_calls_return_identical_bits():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5000, 3))
    freqs = rng.uniform(0, 24000, 40)
    np.testing.assert_array_equal(backend.dft(x, freqs, FS), backend.dft(x, freqs, FS))
    ir = dsp.ImpulseResponse(None, ir_with_peaks(2000, (10, 40), 7), FS, constrain_amplitude=False)
    a = tf.window_frequency_dependent(ir, 5).spectral_data
    np.testing.assert_array_equal(a, tf.window_frequency_dependent(ir, 5).spectral_data)
    sp = 1.0 + 0.2 * (rng.standard_normal((900, 2)) + 1j * rng.standard_normal((900, 2)))
    f, wy = np.linspace(0, FS / 2, 900), window_values("Hann")
    np.testing.assert_array_equal(backend.complex_smoothing(sp, f, 3, "PowerPhase", wy),
                                  backend.complex_smoothing(sp, f, 3, "PowerPhase", wy))


def test_no_frequencies():
    out = backend.dft(np.ones((100, 3)), np.zeros(0), FS)
    assert out.shape == (0, 3) and out.dtype == np.complex128


# ---- guards ---------------------------------------------------------------------------------------------------------
def test_size_guards_raise():
    with pytest.raises(NotImplementedError, match="work bound"):
        backend._dft_guard(2.0 ** 64)
    # the entry answers before it touches a pointer: 2^40 frequencies x 2^24 samples
    ctx = backend.get_context()
    rc = ctx.lib.ds_dft(ctx.handle, None, 1 << 24, 1, None, 1 << 40, float(FS), None, None, 1.0, -70.0, None)
    assert rc == -2 and "work bound" in ctx.last_error()
    rc = ctx.lib.ds_dft_dev(ctx.handle, None, 1, 1 << 24, 1 << 24, None, 1 << 40, float(FS), None, None, 1.0, -70.0, None)
    assert rc == -2 and "work bound" in ctx.last_error()
    # 2^20 bins whose bands all span the spectrum: 1.1e12 band terms
    n = 1 << 20
    lo, hi = np.zeros(n, dtype=np.int32), np.full(n, n, dtype=np.int32)
    one = np.zeros(4)
    rc = ctx.lib.ds_complex_smooth(ctx.handle, backend._ptr(one), n, 1, backend._ptr(lo), backend._ptr(hi), backend._ptr(hi),
                                   backend._ptr(lo), backend._ptr(one), backend._ptr(one), 4, 0, backend._ptr(one))
    assert rc == -2 and "work bound" in ctx.last_error()


def test_argument_errors():
    ir = dsp.ImpulseResponse(None, ir_with_peaks(64, (3,), 8), FS)
    with pytest.raises(ValueError, match="zero samples"):
        tf.window_frequency_dependent(ir, 0.2)
    with pytest.raises(AssertionError, match="only valid for an impulse response"):
        tf.window_frequency_dependent(dsp.Signal(None, np.ones((64, 1)), FS), 5)
    with pytest.raises(ValueError, match="peak outside"):
        backend.windowed_dft(np.ones((64, 1)), np.ones(3), FS, np.ones(3), np.array([64]), 31.5)
