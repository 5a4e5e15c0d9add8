"""GPU parity: the HIP path (through the C-ABI, via the reference-shaped Python
API) against (a) the golden vectors produced by the real reference and (b) the
pinned CPU oracle on seeded inputs.  Tolerance: north_star's 1e-6 relative
(max-norm per output array); the DC bin is excluded when
detrend=True because it is 0/0 rounding noise in the reference itself."""

import os

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd.standard.enums import (FilterBankMode, FilterPassType, SpectrumMethod,
                                           SpectrumScaling, Window)
from dsptoolbox_amd.transfer_functions import TransferFunctionType
from oracle import dsp_oracle as orc
from conftest import load_golden
import route_cases as rcs
import route_oracles as ros
from xform_calls import (deconv_route_case as _deconv_route_case, rfft_route_case as _rfft_route_case,
                         route_call as _route_call)

pytestmark = pytest.mark.gpu
TOL = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = {"hann": Window.Hann, "hamming": Window.Hamming, "blackman": Window.Blackman,
       "boxcar": Window.Boxcar}


@pytest.fixture(autouse=True)
def _fp32_kernels_unless_a_test_asks(monkeypatch):
    """The API sends SHORT Welch spectra / cross-spectral matrices (fewer than 128 frames) through the float64 route
    (backend.SPEC_PRECISION = "auto").  The tests of this file are about the fp32 kernels unless they say otherwise,
    so the default here is "f32"; the tests of the route itself set "auto"."""
    monkeypatch.setattr(backend, "SPEC_PRECISION", "f32")


def inband(w, fs=48000, lo=30.0, hi=19000.0):
    """Bins where the 20 Hz - 20 kHz sweep input has energy.  Outside, H = Gxy/Gxx is
    noise divided by leakage: ill-conditioned in the float64 reference itself."""
    f = np.fft.rfftfreq(w, 1 / fs)
    return (f >= lo) & (f <= hi)


def relmax(a, b, skip_dc=False):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if skip_dc:
        a, b = a[1:], b[1:]
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_library_is_loaded_and_device_present():
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    assert ctx.lib.ds_device_count() >= 1


@pytest.mark.parametrize("spectra", ["f32", "auto"])
def test_welch_golden(spectra, monkeypatch):
    """tests/golden/welch.npz through the fp32 kernels and through the API's default routing (short estimates: float64)."""
    monkeypatch.setattr(backend, "SPEC_PRECISION", spectra)
    _welch_golden_body()


def _welch_golden_body():
    meta, z = load_golden("welch")
    x = z["x"]
    worst = 0.0
    for i, c in enumerate(meta["cases"]):
        d = x if c["data"] == "full" else x[: meta["ragged_len"]]
        sc = SpectrumScaling[c["scaling"]]
        a = backend._welch(d, None, meta["fs"], WIN[c["window"]], c["W"], c["overlap"],
                           c["detrend"], c["average"], sc)
        k = backend._welch(d[:, 0], d[:, 2], meta["fs"], WIN[c["window"]], c["W"], c["overlap"],
                           c["detrend"], c["average"], sc)
        ea = relmax(a, z[f"auto_{i}"], c["detrend"])
        ek = relmax(k, z[f"cross_{i}"], c["detrend"])
        worst = max(worst, ea, ek)
        assert ea < TOL and ek < TOL, (c, ea, ek)
        # quirk 11: median averaging makes even the autospectrum complex128
        assert a.dtype == z[f"auto_{i}"].dtype and k.dtype == np.complex128
    print("welch worst rel-max", worst)


@pytest.mark.parametrize("precision", ["auto", "f32"])
def test_transfer_function_golden(precision, monkeypatch):
    """The reference's H1 / H2 / H3 fixtures through the reference-shaped API: "auto" is what a user
    gets (these small problems take the float64 route), "f32" holds the fp32 register kernels
    (welch1k, 1024-sample windows) to the same reference-produced vectors."""
    monkeypatch.setattr(backend, "TF_PRECISION", precision)
    meta, z = load_golden("transfer_function")
    worst = 0.0
    for i, c in enumerate(meta["cases"]):
        xin = z["x"][:, :1] if c["single_input"] else z["x"]
        y = z["y_single"] if c["single_input"] else z["y_multi"]
        inp = dsp.Signal(None, xin.copy(), meta["fs"])
        out = dsp.Signal(None, y.copy(), meta["fs"])
        inp.set_spectrum_parameters(window_length_samples=1024, window_type=Window.Hann,
                                    overlap_percent=c["overlap"], detrend=c["detrend"],
                                    average="mean", scaling=SpectrumScaling[c["scaling"]])
        sp = dsp.transfer_functions.compute_transfer_function(out, inp, c["W"],
                                                              TransferFunctionType[c["mode"]])
        assert isinstance(sp, dsp.Spectrum) and sp.has_coherence
        e1 = relmax(sp.spectral_data, z[f"tf_{i}"], c["detrend"])
        e2 = relmax(sp.coherence, z[f"coh_{i}"], c["detrend"])
        worst = max(worst, e1, e2)
        if max(e1, e2) > 4e-7:
            print("  tf case", c, e1, e2)
        assert e1 < TOL and e2 < TOL, (c, e1, e2)
        assert np.array_equal(sp.frequency_vector_hz, z[f"f_{i}"])
    print("tf worst rel-max", worst)


def test_stft_golden():
    meta, z = load_golden("stft")
    worst = 0.0
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, z["x"].copy(), meta["fs"])
        s.set_spectrogram_parameters(window_length_samples=c["W"], window_type=Window.Hann,
                                     overlap_percent=c["overlap"],
                                     fft_length_samples=c["fft_length"], detrend=c["detrend"],
                                     padding=c["padding"], scaling=SpectrumScaling[c["scaling"]])
        t, f, st = s.get_spectrogram()
        assert np.allclose(t, z[f"t_{i}"], rtol=1e-14, atol=0)
        assert np.array_equal(f, z[f"f_{i}"])
        assert st.dtype == z[f"stft_{i}"].dtype
        e = relmax(st, z[f"stft_{i}"])
        worst = max(worst, e)
        assert e < TOL, (c, e)
    print("stft worst rel-max", worst)


def test_stft_any_fft_length_golden():
    """fft_length_samples that are not powers of two (255, 384, 1000, 1023, 257 ...) or lie below the
    window length: the reference's rfft(n=fft_length_samples) crops or zero-pads every frame
    (_spectral_methods.py:268) -- outputs of the real reference."""
    meta, z = load_golden("stft_anylen")
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, z["x"].copy(), meta["fs"])
        s.set_spectrogram_parameters(window_length_samples=c["W"], window_type=Window.Hann,
                                     overlap_percent=c["overlap"], fft_length_samples=c["fft_length"],
                                     detrend=c["detrend"], padding=c["padding"],
                                     scaling=SpectrumScaling[c["scaling"]])
        t, f, st = s.get_spectrogram()
        assert np.allclose(t, z[f"t_{i}"], rtol=1e-14, atol=0) and np.array_equal(f, z[f"f_{i}"])
        assert st.shape == z[f"stft_{i}"].shape and st.dtype == z[f"stft_{i}"].dtype
        assert relmax(st, z[f"stft_{i}"]) < TOL, (c, relmax(st, z[f"stft_{i}"]))
    # a larger shape against the oracle: 8 channels, many frames, Bluestein length with grouping
    rng = np.random.default_rng(43)
    x = rng.standard_normal((60000, 8)) * 0.3
    for W, nfft in ((1024, 1500), (512, 500), (2048, 2047)):
        t, f, st = backend._stft(x, 48000, W, Window.Hann, 50, nfft, True, False, SpectrumScaling.FFTBackward)
        rt, rf, rs = orc.stft(x, 48000, W, "hann", 50, nfft, True, False, "FFTBackward")
        assert st.shape == rs.shape and relmax(st, rs) < TOL, (W, nfft, relmax(st, rs))


@pytest.mark.parametrize("spectra", ["f32", "auto"])
def test_csm_golden(spectra, monkeypatch):
    monkeypatch.setattr(backend, "SPEC_PRECISION", spectra)
    _csm_golden_body()


def _csm_golden_body():
    meta, z = load_golden("csm")
    worst = 0.0
    for i, c in enumerate(meta["cases"]):
        if c["method"] != "welch":
            continue
        s = dsp.Signal(None, z["x"].copy(), meta["fs"])
        s.set_spectrum_parameters(method=SpectrumMethod.WelchPeriodogram,
                                  window_length_samples=c["W"], overlap_percent=c["overlap"],
                                  detrend=c["detrend"], scaling=SpectrumScaling[c["scaling"]])
        f, csm = s.get_csm()
        assert np.array_equal(f, z[f"f_{i}"])
        e = relmax(csm, z[f"csm_{i}"], c["detrend"])
        worst = max(worst, e)
        assert e < TOL, (c, e)
        # Hermitian by construction
        assert np.array_equal(csm, np.conj(np.swapaxes(csm, 1, 2)))
    print("csm worst rel-max", worst)


def test_csm_fft_vs_oracle():
    """Signal.get_csm with SpectrumMethod.FFT (_csm_fft): power-of-two length so the
    whole-signal rFFT runs on the device; golden case (n = 1000) needs a non-pow2 FFT."""
    rng = np.random.default_rng(21)
    x = 0.1 * rng.standard_normal((2048, 5)) + 0.2 * rng.standard_normal(2048)[:, None]
    for sc in SpectrumScaling:
        s = dsp.Signal(None, x.copy(), 48000)
        s.set_spectrum_parameters(method=SpectrumMethod.FFT, scaling=sc)
        f, csm = s.get_csm()
        fr, sp = orc.spectrum_fft(x, 48000, "FFTBackward", True)
        ref = orc.csm_fft(sp, sc.name, None, 48000)
        assert np.array_equal(f, fr)
        assert relmax(csm, ref) < TOL, (sc, relmax(csm, ref))
    # golden cases: n = 1000 (not a power of two -> Bluestein whole-signal FFT)
    meta, z = load_golden("csm")
    for i, c in enumerate(meta["cases"]):
        if c["method"] != "fft":
            continue
        s = dsp.Signal(None, z["x"][:1000, :3].copy(), meta["fs"])
        s.set_spectrum_parameters(method=SpectrumMethod.FFT, scaling=SpectrumScaling[c["scaling"]])
        f, csm = s.get_csm()
        assert np.array_equal(f, z[f"f_{i}"])
        assert relmax(csm, z[f"csm_{i}"]) < TOL, (c, relmax(csm, z[f"csm_{i}"]))


def test_spectrum_fft_golden():
    """Signal.get_spectrum with SpectrumMethod.FFT at the reference's next_fast_len lengths
    (3000 = 2^3 3 5^3) and an odd prime-ish length (2999): arbitrary-length DFT on the device."""
    meta, z = load_golden("spectrum_fft")
    worst = 0.0
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, z["x"][: c["n"]].copy(), meta["fs"])
        s.set_spectrum_parameters(method=SpectrumMethod.FFT, scaling=SpectrumScaling[c["scaling"]],
                                  pad_to_fast_length=c["pad_to_fast_length"])
        f, sp = s.get_spectrum()
        assert np.array_equal(f, z[f"f_{i}"])
        assert sp.dtype == z[f"sp_{i}"].dtype
        e = relmax(sp, z[f"sp_{i}"])
        worst = max(worst, e)
        assert e < TOL, (c, e)
    print("spectrum_fft worst rel-max", worst)


def _welch_h1_float32_emulation(x, y, fs, W, hop):
    """The same estimate with numpy/pocketfft in single precision: what ANY fp32 FFT
    pipeline can deliver on this data (test-side yardstick, not an oracle)."""
    import scipy.fft as sf
    from scipy.signal.windows import get_window
    win = get_window("hann", W, fftbins=True)

    def spec(sig):
        f = orc.get_framed_signal(sig, W, hop) * win[:, None, None]
        f -= f.mean(axis=0)
        return sf.rfft(f.astype(np.float32), axis=0).astype(np.complex128)

    X, Y = spec(x), spec(y)
    sxx, syy = np.mean(np.abs(X) ** 2, axis=1), np.mean(np.abs(Y) ** 2, axis=1)
    sxy = np.mean(X.conj() * Y, axis=1)
    return np.sqrt(sxy) / np.sqrt(sxx), np.abs(sxy) / np.sqrt(sxx * syy)


def test_chirp_pair_config1():
    """BASELINE.json configs[0] on the device: the example chirps (192 000 samples = 2^9 3 5^3):
    Welch H1 nfft 4096 and the regularised deconvolution (Bluestein, M = 2^19).

    The fast pink sweep puts 60 dB more energy into the low-frequency frames than the 18 kHz
    bins ever receive, and every frame's fp32 FFT error floor (1e-7 of ITS peak) lands on all
    bins: single-precision numpy/pocketfft is 7.5e-5 off the float64 reference here.  The
    reference-shaped API therefore takes the float64 route for a problem this small
    (backend.TF_PRECISION = "auto" -> ds_welch_tf_x64) and has to meet 1e-6 like everything
    else; the fp32 kernels, asked for explicitly, have to be as good as that float32 pipeline."""
    meta, z = load_golden("chirp_pair")
    c = meta["cases"][0]
    x = z["x_int16"].astype(np.float64)[:, None] / 32768
    y = z["y_int16"].astype(np.float64) / 32768
    inp, out = dsp.Signal(None, x, c["fs"]), dsp.Signal(None, y, c["fs"])
    inp.set_spectrum_parameters(window_length_samples=4096, overlap_percent=50, detrend=True)
    assert backend.TF_PRECISION == "auto"
    sp = dsp.transfer_functions.compute_transfer_function(out, inp, 4096, TransferFunctionType.H1)
    fr = np.fft.rfftfreq(4096, 1 / c["fs"])
    m = (fr >= 30) & (fr <= 18000)  # the chirp's spectrum is within 40 dB of its peak here
    e1, e2 = relmax(sp.spectral_data[m], z["tf"][m]), relmax(sp.coherence[m], z["coh"][m])
    print(f"chirp pair H1 (float64 route) rel-max {e1:.2e}, coherence {e2:.2e}")
    assert e1 < TOL and e2 < TOL
    # whole band, DC excluded (0/0 with detrend): the float64 route needs no in-band mask
    assert relmax(sp.spectral_data[1:], z["tf"][1:]) < TOL and relmax(sp.coherence[1:], z["coh"][1:]) < TOL
    # the fp32 kernels on the same data, against the float32 yardstick
    tf32, coh32 = backend.welch_transfer_function(y, x, c["fs"], 4096, "H1", precision="f32")
    t32, c32 = _welch_h1_float32_emulation(x, y, c["fs"], 4096, 2048)
    e1f, e2f = relmax(tf32[m], z["tf"][m]), relmax(coh32[m], z["coh"][m])
    y1, y2 = relmax(t32[m], z["tf"][m]), relmax(c32[m], z["coh"][m])
    print(f"chirp pair H1 (fp32 kernels) rel-max {e1f:.2e} (numpy float32: {y1:.2e}), coherence {e2f:.2e} ({y2:.2e})")
    assert e1f < max(TOL, 2 * y1) and e2f < max(TOL, 2 * y2)
    ir = dsp.transfer_functions.spectral_deconvolve(out, inp)
    assert ir.time_data.shape == (c["n"], 2)
    pk = float(z["ir_peak"][0])
    eh = np.max(np.abs(ir.time_data[: c["ir_head"]] - z["ir_head"])) / pk
    et = np.max(np.abs(ir.time_data[-c["ir_tail"]:] - z["ir_tail"])) / pk
    print(f"chirp pair deconvolution rel-max head {eh:.2e} tail {et:.2e}")
    assert eh < TOL and et < TOL


def test_welch4096_paired_inputs_vs_oracle():
    """One input channel per output channel (n_cx == n_cy) with a 4096-sample window on the
    three-per-CU register kernels (k_x3 over every input channel, k_px_sum, k_y3): H1 / H2 / H3 and
    coherence within 1e-6 -- the shapes whose generic-kernel results touched 1.0-1.3e-6 in the
    round-1 sweeps (about 100 frames)."""
    rng = np.random.default_rng(23)
    for n, C, det in ((4096 * 50 + 777, 5, True), (2**18, 3, False)):
        x = rng.standard_normal((n, C)) * 0.3
        y = np.stack([np.convolve(x[:, i], rng.standard_normal(12) * np.exp(-np.arange(12) / 4.0))[:n]
                      for i in range(C)], axis=1)
        y += 0.02 * rng.standard_normal(y.shape)
        for mode in ("H1", "H2", "H3"):
            tf, coh = backend.welch_transfer_function(y, x, 48000, 4096, mode, detrend=det)
            rt, rc = orc.compute_transfer_function(y, x, 48000, 4096, mode, detrend=det)
            e1, e2 = relmax(tf, rt, det), relmax(coh, rc, det)
            assert e1 < TOL and e2 < TOL, (n, C, mode, e1, e2)
        # other overlaps: the two-workgroups-per-CU kernels (k_x per input channel, k_px_sum, k_y)
        for ov in (75.0, 25.0):
            tf, coh = backend.welch_transfer_function(y, x, 48000, 4096, "H1", overlap_percent=ov, detrend=det)
            rt, rc = orc.compute_transfer_function(y, x, 48000, 4096, "H1", overlap_percent=ov, detrend=det)
            assert relmax(tf, rt, det) < TOL and relmax(coh, rc, det) < TOL, (n, C, ov)
            k = backend._welch(x, y, 48000, Window.Hann, 4096, ov, det, "mean", SpectrumScaling.FFTBackward)
            r = orc.welch(x, y, 48000, "hann", 4096, ov, det, "mean", "FFTBackward")
            assert relmax(k, r, det) < TOL, (n, C, ov, "csd")


@pytest.mark.parametrize("W", [32, 64, 128, 256, 512, 1024, 2048, 8192, 16384])
def test_welch_wave_kernels_paired_inputs_vs_oracle(W):
    """One input channel per output channel on the wave-level register kernels (256 ... 2048-sample
    windows, 1024 being the reference's default; 32 / 64 / 128-sample windows ride on the 256-point kernels: zero-padded
    frames, every 8th / 4th / 2nd bin kept) and the 8192-sample ones: k_x over every input
    channel, k_px_sum, k_y with the team's own input spectra.  50 % overlap (carried half frame) and 75 %, ragged tails, more
    channels than teams per workgroup."""
    rng = np.random.default_rng(100 + W)
    for n, C, ov, det in ((W * 40 + 333, 5, 50, True), (W * 25, 19, 75, False), (W * 9 + 1, 2, 50, True)):
        x = rng.standard_normal((n, C)) * 0.3
        y = np.stack([np.convolve(x[:, i], rng.standard_normal(12) * np.exp(-np.arange(12) / 4.0))[:n]
                      for i in range(C)], axis=1)
        y += 0.02 * rng.standard_normal(y.shape)
        for mode in ("H1", "H2", "H3"):
            tf, coh = backend.welch_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det)
            rt, rc = orc.compute_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det)
            if mode == "H2":
                # H2 = Gyy / Gyx divides by the cross spectrum: at the nulls of the random 12-tap filters
                # (coherence < 0.1, which the fine bins of the long windows resolve) the fp32 error of
                # Gyx is amplified by 1 / coherence (known limits); those bins are left out
                weak = rc < 0.1
                tf, rt = np.where(weak, 0.0, tf), np.where(weak, 0.0, rt)
            e1, e2 = relmax(tf, rt, det), relmax(coh, rc, det)
            # fp32 kernels, asked for explicitly: below ~40 frames the coherence sits at the 1e-6 mark (DESIGN section 2,
            # limit (ii); tests/sweeps/edge_welch.py) -- 18 frames of 16384 samples read 1.13e-6 on kernels_welch_long.hpp,
            # 0.9e-6 on kernels_welch16384.hpp.  Through the API such estimates take the float64 kernels.
            few = n / (W * (1 - ov / 100)) < 40
            assert e1 < TOL and e2 < (2 * TOL if few else TOL), (W, n, C, mode, e1, e2)
        if W == 16384 or W <= 128:  # one input channel for all output channels, auto spectra
            y1 = np.stack([np.convolve(x[:, 0], rng.standard_normal(6))[:n] for _ in range(3)], axis=1)
            y1 += 0.05 * rng.standard_normal(y1.shape)
            for mode in ("H1", "H3"):
                tf, coh = backend.welch_transfer_function(y1, x[:, :1], 48000, W, mode, overlap_percent=ov, detrend=det)
                rt, rc = orc.compute_transfer_function(y1, x[:, :1], 48000, W, mode, overlap_percent=ov, detrend=det)
                assert relmax(tf, rt, det) < TOL and relmax(coh, rc, det) < TOL, (W, n, C, mode, "one input")
            a = backend._welch(y, None, 48000, Window.Hann, W, ov, det, "mean", SpectrumScaling.PowerSpectralDensity)
            r = orc.welch(y, None, 48000, "hann", W, ov, det, "mean", "PowerSpectralDensity")
            assert relmax(a, r, det) < TOL, (W, n, C, "psd", relmax(a, r, det))
        # the cross spectra of the same channel pairs (ds_welch_csd: the same kernels, finish of kind 2)
        for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.PowerSpectralDensity):
            k = backend._welch(x, y, 48000, Window.Hann, W, ov, det, "mean", sc)
            r = orc.welch(x, y, 48000, "hann", W, ov, det, "mean", sc.name)
            assert k.shape == r.shape and relmax(k, r, det) < TOL, (W, n, C, sc, relmax(k, r, det))


def test_welch_long_windows_golden():
    """The reference's own outputs (tests/golden/welch_long.npz, made by oracle/gen_golden.py from
    dsptoolbox 0.8) for windows of 2048 ... 16384 samples: auto spectra, cross spectra of channel pairs,
    H1 / H2 / H3 with one input channel per output channel and with one for all -- the register kernels
    of every long window against the reference itself."""
    meta, z = load_golden("welch_long")
    x, ym, ys = (z[k].astype(np.float64) for k in ("x", "y_multi", "y_single"))
    for i, c in enumerate(meta["cases"]):
        bins, dc, sc = z[f"bins_{i}"], c["detrend"], SpectrumScaling[c["scaling"]]
        a = backend._welch(ym, None, meta["fs"], Window.Hann, c["W"], c["overlap"], c["detrend"], "mean", sc)
        assert relmax(a[bins], z[f"auto_{i}"], dc) < TOL, (c["W"], "auto")
        k = backend._welch(x, ym, meta["fs"], Window.Hann, c["W"], c["overlap"], c["detrend"], "mean", sc)
        assert relmax(k[bins], z[f"cross_{i}"], dc) < TOL, (c["W"], "cross")
        for key in c["tf"]:
            _, mode, which = key.split("_")
            xin, yout = (x[:, :1], ys) if which == "single" else (x, ym)
            tf, coh = backend.welch_transfer_function(yout, xin, meta["fs"], c["W"], mode, overlap_percent=c["overlap"],
                                                      detrend=c["detrend"], scaling=sc, precision="f32")
            rt, rc = z["tf_" + key], z["coh_" + key]
            if mode == "H2":  # see test_welch_wave_kernels_paired_inputs_vs_oracle
                weak = rc < 0.1
                tf, rt = np.where(weak, 0.0, tf[bins]), np.where(weak, 0.0, rt)
            else:
                tf = tf[bins]
            # 2 TOL: the fixture holds tf / coh rounded to complex64 / float32 (6e-8 of their own)
            assert relmax(tf, rt, dc) < 2 * TOL and relmax(coh[bins], rc, dc) < 2 * TOL, (c["W"], key)


@pytest.mark.parametrize("case", [
    dict(W=8192, n=199273, n_ch=16, ov=75.0, det=True, sc="AmplitudeSpectralDensity", mode="H3", seed=8192),
    dict(W=8192, n=674937, n_ch=33, ov=25.0, det=False, sc="AmplitudeSpectrum", mode="H3", seed=8193),
    # round 3's sweep (fuzz_parity 200 31, case 121): 61 frames of 16384 samples, coherence 1.13e-6 at the Nyquist bin
    dict(W=16384, n=988985, n_ch=16, ov=0.0, det=True, sc="FFTOrthogonal", mode="H2", seed=16384),
])
def test_short_long_window_estimates_from_the_round2_sweep(case):
    """The two shapes of gpurun_out/sweeps_r02.log whose coherence reached 1.8e-6 / 1.1e-6 on the fp32 kernels
    (VERDICT r2, next 3c): 8192-sample windows, 98 / 110 frames, overlaps other than 50 %, amplitude scalings.
    An estimate this short has too few frames to average the fp32 transform rounding down -- across such cases
    the fp32 kernels' worst coherence error is 3-5e-7 (tools/dev/coh_margin.py: a third of what a float32 numpy
    restatement reaches) with a tail to ~2e-6.  The API's "auto" arithmetic now sends estimates of fewer than
    128 frames through the float64 route: asserted at 1e-6 here, with the fp32 kernels held to 3e-6."""
    import sys as _sys
    _sys.path.insert(0, os.path.join(ROOT, "tests", "sweeps"))
    rng = np.random.default_rng(case["seed"])
    n, n_ch = case["n"], case["n_ch"]
    x = rng.standard_normal((n, 1)) * 0.3 + 0.05
    h = rng.standard_normal((32, n_ch)) * np.exp(-np.arange(32) / 6.0)[:, None]
    y = np.stack([np.convolve(x[:, 0], h[:, c])[:n] for c in range(n_ch)], axis=1) + 0.05 * rng.standard_normal((n, n_ch))
    sc = SpectrumScaling[case["sc"]]
    rt, rc = orc.compute_transfer_function_batched(y, x, 48000, case["W"], case["mode"], overlap_percent=case["ov"],
                                                   detrend=case["det"], scaling=sc.name)
    for precision, tol in (("auto", TOL), ("f32", 3e-6)):
        tf, coh = backend.welch_transfer_function(y, x, 48000, case["W"], case["mode"], overlap_percent=case["ov"],
                                                  detrend=case["det"], scaling=sc, precision=precision)
        e_tf, e_coh = relmax(tf, rt, case["det"]), relmax(coh, rc, case["det"])
        print(f"W={case['W']} n={n} {precision}: tf {e_tf:.2e} coherence {e_coh:.2e}")
        assert e_tf < tol and e_coh < tol, (precision, e_tf, e_coh)
    hop = case["W"] - int(case["ov"] / 100 * case["W"])
    assert backend._tf_x64_applies("auto", 1, n_ch, -(-n // hop), case["W"], "mean")
    # the float64 route itself is the reference's arithmetic (16384: the packed half-length transform + split)
    tf, coh = backend.welch_transfer_function(y[:, :3], x, 48000, case["W"], case["mode"], overlap_percent=case["ov"],
                                              detrend=case["det"], scaling=sc, precision="f64")
    assert relmax(tf, rt[:, :3], case["det"]) < 1e-10 and relmax(coh, rc[:, :3], case["det"]) < 1e-10


def test_das_beamformer_device_chain_golden():
    """BeamformerDASFrequency.get_beamformer_map end to end from the microphone signals (missing 3):
    Signal.get_csm(on_device=True) keeps the cross-spectral matrix in HBM, ds_csm_das_prepare_dev treats the
    diagonal there, ds_das_map_dev forms the map; tests/golden/das_signal.npz is the reference's own map."""
    from dsptoolbox_amd.beamforming import BeamformerDASFrequency
    meta, z = load_golden("das_signal")
    s = dsp.Signal(None, z["time_data"].astype(np.float64), meta["fs"])
    s.set_spectrum_parameters(window_length_samples=meta["window"])

    class Grid:  # the reference's geometry classes stay the reference's: stand-ins with its interface
        def __init__(self, n, shape):
            self.number_of_points, self.shape = n, shape

        def reconstruct_map_shape(self, m):
            return np.asarray(m).reshape(self.shape)  # Regular2DGrid: row-major over (x, y)

    for i, c in enumerate(meta["cases"]):
        class Steering:
            def get_vector(self, wave_numbers, grid, mic, _h=z[f"h_{i}"], _n=c["bins"][1] - c["bins"][0]):
                assert len(wave_numbers) == _n  # the same bins as the reference selected
                return _h

        bf = BeamformerDASFrequency(s, None, Grid(c["n_points"], c["grid_shape"]), Steering())
        m = bf.get_beamformer_map(c["center_hz"], c["octave_fraction"], remove_csm_diagonal=c["remove_csm_diagonal"])
        ref = z[f"map_{i}"]
        # (the reference reshapes with its own grid class; compare as flat maps in either order)
        e = min(relmax(m.ravel(), ref.ravel()), relmax(m.ravel(), ref.T.ravel()))
        assert m.size == ref.size and e < 2 * TOL, (c, e)
    # the handle by itself: device matrix == host matrix
    f, dc = s.get_csm(on_device=True)
    f2, csm = s.get_csm()
    assert np.array_equal(f, f2) and relmax(dc.to_host(), csm) < TOL
    dc.free()


def test_fir_complex_taps_golden():
    """Filter.filter_signal with complex taps (missing 5): two real device convolutions, the
    imaginary part of the output lands in Signal.time_data_imaginary (filter_helpers.py:364-371)."""
    import warnings
    meta, z = load_golden("fir_complex")
    for i, c in enumerate(meta["cases"]):
        f = dsp.Filter.from_ba(z[f"b_{i}"], [1.0], meta["fs"])
        s = dsp.Signal(None, z["x"].copy(), meta["fs"])
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            if c["zi"]:
                f.initialize_zi(3)
            out = f.filter_signal(s, channels=c["channels"], activate_zi=c["zi"])
        assert any("complex" in str(w.message) for w in rec)
        assert out.time_data_imaginary is not None
        assert relmax(out.time_data, z[f"re_{i}"]) < TOL and relmax(out.time_data_imaginary, z[f"im_{i}"]) < TOL, c
        assert np.array_equal(s.time_data, z["x"])  # the input is untouched


def test_deconvolve_scaled_spectra_golden():
    """spectral_deconvolve on signals that carry a spectrum scaling (missing 4): the reference
    divides the SCALED spectra -- norms, amplitude and power scalings -- tests/golden/deconv_scaled.npz."""
    meta, z = load_golden("deconv_scaled")
    for i, c in enumerate(meta["cases"]):
        x, y = (z["x"], z["y"]) if c["regularized"] else (z["xn"], z["yn"])
        xin = np.repeat(x, 2, axis=1) * np.array([1.0, 0.8]) if c["per_channel"] else x
        out, inp = dsp.Signal(None, y.copy(), meta["fs"]), dsp.Signal(None, xin.copy(), meta["fs"])
        out.set_spectrum_parameters(method=dsp.SpectrumMethod.FFT, scaling=SpectrumScaling[c["scaling_y"]])
        inp.set_spectrum_parameters(method=dsp.SpectrumMethod.FFT, scaling=SpectrumScaling[c["scaling_x"]])
        ir = dsp.transfer_functions.spectral_deconvolve(out, inp, apply_regularization=c["regularized"],
                                                        padding=c["padding"], keep_original_length=c["keep"])
        ref = z[f"ir_{i}"]
        assert isinstance(ir, dsp.ImpulseResponse) and ir.time_data.shape == ref.shape
        # unregularised: |X| of white noise dips to ~1e-2 of its mean (see fuzz_misc.py)
        tol = TOL if c["regularized"] else 1e-4
        assert relmax(ir.time_data, ref) < tol, (c, relmax(ir.time_data, ref))


def _welch4096_golden(expect_main="welch4096_main"):
    """tests/golden/welch4096.npz (made by oracle/gen_golden.py from dsptoolbox 0.8): 4096-sample
    windows, 50 % overlap, 66 frames of noise; H1 / H2 / H3 x three scalings, one input for all
    outputs and one per output.  fp32 kernels against the reference at 1e-6; `expect_main`: the
    kernel name that has to be among the launches."""
    from dsptoolbox_amd._lib import get_context
    meta, z = load_golden("welch4096")
    x, ym, ys = (z[k].astype(np.float64) / 8192.0 for k in ("x_q13", "y_multi_q13", "y_single_q13"))
    bins = z["bins"]
    ctx = get_context()
    worst = 0.0
    for c in meta["cases"]:
        dc, sc = c["detrend"], SpectrumScaling[c["scaling"]]
        for key in c["tf"]:
            _, mode, which = key.split("_")
            xin, yout = (x[:, :1], ys) if which == "single" else (x, ym)
            ctx.profile_enable(True)
            ctx.profile_report()
            tf, coh = backend.welch_transfer_function(yout, xin, meta["fs"], c["W"], mode, overlap_percent=c["overlap"],
                                                      detrend=dc, scaling=sc, precision="f32")
            launched = ctx.profile_report()
            ctx.profile_enable(False)
            assert expect_main in launched and "welch_finish" in launched, sorted(launched)
            rt, rc = z["tf_" + key], z["coh_" + key]
            tfb = tf[bins]
            if mode == "H2":  # Gyy / Gyx where the coherence vanishes is noise in float64 too
                weak = rc < 0.1
                tfb, rt = np.where(weak, 0.0, tfb), np.where(weak, 0.0, rt)
            e1, e2 = relmax(tfb, rt, dc), relmax(coh[bins], rc, dc)
            worst = max(worst, e1, e2)
            assert e1 < TOL and e2 < TOL, (key, c, e1, e2)
    print("welch4096 golden worst rel-max", worst)


def test_welch4096_headline_shape_golden():
    """The headline kernels k_x3 (+ k_px_sum) + k_y3 + k_welch_finish against the reference itself."""
    _welch4096_golden()


def test_welch4096_cross_spectra_on_register_kernels():
    """ds_welch_csd with a 4096-sample window at 50 % overlap: k_x3 / k_px_sum / k_y3 + finish kind 2."""
    rng = np.random.default_rng(4096)
    for n, C, det in ((4096 * 30 + 55, 4, True), (2**17, 1, False)):
        x = rng.standard_normal((n, C)) * 0.3
        y = np.stack([np.convolve(x[:, i], rng.standard_normal(8))[:n] for i in range(C)], axis=1)
        y += 0.05 * rng.standard_normal(y.shape)
        for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.PowerSpectralDensity):
            from dsptoolbox_amd._lib import get_context
            ctx = get_context()
            ctx.profile_enable(True)
            ctx.profile_report()
            k = backend._welch(x, y, 48000, Window.Hann, 4096, 50, det, "mean", sc)
            launched = ctx.profile_report()
            ctx.profile_enable(False)
            assert "welch4096_main" in launched and "welch_finish" in launched, sorted(launched)
            r = orc.welch(x, y, 48000, "hann", 4096, 50, det, "mean", sc.name)
            assert k.shape == r.shape and relmax(k, r, det) < TOL, (n, C, sc, relmax(k, r, det))


def test_transfer_function_float64_route_vs_oracle():
    """ds_welch_tf_x64: float64 transforms, sums and finish -- the oracle's own precision (1e-11),
    every mode, amplitude and power scalings, one input channel or one per output, ragged tail."""
    rng = np.random.default_rng(17)
    for n, W, ov, det, ncx in ((30011, 1024, 50, True, 1), (9000, 256, 75, False, 3), (50000, 8192, 50, True, 1),
                               (4099, 64, 0, True, 1)):
        x = rng.standard_normal((n, ncx)) * 0.3
        y = np.stack([np.convolve(x[:, min(i, ncx - 1)], rng.standard_normal(9))[:n] for i in range(3)], axis=1)
        y += 1e-4 * rng.standard_normal(y.shape)
        for mode in ("H1", "H2", "H3"):
            for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.PowerSpectralDensity):
                tf, coh = backend.welch_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det,
                                                          scaling=sc, precision="f64")
                rt, rc = orc.compute_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det,
                                                       scaling=sc.name)
                assert tf.dtype == np.complex128 and coh.dtype == np.float64
                assert relmax(tf, rt, det) < 1e-9 and relmax(coh, rc, det) < 1e-9, (n, W, mode, sc)
        # median averaging on the float64 route (single-frame values are picked, so fp32 transform
        # noise is not averaged down: the fp32 kernels need 10 x the tolerance on the coherence)
        for mode in ("H1", "H2"):
            tf, coh = backend.welch_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det,
                                                      average="median", precision="f64")
            rt, rc = orc.compute_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det,
                                                   average="median")
            assert relmax(tf, rt, det) < 1e-9 and relmax(coh, rc, det) < 1e-9, (n, W, mode, "median")
    # what the reference-shaped API does with small problems (backend.TF_PRECISION = "auto"): median
    # averaging and one- or two-frame estimates meet the plain 1e-6, coherence included
    x = rng.standard_normal((5000, 1)) * 0.3
    y = np.stack([np.convolve(x[:, 0], rng.standard_normal(7))[:5000] for _ in range(2)], axis=1)
    inp, out = dsp.Signal(None, x, 48000), dsp.Signal(None, y + 1e-3 * rng.standard_normal(y.shape), 48000)
    for W, avg in ((256, "median"), (4096, "mean"), (2048, "median")):
        inp.set_spectrum_parameters(window_length_samples=W, overlap_percent=50, detrend=True, average=avg)
        sp = dsp.transfer_functions.compute_transfer_function(out, inp, W, TransferFunctionType.H1)
        rt, rc = orc.compute_transfer_function(out.time_data, inp.time_data, 48000, W, "H1", average=avg)
        assert relmax(sp.spectral_data, rt, True) < TOL and relmax(sp.coherence, rc, True) < TOL, (W, avg)
    # since round 4 the float64 route reaches the reference's longest window (a 5000-sample signal: one zero-padded frame)
    tf, coh = backend.welch_transfer_function(y, x, 48000, 32768, "H1", precision="f64")
    rt, rc = orc.compute_transfer_function(y, x, 48000, 32768, "H1")
    assert relmax(tf, rt, True) < 1e-9 and relmax(coh, rc, True) < 1e-9  # (detrend: the DC bin is 0 / 0 in the reference)
    with pytest.raises(NotImplementedError):  # median averaging: at most 4096 frames
        backend.welch_transfer_function(np.zeros((40000, 1)), np.zeros((40000, 1)), 48000, 16, "H1", average="median",
                                        precision="f64")


def test_deconvolve_golden():
    meta, z = load_golden("deconvolve")
    worst = 0.0
    for i, c in enumerate(meta["cases"]):
        tag = c["data"]
        x = z[f"x_{tag}"] if c["den"] == "mono" else z[f"x2_{tag}"]
        inp = dsp.Signal(None, x.copy(), meta["fs"])
        out = dsp.Signal(None, z[f"y_{tag}"].copy(), meta["fs"])
        kw = dict(apply_regularization=c["reg"], start_stop_hz=c["ss"], threshold_db=c["thr"],
                  padding=c["pad"], keep_original_length=c["keep"])
        ir = dsp.transfer_functions.spectral_deconvolve(out, inp, **kw)  # np2: Bluestein path
        assert isinstance(ir, dsp.ImpulseResponse) and ir.constrain_amplitude is False
        e = relmax(ir.time_data, z[f"ir_{i}"])
        worst = max(worst, e)
        assert e < TOL, (c, e)
    print("deconvolve worst rel-max", worst)


def test_fir_golden():
    meta, z = load_golden("fir")
    worst = 0.0
    fs = meta["fs"]
    for i, c in enumerate(meta["cases"]):
        x = z["x_" + c["data"]]
        sig = dsp.Signal(None, x.copy(), fs)
        if c["kind"] == "filter":
            flt = dsp.Filter.from_ba(z[c["taps_key"]], [1.0], fs)
            o = flt.filter_signal(sig, channels=c["channels"])
            assert np.array_equal(sig.time_data, x)  # input untouched
            e = relmax(o.time_data, z[f"y_{i}"])
        else:
            fb = dsp.FilterBank([dsp.Filter.from_ba(b, [1.0], fs) for b in z["bank_taps"]])
            o = fb.filter_signal(sig, FilterBankMode[c["mode"]])
            if c["mode"] == "Parallel":
                assert isinstance(o, dsp.MultiBandSignal)
                e = relmax(o.get_all_time_data()[0], z[f"y_{i}"])
            else:
                assert type(o) is dsp.Signal
                e = relmax(o.time_data, z[f"y_{i}"])
        worst = max(worst, e)
        assert e < TOL, (c, e)
    print("fir worst rel-max", worst)


def test_fir_state_zero_phase_long_golden():
    """activate_zi (incl. the reference's state hand-back quirk), zero_phase (filtfilt) and a
    20001-tap filter (four-step FFT overlap-save) against the reference's outputs."""
    import warnings
    meta, z = load_golden("fir_state")
    fs = meta["fs"]
    x = z["x"]
    for c in meta["cases"]:
        if c["kind"] == "zi_blocks":
            flt = dsp.Filter.from_ba(z[f"b_{c['order']}"], [1.0], fs)
            flt.initialize_zi(2)
            assert np.allclose(np.asarray(flt.zi), z[f"zi0_{c['order']}"], rtol=1e-12, atol=1e-15)
            outs = []
            for k, (a, e) in enumerate(c["blocks"]):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    o = flt.filter_signal(dsp.Signal(None, x[a:e].copy(), fs), activate_zi=True)
                outs.append(o.time_data)
                assert np.asarray(flt.zi).shape == z[f"zi_{c['order']}_{k}"].shape
                assert relmax(np.asarray(flt.zi), z[f"zi_{c['order']}_{k}"]) < TOL
            assert relmax(np.concatenate(outs), z[f"y_zi_{c['order']}"]) < TOL
        elif c["kind"] == "zi_channel":
            flt = dsp.Filter.from_ba(z[f"b_{c['order']}"], [1.0], fs)
            flt.initialize_zi(2)
            o = flt.filter_signal(dsp.Signal(None, x[:c["n"]].copy(), fs), channels=c["channels"],
                                  activate_zi=True)
            assert relmax(o.time_data, z[f"y_zi_ch1_{c['order']}"]) < TOL
            assert relmax(np.asarray(flt.zi), z[f"zi_ch1_{c['order']}"]) < TOL
        elif c["kind"] == "zero_phase":
            flt = dsp.Filter.from_ba(z[f"b_{c['order']}"], [1.0], fs)
            o = flt.filter_signal(dsp.Signal(None, x.copy(), fs), zero_phase=True)
            assert relmax(o.time_data, z[f"y_zp_{c['order']}"]) < TOL
        elif c["kind"] == "bank_zero_phase":
            fb = dsp.FilterBank([dsp.Filter.from_ba(b, [1.0], fs) for b in z["bank_taps"]])
            o = fb.filter_signal(dsp.Signal(None, x.copy(), fs), FilterBankMode[c["mode"]], zero_phase=True)
            got = o.get_all_time_data()[0] if c["mode"] == "Parallel" else o.time_data
            assert relmax(got, z[f"y_bank_zp_{c['mode']}"]) < TOL, c
        elif c["kind"] == "bank_zi":
            fb = dsp.FilterBank([dsp.Filter.from_ba(b, [1.0], fs) for b in z["bank_taps"]])
            fb.initialize_zi(2)
            outs = []
            for a, e in c["blocks"]:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    o = fb.filter_signal(dsp.Signal(None, x[a:e].copy(), fs), FilterBankMode.Parallel,
                                         activate_zi=True)
                outs.append(o.get_all_time_data()[0])
            assert relmax(np.concatenate(outs), z["y_bank_zi"]) < TOL
        elif c["kind"] == "long":
            flt = dsp.Filter.from_ba(z["b_long"], [1.0], fs)
            o = flt.filter_signal(dsp.Signal(None, z["x_long"].astype(np.float64), fs))
            assert relmax(o.time_data, z["y_long"]) < TOL
    with pytest.raises(AssertionError):
        dsp.Filter.from_ba(z["b_64"], [1.0], fs).filter_signal(dsp.Signal(None, x.copy(), fs),
                                                              activate_zi=True, zero_phase=True)


@pytest.mark.parametrize("n_taps,n,n_ch", [(2049, 50001, 3), (3000, 70000, 2), (8193, 40000, 1), (4097, 12288 * 3, 2),
                                            (4097, 5000, 5), (3001, 100000, 2), (2049, 14336 * 4, 4),
                                            (6145, 90000, 3), (1025, 80000, 3), (1501, 50000, 2), (1100, 60000, 2)])
def test_fir_16k_blocks_vs_oracle(n_taps, n, n_ch):
    """The 16384-point block kernel (2049 .. 8193 taps): tap counts whose discarded length is a
    multiple of 4 (interior blocks store whole groups of four behind one compare per quarter) and
    others (element-wise tested stores), odd channel counts, lengths that are / are not whole
    blocks, one short block."""
    rng = np.random.default_rng(n_taps + n)
    x = rng.standard_normal((n, n_ch)) * 0.1
    taps = [rng.standard_normal(n_taps) * np.exp(-np.arange(n_taps) / (n_taps / 5.0)) * 0.05 for _ in range(2)]
    y = backend.fir_filter_bank(x, taps, backend.DS_FB_PARALLEL)
    r = np.transpose(orc.filterbank_fir(taps, x, "Parallel"), (2, 0, 1))
    assert relmax(y, r) < TOL, relmax(y, r)


def test_fir_one_and_two_tap_filters():
    """Degenerate banks (found by tests/sweeps/fuzz_fir.py on the oracle side): gains and two-tap
    filters in the three bank modes."""
    rng = np.random.default_rng(17)
    x = rng.standard_normal((12287, 2)) * 0.2
    for T in (1, 2):
        taps = [rng.standard_normal(T) * 0.5 for _ in range(3)]
        for mode, name in ((backend.DS_FB_PARALLEL, "Parallel"), (backend.DS_FB_SUMMED, "Summed"),
                           (backend.DS_FB_SEQUENTIAL, "Sequential")):
            y = backend.fir_filter_bank(x, taps, mode)
            r = orc.filterbank_fir(taps, x, name)
            if name == "Parallel":
                r = np.transpose(r, (2, 0, 1))
            assert y.shape == r.shape and relmax(y, r) < TOL, (T, name, relmax(y, r))


def test_fir_signal_shorter_than_the_filter():
    """DESIGN section 2, limit (x), closed for small problems: 4097 taps with near-zero leading taps on 100 ... 3000
    samples.  The FFT routes leave 3-4e-5 of the (tiny) output there; such calls take the direct float64 sum."""
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(4097)
    for n, n_ch in ((100, 2), (1000, 1), (3000, 3), (300, 1)):
        x = rng.standard_normal((n, n_ch)) * 0.1
        taps = [rng.standard_normal(4097) * np.hanning(4097) / 64.0 for _ in range(2)]
        ctx.routes()
        y = backend.fir_filter_bank(x, taps, backend.DS_FB_PARALLEL)
        assert ctx.routes() == {"fir@direct_f64"}
        for k in range(2):
            assert relmax(y[k], orc.lfilter_fir(taps[k], x)) < TOL, (n, n_ch, k)


def test_fir_long_filters_vs_oracle():
    """> 8193 taps: overlap-save on the four-step FFT, several blocks, bank modes."""
    rng = np.random.default_rng(91)
    n, t = 300000, 9000
    x = rng.standard_normal((n, 3)) * 0.1
    taps = [rng.standard_normal(t) * np.exp(-np.arange(t) / 1500.0) * 0.05 for _ in range(3)]
    for mode, name in ((backend.DS_FB_PARALLEL, "Parallel"), (backend.DS_FB_SUMMED, "Summed"),
                       (backend.DS_FB_SEQUENTIAL, "Sequential")):
        y = backend.fir_filter_bank(x, taps, mode)
        r = orc.filterbank_fir(taps, x, name)
        if name == "Parallel":
            r = np.transpose(r, (2, 0, 1))
        assert relmax(y, r) < TOL, (name, relmax(y, r))


@pytest.mark.parametrize("fixture", ["istft", "istft_anylen"])
def test_istft_golden_and_round_trip(fixture):
    """transforms.istft against the reference's outputs, and the reference's own fidelity test
    (tests/test_transforms.py:102-134): get_spectrogram -> istft reproduces the signal.  istft_anylen:
    fft_length_samples that are not powers of two (missing 6)."""
    from dsptoolbox_amd.standard.enums import SpectrumScaling as S
    meta, z = load_golden(fixture)
    fs = meta["fs"]
    x = z["x"]
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, x.copy(), fs)
        s.set_spectrogram_parameters(window_length_samples=c["W"], window_type=Window[c["win"]],
                                     overlap_percent=c["ov"], fft_length_samples=c["nfft"], detrend=False,
                                     padding=c["pad"], scaling=S[c["sc"]])
        rec = dsp.transforms.istft(z[f"stft_{i}"], original_signal=s)
        assert relmax(rec.time_data, z[f"rec_sig_{i}"]) < TOL, (c, relmax(rec.time_data, z[f"rec_sig_{i}"]))
        if c["has_par"]:
            rec2 = dsp.transforms.istft(z[f"stft_{i}"], parameters=dict(s._spectrogram_parameters),
                                        sampling_rate_hz=fs)
            assert rec2.time_data.shape == z[f"rec_par_{i}"].shape
            assert relmax(rec2.time_data, z[f"rec_par_{i}"]) < TOL
    # device STFT -> device inverse STFT, larger signal
    rng = np.random.default_rng(31)
    y = rng.standard_normal((100000, 3)) * 0.3
    for W, nfft in (((1024, None), (512, 1024), (4096, None)) if fixture == "istft" else ((512, 768), (256, 1001))):
        s = dsp.Signal(None, y.copy(), fs)
        s.set_spectrogram_parameters(window_length_samples=W, fft_length_samples=nfft)
        t, f, sp = s.get_spectrogram()
        rec = dsp.transforms.istft(sp, original_signal=s)
        assert relmax(rec.time_data, y) < 2 * TOL, (W, relmax(rec.time_data, y))


def test_convolve_rir_on_signal_golden():
    meta, z = load_golden("rir")
    fs = meta["fs"]
    x = z["x"].astype(np.float64)
    for i, c in enumerate(meta["cases"]):
        sig = dsp.Signal(None, x.copy(), fs)
        rir = dsp.ImpulseResponse(None, z[f"h_{i}"].copy(), fs, constrain_amplitude=False)
        o = dsp.room_acoustics.convolve_rir_on_signal(sig, rir, keep_peak_level=c["keep_peak_level"],
                                                      keep_length=c["keep_length"])
        assert o.time_data.shape == z[f"y_{i}"].shape
        assert relmax(o.time_data, z[f"y_{i}"]) < TOL, (c, relmax(o.time_data, z[f"y_{i}"]))
        assert np.array_equal(sig.time_data, x)


def test_library_rccl_communicator_single_rank():
    """ds_comm_unique_id / ds_comm_init / ds_bcast / ds_comm_destroy with a one-rank communicator:
    checks the dlopen of RCCL, the by-value id hand-over and the broadcast call on this GPU (the
    multi-rank use is rehearsed with gloo in tests/test_distributed_cpu.py and by bench.py)."""
    import ctypes as C
    from dsptoolbox_amd._lib import Context, DeviceBuffer
    ctx = Context(0)
    try:
        ident = C.create_string_buffer(128)
        ctx.check(ctx.lib.ds_comm_unique_id(ident), "ds_comm_unique_id")
        assert any(b != 0 for b in ident.raw)
        ctx.check(ctx.lib.ds_comm_init(ctx.handle, 1, 0, ident.raw), "ds_comm_init")
        data = np.arange(4096, dtype=np.float32)
        buf = DeviceBuffer.from_array(ctx, data)
        ctx.check(ctx.lib.ds_bcast(ctx.handle, C.c_void_p(buf.ptr), data.nbytes, 0), "ds_bcast")
        ctx.sync()
        assert np.array_equal(buf.to_array(data.shape, np.float32), data)
        # all-gather of result slices (one rank: its slot is the whole receive buffer)
        out = DeviceBuffer(ctx, data.nbytes)
        ctx.check(ctx.lib.ds_allgather(ctx.handle, C.c_void_p(buf.ptr), C.c_void_p(out.ptr), data.nbytes),
                  "ds_allgather")
        ctx.sync()
        assert np.array_equal(out.to_array(data.shape, np.float32), data)
        ctx.check(ctx.lib.ds_comm_destroy(ctx.handle), "ds_comm_destroy")
        # collectives without a communicator are errors, not crashes
        assert ctx.lib.ds_bcast(ctx.handle, C.c_void_p(buf.ptr), data.nbytes, 0) != 0
        assert ctx.lib.ds_allgather(ctx.handle, C.c_void_p(buf.ptr), C.c_void_p(out.ptr), data.nbytes) != 0
        buf.free()
        out.free()
    finally:
        ctx.close()


def test_measured_copy_bandwidth():
    """ds_measure_copy: the measured denominator bench.py prints next to the nominal 8 TB/s."""
    import ctypes as C
    from dsptoolbox_amd._lib import Context
    ctx = Context(0)
    try:
        gbs = C.c_double(0.0)
        ctx.check(ctx.lib.ds_measure_copy(ctx.handle, 1 << 28, 5, C.byref(gbs)), "ds_measure_copy")
        assert 1000.0 < gbs.value < 8000.0, gbs.value
        assert ctx.lib.ds_measure_copy(ctx.handle, 0, 5, C.byref(gbs)) != 0
    finally:
        ctx.close()


@pytest.mark.timeout(600)
def test_bench_two_ranks_strong_scaling_rehearsal():
    """bench.py --gpus 2 --scaling strong as the driver launches it, with gloo as torch's backend so
    that both ranks can share this one GPU (RCCL refuses two ranks on a device): the per-rank
    shards, the host broadcast of the sweep and the JSON contract of the strong-scaling line."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "5", "--warmup", "2", "--scaling", "strong", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["bcast"] == "host"
    assert out["value"] > 0 and out["roofline"]["frac"] > 0


@pytest.mark.timeout(600)
def test_bench_two_ranks_weak_scaling_rehearsal():
    """bench.py --gpus 2 as the driver launches it for the scaling curve (weak scaling, the default), with
    gloo as torch's backend so that both ranks can share this one GPU: every rank an independent batch,
    value = 2 x units / slowest rank, one JSON line from rank 0."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["bcast"] == "host"
    assert out["value"] > 0 and out["roofline"]["frac"] > 0 and out["steps"] == 10


@pytest.mark.timeout(600)
def test_bench_default_line_contract():
    """`python bench.py` (one GPU, the headline workload, a short run with a reduced CPU leg): ONE JSON
    line with the driver's fields, the roofline object (live kernel time, its raw bracket and the
    bracket's measured fixed cost) and the CPU baseline with its parity against the GPU result."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "5",
                        "--cpu-channels", "2"], cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["steps"] == 40 and out["warmup"] == 5 and out["higher_is_better"] is True
    assert out["vs_baseline"] is None and out["dtype"] == "f32" and out["data"] == "synthetic"
    assert "workload" in out["config"] and "model" not in out["config"]
    roof = out["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12 and 0.05 < roof["frac"] < 1.0
    assert roof["kernel"] == "welch4096_main"
    # frac is the measured kernel time as it is: nothing subtracted, no derived "net" figure
    assert abs(roof["frac"] - roof["algorithmic_per_launch"] / (roof["kernel_avg_ms"] * 1e-3) / 1e9 / roof["peak"]) < 1e-9
    assert "dispatch" in roof["kernel_time_source"] and roof["measured_copy_gbs"] > 1000.0
    assert roof["kernel_avg_ms"] < out["ms_per_step"]
    cpu = out["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] == 1 and cpu["value"] > 0 and "sample" in cpu
    assert cpu["parity_rel_max_vs_gpu"] < TOL
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # default arguments time exactly --steps steps: one region (every 4th of its 40 launches bracketed), no second
    # region, no other workloads
    assert roof["kernel_event_sampling"].endswith("(10 brackets)"), roof["kernel_event_sampling"]
    assert "steady_state" not in out and "workloads" not in out


@pytest.mark.timeout(600)
def test_bench_opt_in_steady_state_and_workloads():
    """`--steady-steps S --workloads`: a second timed region of S steps ("steady_state") and the other BASELINE configs,
    each over --workload-steps steps with its parity against the oracle."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "5", "--cpu-channels", "2",
                        "--steady-steps", "400", "--workloads", "--workload-steps", "40"],
                       cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 40 and out["roofline"]["kernel_event_sampling"].endswith("(10 brackets)")
    ss = out["steady_state"]
    assert ss["steps"] == 400 and ss["kernel"] == "welch4096_main" and ss["kernel_brackets"] == 100
    wl = out["workloads"]
    assert set(wl) == {"welch_h1_1024", "fir_bank", "csm", "deconv", "welch_h1_detrend_off", "short_estimate_api"}
    for name in ("welch_h1_1024", "fir_bank", "csm", "deconv", "welch_h1_detrend_off"):
        assert wl[name]["steps"] == 40 and wl[name]["parity_rel_max_vs_oracle"] < TOL, (name, wl[name])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("workload,names", [("welch_h1", {"tf_real", "tf_imag", "coherence"}),
                                            ("fir_bank", {"y_windows", "y_window_starts"}),
                                            ("csm", {"csm_real", "csm_imag"}), ("deconv", {"ir", "ir_items"})])
def test_bench_dump_outputs(workload, names, tmp_path):
    """`bench.py --dump-outputs DIR`: the results of the last timed step as float32 / float64 .npy files, 64 MB at most,
    and their values against the oracle on the bench's own seeded inputs (the samples of fir_bank and deconv at the
    positions the dump records)."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--steps", "3",
                        "--warmup", "2", "--no-cpu-baseline", "--preheat-ms", "0", "--steady-steps", "0",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == names
    assert all(a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)) for a in got.values())
    assert 0 < sum(a.nbytes for a in got.values()) <= 64 * 10**6
    if workload == "welch_h1":
        # detrended (the default): bins 1 .. 2048, the DC bin being 0 / 0
        from dsptoolbox_amd.generators import sweep_and_responses
        x, y = sweep_and_responses(2**20, 64, 48000)
        rt, rc = orc.compute_transfer_function_batched(y, x, 48000, 4096, "H1", detrend=True, workers=-1)
        band = inband(4096)[1:]
        assert got["coherence"].shape == (2048, 64)
        assert relmax((got["tf_real"] + 1j * got["tf_imag"])[band], rt[1:][band]) < TOL
        assert relmax(got["coherence"][band], rc[1:][band]) < TOL
    elif workload == "fir_bank":  # bench.fir_bank's inputs; two (band, channel) pairs, both windows of each
        from dsptoolbox_amd.generators import fir_bank_taps
        x = np.random.default_rng(3).standard_normal((2**22, 8)) * 0.1
        taps = fir_bank_taps(32, 4097, 48000).astype(np.float32)
        L = got["y_windows"].shape[-1]
        for k, c in ((0, 0), (23, 5)):
            ref = orc.lfilter_fir(taps[k].astype(np.float64), x[:, c])[:, 0]
            for j in range(2):
                s0 = int(got["y_window_starts"][k, c, j])
                assert np.max(np.abs(got["y_windows"][k, c, j] - ref[s0:s0 + L])) < TOL * np.max(np.abs(ref)), (k, c, j)
        assert np.all(got["y_window_starts"][..., 0] == 0) and np.all(got["y_window_starts"][..., 1] >= L)
    elif workload == "csm":  # bench.csm's inputs; DC is excluded as in the bench's own parity (detrended: 0 there)
        from dsptoolbox_amd.generators import mic_array_noise
        _, ref = orc.csm_welch_batched(mic_array_noise(512000, 64, 4), 48000, 1024, "hann", 50, True, "FFTBackward", workers=-1)
        assert relmax((got["csm_real"] + 1j * got["csm_imag"])[1:], ref[1:]) < TOL
    else:  # bench.deconv's inputs; the first four of the dumped items
        from dsptoolbox_amd.generators import exponential_sweep
        n = 8192
        x = exponential_sweep(n, 48000)
        rng = np.random.default_rng(5000)
        h = rng.standard_normal((1024, 2, 256)) * np.exp(-np.arange(256) / 40.0)
        y = np.fft.irfft(np.fft.rfft(x)[None, None, :] * np.fft.rfft(h, n, axis=-1), n, axis=-1)
        y = (y + 1e-3 * rng.standard_normal(y.shape)).astype(np.float32)
        for row, i in enumerate(got["ir_items"][:4].astype(int)):
            ref = orc.spectral_deconvolve(y[i].T.astype(np.float64), x[:, None], 48000)
            assert relmax(got["ir"][row].T, ref) < TOL, (row, i)


def test_das_map_golden_and_large():
    """Delay-and-sum beamformer maps: the reference's outputs (4 steering formulations, with and
    without diagonal removal), and a 64-mic / 3000-point / 40-bin problem against the oracle."""
    meta, z = load_golden("das")
    for i, c in enumerate(meta["cases"]):
        m = dsp.beamforming.delay_and_sum_map(z[f"f_{i}"], z[f"csm_{i}"], z[f"h_{i}"], c["remove_csm_diagonal"])
        assert relmax(m.reshape(c["grid_shape"]), z[f"map_{i}"]) < TOL, (c, relmax(m.reshape(c["grid_shape"]), z[f"map_{i}"]))
    rng = np.random.default_rng(41)
    F, Cn, G = 40, 64, 3000
    a = rng.standard_normal((F, Cn, 70)) + 1j * rng.standard_normal((F, Cn, 70))
    csm = a @ np.conj(np.swapaxes(a, 1, 2)) / 70
    mic = rng.uniform(-0.5, 0.5, (Cn, 3))
    grid = np.c_[rng.uniform(-1, 1, (G, 2)), np.full(G, 1.5)]
    r = np.linalg.norm(mic[:, None, :] - grid[None, :, :], axis=-1)  # (C, G)
    f = np.linspace(1000.0, 2000.0, F)
    h = np.exp(-2j * np.pi * f[:, None, None] / 343.0 * r[None]) / r[None] / Cn
    for rm in (True, False):
        m = dsp.beamforming.delay_and_sum_map(f, csm, h, rm)
        assert relmax(m, orc.das_map(f, csm, h, rm)) < TOL, rm
    q = dsp.beamforming.quadratic_form_map(csm, h)
    assert q.shape == (G, F)
    assert relmax(q, np.einsum("fcg,fcd,fdg->gf", h.conj(), csm, h).real) < TOL


def test_mel_spectrogram_and_mfcc_golden():
    """log_mel_spectrogram / mfcc (STFT, |.|^2, mel contraction, dB, DCT on the device) against
    the reference's outputs.  The values are decibels: the comparison is relative to the largest
    magnitude (some tens of dB), i.e. an absolute error of ~1e-5 dB."""
    from dsptoolbox_amd.standard.enums import SpectrumScaling as S
    meta, z = load_golden("mel")
    fs = meta["fs"]
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, z["x"].copy(), fs)
        s.set_spectrogram_parameters(window_length_samples=c["W"], fft_length_samples=c["nfft"],
                                     scaling=S[c["scaling"]])
        t, f_mel, lm = dsp.transforms.log_mel_spectrogram(s, range_hz=c["range_hz"], n_bands=c["n_bands"],
                                                          generate_plot=False)
        assert np.allclose(t, z[f"t_{i}"]) and np.allclose(f_mel, z[f"fmel_{i}"])
        ref = z[f"logmel_{i}"]
        assert lm.shape == ref.shape
        # Digital silence (the all-zero frame the padding appends) is exactly 0 in the reference and
        # hits its -3076.5 dB floor; on the device that frame shares a complex transform with its
        # neighbour and keeps ~1e-9 of the neighbour's amplitude (fp32), i.e. about -180 dB.
        floor = ref < -1000.0
        assert np.all(lm[floor] < -150.0)
        assert relmax(lm[~floor], ref[~floor]) < TOL, (c, relmax(lm[~floor], ref[~floor]))
        t2, f_mel2, mf = dsp.transforms.mfcc(s, generate_plot=False)
        refm = z[f"mfcc_{i}"]
        assert np.allclose(f_mel2, z[f"fmel2_{i}"]) and mf.shape == refm.shape
        ok = ~np.any(z[f"logmel_{i}"] < -1000.0, axis=0) if ref.shape[0] == refm.shape[0] else \
            np.abs(refm).max(axis=0) < 1e4  # frames that contain a floor value have huge coefficients
        ok = np.broadcast_to(ok[None], refm.shape)
        if np.max(np.abs(refm[ok])) == 0.0:
            # 40 default bands over 129 bins: empty triangles -> NaN filters -> the reference's
            # nan_to_num turns every coefficient into 0; the device does the same
            assert np.array_equal(mf[ok], refm[ok])
        else:
            assert relmax(mf[ok], refm[ok]) < TOL, (c, relmax(mf[ok], refm[ok]))
        mfilt, _ = dsp.transforms.mel_filterbank(np.fft.rfftfreq(c["W"], 1 / fs), c["range_hz"], c["n_bands"])
        assert np.array_equal(mfilt, z[f"mfilt_{i}"])
    with pytest.raises(NotImplementedError):
        dsp.transforms.log_mel_spectrogram(dsp.Signal(None, z["x"].copy(), fs))


def test_fir_design_matches_lfilter():
    """reference tests/test_classes.py:495-512: FIR filter_signal == scipy.signal.lfilter."""
    import scipy.signal as sig
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20000, 3)) * 0.2
    flt = dsp.Filter.fir_filter(150, 1000.0, FilterPassType.Lowpass, 48000)
    s = dsp.Signal(None, x.copy(), 48000)
    o = flt.filter_signal(s)
    ref = sig.lfilter(flt.ba[0], [1.0], x, axis=0)
    assert relmax(o.time_data, ref) < TOL


@pytest.mark.parametrize("W", [8, 64, 512, 2048, 4096, 8192, 16384])
def test_welch_all_lengths_vs_oracle(W):
    rng = np.random.default_rng(W)
    n = max(6 * W + 123, 5000)
    x = rng.standard_normal((n, 3)) * 0.3
    x[:, 2] = np.convolve(x[:, 0], [0.5, 0.3, -0.2, 0.1])[:n] + 0.05 * x[:, 2]
    for det in (True, False):
        a = backend._welch(x, None, 48000, Window.Hann, W, 50, det, "mean",
                           SpectrumScaling.PowerSpectralDensity)
        r = orc.welch(x, None, 48000, "hann", W, 50, det, "mean", "PowerSpectralDensity")
        assert relmax(a, r, det) < TOL
        k = backend._welch(x[:, 0], x[:, 2], 48000, Window.Hann, W, 50, det, "mean",
                           SpectrumScaling.FFTBackward)
        r = orc.welch(x[:, 0], x[:, 2], 48000, "hann", W, 50, det, "mean", "FFTBackward")
        assert relmax(k, r, det) < TOL


def test_transfer_function_median_vs_oracle():
    rng = np.random.default_rng(77)
    n = 30000
    x = rng.standard_normal((n, 1)) * 0.3
    y = np.stack([np.convolve(x[:, 0], rng.standard_normal(16))[:n] for _ in range(3)], axis=1)
    y += 0.05 * rng.standard_normal(y.shape)
    for mode in ("H1", "H2", "H3"):
        for W, sc in ((512, SpectrumScaling.FFTBackward), (4096, SpectrumScaling.PowerSpectralDensity)):
            tf, coh = backend.welch_transfer_function(y, x, 48000, W, mode, average="median", scaling=sc)
            rt, rc = orc.compute_transfer_function(y, x, 48000, W, mode, average="median",
                                                   scaling=sc.name)
            # the median picks single-frame values: no averaging-down of the per-frame fp32 FFT
            # error (~3e-7 per power quantity), the coherence combines three of them, and two
            # nearly equal frames can swap ranks: observed up to 3.2e-6 at 15 frames
            assert relmax(tf, rt, True) < TOL and relmax(coh, rc, True) < 10 * TOL, (mode, W)


def test_median_many_frames_vs_oracle():
    """Median averaging over more frames than eight bins' series fit in LDS: the kernels fall back
    to 4, 2 or 1 bins per workgroup (up to 12 799 frames for Welch, 19 199 for the CSM)."""
    rng = np.random.default_rng(79)
    for n, W, ov in ((120000, 128, 50), (150000, 64, 50), (100000, 64, 75)):   # 1875, 4688, 6250 frames
        x = rng.standard_normal((n, 1)) * 0.3
        y = np.stack([np.convolve(x[:, 0], rng.standard_normal(8))[:n] for _ in range(2)], axis=1)
        y += 0.05 * rng.standard_normal(y.shape)
        tf, coh = backend.welch_transfer_function(y, x, 48000, W, "H1", overlap_percent=ov, average="median")
        rt, rc = orc.compute_transfer_function(y, x, 48000, W, "H1", overlap_percent=ov, average="median")
        assert relmax(tf, rt, True) < 2 * TOL and relmax(coh, rc, True) < 10 * TOL, (n, W, relmax(tf, rt, True))
        psd = backend._welch(y, None, 48000, Window.Hann, W, ov, True, "median", SpectrumScaling.FFTBackward)
        rp = orc.welch(y, None, 48000, "hann", W, ov, True, "median", "FFTBackward")
        assert relmax(psd, rp, True) < 2 * TOL
    x = rng.standard_normal((100000, 3)) * 0.3 + 0.4 * rng.standard_normal((100000, 1))
    f, csm = backend._csm_welch(x, 48000, 64, Window.Hann, 50, True, "median", SpectrumScaling.FFTBackward)
    rf, rcsm = orc.csm_welch(x, 48000, 64, "hann", 50, True, "median", "FFTBackward")   # 3125 frames
    assert relmax(csm, rcsm) < 10 * TOL and orc.rel_l2(csm, rcsm) < TOL


def test_bluestein_table_cache_is_bounded():
    """Whole-signal spectra of ever-changing, non-fast lengths (variable-length recordings): the
    chirp-filter tables are a least-recently-used cache under a byte cap (256 MB), so device
    memory stays flat -- 30 lengths x 16 MB tables would otherwise pin 480 MB for good."""
    import ctypes as C
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        ctx.check(ctx.lib.ds_mem_info(ctx.handle, C.byref(f), C.byref(t)), "ds_mem_info")
        return f.value

    rng = np.random.default_rng(5)
    x = rng.standard_normal((700001, 1)) * 0.1
    lengths = [600011 + 2 * 1013 * i for i in range(30)]  # odd, mostly with large prime factors -> M = 2^21
    backend.rfft_spectrum(x[:lengths[0]], lengths[0])
    free0 = free_bytes()
    for L in lengths:
        sp = backend.rfft_spectrum(x[:L], L)
    ref = np.fft.rfft(x[:L, 0])
    assert relmax(sp[:, 0], ref) < TOL
    free1 = free_bytes()
    assert free0 - free1 < 300 * 2**20, (free0 - free1) / 2**20


def test_default_context_is_per_thread():
    """Two Python threads through the default context at once (ctypes drops the GIL in a call): each
    thread owns a ds_ctx -- stream, workspace -- so concurrent calls do not corrupt each other."""
    import threading
    from dsptoolbox_amd._lib import get_context
    rng = np.random.default_rng(6)
    xs = [rng.standard_normal((40000 + 5000 * i, 3)) * 0.3 for i in range(2)]
    refs = [orc.welch(x, None, 48000, "hann", 1024, 50, True, "mean", "FFTBackward") for x in xs]
    errs, ctxs = [None, None], [None, None]

    def work(i):
        ctxs[i] = get_context().handle.value if hasattr(get_context().handle, "value") else id(get_context())
        worst = 0.0
        for _ in range(20):
            psd = backend._welch(xs[i], None, 48000, Window.Hann, 1024, 50, True, "mean", SpectrumScaling.FFTBackward)
            worst = max(worst, relmax(psd, refs[i], True))
        errs[i] = worst

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert ctxs[0] != ctxs[1]
    assert errs[0] < TOL and errs[1] < TOL, errs


def test_csm_median_vs_oracle():
    """get_csm with average="median": the reference's pair loop of median-averaged _welch calls."""
    rng = np.random.default_rng(78)
    n = 20000
    common = rng.standard_normal(n)
    x = np.stack([0.3 * rng.standard_normal(n) + 0.5 * np.roll(common, 3 * c) for c in range(5)], axis=1)
    for W, det, sc in ((256, True, SpectrumScaling.FFTBackward), (1024, False, SpectrumScaling.PowerSpectralDensity),
                       (512, True, SpectrumScaling.AmplitudeSpectrum)):
        f, csm = backend._csm_welch(x, 48000, W, Window.Hann, 50, det, "median", sc)
        rf, rcsm = orc.csm_welch(x, 48000, W, "hann", 50, det, "median", sc.name)
        assert np.allclose(f, rf)
        # single-frame (median) values carry the full per-frame fp32 error: see the tf test above
        assert relmax(csm, rcsm) < 10 * TOL, (W, relmax(csm, rcsm))
        assert orc.rel_l2(csm, rcsm) < TOL


def test_welch_window_length_limits():
    x = np.zeros((100000, 1))
    with pytest.raises(AssertionError):  # the reference's own limit: 2**3 .. 2**18
        backend._welch(x, None, 48000, Window.Hann, 2**19, 50, True, "mean",
                       SpectrumScaling.FFTBackward)
    with pytest.raises(AssertionError):
        backend._welch(x, None, 48000, Window.Hann, 1000, 50, True, "mean",
                       SpectrumScaling.FFTBackward)


@pytest.mark.parametrize("W", [2**15, 2**16, 2**18])
def test_welch_long_windows_vs_oracle(W):
    """Window lengths beyond the LDS-resident FFT (four-step transform per frame pair)."""
    rng = np.random.default_rng(W)
    n = 5 * W + 1234
    x = rng.standard_normal((n, 3)) * 0.3
    x[:, 2] = np.convolve(x[:, 0], [0.5, 0.3, -0.2, 0.1])[:n] + 0.05 * x[:, 2]
    for det in (True, False):
        a = backend._welch(x, None, 48000, Window.Hann, W, 50, det, "mean",
                           SpectrumScaling.PowerSpectralDensity)
        r = orc.welch(x, None, 48000, "hann", W, 50, det, "mean", "PowerSpectralDensity")
        assert relmax(a, r, det) < TOL
        k = backend._welch(x[:, 0], x[:, 2], 48000, Window.Hann, W, 50, det, "mean",
                           SpectrumScaling.FFTBackward)
        r = orc.welch(x[:, 0], x[:, 2], 48000, "hann", W, 50, det, "mean", "FFTBackward")
        assert relmax(k, r, det) < TOL
    if W == 2**15:
        for mode in ("H1", "H2", "H3"):
            for avg in ("mean", "median"):
                tf, coh = backend.welch_transfer_function(x[:, 1:], x[:, :1], 48000, W, mode, average=avg,
                                                          overlap_percent=75)
                rt, rc = orc.compute_transfer_function(x[:, 1:], x[:, :1], 48000, W, mode, average=avg,
                                                       overlap_percent=75)
                lim = TOL if avg == "mean" else 10 * TOL  # see test_transfer_function_median_vs_oracle
                # channel 1 is independent noise (coherence ~ 1/sqrt(F)): compare the correlated one tightly
                assert relmax(tf[:, 1], rt[:, 1], True) < lim, (mode, avg)
                assert relmax(coh[:, 1], rc[:, 1], True) < lim, (mode, avg)
                if mode == "H1":  # the uncorrelated channel too where the estimator is well conditioned
                    assert orc.rel_l2(tf[1:], rt[1:]) < lim, (mode, avg)  # DC is 0/0 after detrending


@pytest.mark.parametrize("W", [2**15, 2**16, 2**17, 2**18])
def test_welch_long_windows_on_the_register_transform(W):
    """Windows of 2^15 ... 2^18 samples since round 4: decimation in frequency into W / 4096 class sequences, the
    headline kernel's loop on them, fold across the classes (kernels_welch_long.hpp).  One input for all outputs and
    one per output, H1 / H3, odd and even frame counts (a last pair without a second frame), 50 % and 75 % overlap,
    auto and cross spectra; the fp32 kernels against the oracle at 1e-6; the register path must be the one that ran."""
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(W + 1)
    for n, ov in ((4 * W + W // 2 + 77, 50), (3 * W, 50), (2 * W + 999, 75)):
        x = rng.standard_normal((n, 3)) * 0.3
        y = np.stack([np.convolve(x[:, i], rng.standard_normal(6))[:n] for i in range(3)], axis=1) + 0.02 * rng.standard_normal((n, 3))
        ctx.routes()
        for xin in (x[:, :1], x):
            for mode in ("H1", "H3"):
                tf, coh = backend.welch_transfer_function(y, xin, 48000, W, mode, overlap_percent=ov, precision="f32")
                rt, rc = orc.compute_transfer_function(y, xin, 48000, W, mode, overlap_percent=ov)
                paired = xin.shape[1] == 3
                cols = slice(None) if paired else slice(0, 1)  # (one input: channels 1, 2 are almost incoherent with it)
                # few frames on the fp32 kernels: the band tests/sweeps/edge_welch.py documents (tf 4e-6, coh 2e-5)
                assert relmax(tf[:, cols], rt[:, cols], True) < 4 * TOL, (W, n, ov, mode, paired)
                assert relmax(coh[:, cols], rc[:, cols], True) < 20 * TOL, (W, n, ov, mode, paired)
        a = backend._welch(y, None, 48000, Window.Hann, W, ov, True, "mean", SpectrumScaling.PowerSpectralDensity)
        assert relmax(a, orc.welch(y, None, 48000, "hann", W, ov, True, "mean", "PowerSpectralDensity"), True) < TOL
        k = backend._welch(x, y, 48000, Window.Hann, W, ov, False, "mean", SpectrumScaling.FFTBackward)
        assert relmax(k, orc.welch(x, y, 48000, "hann", W, ov, False, "mean", "FFTBackward")) < 2 * TOL
        seen = ctx.routes()
        assert {"welch_long_dif", "welch_long_main", "welch_long_fold"} <= seen and not any(r.startswith("bigfft") for r in seen), seen


def test_chroma_stft_golden():
    """transforms.chroma_stft (STFT, |.|^2 and the pitch-band contraction on the device) against
    the reference's outputs."""
    from dsptoolbox_amd.standard.enums import SpectrumScaling as S
    meta, z = load_golden("chroma")
    for i, c in enumerate(meta["cases"]):
        s = dsp.Signal(None, z["x"].copy(), meta["fs"])
        s.set_spectrogram_parameters(window_length_samples=c["W"], overlap_percent=c["ov"],
                                     padding=c["pad"], scaling=S[c["scaling"]])
        t, chroma, pitch = dsp.transforms.chroma_stft(s, tuning_a_hz=c["tuning"], compression=c["compression"])
        assert np.allclose(t, z[f"t_{i}"])
        assert chroma.shape == z[f"chroma_{i}"].shape and pitch.shape == z[f"pitch_{i}"].shape
        assert relmax(pitch, z[f"pitch_{i}"]) < TOL, (c, relmax(pitch, z[f"pitch_{i}"]))
        assert relmax(chroma, z[f"chroma_{i}"]) < TOL, (c, relmax(chroma, z[f"chroma_{i}"]))
    with pytest.raises(AssertionError):
        dsp.transforms.chroma_stft(s, tuning_a_hz=-1)


def test_fir_streaming_classes_golden():
    """filterbanks.FIRFilterOverlapSave / FIRUniformPartitioned / FIRUniformPartitionedMultichannel
    driven block by block as the reference's tests do (tests/test_classes.py:1527-1580): ALL 15
    golden streams against the reference's own block outputs -- also the three where the reference
    is not the causal convolution (odd fast length with irfft's default length; one delay-line
    index shared by interleaved channels), because the classes run the reference's algorithm on
    device-resident state."""
    from scipy.signal import oaconvolve
    meta, z = load_golden("fir_stream")
    n_ref, n_not_conv = 0, 0
    for i, c in enumerate(meta["cases"]):
        fir, x, bs, C = z[f"fir_{i}"], z[f"x_{i}"], c["blocksize"], c["n_ch"]
        n_blocks = x.shape[0] // bs
        conv0 = np.stack([oaconvolve(x[:, ch], fir[:, 0])[: x.shape[0]] for ch in range(C)], axis=1)
        f1 = dsp.filterbanks.FIRFilterOverlapSave(fir[:, 0].copy())
        f1.prepare(bs, C)
        f2 = dsp.filterbanks.FIRUniformPartitioned.from_filter(dsp.Filter.from_ba(fir[:, 0].copy(), [1.0], 48000))
        f2.prepare(bs, C)
        f3 = dsp.filterbanks.FIRUniformPartitionedMultichannel(fir.copy())
        f3.prepare(bs)
        a1, a2, a3 = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
        for b in range(n_blocks):
            sl = slice(b * bs, (b + 1) * bs)
            for ch in range(C):
                a1[sl, ch] = f1.process_block(x[sl, ch], ch)
                a2[sl, ch] = f2.process_block(x[sl, ch], ch)
            a3[sl] = f3.process_block(x[sl])
        for got, key in ((a1, "ols"), (a2, "upart"), (a3, "multi")):
            ref = z[f"{key}_{i}"]
            assert relmax(got, ref) < TOL, (c, key, relmax(got, ref))
            n_ref += 1
            if key != "multi" and relmax(ref, conv0) > 1e-3:
                n_not_conv += 1  # the reference itself is not the convolution here; we match it anyway
    assert n_ref == 15 and n_not_conv >= 3, (n_ref, n_not_conv)
    # state handling and prepare() bookkeeping
    f1.reset_state()
    assert np.array_equal(f1.process_block(np.zeros(bs), 0), np.zeros(bs))
    f2.reset_state()
    assert np.array_equal(f2.process_block(np.zeros(bs), 0), np.zeros(bs))
    with pytest.raises(NotImplementedError):
        f1.process_sample(0.0, 0)
    with pytest.raises(NotImplementedError):
        f1.set_n_channels(2)
    f = dsp.filterbanks.FIRUniformPartitioned.from_filter(dsp.Filter.from_ba(np.arange(1.0, 1501.0), [1.0], 48000))
    f.prepare(512, 2)
    assert (f.blocksize, f.fft_size, f.n_partitions) == (512, 1024, 3)
    o = dsp.filterbanks.FIRFilterOverlapSave(np.ones(700))
    o.prepare(512, 1)          # next_fast_len(1212) = 1215: odd, the reference's defective case
    assert o.total_length == 1215
    m = dsp.filterbanks.FIRUniformPartitionedMultichannel(np.array([[4.0, 0.0], [2.0, 1.0], [0.0, -1.0]]))
    m.prepare(2)
    assert (m.n_partitions, m.n_channels) == (2, 2)
    with pytest.raises(AssertionError):
        m.process_block(np.zeros((2, 3)))


def test_welch_default_window_kernel_vs_oracle():
    """Welch H1/H2/H3 with windows of 256 / 512 / 1024 samples (1024 = the reference's default) and a
    1-channel input runs on its own kernels (kernels_welch1024.hpp: one team of N/16 lanes per frame
    pair / per chunk and channel).
    Channel counts around the 4-wave workgroup, overlaps 0 / 50 / 75 %, odd frame counts, ragged
    tails, detrend, the three estimators, amplitude and power scalings."""
    rng = np.random.default_rng(99)
    worst = 0.0
    for n_cy, n, ov, det, mode, sc in (
            (1, 40000, 50, True, "H1", SpectrumScaling.FFTBackward),
            (3, 70001, 50, False, "H2", SpectrumScaling.FFTBackward),
            (4, 65536, 75, True, "H3", SpectrumScaling.PowerSpectralDensity),
            (6, 50000, 0, True, "H1", SpectrumScaling.AmplitudeSpectrum),
            (9, 33333, 50, False, "H1", SpectrumScaling.PowerSpectrum),
            (20, 60000, 50, True, "H1", SpectrumScaling.FFTBackward),
            (64, 2**17, 50, True, "H1", SpectrumScaling.FFTBackward),
            (2, 1500, 50, True, "H2", SpectrumScaling.FFTBackward),
            (5, 2100, 50, False, "H1", SpectrumScaling.FFTBackward)):
        x = rng.standard_normal((n, 1)) * 0.4 + 0.1
        h = rng.standard_normal((64, n_cy)) * np.exp(-np.arange(64) / 10.0)[:, None]
        y = np.stack([np.convolve(x[:, 0], h[:, c])[:n] for c in range(n_cy)], axis=1)
        y += 0.05 * rng.standard_normal(y.shape) + 0.02
        for W in (2048, 1024, 512, 256):   # 128 (two waves) / 64 / 32 / 16 lanes per transform
            if n_cy == 64 and W != 1024:
                continue  # the oracle's per-channel frame loops take minutes there
            if W == 2048 and n / (W * (1 - ov / 100)) < 40:
                continue  # fewer than ~40 frames: the fp32 error of single frames is not averaged down
            tf, coh = backend.welch_transfer_function(y, x, 48000, W, mode, overlap_percent=ov,
                                                      detrend=det, scaling=sc)
            rt, rc = orc.compute_transfer_function(y, x, 48000, W, mode, overlap_percent=ov, detrend=det,
                                                   scaling=sc.name)
            sl = slice(1, None) if det else slice(None)  # detrended DC is 0/0 on both sides
            e = max(relmax(tf[sl], rt[sl]), relmax(coh[sl], rc[sl]))
            worst = max(worst, e)
            assert e < TOL, (W, n_cy, n, ov, det, mode, sc, e)
    # auto spectra (Signal.get_spectrum's default parameters) on the same kernels
    for n_ch, n, ov, det, sc in ((1, 30000, 50, True, SpectrumScaling.FFTBackward),
                                 (3, 44100, 75, False, SpectrumScaling.PowerSpectralDensity),
                                 (7, 20000, 0, True, SpectrumScaling.AmplitudeSpectralDensity),
                                 (64, 2**16, 50, True, SpectrumScaling.PowerSpectrum)):
        x = rng.standard_normal((n, n_ch)) * (0.1 + 0.05 * np.arange(n_ch)) + 0.03
        for W in (8192, 4096, 2048, 1024, 512, 256):   # 8192 / 4096: the AUTO variants of those kernels
            if n_ch == 64 and W not in (1024, 4096):
                continue
            psd = backend._welch(x, None, 48000, Window.Hann, W, ov, det, "mean", sc)
            ref = orc.welch(x, None, 48000, "hann", W, ov, det, "mean", sc.name)
            e = relmax(psd, ref, det)
            worst = max(worst, e)
            assert psd.shape == ref.shape and e < TOL, (W, n_ch, n, ov, det, sc, e)
    print("welch 1024-window kernel worst rel-max", worst)


def test_deconvolve_non_fast_lengths_golden():
    """spectral_deconvolve when the signal length is not a fast FFT length (found by
    tests/sweeps/fuzz_misc.py): the reference's irfft(n=N) of a next_fast_len(N)-point spectrum crops the
    spectrum; the device path reproduces that (forward spectrum, cropped product, N-point inverse)."""
    meta, z = load_golden("deconv_nonfast")
    for i, c in enumerate(meta["cases"]):
        ir = dsp.transfer_functions.spectral_deconvolve(
            dsp.Signal(None, z[f"y_{i}"].copy(), meta["fs"]), dsp.Signal(None, z[f"x_{i}"].copy(), meta["fs"]),
            apply_regularization=c["regularized"], padding=c["padding"],
            keep_original_length=c["keep_original_length"])
        assert ir.time_data.shape == z[f"ir_{i}"].shape
        lim = TOL if c["regularized"] else 20 * TOL  # plain Y/X: white-noise |X| dips to ~1e-2 of its mean
        assert relmax(ir.time_data, z[f"ir_{i}"]) < lim, (c, relmax(ir.time_data, z[f"ir_{i}"]))


def test_fused_float64_upload_is_the_same_computation():
    """welch_transfer_function hands large float64 C-order arrays to ds_welch_tf_f64 (threaded cast
    + transpose into pinned chunks, asynchronous 2-D copies); the result must be bit-identical to
    the planar-float32 entry point, for one chunk and for several (32 MB chunks)."""
    rng = np.random.default_rng(321)
    for n, c in ((300001, 5), (2**20, 40)):
        x = rng.standard_normal((n, 1)) * 0.3
        y = rng.standard_normal((n, c)) * 0.2 + 0.5 * x
        tf_a, coh_a = backend.welch_transfer_function(y, x, 48000, 4096, "H1")            # fused path
        yf = np.asfortranarray(y)                                                          # not C-order:
        tf_b, coh_b = backend.welch_transfer_function(yf, x, 48000, 4096, "H1")           # numpy + ds_welch_tf
        # (bin 0 is 0/0 = NaN on both sides with detrend)
        assert np.array_equal(tf_a, tf_b, equal_nan=True) and np.array_equal(coh_a, coh_b, equal_nan=True), (n, c)
        psd_a = backend._welch(y, None, 48000, Window.Hann, 1024, 50, True, "mean", SpectrumScaling.FFTBackward)
        psd_b = backend._welch(yf, None, 48000, Window.Hann, 1024, 50, True, "mean", SpectrumScaling.FFTBackward)
        assert np.array_equal(psd_a, psd_b, equal_nan=True), (n, c)
        # cross spectra of two such arrays: ds_welch_csd_f64 (round 5) against numpy's cast + ds_welch_csd
        from dsptoolbox_amd._lib import get_context
        y2 = np.ascontiguousarray(y[:, ::-1]) + 0.1 * x
        get_context().routes()
        csd_a = backend._welch(y, y2, 48000, Window.Hann, 1024, 50, True, "mean", SpectrumScaling.PowerSpectralDensity)
        csd_b = backend._welch(yf, np.asfortranarray(y2), 48000, Window.Hann, 1024, 50, True, "mean", SpectrumScaling.PowerSpectralDensity)
        assert csd_a.dtype == np.complex128 and np.array_equal(csd_a, csd_b, equal_nan=True), (n, c)
        if c <= 8:
            rk = orc.welch(y, y2, 48000, "hann", 1024, 50, True, "mean", "PowerSpectralDensity")
            assert relmax(csd_a[1:], rk[1:]) < TOL
            for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.AmplitudeSpectrum, SpectrumScaling.PowerSpectrum):
                t_a, f_a, st_a = backend._stft(y, 48000, 1024, Window.Hann, 50, None, False, True, sc)
                t_b, f_b, st_b = backend._stft(yf, 48000, 1024, Window.Hann, 50, None, False, True, sc)
                assert st_a.dtype == st_b.dtype and np.array_equal(st_a, st_b), (n, c, sc)
            taps = [rng.standard_normal(301) * 0.05, rng.standard_normal(301) * 0.05]
            for mode in (backend.DS_FB_PARALLEL, backend.DS_FB_SUMMED, backend.DS_FB_SEQUENTIAL):
                fa = backend.fir_filter_bank(y, taps, mode)
                fb = backend.fir_filter_bank(yf, taps, mode)
                assert fa.shape == fb.shape and fa.dtype == np.float64 and np.array_equal(fa, fb), (n, c, mode)
            _, csm_a = backend._csm_welch(y, 48000, 1024, Window.Hann, 50, True, "mean", SpectrumScaling.FFTBackward)
            _, csm_b = backend._csm_welch(yf, 48000, 1024, Window.Hann, 50, True, "mean", SpectrumScaling.FFTBackward)
            assert np.array_equal(csm_a, csm_b, equal_nan=True), (n, c)


def test_welch_8192_window_kernel_vs_oracle():
    """Welch H1/H2/H3 with an 8192-sample window (kernels_welch8192.hpp: two 4096-point register
    transforms per frame pair, radix-2 decimation in frequency in front): overlaps 0 / 50 / 75 %,
    odd frame counts, ragged tails, detrend, estimators, scalings."""
    rng = np.random.default_rng(8192)
    worst = 0.0
    for n_cy, n, ov, det, mode, sc in (
            (3, 400000, 50, True, "H1", SpectrumScaling.FFTBackward),
            (5, 300001, 75, False, "H2", SpectrumScaling.PowerSpectralDensity),
            (2, 500000, 0, True, "H3", SpectrumScaling.AmplitudeSpectrum),
            (64, 2**19, 50, True, "H1", SpectrumScaling.FFTBackward)):
        x = rng.standard_normal((n, 1)) * 0.4 + 0.1
        h = rng.standard_normal((64, n_cy)) * np.exp(-np.arange(64) / 10.0)[:, None]
        y = np.stack([np.convolve(x[:, 0], h[:, c])[:n] for c in range(n_cy)], axis=1)
        y += 0.05 * rng.standard_normal(y.shape) + 0.02
        tf, coh = backend.welch_transfer_function(y, x, 48000, 8192, mode, overlap_percent=ov, detrend=det,
                                                  scaling=sc)
        rt, rc = orc.compute_transfer_function_batched(y, x, 48000, 8192, mode, overlap_percent=ov,
                                                       detrend=det, scaling=sc.name)
        sl = slice(1, None) if det else slice(None)
        e = max(relmax(tf[sl], rt[sl]), relmax(coh[sl], rc[sl]))
        worst = max(worst, e)
        assert e < TOL, (n_cy, n, ov, det, mode, sc, e)
    print("welch 8192-window kernel worst rel-max", worst)


def test_register_kernels_tiny_and_ragged_signals():
    """Signals shorter than one window, exactly one / two windows, one sample more: single frames,
    frame pairs without a second frame, frames that are mostly zero padding -- on every window length
    that has a register-resident kernel (auto spectra, H1 and the STFT)."""
    rng = np.random.default_rng(123)
    for W in (256, 512, 1024, 2048, 4096, 8192):
        for n in (W // 4, W, W + 1, 3 * W // 2, 2 * W, 5 * W + 17):
            x = rng.standard_normal((n, 3)) * 0.3 + 0.1
            psd = backend._welch(x, None, 48000, Window.Hann, W, 50, False, "mean", SpectrumScaling.PowerSpectralDensity)
            ref = orc.welch(x, None, 48000, "hann", W, 50, False, "mean", "PowerSpectralDensity")
            assert psd.shape == ref.shape and relmax(psd, ref) < TOL, (W, n, relmax(psd, ref))
            tf, coh = backend.welch_transfer_function(x[:, 1:], x[:, :1], 48000, W, "H1", detrend=False)
            rt, rc = orc.compute_transfer_function(x[:, 1:], x[:, :1], 48000, W, "H1", detrend=False)
            # one or two frames: H1 is a ratio of nearly identical numbers; the coherence is 1 +- rounding
            assert tf.shape == rt.shape and np.all(np.isfinite(tf)) and orc.rel_l2(tf, rt) < 20 * TOL, (W, n)
            assert np.max(np.abs(coh - rc)) < 2e-5, (W, n, np.max(np.abs(coh - rc)))
            if W <= 1024:
                for pad in (True, False):
                    t, f, st = backend._stft(x, 48000, W, Window.Hann, 50, None, False, pad, SpectrumScaling.FFTBackward)
                    rt_, rf_, rs = orc.stft(x, 48000, W, "hann", 50, None, False, pad, "FFTBackward")
                    assert st.shape == rs.shape and relmax(st, rs) < TOL, (W, n, pad)


def test_stft_default_frame_kernel_vs_oracle():
    """Frames of 256 ... 2048 points have their own kernel (kernels_stft1024.hpp: one frame pair
    per team of nfft/16 lanes, the transform in registers), frames of 4096 points theirs (kernels_stft4096.hpp: four
    teams of two neighbouring channels per workgroup): channel tiles with idle teams (1, 3, 5, 9, 17 channels), odd and
    even channel and frame counts, padding at both ends, detrend, amplitude and power scalings, overlaps."""
    rng = np.random.default_rng(77)
    worst = 0.0
    for n_ch, n, ov, pad, det, sc in (
            (1, 5000, 50, True, False, SpectrumScaling.FFTBackward),
            (3, 20011, 50, True, True, SpectrumScaling.AmplitudeSpectrum),
            (5, 16384, 75, False, False, SpectrumScaling.PowerSpectralDensity),
            (8, 9999, 0, True, True, SpectrumScaling.PowerSpectrum),
            (9, 30000, 50, False, True, SpectrumScaling.FFTForward),
            (17, 12345, 25, True, False, SpectrumScaling.AmplitudeSpectralDensity),
            (2, 1024, 50, True, False, SpectrumScaling.FFTOrthogonal),
            (64, 8192, 50, True, False, SpectrumScaling.FFTBackward)):
        x = rng.standard_normal((n, n_ch)) * 0.3 + 0.05
        for W in (4096, 2048, 1024, 512, 256, 128, 64, 32):   # 256 threads; 128 (two waves), 64, 32, 16 lanes per transform;
            # 128 / 64 / 32 samples: every 2nd / 4th / 8th bin of the 256-point transform of the zero-padded frame
            t, f, st = backend._stft(x, 48000, W, Window.Hann, ov, None, det, pad, sc)
            rt, rf, rs = orc.stft(x, 48000, W, "hann", ov, None, det, pad, sc.name)
            assert st.shape == rs.shape and np.allclose(t, rt) and np.array_equal(f, rf)
            if det:  # the reference's DC bin after mean removal is rounding noise around 0
                assert np.max(np.abs(st[0])) <= 1e-6 * np.max(np.abs(rs))
            e = relmax(st, rs)
            worst = max(worst, e)
            assert e < TOL, (W, n_ch, n, ov, pad, det, sc, e)
    # shorter windows zero-padded to 1024 points (no detrend: that case stays on the generic kernel)
    for W, nfft, det in ((512, 1024, False), (256, 1024, False), (512, 1024, True), (128, 256, False),
                         (256, 512, False), (128, 512, True), (2048, 4096, False), (512, 4096, False), (1024, 4096, True), (64, 128, False), (16, 64, False), (32, 128, True)):
        x = rng.standard_normal((20000, 3)) * 0.3 + 0.05
        t, f, st = backend._stft(x, 48000, W, Window.Hann, 50, nfft, det, True, SpectrumScaling.FFTBackward)
        rt, rf, rs = orc.stft(x, 48000, W, "hann", 50, nfft, det, True, "FFTBackward")
        assert st.shape == rs.shape
        e = relmax(st, rs)
        worst = max(worst, e)
        assert e < TOL, (W, det, e)
    print("stft 1024-frame kernel worst rel-max", worst)


@pytest.mark.parametrize("n_ch", [2, 5, 20])
def test_istft_channel_tiles_and_fused_overlap_add_vs_oracle(n_ch):
    """The inverse STFT reads ct neighbouring channels per workgroup (k_istft_ct) and, for full-length frames at 50 %
    overlap, adds the overlapping halves in registers and writes finished samples (k_istft_fused): random spectrograms
    (not the transform of any signal: every frame half matters), odd and even frame counts, with and without the
    reference's padding (frame offset 0 / 1 and the empty frame slots at both ends), channel tiles with idle teams,
    several workgroups per channel tile; other overlaps and shorter windows take the two-kernel path."""
    rng = np.random.default_rng(100 + n_ch)
    worst = 0.0
    for W, nfft, ov, pad, n_frames in ((256, None, 50, True, 37), (256, None, 50, False, 300), (1024, None, 50, False, 41),
                                        (1024, None, 50, True, 200), (4096, None, 50, True, 9), (2048, None, 50, False, 130),
                                        (1024, None, 75, True, 40), (512, 1024, 50, False, 30), (1024, None, 25, False, 33)):
        nb = (nfft or W) // 2 + 1
        sp = rng.standard_normal((nb, n_frames, n_ch)) + 1j * rng.standard_normal((nb, n_frames, n_ch))
        sp[0].imag = 0
        sp[-1].imag = 0
        got = dsp.transforms.istft(sp, sampling_rate_hz=48000, window_length_samples=W, window_type=Window.Hann,
                                   overlap_percent=ov, fft_length_samples=nfft, padding=pad,
                                   scaling=SpectrumScaling.FFTBackward)
        ref = orc.istft(sp, 48000, W, "hann", ov, nfft, pad, "FFTBackward")
        assert got.time_data.shape == ref.shape, (W, nfft, ov, pad, got.time_data.shape, ref.shape)
        e = relmax(got.time_data, ref)
        worst = max(worst, e)
        assert e < TOL, (W, nfft, ov, pad, n_frames, e)
    print("istft worst rel-max", worst)


@pytest.mark.parametrize("n_ch", [1, 2, 5, 20])
def test_istft_long_frames_on_the_register_transform(n_ch):
    """Inverse STFT with frames of 8192 ... 262144 points (kernels_istft_long.hpp): class transforms on the 4096-point
    register kernel + the radix-R stage, overlap-add fused for full-length frames at 50 % overlap (R <= 16), windowed
    frames + k_istft_ola otherwise.  Random spectrograms (every frame half matters), odd / even frame counts, with and
    without the reference's padding, odd channel counts (a last pair with one channel, narrow loads), idle teams, shorter
    windows under a longer transform, other overlaps; routes asserted."""
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(8192 + n_ch)
    worst = 0.0
    for W, nfft, ov, pad, n_frames, fused in (
            (8192, None, 50, True, 9, True), (8192, None, 50, False, 30, True), (16384, None, 50, False, 7, True),
            (16384, None, 50, True, 12, True), (32768, None, 50, True, 5, True), (65536, None, 50, False, 4, True),
            (8192, None, 75, True, 10, False), (16384, None, 25, False, 6, False), (4096, 8192, 50, False, 11, False),
            (8192, 32768, 50, True, 6, False), (65536, 131072, 50, False, 3, False), (65536, 262144, 50, True, 2, False),
            (32768, None, 0, False, 3, False), (8192, None, 50, False, 1, True)):
        nb = (nfft or W) // 2 + 1
        sp = rng.standard_normal((nb, n_frames, n_ch)) + 1j * rng.standard_normal((nb, n_frames, n_ch))
        sp[0].imag = 0
        sp[-1].imag = 0
        ctx.routes()
        got = dsp.transforms.istft(sp, sampling_rate_hz=48000, window_length_samples=W, window_type=Window.Hann,
                                   overlap_percent=ov, fft_length_samples=nfft, padding=pad,
                                   scaling=SpectrumScaling.FFTBackward)
        seen = ctx.routes()
        assert "istft_long_cls" in seen and (("istft@long_ola" in seen) == fused) and (("istft@long" in seen) != fused), (W, nfft, ov, seen)
        ref = orc.istft(sp, 48000, W, "hann", ov, nfft, pad, "FFTBackward")
        assert got.time_data.shape == ref.shape, (W, nfft, ov, pad, got.time_data.shape, ref.shape)
        e = relmax(got.time_data, ref)
        worst = max(worst, e)
        assert e < TOL, (W, nfft, ov, pad, n_frames, e)
    print("istft long frames worst rel-max", worst)


def test_stft_8192_and_16384_frame_kernels_vs_oracle():
    """Frames of 8192 / 16384 points (kernels_stft4096.hpp, k_stft_long): two / four decimated 4096-point transforms per
    channel pair, combined at the read-out; two teams (4 channels) / one team (2 channels) per workgroup.  Odd and
    even channel counts (narrow and wide stores, idle teams), one frame and many, padding, detrend (bin 0),
    amplitude / power scalings, zero-padded shorter windows (with detrend: the generic kernel)."""
    rng = np.random.default_rng(8192)
    worst = 0.0
    for n_ch, n, ov, pad, det, sc in (
            (1, 9000, 50, True, False, SpectrumScaling.FFTBackward),
            (3, 70011, 50, True, True, SpectrumScaling.AmplitudeSpectrum),
            (4, 40000, 75, False, False, SpectrumScaling.PowerSpectralDensity),
            (5, 50000, 0, True, True, SpectrumScaling.PowerSpectrum),
            (18, 33000, 25, False, False, SpectrumScaling.FFTOrthogonal),
            (64, 20000, 50, True, False, SpectrumScaling.FFTBackward)):
        x = rng.standard_normal((n, n_ch)) * 0.3 + 0.05
        for W in (8192, 16384):
            t, f, st = backend._stft(x, 48000, W, Window.Hann, ov, None, det, pad, sc)
            rt, rf, rs = orc.stft(x, 48000, W, "hann", ov, None, det, pad, sc.name)
            assert st.shape == rs.shape and np.allclose(t, rt) and np.array_equal(f, rf)
            if det:  # the reference's DC bin after mean removal is rounding noise around 0
                assert np.max(np.abs(st[0])) <= 1e-6 * np.max(np.abs(rs))
            e = relmax(st, rs)
            worst = max(worst, e)
            assert e < TOL, (W, n_ch, n, ov, pad, det, sc, e)
    for W, nfft, det in ((4096, 8192, False), (1024, 8192, False), (2048, 16384, False), (8192, 16384, False),
                         (4096, 8192, True), (8192, 16384, True)):
        x = rng.standard_normal((60000, 3)) * 0.3 + 0.05
        t, f, st = backend._stft(x, 48000, W, Window.Hann, 50, nfft, det, True, SpectrumScaling.FFTBackward)
        rt, rf, rs = orc.stft(x, 48000, W, "hann", 50, nfft, det, True, "FFTBackward")
        assert st.shape == rs.shape
        e = relmax(st, rs)
        worst = max(worst, e)
        assert e < TOL, (W, nfft, det, e)
    print("stft 8192 / 16384 frame kernels worst rel-max", worst)


def test_stft_long_frames_on_the_register_transform():
    """Frames of 2^15 ... 2^18 points (kernels_stft_long.hpp): one decimation-in-frequency pass per frame and channel
    pair, then the 4096-point register transform per class, mirror classes r / R - r read out together.  Odd and even
    channel counts (narrow / wide stores, idle teams, a last pair with one channel), one frame and several, padding,
    detrend (bin 0), amplitude / power scalings, shorter windows zero-padded to the transform; the routes are asserted."""
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(32768)
    worst = 0.0
    for n_ch, n, W, ov, pad, det, sc in (
            (1, 40000, 2**15, 50, True, False, SpectrumScaling.FFTBackward),
            (3, 150011, 2**15, 50, True, True, SpectrumScaling.AmplitudeSpectrum),
            (4, 200000, 2**16, 75, False, False, SpectrumScaling.PowerSpectralDensity),
            (5, 300000, 2**16, 0, True, True, SpectrumScaling.PowerSpectrum),
            (18, 140000, 2**15, 25, False, False, SpectrumScaling.FFTOrthogonal),
            (20, 100000, 2**15, 50, True, False, SpectrumScaling.FFTBackward)):
        x = rng.standard_normal((n, n_ch)) * 0.3 + 0.05
        ctx.routes()
        t, f, st = backend._stft(x, 48000, W, Window.Hann, ov, None, det, pad, sc)
        assert {"stft_long_dif", "stft@long"} <= ctx.routes()
        rt, rf, rs = orc.stft(x, 48000, W, "hann", ov, None, det, pad, sc.name)
        assert st.shape == rs.shape and np.allclose(t, rt) and np.array_equal(f, rf)
        if det:
            assert np.max(np.abs(st[0])) <= 1e-6 * np.max(np.abs(rs))
        e = relmax(st, rs)
        worst = max(worst, e)
        assert e < TOL, (W, n_ch, n, ov, pad, det, sc, e)
    # (the reference's window stops at 2^16 samples, its transform length does not)
    for W, nfft, det, route in ((8192, 2**15, False, True), (2**15, 2**16, False, True), (4096, 2**15, True, False),
                                (2**16, 2**17, False, True), (2**16, 2**18, False, True)):
        x = rng.standard_normal((150000 if nfft < 2**17 else 300000, 3)) * 0.3 + 0.05
        ctx.routes()
        t, f, st = backend._stft(x, 48000, W, Window.Hann, 50, nfft, det, True, SpectrumScaling.FFTBackward)
        assert ("stft@long" in ctx.routes()) == route  # (detrend of a zero-padded frame: the four-step path)
        rt, rf, rs = orc.stft(x, 48000, W, "hann", 50, nfft, det, True, "FFTBackward")
        assert st.shape == rs.shape
        e = relmax(st, rs)
        worst = max(worst, e)
        assert e < TOL, (W, nfft, det, e)
    print("stft long frames worst rel-max", worst)


def test_stft_and_csm_long_windows_vs_oracle():
    rng = np.random.default_rng(5)
    n = 200000
    x = rng.standard_normal((n, 3)) * 0.3 + 0.1
    for W, nfft, pad, det, sc in ((2**15, None, True, True, SpectrumScaling.FFTBackward),
                                  (2**16, None, False, False, SpectrumScaling.AmplitudeSpectrum),
                                  (2**13, 2**15, True, True, SpectrumScaling.PowerSpectralDensity)):
        t, f, st = backend._stft(x, 48000, W, Window.Hann, 50, nfft, det, pad, sc)
        rt, rf, rs = orc.stft(x, 48000, W, "hann", 50, nfft, det, pad, sc.name)
        assert st.shape == rs.shape and np.allclose(t, rt) and np.allclose(f, rf)
        assert relmax(st, rs) < TOL, (W, nfft)
    f, csm = backend._csm_welch(x, 48000, 2**15, Window.Hann, 50, True, "mean", SpectrumScaling.FFTBackward)
    rf, rcsm = orc.csm_welch(x, 48000, 2**15, "hann", 50, True, "mean", "FFTBackward")
    assert relmax(csm, rcsm) < TOL


def test_headline_shape_reduced_vs_oracle():
    """config 2 at reduced channel count / length: 1-channel sweep input, H1, nfft 4096.
    128 frames: a sweep puts each frame's energy into a few bins, so the fp32 FFT error
    floor (1e-7 of the frame peak) is what every other bin sees; it averages down with the
    frame count (coherence error 1.0e-6 at 32 frames, 2.9e-7 at the full 512)."""
    from dsptoolbox_amd.generators import sweep_and_responses
    x, y = sweep_and_responses(n_samples=2**18, n_channels=6, fs_hz=48000)
    for mode in ("H1", "H2", "H3"):
        for det in (True, False):
            tf, coh = backend.welch_transfer_function(y, x, 48000, 4096, mode, detrend=det)
            rt, rc = orc.compute_transfer_function(y, x, 48000, 4096, mode, detrend=det)
            m = inband(4096)
            assert relmax(tf[m], rt[m]) < TOL, (mode, det, relmax(tf[m], rt[m]))
            assert relmax(coh[m], rc[m]) < TOL, (mode, det, relmax(coh[m], rc[m]))


def test_headline_full_size_properties():
    """config 2 at full size (64 ch x 2^20): size-independent checks -- channel
    permutation invariance, linearity in the output gain, coherence in [0, 1]."""
    from dsptoolbox_amd.generators import sweep_and_responses
    x, y = sweep_and_responses(n_samples=2**20, n_channels=64, fs_hz=48000)
    kw = dict(scaling=SpectrumScaling.PowerSpectralDensity, detrend=False)
    tf, coh = backend.welch_transfer_function(y, x, 48000, 4096, "H1", **kw)
    assert tf.shape == (2049, 64) and coh.shape == (2049, 64)
    assert np.all(np.isfinite(tf)) and np.all(coh <= 1 + 1e-5) and np.all(coh >= 0)
    m = inband(4096)
    perm = np.random.default_rng(0).permutation(64)
    tf2, coh2 = backend.welch_transfer_function(3.0 * y[:, perm], x, 48000, 4096, "H1", **kw)
    # two fp32 runs on differently rounded inputs: each within TOL of the float64 truth
    assert relmax(tf2[m], 3.0 * tf[m][:, perm]) < 2 * TOL
    assert relmax(coh2[m], coh[m][:, perm]) < 2 * TOL
    # a subset of channels against the oracle (oracle cost: seconds)
    rt, rc = orc.compute_transfer_function_batched(y[:, :3], x, 48000, 4096, "H1",
                                                   scaling="PowerSpectralDensity", detrend=False)
    assert relmax(tf[m, :3], rt[m]) < TOL
    assert relmax(coh[m, :3], rc[m]) < TOL


@pytest.mark.parametrize("n_ch", [64, 40, 33, 70])
def test_csm_64ch_vs_oracle(n_ch):
    """64 / 40 / 33 channels: one workgroup per bin (bf16-triple kernel, partly filled second tile, odd
    count); 70 channels: two groups of channels (diagonal blocks + one off-diagonal block)."""
    rng = np.random.default_rng(4)
    n = 40000
    x = 0.1 * rng.standard_normal((n, n_ch)) + 0.2 * rng.standard_normal(n)[:, None]
    f, csm = backend._csm_welch(x, 48000, 1024, Window.Hann, 50, True, "mean",
                                SpectrumScaling.FFTBackward)
    fr, ref = orc.csm_welch_batched(x, 48000, 1024, "hann", 50, True, "FFTBackward")
    assert relmax(csm, ref, True) < TOL


@pytest.mark.parametrize("n_ch", [96, 129, 193])
def test_csm_channel_groups_vs_oracle(n_ch):
    """More than 64 channels: groups of 64 (k_csm_group_b3 for the diagonal blocks, k_csm_offdiag_b3 for the
    blocks below it): 2 groups with a half-filled second one, 3 groups with a single channel in the last,
    4 groups with an odd one; coherent sources of either sign, amplitude and power scalings, a bin range."""
    rng = np.random.default_rng(n_ch)
    n, W = 6000, 128
    src = rng.standard_normal((n, 6)) * 0.3 + 0.02
    x = src @ rng.standard_normal((6, n_ch)) + 0.1 * rng.standard_normal((n, n_ch))
    for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.PowerSpectralDensity):
        f, csm = backend._csm_welch(x, 48000, W, Window.Hann, 50, False, "mean", sc)
        fr, ref = orc.csm_welch_batched(x, 48000, W, "hann", 50, False, sc.name)
        assert csm.shape == ref.shape == (W // 2 + 1, n_ch, n_ch)
        # amplitude scaling: the square root amplifies the fp32 error of the many near-zero elements of
        # this rank-6 data (limit (ix): 1.1e-6 at 193 channels); the power scaling has no such step
        lim = TOL if sc == SpectrumScaling.PowerSpectralDensity else 2 * TOL
        assert relmax(csm, ref) < lim, (n_ch, sc, relmax(csm, ref))
        part = backend._csm_welch_bins(x, 48000, W, Window.Hann, 50, False, sc, 3, 41)
        assert relmax(part, ref[3:41]) < lim


@pytest.mark.parametrize("n_ch", [33, 63, 129])
@pytest.mark.parametrize("n_frames", [17, 24, 25])
def test_csm_odd_channels_energy_in_the_last_frames_last_channel(n_ch, n_frames):
    """Odd channel counts on the bf16-triple kernels read frames with 16-byte buffer loads whose second half
    belongs to the next frame's channel 0; the very last one straddles the end of the buffer, and the kernel
    relies on the per-dword range check keeping the in-range half (kernels_csm_b3.hpp, load of the operand
    tiles).  All the energy sits in the last channel of the last frame: a load dropped as a whole would lose it,
    a stray operand would show up in a row that must stay zero.  Frame counts with F % 16 in {1, 8, 9}."""
    W, hop = 128, 64
    n = (n_frames - 2) * hop + W  # the framing appends one zero-padded frame: n_frames frames in all
    rng = np.random.default_rng(n_ch * 100 + n_frames)
    x = np.zeros((n, n_ch))
    x[-hop:, -1] = rng.standard_normal(hop)  # these samples are seen by the last frame alone
    assert orc.get_framed_signal(x, W, hop).shape[1] == n_frames
    f, csm = backend._csm_welch(x, 48000, W, Window.Hann, 50, False, "mean", SpectrumScaling.FFTBackward)
    fr, ref = orc.csm_welch_batched(x, 48000, W, "hann", 50, False, "FFTBackward")
    assert csm.shape == ref.shape
    assert np.abs(ref[:, -1, -1]).max() > 0
    assert relmax(csm, ref) < TOL
    others = csm.copy()
    others[:, -1, -1] = 0
    assert not others.any()
    # and with every channel alive, so that a lost half of ANY straddling load would show
    x = 0.1 * rng.standard_normal((n, n_ch))
    x[-hop:, -1] += rng.standard_normal(hop)
    f, csm = backend._csm_welch(x, 48000, W, Window.Hann, 50, False, "mean", SpectrumScaling.PowerSpectralDensity)
    fr, ref = orc.csm_welch_batched(x, 48000, W, "hann", 50, False, "PowerSpectralDensity")
    assert relmax(csm, ref) < TOL


def test_deconvolve_batch_8192():
    """config 5 shape: stereo responses against one shared sweep, n = 8192."""
    from dsptoolbox_amd.generators import exponential_sweep
    rng = np.random.default_rng(7)
    n = 8192
    x = exponential_sweep(n, 48000)[:, None]
    items = []
    for i in range(6):
        h = rng.standard_normal((2, 64)) * np.exp(-np.arange(64) / 10.0)
        items.append(np.stack([np.convolve(x[:, 0], h[c])[:n] for c in range(2)], axis=1)
                     + 1e-3 * rng.standard_normal((n, 2)))
    inp = dsp.Signal(None, x, 48000)
    for y in items[:2]:
        ir = dsp.transfer_functions.spectral_deconvolve(dsp.Signal(None, y, 48000), inp)
        assert relmax(ir.time_data, orc.spectral_deconvolve(y, x, 48000)) < TOL
    # batched entry point: all items in one call
    den = backend.rfft_spectrum(x, n)
    eps, _ = orc.regularization_eps(den[:, 0], np.fft.rfftfreq(n, 1 / 48000), 48000, None, -30.0)
    inv = backend.regularized_inverse(den, eps)[:, 0]
    out = backend.spectral_division(np.stack(items), n, inv, n)
    for y, o in zip(items, out):
        assert relmax(o, orc.spectral_deconvolve(y, x, 48000)) < TOL


def test_fir_bank_4097_taps():
    """config 3 at reduced length: 4097-tap linear-phase band filters, parallel + summed."""
    from dsptoolbox_amd.generators import fir_bank_taps
    rng = np.random.default_rng(3)
    x = rng.standard_normal((60000, 3)) * 0.1
    taps = fir_bank_taps(4, 4097, 48000)
    y = backend.fir_filter_bank(x, list(taps), backend.DS_FB_PARALLEL)
    ref = orc.filterbank_fir(list(taps), x, "Parallel")  # (N, C, K)
    assert relmax(np.transpose(y, (1, 2, 0)), ref) < TOL
    ys = backend.fir_filter_bank(x, list(taps), backend.DS_FB_SUMMED)
    assert relmax(ys, orc.filterbank_fir(list(taps), x, "Summed")) < TOL
    yq = backend.fir_filter_bank(x, list(taps[:2]), backend.DS_FB_SEQUENTIAL)
    assert relmax(yq, orc.filterbank_fir(list(taps[:2]), x, "Sequential")) < TOL


def test_fir_bank_full_size_properties():
    """config 3 at full size (32 x 4097 taps, 8 x 2^22 samples, 4.3 GB of output kept on the
    device): an impulse train must come out as shifted copies of the taps, wherever the impulses
    fall relative to the 12288-sample block grid; a second run on 2x + the train checks linearity
    on noise at sampled windows."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, get_context
    from dsptoolbox_amd.generators import fir_bank_taps
    ctx = get_context()
    n, n_ch, K, T = 2**22, 8, 32, 4097
    taps = fir_bank_taps(K, T, 48000).astype(np.float32)
    x = np.zeros((n_ch, n), dtype=np.float32)
    pos = {c: np.arange(5000 + 977 * c, n - T, 100003 + 131 * c) for c in range(n_ch)}
    for c in range(n_ch):
        x[c, pos[c]] = 1.0 + 0.25 * c
    d_x = DeviceBuffer.from_array(ctx, x)
    d_t = DeviceBuffer.from_array(ctx, taps)
    d_y = DeviceBuffer(ctx, K * n_ch * n * 4)

    def run():
        ctx.check(ctx.lib.ds_fir_ola_dev(ctx.handle, C.c_void_p(d_x.ptr), n_ch, n, n, C.c_void_p(d_t.ptr), K, T,
                                         backend.DS_FB_PARALLEL, C.c_void_p(d_y.ptr), n), "ds_fir_ola_dev")
        ctx.sync()

    def window(k, c, start, length):
        out = np.empty(length, dtype=np.float32)
        ctx.download(d_y.ptr + 4 * ((k * n_ch + c) * n + start), out)
        return out

    run()
    rng = np.random.default_rng(0)
    worst = 0.0
    for k in (0, 7, 19, 31):
        for c in (0, 3, 7):
            for p0 in rng.choice(pos[c], 5, replace=False):
                got = window(k, c, int(p0), T).astype(np.float64)
                ref = taps[k].astype(np.float64) * (1.0 + 0.25 * c)
                worst = max(worst, np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
            # between impulses (spacing > taps) the output is silent
            gap = window(k, c, int(pos[c][3]) + T + 10, 20000)
            assert np.max(np.abs(gap)) < 1e-6 * np.max(np.abs(taps[k]))
    assert worst < TOL, worst
    # linearity on noise: y(2 a + train) = 2 y(a) + y(train) at sampled windows
    a = (rng.standard_normal((n_ch, n)) * 0.1).astype(np.float32)
    train = [window(5, 2, 12288 * j - 100, 4000) for j in (1, 57, 300)]
    ctx.upload(d_x.ptr, a)
    run()
    ya = [window(5, 2, 12288 * j - 100, 4000) for j in (1, 57, 300)]
    ctx.upload(d_x.ptr, (2.0 * a + x).astype(np.float32))
    run()
    for j, t0, y0 in zip((1, 57, 300), train, ya):
        yc = window(5, 2, 12288 * j - 100, 4000)
        scale = max(np.max(np.abs(y0)), 1e-30)
        assert np.max(np.abs(yc - (2.0 * y0 + t0))) / scale < 4 * TOL
    for d in (d_x, d_t, d_y):
        d.free()


@pytest.mark.parametrize("n_ch", [4, 8, 16, 33, 64])
def test_csm_negative_real_elements_at_the_real_bins(n_ch):
    """Coherent channels with responses of either sign: at DC and Nyquist the cross spectra are real
    and some are NEGATIVE, where the amplitude scalings take the square root on the branch cut -- the
    lower element gets +i sqrt|x| (imaginary part +0), its mirror the conjugate.  (Found by
    tests/sweeps/fuzz_parity.py after the interleaved-tile kernel negated a +0.)"""
    rng = np.random.default_rng(3)
    n, W = 7665, 256
    x = rng.standard_normal((n, 1)) * 0.3 + 0.05
    h = rng.standard_normal((32, n_ch)) * np.exp(-np.arange(32) / 6.0)[:, None]
    y = np.stack([np.convolve(x[:, 0], h[:, c])[:n] for c in range(n_ch)], axis=1) + 0.05 * rng.standard_normal((n, n_ch))
    for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.AmplitudeSpectrum, SpectrumScaling.PowerSpectralDensity):
        f, c = backend._csm_welch(y, 48000, W, Window.Hann, 50.0, False, "mean", sc)
        rf, r = orc.csm_welch_batched(y, 48000, W, "hann", 50.0, False, sc.name)
        if sc != SpectrumScaling.PowerSpectralDensity:  # the case is there: purely imaginary roots at DC
            assert np.any((r[0].real == 0) & (r[0].imag != 0))
        assert relmax(c, r) < TOL, (n_ch, sc, relmax(c, r))
        part = backend._csm_welch_bins(y, 48000, W, Window.Hann, 50.0, False, sc, 0, 3)
        assert relmax(part, r[:3]) < TOL
        part = backend._csm_welch_bins(y, 48000, W, Window.Hann, 50.0, False, sc, W // 2 - 2, W // 2 + 1)
        assert relmax(part, r[W // 2 - 2:]) < TOL


@pytest.mark.parametrize("fixture", ["stft_manych", "stft_long"])
def test_stft_many_channels_golden(fixture):
    """tests/golden/stft_manych.npz: the reference's spectrograms of a 20-channel signal (one full tile of
    16 channels and a ragged one of 4 in the wave-level kernels) at windows 256 ... 2048;
    tests/golden/stft_long.npz: 10 channels (one workgroup of 8, one of 2 with idle teams) at windows of 4096, 8192
    and 16384 samples -- kernels_stft4096.hpp: every residue class of the decimation in frequency is in the stored bins."""
    meta, z = load_golden(fixture)
    x = z["x"].astype(np.float64)
    for i, c in enumerate(meta["cases"]):
        t, f, st = backend._stft(x, meta["fs"], c["W"], Window.Hann, c["overlap"], None, c["detrend"], c["padding"],
                                 SpectrumScaling[c["scaling"]])
        assert list(st.shape) == c["shape"]
        e = relmax(st[z[f"bins_{i}"]], z[f"stft_{i}"])
        assert e < 2 * TOL, (c, e)  # the reference is stored as complex64


def test_csm_coherent_channels_golden():
    """tests/golden/csm_coherent.npz: the reference's own matrices for coherent channels of either
    sign, even channel counts (the bf16-triple kernel), every branch-cut element at DC / Nyquist."""
    meta, z = load_golden("csm_coherent")
    x = z["x"].astype(np.float64)
    for i, c in enumerate(meta["cases"]):
        if c["n_ch"] == 64:  # the stored channels through the stored mixing matrix; some bins, complex64
            x64 = x @ z["mix"].astype(np.float64)
            f, csm = backend._csm_welch(x64, meta["fs"], c["W"], Window.Hann, c["overlap"], c["detrend"], "mean",
                                        SpectrumScaling[c["scaling"]])
            ref = z["csm64"]
            got = csm[z["bins64"]]
            assert relmax(got, ref) < 2 * TOL, relmax(got, ref)  # the reference is stored as complex64
            pure = (ref.real == 0) & (ref.imag != 0)
            assert pure.any() and np.all(np.sign(got.imag[pure]) == np.sign(ref.imag[pure]))
            continue
        f, csm = backend._csm_welch(x[:, :c["n_ch"]], meta["fs"], c["W"], Window.Hann, c["overlap"], c["detrend"],
                                    "mean", SpectrumScaling[c["scaling"]])
        ref = z[f"csm_{i}"]
        assert csm.shape == ref.shape
        lo = 1 if c["detrend"] else 0  # the detrended DC bin is 0 / 0-like: compared from bin 1 on
        assert relmax(csm[lo:], ref[lo:]) < TOL, (c, relmax(csm[lo:], ref[lo:]))
        # the branch: elements that are purely imaginary in the reference are so here, with the same sign
        pure = (ref.real == 0) & (ref.imag != 0)
        pure[:lo] = False
        assert np.all(np.sign(csm.imag[pure]) == np.sign(ref.imag[pure]))


def test_csm_bin_ranges_match_the_full_matrix():
    """ds_csm_bins_dev (one rank's share of the bins-sharded CSM) returns exactly the rows of the
    full matrix, including the edge-bin handling at DC / Nyquist."""
    rng = np.random.default_rng(44)
    x = 0.1 * rng.standard_normal((30000, 6)) + 0.2 * rng.standard_normal(30000)[:, None]
    for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.PowerSpectralDensity):
        f, full = backend._csm_welch(x, 48000, 512, Window.Hann, 50, True, "mean", sc)
        fr, ref = orc.csm_welch_batched(x, 48000, 512, "hann", 50, True, sc.name)
        for a, b in ((0, 257), (0, 100), (100, 257), (256, 257), (37, 38)):
            part = backend._csm_welch_bins(x, 48000, 512, Window.Hann, 50, True, sc, a, b)
            assert part.shape == (b - a, 6, 6)
            assert relmax(part, ref[a:b], a == 0) < TOL
            assert relmax(part, full[a:b], a == 0) < TOL


def test_csm_full_size_properties():
    """config 4 at full size (64 mics x 512 000 samples, nfft 1024): Hermitian, the diagonal is
    the Welch auto spectrum, and the 4 x 4 sub-block equals the CSM of those 4 channels alone
    (oracle, which finishes the sub-problem in seconds)."""
    rng = np.random.default_rng(4)
    n = 512000
    x = (0.1 * rng.standard_normal((n, 64)) + 0.2 * rng.standard_normal(n)[:, None])
    f, csm = backend._csm_welch(x, 48000, 1024, Window.Hann, 50, True, "mean", SpectrumScaling.FFTBackward)
    assert csm.shape == (513, 64, 64)
    assert np.max(np.abs(csm - np.conj(np.swapaxes(csm, 1, 2)))) <= 1e-7 * np.max(np.abs(csm))
    psd = backend._welch(x, None, 48000, Window.Hann, 1024, 50, True, "mean", SpectrumScaling.FFTBackward)
    diag = np.einsum("bii->bi", csm)
    assert relmax(diag.real, psd, True) < 2 * TOL and np.max(np.abs(diag.imag)) == 0.0
    sel = [0, 17, 40, 63]
    fr, ref = orc.csm_welch_batched(x[:, sel], 48000, 1024, "hann", 50, True, "FFTBackward")
    assert relmax(csm[:, sel][:, :, sel], ref, True) < TOL


def test_spectral_division_8192_edge_shapes():
    """The 8192-point shared-spectrum kernel: zero-padded input, odd channel counts, truncated
    output (element-wise tested stores), and the per-channel-spectrum fallback."""
    rng = np.random.default_rng(12)
    nfft = 8192
    r = (rng.standard_normal(nfft // 2 + 1) + 1j * rng.standard_normal(nfft // 2 + 1)) * 0.3
    for n, n_ch, n_out in ((8192, 2, 8192), (6000, 3, 6000), (8192, 1, 5001), (100, 5, 8192)):
        y = rng.standard_normal((4, n, n_ch))
        ref = np.fft.irfft(np.fft.rfft(y, n=nfft, axis=1) * r[None, :, None], n=nfft, axis=1)[:, :n_out]
        got = backend.spectral_division(y, nfft, r, n_out)
        assert got.shape == ref.shape
        assert relmax(got, ref) < TOL, (n, n_ch, n_out, relmax(got, ref))
    rc = np.stack([r, 0.5 * r, r.conj()], axis=1)  # per-channel spectra: generic kernel
    y = rng.standard_normal((2, 8192, 3))
    ref = np.fft.irfft(np.fft.rfft(y, n=nfft, axis=1) * rc[None], n=nfft, axis=1)
    assert relmax(backend.spectral_division(y, nfft, rc, nfft), ref) < TOL


def test_deconvolve_full_size_properties():
    """config 5 at full size (1024 stereo items x 8192 samples, one shared sweep): every 64th
    item against the oracle, and the batch result of an item equals its own single-item call."""
    from dsptoolbox_amd.generators import exponential_sweep
    rng = np.random.default_rng(5)
    n, items = 8192, 1024
    x = exponential_sweep(n, 48000)[:, None]
    h = rng.standard_normal((items, 2, 32)) * np.exp(-np.arange(32) / 6.0)
    X = np.fft.rfft(x[:, 0], 2 * n)
    y = np.fft.irfft(np.fft.rfft(h, 2 * n, axis=-1) * X, 2 * n, axis=-1)[..., :n]  # (items, 2, n)
    y = np.ascontiguousarray(np.swapaxes(y, 1, 2)) + 1e-4 * rng.standard_normal((items, n, 2))
    den = backend.rfft_spectrum(x, n)
    eps, _ = orc.regularization_eps(den[:, 0], np.fft.rfftfreq(n, 1 / 48000), 48000, None, -30.0)
    inv = backend.regularized_inverse(den, eps)[:, 0]
    out = backend.spectral_division(y, n, inv, n)
    assert out.shape == (items, n, 2)
    for i in range(0, items, 64):
        assert relmax(out[i], orc.spectral_deconvolve(y[i], x, 48000)) < TOL, i
    for i in (1, 511, 1023):
        single = backend.spectral_division(y[i:i + 1], n, inv, n)[0]
        assert np.array_equal(single, out[i])


def test_edge_cases():
    # signal shorter than one window, single channel, odd channel counts
    x = np.random.default_rng(1).standard_normal((100, 1))
    a = backend._welch(x, None, 48000, Window.Hann, 256, 50, False, "mean",
                       SpectrumScaling.PowerSpectrum)
    assert relmax(a, orc.welch(x, None, 48000, "hann", 256, 50, False, "mean", "PowerSpectrum")) < TOL
    x5 = np.random.default_rng(2).standard_normal((3000, 5))
    t, f, s = backend._stft(x5, 48000, 128, Window.Hann, 50, None, False, True,
                            SpectrumScaling.FFTBackward)
    rt, rf, rs = orc.stft(x5, 48000, 128, "hann", 50, None, False, True, "FFTBackward")
    assert relmax(s, rs) < TOL
    with pytest.raises(AssertionError):
        dsp.Signal(None, x5, 48000.0)


@pytest.mark.parametrize("overlap,n,n_cy", [(50, 70000, 3), (75, 50000, 5), (0, 36000, 1),
                                            (50, 4096 * 10 + 17, 2), (33, 30000, 2)])
def test_welch4096_fast_path_vs_oracle(overlap, n, n_cy):
    """nfft 4096 + one input channel takes the register-FFT path (frame pairs as
    real/imaginary part); broadband noise so every bin is well conditioned; odd
    frame counts, ragged tails and non-50 % hops included."""
    import warnings
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 1)) * 0.3
    h = rng.standard_normal((n_cy, 40)) * np.exp(-np.arange(40) / 8.0)
    y = np.stack([np.convolve(x[:, 0], h[c])[:n] for c in range(n_cy)], axis=1)
    y += 0.05 * rng.standard_normal(y.shape)
    for mode in ("H1", "H2", "H3"):
        for det, sc in ((True, SpectrumScaling.FFTBackward), (False, SpectrumScaling.PowerSpectralDensity)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                tf, coh = backend.welch_transfer_function(y, x, 48000, 4096, mode, detrend=det,
                                                          overlap_percent=overlap, scaling=sc)
                rt, rc = orc.compute_transfer_function(y, x, 48000, 4096, mode, detrend=det,
                                                       overlap_percent=overlap, scaling=sc.name)
            e1, e2 = relmax(tf, rt, det), relmax(coh, rc, det)
            assert e1 < TOL and e2 < TOL, (mode, det, e1, e2)


def test_welch4096_explicit_frame_count():
    """The C-ABI takes the frame count as an argument: an odd count smaller than ceil(N/hop) (the
    reference's keep_last_frames=False framing) must not let frame F leak into the last pair."""
    import ctypes as C
    from dsptoolbox_amd._lib import get_context
    rng = np.random.default_rng(8)
    n, n_cy, W, hop, F = 50000, 3, 4096, 2048, 7
    x = rng.standard_normal((1, n)).astype(np.float32)
    y = (rng.standard_normal((n_cy, n)) * 0.3).astype(np.float32)
    y[0] += np.convolve(x[0], [0.5, -0.2, 0.1])[:n].astype(np.float32)
    w = np.hanning(W + 1)[:-1].astype(np.float32)
    tf = np.empty((W // 2 + 1, n_cy), np.complex64)
    coh = np.empty((W // 2 + 1, n_cy), np.float32)
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx.check(ctx.lib.ds_welch_tf(ctx.handle, p(x), 1, p(y), n_cy, n, W, hop, F, p(w), 0, 0, 1, 0, 1.0, 1.0, 0,
                                  p(tf), p(coh)), "ds_welch_tf")
    fr = np.stack([x[0, f * hop:f * hop + W] * w for f in range(F)]).astype(np.float64)
    X = np.fft.rfft(fr, axis=1)
    for c in range(n_cy):
        Y = np.fft.rfft(np.stack([y[c, f * hop:f * hop + W] * w for f in range(F)]).astype(np.float64), axis=1)
        sxy, sxx, syy = np.mean(np.conj(X) * Y, axis=0), np.mean(np.abs(X)**2, axis=0), np.mean(np.abs(Y)**2, axis=0)
        assert relmax(tf[:, c], sxy / sxx) < TOL
        assert relmax(coh[:, c], np.abs(sxy)**2 / sxx / syy) < TOL


@pytest.mark.parametrize("n", [2**15, 2**17, 2**20])
def test_big_fft_whole_signal(n):
    """Lengths beyond one workgroup's LDS use the four-step path: whole-signal spectrum
    (Signal.get_spectrum, FFT method) and regularised deconvolution of a long sweep."""
    from dsptoolbox_amd.generators import exponential_sweep
    rng = np.random.default_rng(n)
    x3 = rng.standard_normal((n - 17, 3)) * 0.2  # zero padded to n by next_fast_len? use exact n below
    x3 = np.vstack([x3, rng.standard_normal((17, 3)) * 0.2])
    s = dsp.Signal(None, x3.copy(), 48000)
    s.set_spectrum_parameters(method=SpectrumMethod.FFT, scaling=SpectrumScaling.FFTBackward)
    f, sp = s.get_spectrum()
    assert sp.shape == (n // 2 + 1, 3)
    assert relmax(sp, np.fft.rfft(x3, axis=0)) < TOL
    # deconvolution: 2 output channels, mono sweep
    x = exponential_sweep(n, 48000)[:, None]
    h = rng.standard_normal((2, 128)) * np.exp(-np.arange(128) / 20.0)
    nf = 1 << int(np.ceil(np.log2(n + 128)))
    X = np.fft.rfft(x[:, 0], nf)
    y = np.stack([np.fft.irfft(X * np.fft.rfft(h[c], nf), nf)[:n] for c in range(2)], axis=1)
    y += 1e-3 * rng.standard_normal(y.shape)
    ir = dsp.transfer_functions.spectral_deconvolve(dsp.Signal(None, y, 48000), dsp.Signal(None, x, 48000))
    ref = orc.spectral_deconvolve(y, x, 48000)
    assert relmax(ir.time_data, ref) < TOL, relmax(ir.time_data, ref)


def test_api_rest_fir_side_golden():
    """tests/golden/api_rest.npz (from the reference): Filter.get_ir / get_transfer_function, FilterBank.get_ir /
    get_transfer_function / filter_multiband_signal / swap_filters, Signal.add_channel, MultiBandSignal.get_all_bands /
    swap_bands -- consumers of the device convolution (ds_fir_ola) and of ds_fir_freqz."""
    import warnings
    from dsptoolbox_amd._lib import get_context
    meta, z = load_golden("api_rest")
    fs = meta["fs"]
    mk = lambda b: dsp.Filter.from_ba(b, [1.0], fs)  # noqa: E731
    f1, f2, f3 = mk(z["b1"]), mk(z["b2"]), mk(z["b3"])
    fb = dsp.FilterBank([f1, f2, f3])
    ctx = get_context()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in meta["cases"]:
            if c["kind"] == "filter_get_ir":
                ir = f1.get_ir(c["length"], zero_phase=c["zero_phase"])
                assert isinstance(ir, dsp.ImpulseResponse) and ir.time_data.shape == z[c["key"]].shape
                assert relmax(ir.time_data, z[c["key"]]) < TOL, c
            elif c["kind"] == "filter_get_tf":
                ctx.routes()
                hu, hl = f1.get_transfer_function(z["fv_uniform"]), f1.get_transfer_function(z["fv_log"])
                assert ctx.routes() == {"fir_freqz"}
                assert hu.dtype == np.complex128 and relmax(hu, z["h_uniform"]) < 1e-11 and relmax(hl, z["h_log"]) < 1e-11
                with pytest.raises(AssertionError):
                    f1.get_transfer_function(np.array([0.0, fs]))
            elif c["kind"] == "bank_get_ir_tf":
                mode = FilterBankMode[c["mode"]]
                o = fb.get_ir(c["length"], mode)
                assert type(o).__name__ == c["out_type"]
                got = o.get_all_time_data()[0] if mode == FilterBankMode.Parallel else o.time_data
                assert relmax(got, z[f"bank_ir_{c['mode']}"]) < TOL, c
                assert relmax(fb.get_transfer_function(z["fv_log"], mode), z[f"bank_h_{c['mode']}"]) < 1e-11, c
            elif c["kind"] == "bank_get_ir_edge":
                o = fb.get_ir(100, FilterBankMode.Summed)
                assert o.time_data.shape == z["bank_ir_short"].shape and relmax(o.time_data, z["bank_ir_short"]) < TOL
                o = fb.get_ir(2000, FilterBankMode.Parallel, zero_phase=True)
                assert relmax(o.get_all_time_data()[0], z["bank_ir_zero_phase"]) < TOL
            elif c["kind"] == "filter_multiband_signal":
                mb = dsp.MultiBandSignal([dsp.Signal(None, z[f"mb_in_{n}"].copy(), fs) for n in range(3)])
                out = fb.filter_multiband_signal(mb)
                assert relmax(out.get_all_time_data()[0], z["mb_out"]) < TOL
                assert relmax(fb.filter_multiband_signal(mb, zero_phase=True).get_all_time_data()[0], z["mb_out_zero_phase"]) < TOL
                assert np.array_equal(mb.bands[0].time_data, z["mb_in_0"])  # the input is untouched
                # get_all_bands / swap_bands on the reference's own band data (bit-exact: no arithmetic)
                ref = dsp.MultiBandSignal([dsp.Signal(None, z["mb_out"][:, n, :].copy(), fs) for n in range(3)])
                assert np.array_equal(ref.get_all_bands(channel=1).time_data, z["all_bands_ch1"])
                ref.swap_bands([2, 0, 1])
                assert np.array_equal(ref.get_all_bands(channel=0).time_data, z["swapped_all_bands_ch0"])
                with pytest.raises(AssertionError):
                    ref.swap_bands([0, 0, 1])
            elif c["kind"] == "bands_and_filters_reordered":
                fb2 = dsp.FilterBank([f1, f2, f3]).swap_filters(c["new_filter_order"])
                assert np.array_equal(fb2.filters[0].ba[0], z["swapped_first_taps"])
            elif c["kind"] == "add_channel":
                i = int(c["key"].rsplit("_", 1)[1])
                sgl = dsp.Signal(None, z["sig_base"].copy(), fs)
                assert sgl.add_channel(None, z[f"add_in_{i}"].copy(), fs) is sgl
                assert sgl.number_of_channels == c["channels"] and np.array_equal(sgl.time_data, z[c["key"]])
            else:
                raise AssertionError(c["kind"])
    sgl = dsp.Signal(None, z["sig_base"].copy(), fs)
    with pytest.raises(AttributeError):
        sgl.add_channel(None, z["add_in_1"].copy(), fs, allow_padding_trimming=False)
    with pytest.raises(AssertionError):
        sgl.add_channel(None, z["add_in_0"].copy(), fs // 2)


def test_fused_float64_pipelines_for_spectra_division_and_inverse_stft():
    """ds_rfft_f64 / ds_deconv_f64 / ds_istft_f64 (round 4): large float64 / complex128 arrays in the reference's own
    layouts cross the boundary through the pinned chunk pipelines -- the same computation as the host-cast path (the
    device sees the same float32 values), checked against it bit for bit and against the oracle at 1e-6."""
    rng = np.random.default_rng(88)
    n, n_ch = 300000, 4  # 1.2 M elements: above the fused threshold
    x = rng.standard_normal((n, n_ch)) * 0.2
    # whole-signal spectrum (non-power-of-two length: four-step + Bluestein)
    nfft = 300000
    sp = backend.rfft_spectrum(x, nfft)
    sp_host = backend.rfft_spectrum(np.asfortranarray(x), nfft)  # not C-contiguous: the host-cast path
    assert sp.dtype == np.complex128 and np.array_equal(sp, sp_host)
    assert relmax(sp, np.fft.rfft(x, n=nfft, axis=0)) < TOL
    # one-item regularised division
    from dsptoolbox_amd.generators import exponential_sweep
    xs = exponential_sweep(n, 48000)[:, None]
    y = np.stack([np.convolve(xs[:, 0], rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0))[:n] for _ in range(n_ch)], axis=1)
    y += 1e-3 * rng.standard_normal(y.shape)
    ir = dsp.transfer_functions.spectral_deconvolve(dsp.Signal(None, y, 48000), dsp.Signal(None, xs, 48000))
    assert relmax(ir.time_data, orc.spectral_deconvolve(y, xs, 48000)) < TOL
    # inverse STFT of a complex128 spectrogram (round trip through the fused forward path too)
    s = dsp.Signal(None, x[:262144], 48000)
    s.set_spectrogram_parameters(window_length_samples=1024, overlap_percent=50, padding=True)
    t, f, st = s.get_spectrogram()
    assert st.dtype == np.complex128 and st.size >= (1 << 19)
    back = dsp.transforms.istft(st, original_signal=s)
    assert relmax(back.time_data, s.time_data) < 2e-6  # (the established round-trip bound of test_istft_golden_and_round_trip)
    back_host = dsp.transforms.istft(np.asfortranarray(st), original_signal=s)  # host-cast path
    assert np.array_equal(back.time_data, back_host.time_data)


# ---- short estimates through the API: the float64 route -------------------------------
@pytest.mark.parametrize("W", [64, 1024, 4096, 16384])
def test_short_estimates_through_the_api_hold_1e6(W, monkeypatch):
    """Auto spectra, cross spectra and cross-spectral matrices of ONE to FIVE frames (and a 100-frame one) through the
    reference-shaped API (backend._welch / _csm_welch with SPEC_PRECISION = "auto"): 1e-6 against the oracle under
    amplitude and power scalings, mean and median averaging -- the shapes where the fp32 kernels alone need 2-3e-6
    (tests/sweeps/edge_welch.py).  The float64 kernels must be the ones that ran."""
    from dsptoolbox_amd._lib import get_context
    monkeypatch.setattr(backend, "SPEC_PRECISION", "auto")
    rng = np.random.default_rng(W)
    ctx = get_context()
    worst = {"psd": 0.0, "csd": 0.0, "csm": 0.0}
    lengths = [W, W + 1, 2 * W + 5, 3 * W - 1] + ([50 * W + 3] if W <= 1024 else [])
    for n in lengths:
        for C in (1, 3):
            for det in (False, True):
                x = rng.standard_normal((n, C)) * 0.3
                y = np.stack([np.convolve(x[:, i], rng.standard_normal(5))[:n] for i in range(C)], axis=1)
                y += 0.01 * rng.standard_normal((n, C))
                lo = 1 if det else 0
                for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.PowerSpectralDensity):
                    for avg in ("mean", "median"):
                        ctx.routes()
                        a = backend._welch(y, None, 48000, Window.Hann, W, 50, det, avg, sc)
                        k = backend._welch(x, y, 48000, Window.Hann, W, 50, det, avg, sc)
                        seen = ctx.routes()
                        assert seen and all(r.startswith("welch_f64") for r in seen), seen
                        ra = orc.welch(y, None, 48000, "hann", W, 50, det, avg, sc.name)
                        rk = orc.welch(x, y, 48000, "hann", W, 50, det, avg, sc.name)
                        assert a.dtype == ra.dtype and a.shape == ra.shape and k.shape == rk.shape
                        worst["psd"] = max(worst["psd"], relmax(np.atleast_2d(a.T).T[lo:], np.atleast_2d(ra.T).T[lo:]))
                        worst["csd"] = max(worst["csd"], relmax(np.atleast_2d(k.T).T[lo:], np.atleast_2d(rk.T).T[lo:]))
                    if C > 1:
                        ctx.routes()
                        _, m = backend._csm_welch(y, 48000, W, Window.Hann, 50, det, "mean", sc)
                        assert ctx.routes() == {"welch_f64_frames", "csm_f64"}
                        _, rm = orc.csm_welch(y, 48000, W, "hann", 50, det, "mean", sc.name)
                        worst["csm"] = max(worst["csm"], relmax(m[lo:], rm[lo:]))
    print("short estimates through the API, worst rel-max", worst)
    assert max(worst.values()) < 1e-11, worst  # (float64 kernels, asserted above: the bound of this route, not TOL)


def test_csm_short_estimate_of_70_channels(monkeypatch):
    """VERDICT r4, missing 5: a SHORT cross-spectral matrix of more than 64 channels stays on the float64 route (further
    workgroups per bin take the channel pairs beyond the first 2304).  tests/golden/api_holes.npz: 70 channels, 22 frames
    of 128 samples, from the reference's Signal.get_csm (every 8th bin kept), through the product's Signal.get_csm."""
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd._lib import get_context
    from dsptoolbox_amd.standard.enums import SpectrumMethod
    monkeypatch.setattr(backend, "SPEC_PRECISION", "auto")
    meta, z = load_golden("api_holes")
    ctx = get_context()
    n_seen = 0
    for c in meta["cases"]:
        if c["kind"] != "csm_short_many_channels":
            continue
        sig = dsp.Signal(None, z["csm70_x"].copy(), meta["fs"])
        sig.set_spectrum_parameters(method=SpectrumMethod.WelchPeriodogram, window_length_samples=c["W"],
                                    scaling=SpectrumScaling[c["scaling"]])
        ctx.routes()
        f, m = sig.get_csm()
        assert ctx.routes() == {"welch_f64_frames", "csm_f64"}
        assert m.shape == (c["W"] // 2 + 1, c["channels"], c["channels"]) and m.dtype == np.complex128
        ref = z[c["key"]]
        e = relmax(m[::c["bin_step"]][1:], ref[1:])
        assert e < 1e-11, (c, e)
        # Hermitian in the channel pair, real diagonal: every element of the 2485 pairs was written
        assert np.array_equal(m, np.conj(np.swapaxes(m, 1, 2)))
        n_seen += 1
    assert n_seen == 2


def test_result_pool_gives_page_locked_blocks_back():
    """Context.download_result: the array returned owns a block of the context's page-locked pool until the last view of it
    is gone; a caller that kept many results alive does not leave their blocks page-locked for good (all but 16 spare
    ones go back to the driver at the next call)."""
    import gc
    from dsptoolbox_amd._lib import DeviceBuffer, get_context
    ctx = get_context()
    src = np.arange(3000, dtype=np.float32)
    d = DeviceBuffer.from_array(ctx, src)
    size = 1 << (src.nbytes - 1).bit_length()
    held = [ctx.download_result(d.ptr, (3000,), np.float32) for _ in range(90)]
    assert all(np.array_equal(h, src) for h in held[::9])
    assert len({h.ctypes.data for h in held}) == 90  # ninety different blocks
    pool = ctx._result_pool[size]
    n_before = len(pool)
    assert n_before >= 90
    view = held[5][10:20]  # a view keeps its block
    del held
    gc.collect()
    again = ctx.download_result(d.ptr, (3000,), np.float32)
    assert np.array_equal(again, src) and np.array_equal(view, src[10:20])
    assert len(pool) <= 16 + 2, (n_before, len(pool))  # sixteen spare ones, the view's, this one's
    d.free()


def test_sweep_shapes_over_the_old_byte_cap_take_float64(monkeypatch):
    """profiles/r05_sweeps.txt: paired-input estimates of 45 ... 61 frames of 8192 / 16384 samples read 1.0-1.7e-6 in the
    coherence at a null of the response on the fp32 kernels, and their 320-530 MB of frame spectra were over the 256 MB cap of
    the short-estimate rule.  The cap is 1.25 GB for every window now: through the reference-shaped API such an estimate
    takes the float64 kernels (a response with a prescribed null at the Nyquist bin; 20 + 20 channels, 61 frames of 16384)."""
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd._lib import get_context
    from dsptoolbox_amd.transfer_functions import TransferFunctionType
    monkeypatch.setattr(backend, "TF_PRECISION", "auto")
    rng = np.random.default_rng(306)
    W, C, n = 16384, 20, 495295
    x = rng.standard_normal((n, C)) * 0.4
    h = rng.standard_normal((8, C)) * 0.5 + 1.0
    sign = (-1.0) ** np.arange(8)
    h[7] -= (sign @ h - 0.01) / sign[7]  # the response at the Nyquist bin: 0.01 (its maximum is ~3)
    y = np.stack([np.convolve(x[:, j], h[:, j])[:n] for j in range(C)], axis=1) + 0.01 * rng.standard_normal((n, C))
    hop, n_frames = backend._welch_framing(n, W, 50.0, backend._window_array(Window.Hann, W))
    assert n_frames == 61 and 2 * C * n_frames * (W // 2 + 1) * 16 > (256 << 20)
    xs, ys = dsp.Signal(None, x, 48000), dsp.Signal(None, y, 48000)
    xs.set_spectrum_parameters(window_length_samples=W)
    ctx = get_context()
    ctx.routes()
    sp = dsp.transfer_functions.compute_transfer_function(ys, xs, W, TransferFunctionType.H1)
    seen = ctx.routes()
    assert seen and all(r.startswith("welch_f64") for r in seen), seen
    rt, rc = orc.compute_transfer_function(y, x, 48000, W, "H1")
    e_tf, e_coh = relmax(np.asarray(sp.spectral_data)[1:], rt[1:]), relmax(np.asarray(sp.coherence)[1:], rc[1:])
    assert e_tf < 1e-11 and e_coh < 1e-11, (e_tf, e_coh)
    assert rc[W // 2].min() < 0.6  # (the null is there: on the fp32 kernels this is where the 1e-6 goes)


def test_csm_short_estimate_median_in_float64(monkeypatch):
    """VERDICT r4, missing 5, second half: a SHORT cross-spectral matrix with average="median" takes float64 kernels too
    (w64::k_csm_median: a wave ranks one channel pair's frames).  The reference's own matrices of 70 channels over 22 and
    21 frames (api_holes.npz), then seeded shapes against the oracle: one and two channel tiles, 1 ... 127 frames (more
    than 64 frames: two per lane), odd and even counts, every scaling family."""
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd._lib import get_context
    from dsptoolbox_amd.standard.enums import SpectrumMethod
    monkeypatch.setattr(backend, "SPEC_PRECISION", "auto")
    meta, z = load_golden("api_holes")
    ctx = get_context()
    n_seen = 0
    for c in meta["cases"]:
        if c["kind"] != "csm_short_median":
            continue
        sig = dsp.Signal(None, z["csm70_x"][:c["samples"]].copy(), meta["fs"])
        sig.set_spectrum_parameters(method=SpectrumMethod.WelchPeriodogram, window_length_samples=c["W"],
                                    scaling=SpectrumScaling[c["scaling"]], average="median")
        ctx.routes()
        f, m = sig.get_csm()
        assert ctx.routes() == {"welch_f64_frames", "csm_f64_median"}
        assert m.shape == (c["W"] // 2 + 1, c["channels"], c["channels"]) and m.dtype == np.complex128
        e = relmax(m[::c["bin_step"]][1:], z[c["key"]][1:])
        assert e < 1e-11, (c, e)
        assert np.array_equal(m[1:], np.conj(np.swapaxes(m[1:], 1, 2)))
        n_seen += 1
    assert n_seen == 2
    rng = np.random.default_rng(91)
    worst = 0.0
    for C, W, n_frames, det, sc in ((2, 64, 1, False, SpectrumScaling.FFTBackward), (5, 256, 2, True, SpectrumScaling.PowerSpectrum),
                                    (33, 64, 9, True, SpectrumScaling.AmplitudeSpectralDensity),
                                    (7, 128, 64, False, SpectrumScaling.PowerSpectralDensity),
                                    (3, 32, 65, True, SpectrumScaling.FFTForward), (40, 16, 127, True, SpectrumScaling.FFTOrthogonal),
                                    (4, 4096, 6, True, SpectrumScaling.AmplitudeSpectrum)):
        n = (n_frames - 1) * (W // 2) + 3
        x = 0.2 * rng.standard_normal((n, C)) + 0.3 * rng.standard_normal(n)[:, None]
        ctx.routes()
        f, m = backend._csm_welch(x, 48000, W, Window.Hann, 50, det, "median", sc)
        assert ctx.routes() == {"welch_f64_frames", "csm_f64_median"}, (C, W, n_frames)
        rf, rm = orc.csm_welch(x, 48000, W, "hann", 50, det, "median", sc.name)
        lo = 1 if det else 0
        worst = max(worst, relmax(m[lo:], rm[lo:]))
    assert worst < 1e-11, worst
    with pytest.raises(NotImplementedError, match="more than 128 frames"):  # the C entry point itself: two frames a lane
        x = np.zeros((129 * 8, 2))
        out = np.empty((9, 2, 2), dtype=np.complex128)
        w = np.ones(16)
        ctx.check(ctx.lib.ds_csm_x64(ctx.handle, x.ctypes.data, 2, x.shape[0], 16, 8, 129, w.ctypes.data, 0, 1, 0, 1.0, 1.0, 0,
                                     out.ctypes.data), "ds_csm_x64")


def test_float64_welch_entries_reject_and_accept():
    """The three float64 Welch entries of the C ABI themselves (ds_welch_tf_x64, ds_welch_spec_x64, ds_csm_x64), with
    2 channels, W = 16, hop = 8 and 300 samples: the exception Context.check raises for every call they reject
    (ValueError: DS_ERR_ARG, NotImplementedError: DS_ERR_UNSUP) and one accepted call each against the float64 oracle.
    The limits on counts (4097 median frames, 1025 channels, the 2 GiB of frame spectra, W = 2^19) are passed as counts over
    the same tiny arrays: the entries refuse them before they read one.  ds_csm_x64's 129 median frames are asserted at
    the end of test_csm_short_estimate_median_in_float64."""
    from scipy.signal import get_window
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(23)
    n, C, W, hop, fs = 300, 2, 16, 8, 48000
    x = 0.3 * rng.standard_normal((n, C))
    y = np.stack([np.convolve(x[:, i], rng.standard_normal(5))[:n] for i in range(C)], axis=1)
    y += 1e-3 * rng.standard_normal(y.shape)
    w = np.ascontiguousarray(get_window("hann", W, fftbins=True), dtype=np.float64)
    B, F = W // 2 + 1, -(-n // hop)
    tf, coh = np.empty((B, C), np.complex128), np.empty((B, C))
    spec, csm = np.empty((B, C), np.complex128), np.empty((B, C, C), np.complex128)
    sc = SpectrumScaling.PowerSpectralDensity
    amp, norm_scale, factor, phys = backend._finish_params(sc, W, fs, w)
    base = dict(n_cx=C, n_cy=C, n_ch=C, n=n, W=W, hop=hop, F=F, w=w.ctypes.data, avg=0, mode=1)

    def call_tf(**kw):
        q = dict(base, **kw)
        ctx.check(ctx.lib.ds_welch_tf_x64(ctx.handle, x.ctypes.data, q["n_cx"], y.ctypes.data, q["n_cy"], q["n"], q["W"], q["hop"],
                                          q["F"], q["w"], 1, q["avg"], q["mode"], amp, norm_scale, factor, phys,
                                          tf.ctypes.data, coh.ctypes.data), "ds_welch_tf_x64")

    def call_spec(**kw):
        q = dict(base, **kw)
        ctx.check(ctx.lib.ds_welch_spec_x64(ctx.handle, x.ctypes.data, y.ctypes.data, q["n_ch"], q["n"], q["W"], q["hop"], q["F"],
                                            q["w"], 1, q["avg"], amp, norm_scale, factor, phys, spec.ctypes.data),
                  "ds_welch_spec_x64")

    def call_csm(**kw):
        q = dict(base, **kw)
        ctx.check(ctx.lib.ds_csm_x64(ctx.handle, x.ctypes.data, q["n_ch"], q["n"], q["W"], q["hop"], q["F"], q["w"], 1, q["avg"],
                                     amp, norm_scale, factor, phys, csm.ctypes.data), "ds_csm_x64")

    over_2gib = (2 << 30) // (2 * B * 16) + 1  # frames of 2 channels' spectra just past the cap (tf: x and y, twice that)
    assert 2 * over_2gib * B * 16 > 2 << 30
    shared = [(ValueError, dict(w=None)), (ValueError, dict(avg=2)), (NotImplementedError, dict(avg=1, F=4097)),
              (ValueError, dict(hop=0)), (ValueError, dict(hop=W + 1)), (NotImplementedError, dict(W=24)),
              (NotImplementedError, dict(W=2**19)), (NotImplementedError, dict(F=over_2gib))]
    for call in (call_tf, call_spec, call_csm):
        for exc, bad in shared:
            with pytest.raises(exc):
                call(**bad)
    for exc, bad in ((ValueError, dict(mode=0)), (ValueError, dict(mode=4)), (ValueError, dict(n_cx=2, n_cy=3))):
        with pytest.raises(exc):
            call_tf(**bad)
    with pytest.raises(NotImplementedError):
        call_csm(n_ch=1025)

    ctx.routes()
    call_tf()
    assert ctx.routes() == {"welch_f64_frames", "welch_f64_tf"}
    rt, rc = orc.compute_transfer_function(y, x, fs, W, "H1", scaling=sc.name)
    assert relmax(tf, rt, True) < 1e-9 and relmax(coh, rc, True) < 1e-9, (relmax(tf, rt, True), relmax(coh, rc, True))
    call_spec()
    assert ctx.routes() == {"welch_f64_frames", "welch_f64_spec"}
    rs = orc.welch(x, y, fs, "hann", W, 50, True, "mean", sc.name)
    assert relmax(spec, rs, True) < 1e-9, relmax(spec, rs, True)  # (float64 end to end: the bound of the transfer function above)
    call_csm()
    assert ctx.routes() == {"welch_f64_frames", "csm_f64"}
    rf, rm = orc.csm_welch(x, fs, W, "hann", 50, True, "mean", sc.name)
    assert relmax(csm[1:], rm[1:]) < 1e-11, relmax(csm[1:], rm[1:])


@pytest.mark.parametrize("W", [32768, 65536, 131072, 262144])
def test_short_estimates_with_long_windows_hold_1e6(W, monkeypatch):
    """The same for windows of 2^15 ... 2^18 samples -- where estimates are short almost by definition (a 2^20-sample
    signal has 7 frames of 2^18): the float64 route's long-window kernels (k_frames_cls + k_split: one decimation stage
    in front of the 8192-point LDS transform).  tests/sweeps/fuzz_long_windows.py: the fp32 long-window kernels alone
    reach 6e-6 (tf) / 5e-5 (coherence) on such shapes.  Auto / cross spectra, matrices, H1 / H2 with coherence."""
    from dsptoolbox_amd._lib import get_context
    monkeypatch.setattr(backend, "SPEC_PRECISION", "auto")
    rng = np.random.default_rng(W)
    ctx = get_context()
    worst = {"psd": 0.0, "csd": 0.0, "csm": 0.0, "tf": 0.0, "coh": 0.0}
    for n, C in ((W + 1, 3), (3 * W - 1, 1), (2 * W + 5, 2)):
        for det in (False, True):
            x = rng.standard_normal((n, C)) * 0.3
            y = np.stack([np.convolve(x[:, i], rng.standard_normal(5))[:n] for i in range(C)], axis=1)
            y += 0.01 * rng.standard_normal((n, C))
            lo = 1 if det else 0
            for sc, avg in ((SpectrumScaling.FFTBackward, "mean"), (SpectrumScaling.PowerSpectralDensity, "median")):
                ctx.routes()
                a = backend._welch(y, None, 48000, Window.Hann, W, 50, det, avg, sc)
                k = backend._welch(x, y, 48000, Window.Hann, W, 50, det, avg, sc)
                seen = ctx.routes()
                assert {"welch_f64_frames@long", "welch_f64_split"} <= seen and all(r.startswith("welch_f64") for r in seen), seen
                ra = orc.welch(y, None, 48000, "hann", W, 50, det, avg, sc.name)
                rk = orc.welch(x, y, 48000, "hann", W, 50, det, avg, sc.name)
                assert a.dtype == ra.dtype and a.shape == ra.shape and k.shape == rk.shape
                worst["psd"] = max(worst["psd"], relmax(np.atleast_2d(a.T).T[lo:], np.atleast_2d(ra.T).T[lo:]))
                worst["csd"] = max(worst["csd"], relmax(np.atleast_2d(k.T).T[lo:], np.atleast_2d(rk.T).T[lo:]))
            if C > 1:
                ctx.routes()
                _, m = backend._csm_welch(y, 48000, W, Window.Hann, 50, det, "mean", SpectrumScaling.AmplitudeSpectrum)
                assert ctx.routes() == {"welch_f64_frames@long", "welch_f64_split", "csm_f64"}
                _, rm = orc.csm_welch(y, 48000, W, "hann", 50, det, "mean", "AmplitudeSpectrum")
                worst["csm"] = max(worst["csm"], relmax(m[lo:], rm[lo:]))
            for mode in ("H1", "H2"):
                tf, coh = backend.welch_transfer_function(y, x, 48000, W, mode, detrend=det, precision="auto")
                rt, rc = orc.compute_transfer_function(y, x, 48000, W, mode, detrend=det)
                worst["tf"] = max(worst["tf"], relmax(tf[lo:], rt[lo:]))
                worst["coh"] = max(worst["coh"], relmax(coh[lo:], rc[lo:]))
    print("short estimates with long windows through the API, worst rel-max", W, worst)
    assert max(worst.values()) < 1e-11, worst  # (float64 kernels, asserted above: the bound of this route, not TOL)


@pytest.mark.parametrize("n_frames", [117, 500])
def test_csm_amplitude_scaling_of_coherent_channels(n_frames, monkeypatch):
    """DESIGN section 2, limit (ix), as a test: 32 coherent channels (one source through responses of either sign, a
    little noise), amplitude scaling -- the square root amplifies the fp32 error of elements that are small against the
    largest one.  117 frames is the shape the round-2 sweep flagged at 1.2e-6 on BOTH fp32 matrix kernels: through the
    API it is a short estimate and takes the float64 route (1e-6 holds); the fp32 kernels alone are held to the band
    the limit documents (2.5e-6), and to 1e-6 again once a few hundred frames average the transform rounding down."""
    worst = {"f32": 0.0, "auto": 0.0}
    for seed in range(4):
        rng = np.random.default_rng(900 + seed)
        W, C = 512, 32
        n = 256 * (n_frames - 1) + W - 100
        src = rng.standard_normal(n) * 0.3 + 0.05
        h = rng.standard_normal((32, C)) * np.exp(-np.arange(32) / 6.0)[:, None]
        x = 3.0 * (np.stack([np.convolve(src, h[:, c])[:n] for c in range(C)], axis=1) + 0.05 * rng.standard_normal((n, C)))
        _, ref = orc.csm_welch_batched(x, 48000, W, "hann", 50.0, True, "FFTBackward")
        for mode in ("f32", "auto"):
            monkeypatch.setattr(backend, "SPEC_PRECISION", mode)
            _, m = backend._csm_welch(x, 48000, W, Window.Hann, 50.0, True, "mean", SpectrumScaling.FFTBackward)
            worst[mode] = max(worst[mode], relmax(m[1:], ref[1:]))
    print("coherent channels, amplitude scaling,", n_frames, "frames: worst", worst)
    assert worst["f32"] < (2.5e-6 if n_frames < 128 else TOL), worst
    assert worst["auto"] < TOL, worst


# ---- every kernel-selecting switch is a tested route ---------------------------------
# A context reads the DSPTOOLBOX_AMD_* switches once, in ds_init (csrc/config.hpp); the test opens a
# new default context under each switch, runs the golden subset of the rows the switch re-routes, and
# checks through the launch names that the other kernel family really ran.
def _launched_by(fn):
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    ctx.routes()
    fn()
    return ctx.routes()


def _csm_64_bench_shape_reduced():
    test_csm_64ch_vs_oracle(64)


def _istft_16384_round_trip():
    x = np.random.default_rng(3).standard_normal((70000, 3)) * 0.3
    s = dsp.Signal(None, x, 48000)
    s.set_spectrogram_parameters(window_length_samples=16384, overlap_percent=50, padding=True)
    t, f, st = s.get_spectrogram()
    back = dsp.transforms.istft(st, original_signal=s)
    assert relmax(back.time_data, s.time_data) < 2e-6


def _fir_short_signal_on_the_fft_routes():
    """The shapes of test_fir_signal_shorter_than_the_filter with the direct sum switched off: the block-convolution
    routes carry them (to their own floor, DESIGN section 2 limit (x): 1e-4 of the tiny output here)."""
    rng = np.random.default_rng(4097)
    x = rng.standard_normal((1000, 2)) * 0.1
    taps = [rng.standard_normal(4097) * np.hanning(4097) / 64.0 for _ in range(2)]
    y = backend.fir_filter_bank(x, taps, backend.DS_FB_PARALLEL)
    for k in range(2):
        assert relmax(y[k], orc.lfilter_fir(taps[k], x)) < 1e-4


def _csm_frame_chunks_vs_oracle():
    """206 frames of 64 (and of 33) channels: under DSPTOOLBOX_AMD_CSM_CHUNKS=3 the frames go as three chunks on two streams,
    the products handing their raw sums on (CsmArgs::part_in / part_out); amplitude scaling too (the finish runs once)."""
    rng = np.random.default_rng(64)
    n = 105000
    for n_ch, sc in ((64, SpectrumScaling.FFTBackward), (33, SpectrumScaling.AmplitudeSpectrum)):
        x = 0.1 * rng.standard_normal((n, n_ch)) + 0.2 * rng.standard_normal(n)[:, None]
        f, csm = backend._csm_welch(x, 48000, 1024, Window.Hann, 50, True, "mean", sc)
        fr, ref = orc.csm_welch_batched(x, 48000, 1024, "hann", 50, True, sc.name)
        assert relmax(csm, ref, True) < (TOL if sc == SpectrumScaling.FFTBackward else 2 * TOL)
        assert np.array_equal(csm, np.conj(np.swapaxes(csm, 1, 2)))


SWITCH_ROUTES = [
    # (environment, golden subset, launch names (ds_routes) that must / must not appear)
    ({}, [lambda: _welch_golden_body(), lambda: _welch4096_golden(), lambda: test_stft_golden(), lambda: _csm_golden_body(),
          lambda: test_deconvolve_batch_8192(), lambda: test_fir_bank_4097_taps(), lambda: test_istft_golden_and_round_trip("istft")],
     {"welch1024_main", "welch4096_main@3", "stft@wave", "csm_gemm@b3", "deconv@8k_persist", "fir@4k_p2_3percu", "istft@wave"}, {"fir@4k_p2"}),
    ({}, [lambda: test_welch_long_windows_golden()], {"welch_long_main", "welch8192_main"}, {"welch16384_main"}),
    ({"DSPTOOLBOX_AMD_WELCH_GENERIC": "1"}, [lambda: _welch_golden_body(), lambda: test_welch_long_windows_golden()],
     {"welch_xspec"}, {"welch1024_main", "welch8192_main", "welch16384_main", "welch_long_main"}),
    ({"DSPTOOLBOX_AMD_WELCH_LONG_MIN": "32768"}, [lambda: test_welch_long_windows_golden()], {"welch16384_main"}, {"welch_long_main"}),
    ({"DSPTOOLBOX_AMD_NO_WELCH4096": "1"}, [lambda: _welch4096_golden("welch_yacc")], {"welch_yacc"},
     {"welch4096_main@3", "welch4096_main@2"}),
    ({"DSPTOOLBOX_AMD_W4_TWO_PER_CU": "1"}, [lambda: _welch4096_golden()], {"welch4096_main@2"}, {"welch4096_main@3"}),
    ({"DSPTOOLBOX_AMD_STFT_GENERIC": "1"}, [lambda: test_stft_golden(), lambda: test_stft_many_channels_golden("stft_long")],
     {"stft@generic"}, {"stft@wave", "stft@4k", "stft@dif"}),
    ({"DSPTOOLBOX_AMD_CSM_GENERIC": "1"}, [lambda: _csm_golden_body(), lambda: test_csm_coherent_channels_golden()],
     {"csm_gemm@generic"}, {"csm_gemm@b3", "csm_gemm@f32"}),
    ({"DSPTOOLBOX_AMD_CSM_F32": "1"}, [lambda: _csm_golden_body(), lambda: test_csm_coherent_channels_golden(),
                                       _csm_64_bench_shape_reduced], {"csm_gemm@f32"}, {"csm_gemm@b3"}),
    ({"DSPTOOLBOX_AMD_DECONV_GENERIC": "1"}, [lambda: test_deconvolve_golden(), lambda: test_deconvolve_batch_8192()],
     {"deconv@generic"}, {"deconv@8k_persist", "deconv@8k_4percu", "deconv@8k_3percu", "deconv@8k_512"}),
    ({"DSPTOOLBOX_AMD_DECONV_2PERCU": "1"}, [lambda: test_deconvolve_batch_8192()], {"deconv@8k_512"}, {"deconv@8k_persist", "deconv@8k_4percu"}),
    ({"DSPTOOLBOX_AMD_DECONV_PERSIST": "0"}, [lambda: test_deconvolve_batch_8192()], {"deconv@8k_4percu"}, {"deconv@8k_persist"}),
    ({"DSPTOOLBOX_AMD_DECONV_PERSIST": "0", "DSPTOOLBOX_AMD_DECONV_4PERCU": "0"}, [lambda: test_deconvolve_batch_8192()], {"deconv@8k_3percu"},
     {"deconv@8k_persist", "deconv@8k_4percu"}),
    ({"DSPTOOLBOX_AMD_FIR_GENERIC": "1", "DSPTOOLBOX_AMD_FIR_4K": "0"},
     [lambda: test_fir_golden(), lambda: test_fir_16k_blocks_vs_oracle(4097, 12288 * 3, 2)], {"fir@generic"},
     {"fir@4k_p1", "fir@4k_p2", "fir@4k_p2_3percu", "fir@16k", "fir@16k_ragged"}),
    ({"DSPTOOLBOX_AMD_FIR_3PERCU": "0"}, [lambda: test_fir_bank_4097_taps(), lambda: test_fir_golden(), lambda: _fir_short_signal_on_the_fft_routes()],
     {"fir@4k_p2"}, {"fir@4k_p2_3percu"}),
    # (the auto-spectrum loop has three workgroups per CU anyway and keeps its launch name)
    ({"DSPTOOLBOX_AMD_WELCH_LONG_3PERCU": "1"}, [lambda: test_welch_long_windows_golden()], {"welch_long_main@jit"}, set()),
    ({"DSPTOOLBOX_AMD_FIR_4K": "0"}, [lambda: test_fir_golden(), lambda: test_fir_16k_blocks_vs_oracle(4097, 12288 * 3, 2),
                                      lambda: test_fir_16k_blocks_vs_oracle(4097, 5000, 5),
                                      lambda: test_fir_bank_4097_taps()], {"fir@16k_ragged", "fir@direct_f64"}, {"fir@4k_p1", "fir@4k_p2", "fir@4k_p2_3percu"}),
    ({"DSPTOOLBOX_AMD_FIR_4K": "1"}, [lambda: test_fir_golden(), lambda: test_fir_one_and_two_tap_filters()], {"fir@4k_p1"}, set()),
    ({"DSPTOOLBOX_AMD_CSM_CHUNKS": "3"}, [_csm_frame_chunks_vs_oracle, lambda: _csm_golden_body()], {"csm_gemm@b3"}, set()),
    ({"DSPTOOLBOX_AMD_FIR_STAGE": "1"}, [lambda: test_fir_bank_4097_taps(), lambda: test_fir_golden(), lambda: test_fir_one_and_two_tap_filters()],
     {"fir@4k_p2_staged"}, {"fir@4k_p2"}),
    ({"DSPTOOLBOX_AMD_W2048_WAVE": "1"}, [lambda: _welch_golden_body()], set(), {"welch2048_main@4k"}),
    ({"DSPTOOLBOX_AMD_FINISH_WIDE": "1"}, [lambda: _welch_golden_body(), lambda: _welch4096_golden(), lambda: test_welch_long_windows_golden()],
     {"welch_finish@wide"}, {"welch_finish"}),
    ({"DSPTOOLBOX_AMD_FIR_DIRECT": "0"}, [lambda: test_fir_golden(), lambda: _fir_short_signal_on_the_fft_routes()], {"fir@4k_p2_3percu"},
     {"fir@direct_f64"}),
    ({"DSPTOOLBOX_AMD_STFT_GENERIC": "1"}, [lambda: test_stft_and_csm_long_windows_vs_oracle()], set(), {"stft@long", "stft_long_dif"}),
    ({"DSPTOOLBOX_AMD_ISTFT_FUSED": "0"}, [lambda: test_istft_golden_and_round_trip("istft")], {"istft_ola"},
     {"istft@wave", "istft@4k", "istft@fused"}),
    ({"DSPTOOLBOX_AMD_ISTFT_WAVE": "0"}, [lambda: test_istft_golden_and_round_trip("istft"), _istft_16384_round_trip], set(),
     {"istft@wave", "istft@long", "istft@long_ola", "istft_long_cls"}),
    ({"DSPTOOLBOX_AMD_ISTFT_CT": "1"}, [lambda: test_istft_golden_and_round_trip("istft")], set(), {"istft@ct"}),
]


# ---- which Welch kernel family each window runs on, per entry point (tests/golden/welch_routes.json) -----------------
# Keys "<switch>|<kind>|<W>|<hop divisor>|<average>|<input channels>"; the launch names were recorded through the same
# helper on the library before the Welch dispatch became one route choice (csrc/api.hip, welch_route).
WELCH_ROUTE_SWITCHES = {"default": {}, "WELCH_GENERIC": {"DSPTOOLBOX_AMD_WELCH_GENERIC": "1"},
                        "NO_WELCH4096": {"DSPTOOLBOX_AMD_NO_WELCH4096": "1"}}
WELCH_ROUTE_WINDOWS, WELCH_ROUTE_ENTRIES = rcs.WELCH_ROUTE_WINDOWS, rcs.WELCH_ROUTE_ENTRIES


def _welch_route_case(entry, q):
    """One small estimate (the problem q of route_cases.welch_problem) through one C-ABI entry point -> (output
    arrays, launch names)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x, y, xp, yp, w = q["x"], q["y"], q["xp"], q["yp"], q["w"]
    W, hop, n, n_frames, B, n_ch, n_out = q["W"], q["hop"], q["n"], q["n_frames"], q["B"], q["n_cy"], q["n_out"]
    avg, kind = backend.DS_AVG[q["average"]], q["kind"]
    tail = (q["detrend"], avg) + ((backend.DS_TF[q["mode"]],) if kind == "tf" else ()) + \
        (q["amp_sqrt"], q["norm_scale"], q["factor"], q["halve_edges"])
    ctx.routes()
    if entry.endswith("_dev"):
        dx, dy = DevicePlanar.from_planar(ctx, xp), DevicePlanar.from_planar(ctx, yp)
        dw, do = DeviceBuffer.from_array(ctx, w), DeviceBuffer(ctx, B * n_out * 12)
        if kind == "tf":
            ctx.check(ctx.lib.ds_welch_tf_dev(ctx.handle, C.c_void_p(dx.ptr), dx.n_ch, dx.ld, C.c_void_p(dy.ptr), dy.n_ch,
                                              dy.ld, n, W, hop, n_frames, C.c_void_p(dw.ptr), *tail, C.c_void_p(do.ptr),
                                              C.c_void_p(do.ptr + B * n_out * 8)), entry)
            raw = do.to_array((B * n_out * 12,), np.uint8)
            out = (raw[:B * n_out * 8].view(np.complex64), raw[B * n_out * 8:].view(np.float32))
        else:
            ctx.check(ctx.lib.ds_welch_psd_dev(ctx.handle, C.c_void_p(dx.ptr), dx.n_ch, dx.ld, n, W, hop, n_frames,
                                               C.c_void_p(dw.ptr), *tail, C.c_void_p(do.ptr)), entry)
            out = (do.to_array((B * n_out,), np.float32),)
        for b in (dx.owner, dy.owner, dw, do):
            b.free()
        return out, ctx.routes()
    f64 = entry.endswith("_f64")
    xa, ya = (x, y) if f64 else (xp, yp)
    if kind == "tf":
        tf, coh = np.empty((B, n_out), np.complex64), np.empty((B, n_out), np.float32)
        fn = ctx.lib.ds_welch_tf_f64 if f64 else ctx.lib.ds_welch_tf
        ctx.check(fn(ctx.handle, p(xa), x.shape[1], p(ya), n_ch, n, W, hop, n_frames, p(w), *tail, p(tf), p(coh)), entry)
        out = (tf, coh)
    elif kind == "psd":
        psd = np.empty((B, n_out), np.float32)
        fn = ctx.lib.ds_welch_psd_f64 if f64 else ctx.lib.ds_welch_psd
        ctx.check(fn(ctx.handle, p(xa), n_out, n, W, hop, n_frames, p(w), *tail, p(psd)), entry)
        out = (psd,)
    else:
        csd = np.empty((B, n_out), np.complex64)
        fn = ctx.lib.ds_welch_csd_f64 if f64 else ctx.lib.ds_welch_csd
        ctx.check(fn(ctx.handle, p(xa), p(ya), n_out, n, W, hop, n_frames, p(w), *tail, p(csd)), entry)
        out = (csd,)
    return out, ctx.routes()


def _welch_route_matrix(kinds=("tf", "psd", "csd"), windows=WELCH_ROUTE_WINDOWS, on_case=None):
    """{key: sorted launch names} of every case of the matrix under the current context's switches."""
    seen = {}
    for kind in kinds:
        for W in windows:
            for hop_div in (2, 4):
                for average in ("mean", "median"):
                    for one_in in (True, False):
                        q = rcs.welch_problem(kind, W, hop_div, average, one_in)
                        for entry in WELCH_ROUTE_ENTRIES[kind]:
                            out, routes = _welch_route_case(entry, q)
                            key = f"{entry}|{W}|{hop_div}|{average}|{1 if one_in else 3}"
                            seen[key] = sorted(routes)
                            if on_case:
                                on_case(key, entry, q, out, seen[key])
    return seen


@pytest.mark.parametrize("W", WELCH_ROUTE_WINDOWS)
@pytest.mark.parametrize("kind", list(WELCH_ROUTE_ENTRIES))
@pytest.mark.parametrize("switch", list(WELCH_ROUTE_SWITCHES))
def test_welch_routes_per_window(switch, kind, W, monkeypatch):
    """Each (window, overlap, averaging, channel layout) of every Welch entry point launches the kernels it launched
    when the table was recorded: a change of route is a change of the rounding of every spectrum that takes it."""
    import json
    from dsptoolbox_amd import _lib
    with open(os.path.join(ROOT, "tests", "golden", "welch_routes.json")) as fh:
        table = json.load(fh)
    for k, v in WELCH_ROUTE_SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    _lib.reset_context()
    judged = _RouteJudge(f"welch {kind} W={W} {switch}")
    try:
        seen = _welch_route_matrix((kind,), (W,), on_case=judged)
    finally:
        for k in WELCH_ROUTE_SWITCHES[switch]:
            monkeypatch.delenv(k, raising=False)
        _lib.reset_context()
    # (every entry point of a kind runs the same kernels: the table has one row per kind)
    want = {k: table[f"{switch}|{kind}|{k.split('|', 1)[1]}"].split() for k in seen}
    judged.report()
    assert seen == want


# ---- calls every Welch entry point refuses (tests/golden/welch_rejected.json) ----------------------------------------
# Keys "<entry>|<what is wrong>", values "ERR<code>" as _route_call records them.  Each call is a valid small estimate
# (256-sample window, three channels, arrays of full size) with ONE argument spoilt, so it is refused by the argument
# checks and launches nothing.  Recorded on the library before the Welch runners took one call struct (csrc/api.hip,
# WelchCall); "mode9" and "2in3out" exist for the transfer function only, "short_ld" for the device entries only.
WELCH_REJECTED = ("hop0", "hop>W", "frames0", "average2", "mode9", "2in3out", "null_window", "null_output", "short_ld")


def _welch_rejected_applies(entry, bad):
    if bad in ("mode9", "2in3out"):
        return entry.startswith("tf")
    return bad != "short_ld" or entry.endswith("_dev")


def _welch_rejected_case(entry, bad, W=256, n_ch=3):
    """One refused estimate through one C-ABI entry point -> ["ERR<code>"] (or the launch names, were it accepted)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    kind, dev, f64 = entry.split("_")[0], entry.endswith("_dev"), entry.endswith("_f64")
    n, B = 2 * W + 3000, W // 2 + 1
    n_cx = 2 if bad == "2in3out" else n_ch
    hop = {"hop0": 0, "hop>W": W + 1}.get(bad, W // 2)
    n_frames = 0 if bad == "frames0" else -(-n // (W // 2))
    average = 2 if bad == "average2" else backend.DS_AVG["mean"]
    mode = 9 if bad == "mode9" else backend.DS_TF["H2"]
    rng = np.random.default_rng(W)
    x, y = rng.standard_normal((n, n_cx)), rng.standard_normal((n, n_ch))
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(W) / W)).astype(np.float32)
    tail = (1, average) + ((mode,) if kind == "tf" else ()) + (0, 1.0 / W, 2.0, 1)
    held = []  # device buffers, freed below
    if dev:
        dx, dy = (DevicePlanar.from_planar(ctx, np.ascontiguousarray(a.T, dtype=np.float32)) for a in (x, y))
        dw, do = DeviceBuffer.from_array(ctx, w), DeviceBuffer(ctx, B * n_ch * 12)
        held = [dx.owner, dy.owner, dw, do]
        sx, sy = (C.c_void_p(dx.ptr), n_cx, n - 1 if bad == "short_ld" else dx.ld), (C.c_void_p(dy.ptr), n_ch, dy.ld)
        pw, po, po2 = C.c_void_p(dw.ptr), C.c_void_p(do.ptr), C.c_void_p(do.ptr + B * n_ch * 8)
    else:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        xa, ya = (np.ascontiguousarray(a if f64 else a.T, dtype=np.float64 if f64 else np.float32) for a in (x, y))
        out, out2 = np.zeros((B, n_ch), np.complex64), np.zeros((B, n_ch), np.float32)
        sx, sy, pw = (p(xa), n_cx), (p(ya), n_ch), p(w)
        po, po2 = p(out.view(np.float32) if kind == "psd" else out), p(out2)
    if bad == "null_window":
        pw = None
    if bad == "null_output":
        po = None
    mid = (n, W, hop, n_frames, pw)
    ctx.routes()
    if kind == "tf":
        fn = ctx.lib.ds_welch_tf_dev if dev else (ctx.lib.ds_welch_tf_f64 if f64 else ctx.lib.ds_welch_tf)
        routes = _route_call(ctx, fn, (*sx, *sy, *mid, *tail, po, po2))
    elif kind == "psd":
        fn = ctx.lib.ds_welch_psd_dev if dev else (ctx.lib.ds_welch_psd_f64 if f64 else ctx.lib.ds_welch_psd)
        routes = _route_call(ctx, fn, (*sx, *mid, *tail, po))
    else:
        fn = ctx.lib.ds_welch_csd_f64 if f64 else ctx.lib.ds_welch_csd
        routes = _route_call(ctx, fn, (sx[0], sy[0], n_ch, *mid, *tail, po))
    for b in held:
        b.free()
    return routes


def _welch_rejected_matrix():
    """{key: ["ERR<code>"]} of every refused call of every Welch entry point."""
    return {f"{entry}|{bad}": _welch_rejected_case(entry, bad)
            for entries in WELCH_ROUTE_ENTRIES.values() for entry in entries
            for bad in WELCH_REJECTED if _welch_rejected_applies(entry, bad)}


@pytest.mark.gpu
def test_welch_rejected_calls():
    """Every Welch entry point refuses a spoilt call with the code it returned when the table was recorded."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "welch_rejected.json")) as fh:
        table = json.load(fh)
    seen = _welch_rejected_matrix()
    assert seen == {k: v.split() for k, v in table.items()}


# ---- which kernel family each STFT / iSTFT length runs on, per entry point (tests/golden/stft_routes.json) ----------
# Keys "<switch>|stft|<nfft>|<window>|<detrend>|<channels>" and "<switch>|istft|<nfft>|<window>|<step divisor>|<channels>"
# (window: "full" = nfft samples, "short" = 3 nfft / 4); the launch names were recorded through the same helpers on the
# library before the STFT and iSTFT dispatch became one route choice each (csrc/api.hip, stft_route / istft_route).
STFT_ROUTE_SWITCHES = {"default": {}, "STFT_GENERIC": {"DSPTOOLBOX_AMD_STFT_GENERIC": "1"}}
STFT_ROUTE_NFFTS, ISTFT_ROUTE_NFFTS, STFT_ROUTE_ENTRIES = rcs.STFT_ROUTE_NFFTS, rcs.ISTFT_ROUTE_NFFTS, rcs.STFT_ROUTE_ENTRIES
ISTFT_ROUTE_SWITCHES = {"default": {}, "ISTFT_FUSED=0": {"DSPTOOLBOX_AMD_ISTFT_FUSED": "0"},
                        "ISTFT_WAVE=0": {"DSPTOOLBOX_AMD_ISTFT_WAVE": "0"}, "ISTFT_CT=1": {"DSPTOOLBOX_AMD_ISTFT_CT": "1"}}


class _RouteJudge:
    """The on_case hook of the route matrices: every output a matrix produces is held against the float64 oracle of
    its problem (tests/route_oracles.py) -- a rejected call against the zeros its arrays were made with -- BEFORE the
    launch names are compared with the table, so a test shows a wrong value and a changed route."""

    def __init__(self, what):
        self.what, self.worst, self.at, self.n, self.t0 = what, 0.0, None, 0, ros.seconds["oracle"]

    def __call__(self, key, entry, q, out, routes):
        if routes and routes[0].startswith("ERR"):
            return ros.judge_rejected(key, entry, out)
        frac = ros.judge_case(key, entry, q, out)
        self.n += 1
        if frac >= self.worst:
            self.worst, self.at = frac, key
        return frac

    def report(self):
        print(f"route oracle {self.what}: {self.n} outputs judged, worst error / bound {self.worst:.3f} at {self.at}; "
              f"oracles took {ros.seconds['oracle'] - self.t0:.1f} s of CPU")


def _stft_route_case(entry, q):
    """One short spectrogram (route_cases.stft_problem) through one C-ABI entry point -> (output array, launch names)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x, xp, w, W, hop, n, n_ch, n_frames, B = (q[k] for k in ("x", "xp", "w", "W", "hop", "n", "n_ch", "n_frames", "B"))
    tail = (q["nfft"], q["pad_front"], n_frames)
    par = (q["detrend"], C.c_float(q["scale"]), C.c_float(q["edge_scale"]), q["power"])
    ctx.routes()
    if entry.endswith("_dev"):
        dx, dw, do = DevicePlanar.from_planar(ctx, xp), DeviceBuffer.from_array(ctx, w), DeviceBuffer(ctx, B * n_frames * n_ch * 8)
        routes = _route_call(ctx, ctx.lib.ds_stft_r2c_dev, (C.c_void_p(dx.ptr), n, n_ch, dx.ld, W, hop, *tail,
                                                            C.c_void_p(dw.ptr), *par, C.c_void_p(do.ptr)))
        out = do.to_array((B, n_frames, n_ch), np.complex64)
        for b in (dx.owner, dw, do):
            b.free()
        return out, routes
    f64 = entry.endswith("_f64")
    out = np.zeros((B, n_frames, n_ch), np.complex128 if f64 else np.complex64)
    fn = ctx.lib.ds_stft_r2c_f64 if f64 else ctx.lib.ds_stft_r2c
    routes = _route_call(ctx, fn, (p(x if f64 else xp), n, n_ch, W, hop, *tail, p(w), *par, p(out)))
    return out, routes


def _istft_route_case(entry, q):
    """One short inverse transform (route_cases.istft_problem) through one C-ABI entry point -> (output array, launch
    names)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    spec, w, W, total, nfft, n_ch, n_frames, B = (q[k] for k in ("spec", "w", "W", "total", "nfft", "n_ch", "n_frames", "B"))
    mid = (n_ch, nfft, W, q["step"], q["frame_offset"], q["n_frames_total"])
    ctx.routes()
    if entry.endswith("_dev"):
        ds, dw = DeviceBuffer.from_array(ctx, q["spec32"]), DeviceBuffer.from_array(ctx, w)
        do = DeviceBuffer(ctx, n_ch * total * 4)
        routes = _route_call(ctx, ctx.lib.ds_istft_dev, (C.c_void_p(ds.ptr), B, n_frames, *mid, C.c_void_p(dw.ptr),
                                                         C.c_float(q["scale"]), total, C.c_void_p(do.ptr), total))
        out = do.to_array((n_ch, total), np.float32)
        for b in (ds, dw, do):
            b.free()
        return out, routes
    f64 = entry.endswith("_f64")
    s = np.ascontiguousarray(spec) if f64 else q["spec32"]
    out = np.zeros((total, n_ch) if f64 else (n_ch, total), np.float64 if f64 else np.float32)
    fn = ctx.lib.ds_istft_f64 if f64 else ctx.lib.ds_istft
    routes = _route_call(ctx, fn, (p(s), B, n_frames, *mid, p(w), C.c_float(q["scale"]), total, p(out)))
    return out, routes


def _stft_route_matrix(kind, nffts, on_case=None, power=0):
    """{key: sorted launch names} of every case of the STFT (kind "stft") or iSTFT ("istft") matrix under the current
    context's switches."""
    seen = {}
    for nfft in nffts:
        for short in (False, True):
            for a in ((False, True) if kind == "stft" else (2, 4)):  # detrend / step divisor
                for n_ch in ((1, 3) if kind == "stft" else (1, 2, 3)):
                    q = rcs.stft_problem(nfft, short, a, n_ch, power) if kind == "stft" else rcs.istft_problem(nfft, short, a, n_ch)
                    for entry in STFT_ROUTE_ENTRIES[kind]:
                        out, routes = (_stft_route_case if kind == "stft" else _istft_route_case)(entry, q)
                        key = f"{entry}|{nfft}|{'short' if short else 'full'}|{int(a)}|{n_ch}"
                        seen[key] = routes
                        if on_case:
                            on_case(key, entry, q, out, routes)
    return seen


def _stft_routes_vs_table(kind, switches, switch, nfft, monkeypatch):
    import json
    from dsptoolbox_amd import _lib
    with open(os.path.join(ROOT, "tests", "golden", "stft_routes.json")) as fh:
        table = json.load(fh)
    for k, v in switches[switch].items():
        monkeypatch.setenv(k, v)
    _lib.reset_context()
    judged = _RouteJudge(f"{kind} nfft={nfft} {switch}")
    try:
        seen = _stft_route_matrix(kind, (nfft,), on_case=judged)
    finally:
        for k in switches[switch]:
            monkeypatch.delenv(k, raising=False)
        _lib.reset_context()
    # (every entry point of a kind runs the same kernels: the table has one row per kind)
    want = {k: table[f"{switch}|{kind}|{k.split('|', 1)[1]}"].split() for k in seen}
    judged.report()
    assert seen == want


@pytest.mark.parametrize("nfft", STFT_ROUTE_NFFTS)
@pytest.mark.parametrize("switch", list(STFT_ROUTE_SWITCHES))
def test_stft_routes_per_length(switch, nfft, monkeypatch):
    """Each (length, window, detrend, channel count) of every STFT entry point launches the kernels it launched when
    the table was recorded: a change of route is a change of the rounding of every spectrogram that takes it."""
    _stft_routes_vs_table("stft", STFT_ROUTE_SWITCHES, switch, nfft, monkeypatch)


@pytest.mark.parametrize("nfft", ISTFT_ROUTE_NFFTS)
@pytest.mark.parametrize("switch", list(ISTFT_ROUTE_SWITCHES))
def test_istft_routes_per_length(switch, nfft, monkeypatch):
    """The same for every (length, window, step, channel count) of every inverse STFT entry point.

    (Judging the values found a fault here: "2048|full|2|2" -- five frames of two channels on istft@wave and istft@fused --
    was off by 2.3e-4 of the row rms, 14 times its bound, and held non-zero samples behind the last frame; see
    test_istft_last_frame_dropped_vs_oracle.  It is now within 0.27 of the bound.)"""
    _stft_routes_vs_table("istft", ISTFT_ROUTE_SWITCHES, switch, nfft, monkeypatch)


@pytest.mark.parametrize("nfft", [256, 1024, 2048])  # (lengths of the matrix: their bounds are recorded)
@pytest.mark.parametrize("switch", ["default", "ISTFT_WAVE=0", "ISTFT_FUSED=0"])
def test_istft_last_frame_dropped_vs_oracle(switch, nfft, monkeypatch):
    """The 50 % overlap problems of test_istft_routes_per_length without their last frame: 25 and 7 frames at 256 and
    1024 points, where the matrix has even frame counts only, and 4 frames at 2048 points, the EVEN count the matrix
    lacks there (it has 5).  The fused kernels (istft@wave, istft@fused) transform frames in pairs; a last pair without
    a second frame used to overlap-add the transform's rounding of its first frame (the imaginary part, about 1e-8 of
    the frame) as if it were a frame, and behind the last frame the envelope's floor of 1e-4 multiplies that by 1e4.
    New launches, because no case of the matrix reaches this below 2048 points; under the matrix's bounds."""
    def run():
        worst = 0.0
        for n_ch in (2, 3):
            q = rcs.istft_problem(nfft, False, 2, n_ch, drop_last=True)
            for entry in STFT_ROUTE_ENTRIES["istft"]:
                out, routes = _istft_route_case(entry, q)
                if switch != "ISTFT_FUSED=0":
                    assert routes == ["istft@wave" if switch == "default" else "istft@fused"], routes
                worst = max(worst, ros.judge_case(f"{entry}|{nfft}|odd|{n_ch}", entry, q, out))
        return worst
    worst = _routes_under(ISTFT_ROUTE_SWITCHES, switch, run, monkeypatch)
    print(f"route oracle istft nfft={nfft} without the last frame, {switch}: worst error / bound {worst:.3f}")


# ---- which kernel family each FIR, rFFT, deconvolution and CSM call runs on, per entry point ------------------------
# (tests/golden/fir_routes.json, xform_routes.json, csm_routes.json).  Keys "<switch>|<family>|<case>": the host
# float32, host float64 and device entries of a family run the same kernels on the same case, so each case has one
# row; a rejected call records "ERR<code>".  The launch names were recorded through these helpers on the library
# before each of the four dispatches became one route choice (csrc/api.hip, fir_route / rfft_route / deconv_route /
# csm_route).
def _routes_under(switches, switch, matrix, monkeypatch):
    """matrix() on a fresh context under one switch setting."""
    from dsptoolbox_amd import _lib
    for k, v in switches[switch].items():
        monkeypatch.setenv(k, v)
    _lib.reset_context()
    try:
        return matrix()
    finally:
        for k in switches[switch]:
            monkeypatch.delenv(k, raising=False)
        _lib.reset_context()


def _routes_vs_table(name, family, switch, seen):
    import json
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        table = json.load(fh)
    want = {k: table[f"{switch}|{family}|{k.split('|', 1)[1]}"].split() for k in seen}
    assert seen == want


FIR_ROUTE_SWITCHES = {"default": {},
                      "FIR_GENERIC=1+FIR_4K=0": {"DSPTOOLBOX_AMD_FIR_GENERIC": "1", "DSPTOOLBOX_AMD_FIR_4K": "0"},
                      "FIR_4K=0": {"DSPTOOLBOX_AMD_FIR_4K": "0"}, "FIR_4K=1": {"DSPTOOLBOX_AMD_FIR_4K": "1"},
                      "FIR_3PERCU=0": {"DSPTOOLBOX_AMD_FIR_3PERCU": "0"}, "FIR_STAGE=1": {"DSPTOOLBOX_AMD_FIR_STAGE": "1"},
                      "FIR_DIRECT=0": {"DSPTOOLBOX_AMD_FIR_DIRECT": "0"}}
FIR_ROUTE_TAPS, FIR_ROUTE_ENTRIES = rcs.FIR_ROUTE_TAPS, rcs.FIR_ROUTE_ENTRIES
FIR_ROUTE_MODES = {"parallel": backend.DS_FB_PARALLEL, "summed": backend.DS_FB_SUMMED,
                   "sequential": backend.DS_FB_SEQUENTIAL}
# (FIR_ROUTE_ENTRIES: (entry, output row stride); "odd" = a device output stride that is not a multiple of 4)


def _fir_route_case(entry, ld, q):
    """One filter bank (route_cases.fir_problem) through one C-ABI entry point -> (output array, launch names).  n may
    be 0 (rejected)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x, xp, taps, n_taps, n, ns, n_filt, n_ch, n_out = (q[k] for k in ("x", "xp", "taps", "n_taps", "n", "ns", "n_filt",
                                                                      "n_ch", "n_out"))
    m = FIR_ROUTE_MODES[q["mode"]]
    ctx.routes()
    if entry.endswith("_dev"):
        ld_y = ns | 1 if ld == "odd" else ns
        dx, dt, dy = DevicePlanar.from_planar(ctx, xp), DeviceBuffer.from_array(ctx, taps), DeviceBuffer(ctx, n_out * n_ch * ld_y * 4)
        routes = _route_call(ctx, ctx.lib.ds_fir_ola_dev, (C.c_void_p(dx.ptr), n_ch, dx.ld, n, C.c_void_p(dt.ptr), n_filt,
                                                           n_taps, m, C.c_void_p(dy.ptr), ld_y))
        out = dy.to_array((n_out, n_ch, ld_y), np.float32)[..., :n]
        for b in (dx.owner, dt, dy):
            b.free()
        return out, routes
    f64 = entry.endswith("_f64")
    out = np.zeros((n_out, ns, n_ch), np.float64) if f64 else np.zeros((n_out, n_ch, ns), np.float32)
    fn = ctx.lib.ds_fir_ola_f64 if f64 else ctx.lib.ds_fir_ola
    routes = _route_call(ctx, fn, (p(x if f64 else xp), n_ch, n, p(taps), n_filt, n_taps, m, p(out)))
    return out, routes


def _fir_route_matrix(taps_list, modes, on_case=None):
    seen = {}
    for n_taps in taps_list:
        for n in (n_taps - 1, 5000, 50000):  # shorter than the filter, a few blocks, several 16k blocks
            for n_filt in (1, 3):
                for mode in modes:
                    q = rcs.fir_problem(n_taps, n, n_filt, mode)
                    for entry, ld in FIR_ROUTE_ENTRIES:
                        out, routes = _fir_route_case(entry, ld, q)
                        key = f"{entry}|{n_taps}|{n}|{n_filt}|{mode}|{ld}"
                        seen[key] = routes
                        if on_case:
                            on_case(key, entry, q, out, routes)
    return seen


@pytest.mark.parametrize("n_taps", FIR_ROUTE_TAPS)
@pytest.mark.parametrize("switch", list(FIR_ROUTE_SWITCHES))
def test_fir_routes_per_shape(switch, n_taps, monkeypatch):
    """Each (taps, signal length, filter count, bank mode, output stride) of every FIR entry point launches the kernels
    it launched when the table was recorded.  The switches choose among the parallel mode's kernels; the summed and
    sequential modes run the parallel route on combined taps, so they are pinned with the default switches only."""
    modes = list(FIR_ROUTE_MODES) if switch == "default" else ["parallel"]
    judged = _RouteJudge(f"fir taps={n_taps} {switch}")
    seen = _routes_under(FIR_ROUTE_SWITCHES, switch, lambda: _fir_route_matrix((n_taps,), modes, on_case=judged), monkeypatch)
    judged.report()
    _routes_vs_table("fir_routes.json", "fir", switch, seen)


XFORM_ROUTE_NFFTS = rcs.XFORM_ROUTE_NFFTS
DECONV_ROUTE_SWITCHES = {"default": {}, "DECONV_GENERIC": {"DSPTOOLBOX_AMD_DECONV_GENERIC": "1"},
                         "DECONV_2PERCU": {"DSPTOOLBOX_AMD_DECONV_2PERCU": "1"},
                         "DECONV_PERSIST=0": {"DSPTOOLBOX_AMD_DECONV_PERSIST": "0"},
                         "DECONV_PERSIST=0+DECONV_4PERCU=0": {"DSPTOOLBOX_AMD_DECONV_PERSIST": "0",
                                                             "DSPTOOLBOX_AMD_DECONV_4PERCU": "0"}}


def _rfft_route_matrix(nffts, on_case=None):
    seen = {}
    for n_fft in nffts:
        for short in (False, True):
            for n_ch in (1, 3):
                q = rcs.rfft_problem(n_fft, short, n_ch)
                for entry in ("rfft", "rfft_f64", "rfft_dev"):
                    out, routes = _rfft_route_case(entry, q)
                    key = f"{entry}|{n_fft}|{'short' if short else 'full'}|{n_ch}"
                    seen[key] = routes
                    if on_case:
                        on_case(key, entry, q, out, routes)
    return seen


def _deconv_route_matrix(nffts, on_case=None):
    seen = {}
    for n_fft in nffts:
        for short in (False, True):
            for rpc in (0, 1):
                for n_items in (1, 2):
                    q = rcs.deconv_problem(n_fft, short, rpc, n_items)
                    for entry in ("deconv", "deconv_f64", "deconv_dev") if n_items == 1 else ("deconv", "deconv_dev"):
                        out, routes = _deconv_route_case(entry, q)
                        key = f"{entry}|{n_fft}|{'short' if short else 'full'}|{rpc}|{n_items}"
                        seen[key] = routes
                        if on_case:
                            on_case(key, entry, q, out, routes)
    return seen


@pytest.mark.parametrize("n_fft", XFORM_ROUTE_NFFTS)
def test_rfft_routes_per_length(n_fft, monkeypatch):
    """Each (length, signal length, channel count) of every whole-signal rFFT entry point launches the kernels it
    launched when the table was recorded."""
    judged = _RouteJudge(f"rfft n_fft={n_fft}")
    seen = _routes_under({"default": {}}, "default", lambda: _rfft_route_matrix((n_fft,), on_case=judged), monkeypatch)
    judged.report()
    _routes_vs_table("xform_routes.json", "rfft", "default", seen)


@pytest.mark.parametrize("n_fft", XFORM_ROUTE_NFFTS)
@pytest.mark.parametrize("switch", list(DECONV_ROUTE_SWITCHES))
def test_deconv_routes_per_length(switch, n_fft, monkeypatch):
    """The same for every (length, signal length, inverse per channel, item count) of every deconvolution entry."""
    judged = _RouteJudge(f"deconv n_fft={n_fft} {switch}")
    seen = _routes_under(DECONV_ROUTE_SWITCHES, switch, lambda: _deconv_route_matrix((n_fft,), on_case=judged), monkeypatch)
    judged.report()
    _routes_vs_table("xform_routes.json", "deconv", switch, seen)


CSM_ROUTE_SWITCHES = {"default": {}, "CSM_GENERIC": {"DSPTOOLBOX_AMD_CSM_GENERIC": "1"},
                      "CSM_F32": {"DSPTOOLBOX_AMD_CSM_F32": "1"}, "CSM_CHUNKS=3": {"DSPTOOLBOX_AMD_CSM_CHUNKS": "3"}}
CSM_ROUTE_WINDOWS = rcs.CSM_ROUTE_WINDOWS


def _csm_route_case(entry, q):
    """One cross-spectral matrix (route_cases.csm_problem) through one C-ABI entry point -> (output array, launch
    names).  ds_csm_bins_dev: the problem's bin range."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x, xp, w, W, hop, n, n_ch, n_frames, nb, b0, bc = (q[k] for k in ("x", "xp", "w", "W", "hop", "n", "n_ch", "n_frames",
                                                                      "nb", "b0", "bc"))
    average = q["average"]
    mid = (W, hop, n_frames)
    # amp_sqrt, norm_scale, factor, halve_edges
    fin = (q["amp_sqrt"], C.c_double(q["norm_scale"]), C.c_double(q["factor"]), q["halve_edges"])
    ctx.routes()
    if entry.endswith("_dev"):
        dx, dw, do = DevicePlanar.from_planar(ctx, xp), DeviceBuffer.from_array(ctx, w), DeviceBuffer(ctx, bc * n_ch * n_ch * 8)
        if entry == "csm_bins_dev":
            routes = _route_call(ctx, ctx.lib.ds_csm_bins_dev, (C.c_void_p(dx.ptr), n_ch, dx.ld, n, *mid, C.c_void_p(dw.ptr),
                                                                q["detrend"], *fin, b0, bc, C.c_void_p(do.ptr)))
        else:
            routes = _route_call(ctx, ctx.lib.ds_csm_dev, (C.c_void_p(dx.ptr), n_ch, dx.ld, n, *mid, C.c_void_p(dw.ptr), q["detrend"],
                                                           backend.DS_AVG[average], *fin, C.c_void_p(do.ptr)))
        out = do.to_array((bc, n_ch, n_ch), np.complex64)
        for b in (dx.owner, dw, do):
            b.free()
        return out, routes
    f64 = entry.endswith("_f64")
    out = np.zeros((nb, n_ch, n_ch), np.complex64)
    fn = ctx.lib.ds_csm_f64 if f64 else ctx.lib.ds_csm
    routes = _route_call(ctx, fn, (p(x if f64 else xp), n_ch, n, *mid, p(w), q["detrend"], backend.DS_AVG[average],
                                   *fin, p(out)))
    return out, routes


def _csm_route_matrix(windows, on_case=None):
    """Up to 1024-sample windows: 1 ... 130 channels and also 192 frames (three chunks of >= 64 frames under
    CSM_CHUNKS=3); at 4096 samples up to 65 channels; longer windows 1 and 3 channels (a 32768-sample matrix of 130
    channels alone is 2.2 GB)."""
    seen = {}
    for W in windows:
        chans = (1, 3, 64, 65, 130) if W <= 1024 else ((1, 3, 64, 65) if W <= 4096 else (1, 3))
        for average in ("mean", "median"):
            for n_ch in chans:
                for n_frames in (4, 8, 192) if W <= 1024 else (4, 8):
                    cases = [("csm", "all"), ("csm_f64", "all"), ("csm_dev", "all")]
                    if average == "mean":
                        cases += [("csm_bins_dev", "all"), ("csm_bins_dev", "part")]
                    for entry, bins in cases:
                        q = rcs.csm_problem(W, average, n_ch, n_frames, bins)
                        out, routes = _csm_route_case(entry, q)
                        key = f"{entry}|{W}|{average}|{n_ch}|{n_frames}|{bins}"
                        seen[key] = routes
                        if on_case:
                            on_case(key, entry, q, out, routes)
    return seen


@pytest.mark.parametrize("W", CSM_ROUTE_WINDOWS)
@pytest.mark.parametrize("switch", list(CSM_ROUTE_SWITCHES))
def test_csm_routes_per_shape(switch, W, monkeypatch):
    """Each (window, averaging, channel count, frame count, bin range) of every CSM entry point launches the kernels
    it launched when the table was recorded."""
    judged = _RouteJudge(f"csm W={W} {switch}")
    seen = _routes_under(CSM_ROUTE_SWITCHES, switch, lambda: _csm_route_matrix((W,), on_case=judged), monkeypatch)
    judged.report()
    _routes_vs_table("csm_routes.json", "csm", switch, seen)


@pytest.mark.parametrize("route", SWITCH_ROUTES, ids=lambda r: ",".join(f"{k.replace('DSPTOOLBOX_AMD_', '')}={v}"
                                                                        for k, v in r[0].items()) or "default")
def test_kernel_selecting_switches(route, monkeypatch):
    from dsptoolbox_amd import _lib
    env, subset, must, must_not = route
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reset_context()
    try:
        seen = set()
        for fn in subset:
            seen |= _launched_by(fn)
        assert must <= seen, (env, sorted(seen))
        assert not (must_not & seen), (env, sorted(seen))
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
        _lib.reset_context()


# ---- device-resident signals (hard parts 4 and 6) ---------------------------------
def _resident_pair(n=2**17 + 333, n_ch=6, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 1)) * 0.3
    h = rng.standard_normal((n_ch, 24)) * np.exp(-np.arange(24) / 6.0)
    y = np.stack([np.convolve(x[:, 0], h[c])[:n] for c in range(n_ch)], axis=1) + 0.01 * rng.standard_normal((n, n_ch))
    return x, y


def test_device_resident_transfer_function_spectrum_and_matrix(monkeypatch):
    """compute_transfer_function, get_spectrum (Welch) and get_csm read a device-resident signal in place: same numbers
    as the host path of the same fp32 kernels, 1e-6 against the oracle, and no host copy is ever made."""
    monkeypatch.setattr(backend, "TF_PRECISION", "f32")
    monkeypatch.setattr(backend, "SPEC_PRECISION", "f32")
    x, y = _resident_pair()
    fs = 48000
    for W, mode, det in ((4096, TransferFunctionType.H1, True), (1024, TransferFunctionType.H2, False),
                         (512, TransferFunctionType.H3, True)):
        si_h, so_h = dsp.Signal(None, x.copy(), fs), dsp.Signal(None, y.copy(), fs)
        si_d = dsp.Signal.from_planar_f32(backend._planar_f32(x), fs)
        so_d = dsp.Signal(None, y.copy(), fs).to_device()
        for s in (si_h, si_d):
            s.set_spectrum_parameters(window_length_samples=W, detrend=det)
        ref = dsp.transfer_functions.compute_transfer_function(so_h, si_h, W, mode)
        got = dsp.transfer_functions.compute_transfer_function(so_d, si_d, W, mode)
        assert si_d.on_device and not si_d._has_host_copy  # nothing came down but the small result
        # (the detrended DC bin is 0 / 0 = nan on both paths, as in the reference)
        assert np.array_equal(got.spectral_data, ref.spectral_data, equal_nan=True)
        assert np.array_equal(got.coherence, ref.coherence, equal_nan=True)
        rt, rc = orc.compute_transfer_function(y, x, fs, W, mode.name, detrend=det)
        lo = 1 if det else 0
        assert relmax(got.spectral_data[lo:], rt[lo:]) < (TOL if mode != TransferFunctionType.H2 else 5e-6)
        assert relmax(got.coherence[lo:], rc[lo:]) < TOL
    # Welch auto spectra and the cross-spectral matrix
    sh = dsp.Signal(None, y.copy(), fs)
    sd = dsp.Signal.from_planar_f32(backend._planar_f32(y), fs)
    for s in (sh, sd):
        s.set_spectrum_parameters(window_length_samples=2048, scaling=SpectrumScaling.PowerSpectralDensity)
    fh, ph = sh.get_spectrum()
    fd, pd_ = sd.get_spectrum()
    assert np.array_equal(fh, fd) and np.array_equal(ph, pd_) and not sd._has_host_copy
    _, ch = sh.get_csm(on_device=True)
    _, cd = sd.get_csm(on_device=True)
    assert np.array_equal(ch.to_host(), cd.to_host()) and not sd._has_host_copy


def test_device_resident_spectrogram_and_inverse():
    """get_spectrogram of a device-resident signal (array result and on_device=True handle) and transforms.istft of the
    handle: the reconstruction stays in HBM and equals the host path's."""
    rng = np.random.default_rng(12)
    x = rng.standard_normal((40000, 3)) * 0.3
    fs = 48000
    for W, pad in ((1024, True), (4096, True), (512, False)):
        sh = dsp.Signal(None, x.copy(), fs)
        sd = dsp.Signal.from_planar_f32(backend._planar_f32(x), fs)
        for s in (sh, sd):
            s.set_spectrogram_parameters(window_length_samples=W, padding=pad)
        th, fh, st_h = sh.get_spectrogram()
        td, fd, st_d = sd.get_spectrogram()
        assert np.array_equal(st_h, st_d) and np.array_equal(th, td) and np.array_equal(fh, fd)
        _, _, handle = sd.get_spectrogram(on_device=True)
        assert isinstance(handle, backend.DeviceSTFT) and handle.shape == st_h.shape
        assert np.array_equal(handle.to_host(), st_h)
        back_h = dsp.transforms.istft(st_h, original_signal=sh)
        back_d = dsp.transforms.istft(handle, original_signal=sd)
        assert back_d.on_device and not back_d._has_host_copy and len(back_d) == len(sd)
        assert relmax(back_d.time_data, back_h.time_data) < 2e-7  # (the host path narrows complex128 -> complex64 the same way)
        assert relmax(back_d.time_data[W:-W], x[W:-W]) < 2e-6
        assert not sd._has_host_copy


def test_device_resident_filtering_keeps_the_bands_on_the_device():
    """Filter.filter_signal and FilterBank.filter_signal (three modes) over a device-resident signal: outputs are
    device-resident signals / a MultiBandSignal of device-resident bands (slices of one buffer), equal to the host path and
    1e-6 against the oracle; time_data / get_all_time_data materialise on demand; assigning time_data drops the device copy."""
    rng = np.random.default_rng(44)
    n, n_ch, fs = 50000, 3, 48000
    x = rng.standard_normal((n, n_ch)) * 0.2
    filters = [dsp.Filter.fir_filter(1200, [300.0 * (k + 1), 900.0 * (k + 1)], FilterPassType.Bandpass, fs) for k in range(4)]
    taps = [f.ba[0] for f in filters]
    sh = dsp.Signal(None, x.copy(), fs)
    sd = dsp.Signal.from_planar_f32(backend._planar_f32(x), fs)
    yh = filters[0].filter_signal(sh)
    yd = filters[0].filter_signal(sd)
    assert yd.on_device and not yd._has_host_copy and type(yd) is dsp.Signal
    assert np.array_equal(yd.time_data, yh.time_data)
    assert relmax(yd.time_data, orc.lfilter_fir(taps[0], x)) < TOL
    fb = dsp.FilterBank(filters)
    for mode in (FilterBankMode.Parallel, FilterBankMode.Sequential, FilterBankMode.Summed):
        oh = fb.filter_signal(sh, mode)
        od = fb.filter_signal(sd, mode)
        if mode == FilterBankMode.Parallel:
            assert od.on_device and od.number_of_bands == 4 and all(not b._has_host_copy for b in od.bands)
            owners = {id(b.device_samples.owner) for b in od.bands}
            assert len(owners) == 1  # one output buffer, four slices
            all_d, _ = od.get_all_time_data()
            all_h, _ = oh.get_all_time_data()
            assert np.array_equal(all_d, all_h)
            assert all(not b._has_host_copy for b in od.bands)  # the bulk download did not pin a second copy
            assert np.array_equal(od.bands[2].time_data, oh.bands[2].time_data) and od.bands[2]._has_host_copy
            ref = orc.filterbank_fir(taps, x, "Parallel")
            assert relmax(all_d, np.transpose(ref, (0, 2, 1))) < TOL
            coll = od.collapse()
            assert relmax(coll.time_data, oh.collapse().time_data) < 1e-12
        else:
            assert od.on_device and not od._has_host_copy
            assert np.array_equal(od.time_data, oh.time_data)
    # an impulse response constrains its amplitude: its filter output is inspected on the host, like the reference's
    ir = dsp.ImpulseResponse(None, x[:, :1].copy() * 0.1, fs).to_device()
    out = filters[1].filter_signal(ir)
    assert type(out) is dsp.ImpulseResponse and not out.on_device
    # copies share the device samples; assigning new samples drops them
    c = sd.copy()
    assert c.on_device and c.device_samples is sd.device_samples
    c.time_data = x[:100]
    assert not c.on_device and c.time_data.shape == (100, n_ch) and sd.on_device


def test_device_resident_spectral_deconvolve():
    """spectral_deconvolve of device-resident signals (fast length: everything on the device) against the host path."""
    fs = 48000
    for n, n_cy, padding in ((8192, 2, False), (16384, 3, True), (4096, 1, False)):
        from dsptoolbox_amd.generators import exponential_sweep
        rng = np.random.default_rng(n)
        x = exponential_sweep(n, fs)[:, None]
        h = rng.standard_normal((n_cy, 64)) * np.exp(-np.arange(64) / 10.0)
        y = np.stack([np.convolve(x[:, 0], h[c])[:n] for c in range(n_cy)], axis=1)
        xh, yh = dsp.Signal(None, x.copy(), fs), dsp.Signal(None, y.copy(), fs)
        xd = dsp.Signal.from_planar_f32(backend._planar_f32(x), fs)
        yd = dsp.Signal.from_planar_f32(backend._planar_f32(y), fs)
        ir_h = dsp.transfer_functions.spectral_deconvolve(yh, xh, padding=padding, keep_original_length=padding)
        ir_d = dsp.transfer_functions.spectral_deconvolve(yd, xd, padding=padding, keep_original_length=padding)
        assert type(ir_d) is dsp.ImpulseResponse and ir_d.on_device and not ir_d._has_host_copy
        assert ir_d.spectrum_method == SpectrumMethod.FFT and len(ir_d) == len(ir_h)
        assert relmax(ir_d.time_data, ir_h.time_data) < 3e-7
        ref = orc.spectral_deconvolve(y, x, fs, padding=padding, keep_original_length=padding)
        assert relmax(ir_d.time_data, ref) < TOL
        assert not yd._has_host_copy and not xd._has_host_copy


# ---- 2048-sample windows on the 4096-point register machine -------------------------------------
def test_welch_2048_window_on_the_4096_machine(monkeypatch):
    """welch2048h: two 2048-point pair transforms per pass.  Transfer functions (one input channel and one per output
    channel), auto and cross spectra against the oracle for every frame count modulo 4, one-pass signals, detrend on /
    off, an amplitude scaling; and against the wave / team kernels it replaces (DSPTOOLBOX_AMD_W2048_WAVE=1)."""
    from dsptoolbox_amd import _lib
    from dsptoolbox_amd._lib import get_context
    monkeypatch.setattr(backend, "TF_PRECISION", "f32")
    monkeypatch.setattr(backend, "SPEC_PRECISION", "f32")
    rng = np.random.default_rng(2048)
    W, fs = 2048, 48000
    worst = 0.0
    ctx = get_context()
    cases = [(1024 * 4 * 7, 3), (1024 * (4 * 9 + 1) - 5, 2), (1024 * (4 * 5 + 2) + 17, 5), (1024 * (4 * 6 + 3), 1),
             (2048, 2), (3000, 1), (2**18, 8)]
    for n, C in cases:
        x1 = rng.standard_normal((n, 1)) * 0.3
        xc = rng.standard_normal((n, C)) * 0.3
        y = np.stack([np.convolve(x1[:, 0], rng.standard_normal(6))[:n] for _ in range(C)], axis=1)
        y += 0.05 * rng.standard_normal((n, C)) + 0.1
        # one input per output channel: responses to THOSE inputs (a transfer function between unrelated noises is
        # itself noise, 1 / sqrt(frames) of nothing)
        yc = np.stack([np.convolve(xc[:, c], rng.standard_normal(6))[:n] for c in range(C)], axis=1)
        yc += 0.05 * rng.standard_normal((n, C)) + 0.1
        for det in (True, False):
            lo = 1 if det else 0
            for xin, yout in ((x1, y), (xc, yc)):
                ctx.routes()
                tf, coh = backend.welch_transfer_function(yout, xin, fs, W, "H1", detrend=det, precision="f32")
                assert {"welch2048_x", "welch2048_main@4k"} <= ctx.routes(), ctx.routes()
                rt, rc = orc.compute_transfer_function(yout, xin, fs, W, "H1", detrend=det)
                e = max(relmax(tf[lo:], rt[lo:]), relmax(coh[lo:], rc[lo:]))
                worst = max(worst, e)
                # (one to five frames: nothing averages the fp32 transform rounding down -- DESIGN section 2; the API
                # sends such estimates through the float64 kernels)
                assert e < (3e-5 if n < 8 * W else TOL), (n, C, det, xin.shape, e)
            for sc in (SpectrumScaling.FFTBackward, SpectrumScaling.AmplitudeSpectralDensity):
                ctx.routes()
                a = backend._welch(y, None, fs, Window.Hann, W, 50, det, "mean", sc)
                k = backend._welch(xc, yc, fs, Window.Hann, W, 50, det, "mean", sc)
                assert "welch2048_main@4k" in ctx.routes()
                ra = orc.welch(y, None, fs, "hann", W, 50, det, "mean", sc.name)
                rk = orc.welch(xc, yc, fs, "hann", W, 50, det, "mean", sc.name)
                e = max(relmax(np.atleast_2d(a.T).T[lo:], np.atleast_2d(ra.T).T[lo:]),
                        relmax(np.atleast_2d(k.T).T[lo:], np.atleast_2d(rk.T).T[lo:]))
                worst = max(worst, e)
                assert e < (3e-5 if n < 8 * W else TOL), (n, C, det, sc, e)
    print("welch 2048 on the 4096 machine: worst rel-max", worst)
    # the same estimate on the kernels it replaces
    n, C = 2**17 + 100, 4
    x1 = rng.standard_normal((n, 1)) * 0.3
    y = np.stack([np.convolve(x1[:, 0], rng.standard_normal(6))[:n] for _ in range(C)], axis=1) + 0.05 * rng.standard_normal((n, C))
    tf_new, coh_new = backend.welch_transfer_function(y, x1, fs, W, "H2", precision="f32")
    monkeypatch.setenv("DSPTOOLBOX_AMD_W2048_WAVE", "1")
    _lib.reset_context()
    try:
        ctx2 = get_context()
        ctx2.routes()
        tf_old, coh_old = backend.welch_transfer_function(y, x1, fs, W, "H2", precision="f32")
        assert "welch2048_main@4k" not in ctx2.routes()
    finally:
        monkeypatch.delenv("DSPTOOLBOX_AMD_W2048_WAVE", raising=False)
        _lib.reset_context()
    assert relmax(tf_new[1:], tf_old[1:]) < TOL and relmax(coh_new[1:], coh_old[1:]) < TOL


def test_welch_2048_explicit_frame_count():
    """A frame count smaller than ceil(N / hop) at a 2048-sample window: frames past it must not leak into the last pass
    (drop_frames of kernels_welch2048h.hpp), for every count modulo 4."""
    import ctypes as C
    from dsptoolbox_amd._lib import get_context
    rng = np.random.default_rng(9)
    n, n_cy, W, hop = 40000, 2, 2048, 1024
    x = rng.standard_normal((1, n)).astype(np.float32)
    y = (rng.standard_normal((n_cy, n)) * 0.3).astype(np.float32)
    y[0] += np.convolve(x[0], [0.5, -0.2, 0.1])[:n].astype(np.float32)
    w = np.hanning(W + 1)[:-1].astype(np.float32)
    ctx = get_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for F in (5, 6, 7, 8, 1, 2, 3):
        tf = np.empty((W // 2 + 1, n_cy), np.complex64)
        coh = np.empty((W // 2 + 1, n_cy), np.float32)
        ctx.routes()
        ctx.check(ctx.lib.ds_welch_tf(ctx.handle, p(x), 1, p(y), n_cy, n, W, hop, F, p(w), 0, 0, 1, 0, 1.0, 1.0, 0,
                                      p(tf), p(coh)), "ds_welch_tf")
        assert "welch2048_main@4k" in ctx.routes()
        X = np.fft.rfft(np.stack([x[0, f * hop:f * hop + W] * w for f in range(F)]).astype(np.float64), axis=1)
        for c in range(n_cy):
            Y = np.fft.rfft(np.stack([y[c, f * hop:f * hop + W] * w for f in range(F)]).astype(np.float64), axis=1)
            sxy, sxx, syy = np.mean(np.conj(X) * Y, axis=0), np.mean(np.abs(X)**2, axis=0), np.mean(np.abs(Y)**2, axis=0)
            tol = TOL if F >= 5 else 3e-5  # (one to three frames: nothing averages the fp32 transform rounding down)
            assert relmax(tf[:, c], sxy / sxx) < tol, (F, c)
            assert relmax(coh[:, c], np.abs(sxy)**2 / sxx / syy) < tol, (F, c)


def test_deconvolve_persistent_kernel_edges():
    """deconv8k::k_deconv_p through ds_deconv_dev: more units than the 2 x CUs workgroups of the persistent grid (every
    workgroup takes a second unit: the prefetch and the zero-record descriptor past the last one), an odd channel count (the
    last pair has one channel), inputs shorter than the transform (zero padded by the range check) and fewer output samples
    than the transform; against numpy in float64.  Also the one-item call (a grid of one)."""
    import ctypes as C
    from dsptoolbox_amd._lib import DeviceBuffer, get_context
    ctx = get_context()
    rng = np.random.default_rng(8192)
    n_fft = 8192
    r = (rng.standard_normal(n_fft // 2 + 1) + 1j * rng.standard_normal(n_fft // 2 + 1)).astype(np.complex64)
    r *= np.exp(-np.arange(n_fft // 2 + 1) / 2000.0).astype(np.float32)
    rr = r.astype(np.complex128)
    d_r = DeviceBuffer.from_array(ctx, r)
    for items, n_ch, n, n_out in ((150, 5, 5000, 6000), (1, 2, 8192, 8192), (260, 4, 8192, 8192), (3, 1, 100, 8192)):
        y = (rng.standard_normal((items, n_ch, n)) * 0.1).astype(np.float32)
        d_y = DeviceBuffer.from_array(ctx, y)
        d_o = DeviceBuffer(ctx, items * n_ch * n_out * 4)
        ctx.routes()
        ctx.check(ctx.lib.ds_deconv_dev(ctx.handle, C.c_void_p(d_y.ptr), items, n_ch, n, n, n_fft, C.c_void_p(d_r.ptr), 0, n_out,
                                        n_out, C.c_void_p(d_o.ptr)), "ds_deconv_dev")
        assert {"deconv_rperm", "deconv@8k_persist"} <= ctx.routes()
        got = d_o.to_array((items, n_ch, n_out), np.float32)
        ref = np.fft.irfft(np.fft.rfft(y.astype(np.float64), n_fft, axis=-1) * rr, n_fft, axis=-1)[..., :n_out]
        assert relmax(got, ref) < TOL, (items, n_ch, n, n_out, relmax(got, ref))
        for d in (d_y, d_o):
            d.free()
    d_r.free()


def test_device_resident_spectrogram_features():
    """log_mel_spectrogram / mfcc / chroma_stft of a device-resident signal read its samples in place and give the host path's
    numbers (same kernels: identical), without materialising time_data."""
    rng = np.random.default_rng(77)
    x = rng.standard_normal((30000, 2)) * 0.2
    sh = dsp.Signal(None, x.copy(), 48000)
    sd = dsp.Signal.from_planar_f32(backend._planar_f32(x), 48000)
    for s in (sh, sd):
        s.set_spectrogram_parameters(window_length_samples=1024)
    th, fh, mh = dsp.transforms.log_mel_spectrogram(sh, generate_plot=False)[:3]
    td, fd, md = dsp.transforms.log_mel_spectrogram(sd, generate_plot=False)[:3]
    assert np.array_equal(mh, md) and np.array_equal(th, td) and not sd._has_host_copy
    ch = dsp.transforms.chroma_stft(sh, plot_channel=-1)
    cd = dsp.transforms.chroma_stft(sd, plot_channel=-1)
    assert np.array_equal(ch[1], cd[1]) and np.array_equal(ch[2], cd[2])
    assert not sd._has_host_copy
