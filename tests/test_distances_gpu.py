"""distances on the device: snr and si_sdr (csrc/kernels_dist.hpp through ds_pair_moments) and fw_snr_seg
(ds_fw_snr_seg: the complex recursion, the framing, the float64 transform per column, the reduction) against the long
double oracles within the bounds of ciir_cases.py; every function against the reference's golden values; clipping;
the chunked walk over the frames; resident signals; bit-identical repeats."""

import os

import numpy as np
import pytest

import ciir_cases as cc
import ciir_oracle as co
import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 8000
d = dsp.distances
SPECTRUM = dict(window_length_samples=256)


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "gammatone", "cases.npz"))


def sig(a, fs=FS):
    return dsp.Signal(None, np.array(a, dtype=np.float64), fs, constrain_amplitude=False)


# ---- snr, si_sdr --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.PAIR_JUDGED)
def test_snr_and_si_sdr_against_the_oracle(name):
    s, h = cc.pair_problem(name)
    for fn, out, ref in (("si_sdr", d.si_sdr(sig(s), sig(h)), co.si_sdr_ld(s, h)), ("snr", d.snr(sig(h), sig(s)), co.snr_ld(h, s))):
        assert out.shape == (h.shape[1],) and out.dtype == np.float64
        e, tol = float(np.max(np.abs(out - ref))), cc.pair_tolerance(name, fn)
        print(f"{name} {fn}: {e:.2e} dB (bound {tol:.2e})")
        assert e <= tol, (name, fn, e, tol)


def test_pair_sums_of_one_sample_and_repeats():
    s, h = cc.pair_problem("n1")
    m = backend.pair_moments(s, h)
    ref = np.stack([s[0] ** 2, h[0] ** 2, s[0] * h[0], s[0], h[0], h[0] ** 2], axis=1).astype(np.longdouble)
    e = float(np.max(np.abs(m - ref) / np.abs(ref)))
    print(f"the six sums of one sample: {e:.2e} relative")
    assert e <= 2 * cc.EPS  # (each is one rounded product)
    s, h = cc.pair_problem(f"n{cc.PAIR_SPAN + 1}")
    assert np.array_equal(backend.pair_moments(s, h), backend.pair_moments(s, h))


def test_golden_snr_si_sdr_and_spectral_distances():
    z = golden()
    x, xhat = z["x"].astype(np.float64), z["xhat"].astype(np.float64)
    for key, out in (("snr_33", d.snr(sig(x), sig(xhat))), ("snr_13", d.snr(sig(x), sig(xhat[:, :1]))),
                     ("si_sdr_33", d.si_sdr(sig(x), sig(xhat))), ("si_sdr_13", d.si_sdr(sig(x[:, :1]), sig(xhat)))):
        e = float(np.max(np.abs(out - z[key])))
        print(f"{key}: {e:.2e} dB from the reference")
        assert e <= 1e-11  # (700 terms in float64 on either side, si_sdr down to -60 dB)
    for name, fn in (("log_spectral", d.log_spectral), ("itakura_saito", d.itakura_saito)):
        for key, kw in (("33", dict(f_range_hz=[100, 3500])), ("raw", dict(f_range_hz=[100, 3500], energy_normalization=False))):
            out = fn(sig(x), sig(xhat), spectrum_parameters=SPECTRUM, **kw)
            e = float(np.max(np.abs(out / z[f"{name}_{key}"] - 1)))
            print(f"{name}_{key}: {e:.2e} relative to the reference")
            # a 700-sample signal takes the float64 Welch route, whose spectra are held to 1e-11 of a channel's rms
            # (x64_cases.CAP); the bins of this broadband input lie within 1e2 of it, and the integrand is smooth
            assert e <= 1e-9


def test_resident_signals_give_the_fp32_rounded_answer():
    s, h = cc.pair_problem("broadcast")
    s32, h32 = s.astype(np.float32).astype(np.float64), h.astype(np.float32).astype(np.float64)
    a, b = sig(s32).to_device(), sig(h32).to_device()
    assert a.on_device and b.on_device
    e = float(np.max(np.abs(d.si_sdr(a, b) - co.si_sdr_ld(s32, h32))))
    e = max(e, float(np.max(np.abs(d.snr(b, a) - co.snr_ld(h32, s32)))))
    print(f"resident snr / si_sdr: {e:.2e} dB")
    assert e <= cc.pair_tolerance("broadcast", "si_sdr") + cc.pair_tolerance("broadcast", "snr")


# ---- fw_snr_seg --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.FW))
def test_fw_snr_seg_against_the_oracle(name):
    x, xhat, _, value, _ = cc.fw_problem(name)
    out = cc.fw_call(name, x, xhat)
    assert out.shape == value.shape and out.dtype == np.float64
    e, tol = float(np.max(np.abs(out - value))), cc.fw_tolerance(name)
    print(f"{name}: {out} dB, {e:.2e} dB from the oracle (bound {tol:.2e})")
    assert e <= tol, (name, e, tol)


def test_fw_snr_seg_chunk_edge_inside_a_three_frame_call(monkeypatch):
    name = "fs8000_n601"  # three frames
    x, xhat, frames, value, _ = cc.fw_problem(name)
    assert len(frames[0]) == 3
    whole = cc.fw_call(name, x, xhat)
    for chunk in (1, 2):
        monkeypatch.setattr(backend, "FW_SNR_CHUNK_FRAMES", chunk)
        assert np.array_equal(cc.fw_call(name, x, xhat), whole), chunk
    assert abs(whole[0] - value[0]) <= cc.fw_tolerance(name)


def test_fw_snr_seg_identical_pair_clips_to_the_upper_limit():
    x = cc.fw_problem("fs8000_long")[0]
    out = d.fw_snr_seg(sig(x), sig(x * (1 + 1e-4)), f_range_hz=[100, 3500])
    print("x against x (1 + 1e-4):", out)
    assert np.array_equal(out, [35.0, 35.0])


def test_fw_snr_seg_golden_resident_and_repeats():
    z = golden()
    x, xhat = z["x"].astype(np.float64), z["xhat"].astype(np.float64)
    for key, a in (("fw_snr_seg_33", x), ("fw_snr_seg_13", x[:, :1])):
        out = d.fw_snr_seg(sig(a), sig(xhat), f_range_hz=[100, 3500])
        e = float(np.max(np.abs(out - z[key])))
        print(f"{key}: {out}, {e:.2e} dB from the reference")
        assert e <= 4 * cc.HOST_MARGIN * 1e-4  # (700 samples are three frames: the perturbed-oracle change of fs8000_n601, rounded up)
        assert np.array_equal(out, d.fw_snr_seg(sig(a), sig(xhat), f_range_hz=[100, 3500]))
    # the samples above are float32 values: resident signals hold them exactly
    res = d.fw_snr_seg(sig(x).to_device(), sig(xhat).to_device(), f_range_hz=[100, 3500])
    assert np.array_equal(res, d.fw_snr_seg(sig(x), sig(xhat), f_range_hz=[100, 3500]))
