"""The direct sums without a GPU: numpy restatements of the reference's dft, window_frequency_dependent and
complex_smoothing (the direct sums in the reference's own statements; the smoothing bands from the package's host
index code, which is judged with them) are held to every case of tests/golden/direct/cases.npz within 5e-13 of the
channel's largest magnitude; a long-double DFT with exactly reduced phase agrees with the reference's outputs within
1e-11; dropping the window terms below 2^-70 changes a windowed sum by less than 1e-15; the new names exist and the work
bounds of the Python side are the header's."""

import json
import os
import re

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._build import LIB_PATH
from test_smoothing_host import channel_error

HERE = os.path.dirname(os.path.abspath(__file__))
FS = 48000
LONG_SEED = 65536
_GOLDEN = None


def golden():
    """(arrays, meta) of tests/golden/direct/cases.npz, loaded once; the signals widened to float64 and the 65536-sample
    one rebuilt from its seed as tools/gen_golden_direct.py builds it."""
    global _GOLDEN
    if _GOLDEN is None:
        f = np.load(os.path.join(HERE, "golden", "direct", "cases.npz"))
        z = {k: f[k] for k in f.files if k != "meta"}
        for k in z:
            if z[k].dtype == np.float32:
                z[k] = z[k].astype(np.float64)
        x = np.random.default_rng(LONG_SEED).standard_normal((65536, 1)) * np.exp(-np.arange(65536) / 9000.0)[:, None]
        x = x.astype(np.float32).astype(np.float64)
        assert np.array_equal(np.concatenate([x[:16, 0], [x.sum()]]), z["sig65536_probe"]), "the seeded signal changed"
        z["sig65536"] = x
        _GOLDEN = (z, json.loads(str(f["meta"])))
    return _GOLDEN


# ---- restatements ---------------------------------------------------------------------------------------------------
def ref_dft(x, freqs_hz, fs):
    """transforms.dft (transforms/transforms.py:1315-1327 and _dft_backend)."""
    time_data = x.astype(np.complex128, order="C")
    f_normalized = (freqs_hz * (time_data.shape[0] / fs)).astype(np.complex128)
    dft_factor = (-2j * np.pi * np.linspace(0.0, 1.0, time_data.shape[0], endpoint=False)).astype(np.complex128)
    return np.stack([np.exp(dft_factor * fn) @ time_data for fn in f_normalized]) if len(freqs_hz) else \
        np.zeros((0, x.shape[1]), dtype=np.complex128)


def ref_windowed_sum(x, f, fs, alpha, peak, half, kept_distance=None):
    """_fdw_backend on the reference's arrays; kept_distance [F]: terms further from the peak are dropped."""
    length, n_ch = x.shape
    n = np.zeros_like(x)
    for ch in range(n_ch):
        n[:, ch] = np.arange(-peak[ch], length - peak[ch])
    dist = np.abs(n)
    n = (-0.5 * (n / half) ** 2.0).astype(np.complex128)
    alpha = np.asarray(alpha).astype(np.complex128)
    freqs_normalized = (f * (length / fs)).astype(np.complex128)
    dft_factor = np.repeat(-2j * np.pi * np.linspace(0.0, 1.0, length, endpoint=False)[..., None], repeats=n_ch,
                           axis=1).astype(np.complex128)
    time_data = x.astype(np.complex128)
    spec = np.zeros((len(f), n_ch), dtype=np.complex128)
    for ind in range(len(f)):
        terms = np.exp(dft_factor * freqs_normalized[ind] + alpha[ind] * n) * time_data
        if kept_distance is not None:
            terms = np.where(dist <= kept_distance[ind], terms, 0.0)
        spec[ind, :] = np.sum(terms, axis=0)
    return spec


def ref_fdw_parameters(x, fs, cycles, end_db):
    """transfer_functions.py:1335-1358."""
    end_window_value = 10 ** (end_db / 20.0)
    f = np.fft.rfftfreq(x.shape[0], 1 / fs)[1:]
    cycles_per_freq_samples = np.round(fs / f * cycles).astype(int)
    half = (x.shape[0] - 1) / 2
    alpha_factor = np.log(1 / (end_window_value) ** 2) ** 0.5 * half
    ind_max = np.argmax(np.abs(x), axis=0)
    alpha = (alpha_factor / cycles_per_freq_samples) ** 2.0
    return f, alpha, ind_max, half


def ref_fdw(x, fs, cycles, end_db, drop_below_log2=None):
    f, alpha, peak, half = ref_fdw_parameters(x, fs, cycles, end_db)
    kept = None if drop_below_log2 is None else backend._windowed_kept_distance(alpha, half, len(x), drop_below_log2)
    return np.pad(ref_windowed_sum(x, f, fs, alpha, peak, half, kept), ((1, 0), (0, 0)))


def ref_band_sums(spectrum, freqs, octave_fraction, window_y):
    """_complex_smoothing_backend with the bands of backend._csmooth_indices."""
    window_x = np.linspace(-1.0, 1.0, len(window_y), endpoint=True)
    ind_low, ind_high, window_length, passed = backend._csmooth_indices(freqs, octave_fraction)
    out = np.zeros_like(spectrum)
    for i in range(len(spectrum)):
        if passed[i]:
            out[i] = spectrum[i]
            continue
        window = np.interp(np.logspace(np.log10(3.0), np.log10(1.0), window_length[i])[:ind_high[i] - ind_low[i]] - 2.0,
                           window_x, window_y).astype(np.complex128)
        window /= window.sum()
        out[i] = window @ spectrum[ind_low[i]:ind_high[i]]
    return out


def ref_csmooth(sp, f, octave_fraction, domain, window_y):
    """transfer_functions.complex_smoothing from the spectrum on (transfer_functions.py:1827-1875)."""
    sp = np.asarray(sp, dtype=np.complex128)
    bs = lambda v: ref_band_sums(np.asarray(v, dtype=np.complex128), f, octave_fraction, window_y)  # noqa: E731
    if domain == "RealImaginary":
        return bs(sp)
    if domain == "MagnitudePhase":
        o = bs(np.abs(sp) + 1j * np.unwrap(np.angle(sp), axis=0))
        return np.real(o) * np.exp(1j * np.imag(o))
    if domain == "PowerPhase":
        o = bs(np.abs(sp) ** 2.0 + 1j * np.unwrap(np.angle(sp), axis=0))
        return np.real(o) ** 0.5 * np.exp(1j * np.imag(o))
    if domain == "Power":
        return np.real(bs(np.abs(sp) ** 2.0)) ** 0.5 * np.exp(1j * np.angle(sp))
    if domain == "Magnitude":
        return np.real(bs(np.abs(sp))) * np.exp(1j * np.angle(sp))
    assert domain == "EquivalentComplex"
    return np.real(bs(np.abs(sp) ** 2.0)) ** 0.5 * np.exp(1j * np.angle(bs(sp)))


def longdouble_dft(x, freqs_hz, fs):
    """The sum in long double: the phase f n / fs is reduced to (-1/2, 1/2] turns exactly (f / fs first, then the
    product), so its error does not grow with n beyond the product's one rounding at 2^-64."""
    ld = np.longdouble
    n = np.arange(x.shape[0], dtype=ld)
    xl = x.astype(ld)
    out = np.empty((len(freqs_hz), x.shape[1]), dtype=np.complex128)
    for k, f in enumerate(freqs_hz):
        r = ld(f) / ld(fs)
        t = (r - np.rint(r)) * n
        ang = (t - np.rint(t)) * (-2 * _PI_LD)
        out[k] = ((np.cos(ang)[:, None] * xl).sum(axis=0)).astype(np.float64) \
            + 1j * ((np.sin(ang)[:, None] * xl).sum(axis=0)).astype(np.float64)
    return out


_PI_LD = np.longdouble(4) * np.arctan(np.longdouble(1))
WINDOWS = {"Hann": dsp.Window.Hann, "Hamming": dsp.Window.Hamming}


def window_values(name):
    return WINDOWS[name](3000, True).astype(np.float64)


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_new_names_exist():
    assert callable(dsp.transforms.dft) and "dft" in dsp.transforms.__all__
    tf = dsp.transfer_functions
    assert callable(tf.window_frequency_dependent) and callable(tf.complex_smoothing)
    assert [m.name for m in tf.SmoothingDomain] == ["RealImaginary", "PowerPhase", "MagnitudePhase", "Power", "Magnitude",
                                                    "EquivalentComplex"]
    assert dsp.SmoothingDomain is tf.SmoothingDomain
    assert tuple(m.name for m in tf.SmoothingDomain) == backend.SMOOTHING_DOMAINS
    header = open(os.path.join(HERE, "..", "include", "dsptoolbox_amd.h")).read()
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", header))
    assert {"ds_dft", "ds_dft_dev", "ds_complex_smooth"} <= declared
    for code, name in enumerate(("REAL_IMAGINARY", "POWER_PHASE", "MAGNITUDE_PHASE", "POWER", "MAGNITUDE",
                                 "EQUIVALENT_COMPLEX")):
        assert re.search(rf"#define DS_SMOOTH_{name}\s+{code}\b", header)
    if os.path.exists(LIB_PATH):
        from dsptoolbox_amd._lib import load_library
        lib = load_library()
        for name in ("ds_dft", "ds_dft_dev", "ds_complex_smooth"):
            assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_dft_restatement_matches_the_reference():
    z, meta = golden()
    for i, case in enumerate(meta["dft"]):
        ref = z[f"dft_{i}_out"]
        out = ref_dft(z[case["sig"]], z["dft_freqs"], FS)
        assert out.shape == ref.shape
        e = channel_error(out, ref)
        print(f"dft {case['sig']}: restatement {e:.2e}")
        assert e <= 5e-13, (case, e)


def test_long_double_dft_agrees_with_the_reference():
    z, meta = golden()
    for i, case in enumerate(meta["dft"]):
        e = channel_error(longdouble_dft(z[case["sig"]], z["dft_freqs"], FS), z[f"dft_{i}_out"])
        print(f"dft {case['sig']}: reference against long double {e:.2e}")
        assert e <= 1e-11, (case, e)


def test_windowed_restatement_and_skip_rule():
    z, meta = golden()
    for i, case in enumerate(meta["fdw"]):
        x, ref = z[case["sig"]], z[f"fdw_{i}_out"]
        full = ref_fdw(x, FS, case["cycles"], case["end_db"])
        assert full.shape == ref.shape
        e = channel_error(full, ref)
        skipped = ref_fdw(x, FS, case["cycles"], case["end_db"], backend.DFT_MIN_WEIGHT_LOG2)
        d = channel_error(skipped, full)
        f, alpha, peak, half = ref_fdw_parameters(x, FS, case["cycles"], case["end_db"])
        share = backend._windowed_kept_terms(alpha, peak, half, len(x)) / (len(f) * x.size)
        print(f"fdw {case}: restatement {e:.2e}, skip changes {d:.2e}, {100 * share:.1f} % of the terms kept")
        assert e <= 5e-13, (case, e)
        assert d < 1e-15, (case, d)


def test_windowed_parameters_are_the_reference_statements():
    z, meta = golden()
    for case in meta["fdw"]:
        x = z[case["sig"]]
        got = dsp.transfer_functions._fdw_parameters(x, FS, case["cycles"], case["end_db"])
        for a, b in zip(got, ref_fdw_parameters(x, FS, case["cycles"], case["end_db"])):
            np.testing.assert_array_equal(a, b)
    # the skip distance: the weight at it reaches 2^-70, one sample further it does not
    f, alpha, peak, half = ref_fdw_parameters(z["ir4097"], FS, 5, -50.0)
    d = backend._windowed_kept_distance(alpha, half, 4097).astype(np.float64)
    inside = d < 4097
    assert inside.any() and (~inside).any()
    assert np.all(np.exp((alpha * (-0.5 * (d / half) ** 2))[inside]) >= 2.0 ** -70 * (1 - 1e-9))
    assert np.all(np.exp((alpha * (-0.5 * ((d + 1) / half) ** 2))[inside]) < 2.0 ** -70)
    with pytest.raises(ValueError, match="zero samples"):
        dsp.transfer_functions._fdw_parameters(z["ir1000"], FS, 0.2, -50.0)


def test_smoothing_restatement_matches_the_reference():
    z, meta = golden()
    worst = 0.0
    for i, case in enumerate(meta["smooth"]):
        name = case["sig"]
        out = ref_csmooth(z[f"{name}_spectrum"], z[f"{name}_freqs"], case["fraction"], case["domain"],
                          window_values(case["window"]))
        e = channel_error(out, z[f"smooth_{i}_out"])
        worst = max(worst, e)
        assert e <= 5e-13, (case, e)
    print(f"complex smoothing restatement: worst {worst:.2e}")


def test_band_indices():
    f = np.fft.rfftfreq(1000, 1 / FS)
    lo, hi, wlen, passed = backend._csmooth_indices(f, 3)
    assert lo.dtype == hi.dtype == wlen.dtype == passed.dtype == np.int32
    factor = 2.0 ** (1.0 / 3 / 2.0)
    for i in (0, 1, 2, 7, 100, 499, 500):  # the scalar statements of the reference
        a = i - int((f[i] - f[i] / factor) / (f[1] - f[0]) + 0.5)
        b = i + int((f[i] * factor - f[i]) / (f[1] - f[0]) + 0.5) + 1
        assert wlen[i] == b - a and lo[i] == max(a, 0) and hi[i] == min(b, len(f))
        assert bool(passed[i]) == (max(a, 0) + 2 >= min(b, len(f)))
    assert passed[0] and passed[1] and not passed[-1] and hi[-1] == len(f) and wlen[-1] > hi[-1] - lo[-1]


def test_work_bound_guards():
    z, meta = golden()
    backend._dft_guard(45.0 * 65536 * 1)
    backend._dft_guard(1024.0 * 2 ** 20 * 8)      # the largest shape the timing tool runs
    backend._dft_guard(32768.0 * 65536 * 8, True)  # ... and its windowed one with nothing skipped
    backend._csmooth_guard(65537.0 ** 2 * 0.24 / 2 * 8)
    with pytest.raises(NotImplementedError, match="work bound"):
        backend._dft_guard(2.0 ** 40 * 2.0 ** 24)
    with pytest.raises(NotImplementedError, match="work bound"):
        backend._dft_guard(2.0 ** 40, True)
    with pytest.raises(NotImplementedError, match="work bound"):
        backend._csmooth_guard(2.0 ** 40)
    text = open(os.path.join(HERE, "..", "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    for name, value in (("kDftMaxWork", backend.DFT_MAX_WORK), ("kDftWindowedMaxWork", backend.DFT_WINDOWED_MAX_WORK),
                        ("kCsmoothMaxWork", backend.CSMOOTH_MAX_WORK)):
        assert f"{name} = {value:.0e}".replace("e+", "e") in text


def test_arguments_are_checked_before_the_device():
    ir = dsp.ImpulseResponse(None, np.eye(64)[:, :1] + 0.0, FS)
    with pytest.raises(AssertionError, match="only valid for an impulse response"):
        dsp.transfer_functions.window_frequency_dependent(dsp.Signal(None, np.ones((64, 1)), FS), 5)
    with pytest.raises(AssertionError, match="less than 0 dB"):
        dsp.transfer_functions.window_frequency_dependent(ir, 5, 0.0)
    with pytest.raises(ValueError, match="zero samples"):
        dsp.transfer_functions.window_frequency_dependent(ir, 0.2)
    with pytest.raises(AssertionError, match="greater than 0"):
        dsp.transfer_functions.complex_smoothing(ir, 0.0, dsp.SmoothingDomain.Power)
    with pytest.raises(ValueError, match="Invalid smoothing domain"):
        dsp.transfer_functions.complex_smoothing(ir, 3.0, "Loudness")
    with pytest.raises(ValueError, match="Invalid smoothing domain"):
        backend.complex_smoothing(np.ones((8, 1), dtype=complex), np.arange(8.0), 3, "Loudness", np.ones(3000))
