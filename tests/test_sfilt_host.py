"""The structure filters on the CPU: the bounds of sfilt_cases.py measured again from the float64 emulation of the blocked
algorithm, what the bounds reject, the constants the cases mirror, the classes' constructors, assertions, conversions and
one-sample steps against the reference's golden vectors, every refusal, and the API surface."""

import json
import os
import re
import warnings

import numpy as np
import pytest
from scipy.signal import lfilter

import dsptoolbox_amd as dsp
import sfilt_cases as sc
import sfilt_oracle as so
from dsptoolbox_amd import backend
from dsptoolbox_amd.filterbanks import KautzFilter, LatticeLadderFilter, WarpedFIR, WarpedIIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sfilt", "cases.npz"))
    return z, json.loads(str(z["meta"]))


# ---- the cases and their bounds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_emulation_gives_the_recorded_bound(name):
    e = sc.error(name, *sc.emulate(name)) / sc.EPS
    rec = sc.SFILT_EMULATION[name]
    print(f"{name}: emulation {e:.3g} eps64 (recorded {rec:.3g}), bound {sc.tolerance(name):.2e}")
    assert rec / sc.HOST_MARGIN / 2 <= e <= rec * sc.HOST_MARGIN, (name, e, rec)
    assert sc.tolerance(name) <= 1e-6  # (a case that cannot meet the project's contract is not a valid case)


def test_every_case_is_a_structure_the_host_entry_accepts():
    assert set(sc.SFILT_EMULATION) == set(sc.CASES)
    for name, spec in sc.CASES.items():
        s = sc.structure(spec["kind"], spec["d"])
        limit = sc.MAX_GAIN_WARPED_IIR if spec["kind"] == "warped_iir" else sc.MAX_GAIN
        assert so.n_states(s) == spec["d"] <= sc.MAX_D and so.carry_gain(s) < limit / 2, name
        kind, coef, d, aux = sc.pack(s)
        assert d == spec["d"] and coef.dtype == np.float64 and coef.ndim == 1


@pytest.mark.parametrize("name", ["iir_lattice_d5_n4097", "sos_lattice_d64_n4097_zi", "warped_fir_d64_n4097_zi",
                                  "warped_iir_d5_n4097", "kautz_d64_n4097_zi", "fir_lattice_d64_n4097_zi"])
def test_bound_rejects_broken_carries(name):
    tol = sc.tolerance(name)
    off = sc.error(name, *sc.emulate(name, phi_power_offset=1))
    dropped = sc.error(name, *sc.emulate(name, drop_state=sc.CASES[name]["d"] // 2))
    print(f"{name}: Phi one power off {off:.2e}, a carried state dropped {dropped:.2e}, bound {tol:.2e}")
    assert off > 100 * tol and dropped > 100 * tol


def _constant(header, name, kind="int"):
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", header)).read()
    m = re.search(r"constexpr %s %s = ([^;]+);" % (kind, name), src)
    assert m, (header, name)
    return float(m.group(1))


def test_case_constants_match_the_sources():
    assert _constant("carry_tables.hpp", "L") == sc.L and _constant("carry_tables.hpp", "B") == sc.B
    assert _constant("kernels_sfilt.hpp", "MAX_D") == sc.MAX_D == backend.SFILT_MAX_STATES
    assert _constant("kernels_sfilt.hpp", "MAX_GAIN", "double") == sc.MAX_GAIN
    assert _constant("kernels_sfilt.hpp", "MAX_GAIN_WARPED_IIR", "double") == sc.MAX_GAIN_WARPED_IIR
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "kernels_sfilt.hpp")).read()
    kinds = re.search(r"enum Kind \{([^}]+)\}", src).group(1)
    for name, value in sc.KIND_ID.items():
        assert re.search(r"\b%s = %d\b" % (name.upper(), value), kinds), name
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    for name, value in sc.KIND_ID.items():
        assert re.search(r"#define DS_SFILT_%s %d\b" % (name.upper(), value), header), name


def test_the_step_functions_agree_with_scipy_where_scipy_has_the_filter():
    """A warped IIR filter at lambda = 0 is lfilter; so is an IIR lattice-ladder made from b, a."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 2))
    b, a = np.array([0.3, -0.2, 0.5, 0.1]), np.array([1.0, -0.9, 0.5, -0.1])
    want = lfilter(b, a, x, axis=0)
    s = dict(kind="warped_iir", lam=0.0, b=b, sigma=so.warped_sigmas(a, 0.0))
    assert so.stream_error(so.serial(s, x, dtype=np.float64)[0], want) < 1e-13
    lat = LatticeLadderFilter.from_filter(dsp.Filter.from_ba(b, a, 48000))
    assert so.stream_error(so.serial(dict(kind="iir_lattice", k=lat.k, c=lat.c), x, dtype=np.float64)[0], want) < 1e-13


# ---- the classes against the reference's golden vectors --------------------------------------------------------------
def _per_sample(f, x, set_channels=True):
    if set_channels:
        f.set_n_channels(x.shape[1])
    return np.array([[f.process_sample(x[n, c], c) for c in range(x.shape[1])] for n in range(len(x))])


def _lattice_filter(z, case, fs):
    name = case["name"]
    if case["filter"] == "sos":
        return dsp.Filter.from_sos(z[f"lat_{name}_sos"], fs)
    return dsp.Filter.from_ba(z[f"lat_{name}_b"], z[f"lat_{name}_a"], fs)


def test_lattice_from_filter_and_process_sample_match_the_reference(golden):
    z, meta = golden
    x, cut = z["x"].astype(np.float64), meta["cut"]
    for case in meta["lattice"]:
        name = case["name"]
        lat = LatticeLadderFilter.from_filter(_lattice_filter(z, case, meta["fs"]))
        np.testing.assert_allclose(lat.k, z[f"lat_{name}_k"], rtol=1e-12, atol=1e-15)
        if f"lat_{name}_c" in z:
            np.testing.assert_allclose(lat.c, z[f"lat_{name}_c"], rtol=1e-12, atol=1e-15)
            assert lat.iir_filter and lat.sos_filtering == (lat.k.ndim == 2)
        else:
            assert lat.c is None and not lat.iir_filter
        assert lat.state.shape == ((len(lat.k), 2, 1) if lat.sos_filtering else (len(lat.k), 1))
        y1 = _per_sample(lat, x[:cut])
        assert so.stream_error(y1, z[f"lat_{name}_y1"]) <= 1e-12 and lat.state.shape == z[f"lat_{name}_s1"].shape
        np.testing.assert_allclose(lat.state, z[f"lat_{name}_s1"], rtol=1e-10, atol=1e-13)
        y2 = _per_sample(lat, x[cut:], set_channels=False)  # (continues from the state the first part left)
        assert so.stream_error(y2, z[f"lat_{name}_y2"]) <= 1e-12
        np.testing.assert_allclose(lat.state, z[f"lat_{name}_s2"], rtol=1e-10, atol=1e-13)
        lat.reset_state()
        assert not lat.state.any()


def test_lattice_constructor_assertions():
    k1, k2 = np.array([0.5, -0.2]), np.array([[0.5, -0.2]])
    with pytest.raises(AssertionError, match="Sampling rate"):
        LatticeLadderFilter(k1)
    with pytest.raises(AssertionError, match="len\\(k_coefficients\\) \\+ 1"):
        LatticeLadderFilter(k1, np.ones(2), 48000)
    with pytest.raises(AssertionError, match="C coefficients cannot be None"):
        LatticeLadderFilter(k2, None, 48000)
    with pytest.raises(AssertionError, match="3 c coefficients"):
        LatticeLadderFilter(k2, np.ones((1, 2)), 48000)
    with pytest.raises(AssertionError, match="do not match"):
        LatticeLadderFilter(k2, np.ones((2, 3)), 48000)
    with pytest.raises(AssertionError, match="vector or a matrix"):
        LatticeLadderFilter(np.ones((1, 1, 1)), None, 48000)
    with pytest.raises(AssertionError, match="reflection coefficient"):  # a linear-phase FIR filter
        LatticeLadderFilter.from_filter(dsp.Filter.from_ba(np.array([1.0, 2.0, 1.0]), np.array([1.0]), 48000))
    with pytest.raises(AssertionError, match="At least one channel"):
        LatticeLadderFilter(k1, None, 48000).set_n_channels(0)


def test_warped_classes_match_the_reference(golden):
    z, meta = golden
    x = z["x"].astype(np.float64)
    for case in meta["warped"]:
        name, lam = case["name"], case["lam"]
        b = z[f"wrp_{name}_b"]
        if f"wrp_{name}_a" in z:
            a = z[f"wrp_{name}_a"]
            w = WarpedIIR(b, a, lam, meta["fs"])
            np.testing.assert_allclose(w.sigmas, z[f"wrp_{name}_sigmas"], rtol=1e-13)
            np.testing.assert_allclose(w.sigmas, so.warped_sigmas(a / a[0], lam), rtol=1e-13)
            assert w.N == max(len(a), len(b)) and w.a[0] == 1.0 and np.array_equal(w.b, b / a[0])
        else:
            w = WarpedFIR(b, lam, meta["fs"])
            assert w.N == len(b) and w.order == len(b) - 1
        assert w.buffer.shape == (w.N, 1)
        assert so.stream_error(_per_sample(w, x), z[f"wrp_{name}_y"]) <= 1e-12
        assert w.buffer.shape == (w.N, 2) and w.buffer.any()
        w.reset_state()
        assert not w.buffer.any()
    fir = dsp.Filter.from_ba(np.array([1.0, 0.5, 0.25]), np.array([1.0]), 48000)
    iir = dsp.Filter.from_ba(np.array([1.0, 0.5]), np.array([1.0, -0.5]), 48000)
    assert type(WarpedFIR.from_filter(fir, 0.3)) is WarpedFIR and type(WarpedIIR.from_filter(iir, 0.3)) is WarpedIIR
    with pytest.raises(AssertionError, match="FIR"):
        WarpedFIR.from_filter(iir, 0.3)
    with pytest.raises(AssertionError, match="IIR"):
        WarpedIIR.from_filter(fir, 0.3)
    with pytest.raises(AssertionError, match="Warping factor"):
        WarpedFIR(np.ones(3), 1.0, 48000)
    with pytest.raises(AssertionError, match="single dimension"):
        WarpedIIR(np.ones((2, 2)), np.ones(2), 0.3, 48000)


def test_warped_iir_without_warping_is_lfilter(golden):
    z, meta = golden
    x = z["x"].astype(np.float64)
    b, a = z["wrp_iir_zero_b"], z["wrp_iir_zero_a"]
    w = WarpedIIR(b, a, 0.0, meta["fs"])
    assert so.stream_error(_per_sample(w, x), lfilter(b, a, x, axis=0)) <= 1e-12
    assert so.stream_error(z["wrp_iir_zero_y"], lfilter(b, a, x, axis=0)) <= 1e-12
    np.testing.assert_allclose(np.sort_complex(w.poles()), np.sort_complex(np.roots(a)), rtol=1e-9)


def test_kautz_class_matches_the_reference(golden):
    z, meta = golden
    x = z["x"].astype(np.float64)
    kz = KautzFilter(z["kz_poles"], meta["fs"])
    assert (kz.n_real_poles, kz.n_complex_poles, kz.total_n_poles) == (2, 6, 8)
    assert np.array_equal(kz.coefficients_real_poles, np.ones(2)) and np.array_equal(kz.coefficients_complex_poles, np.ones(6))
    assert kz.set_filter_coefficients(z["kz_c_real"], z["kz_c_complex"]) is kz
    # (the reference runs one lfilter per tap and all-pass, this class one shared direct-form-II state per pole: rounding)
    assert so.stream_error(_per_sample(kz, x), z["kz_y"]) <= 1e-12
    kz.reset_state()
    assert so.stream_error(_per_sample(kz, x[:50]), z["kz_y"][:50]) <= 1e-12
    s = so.kautz_structure(z["kz_poles"], z["kz_c_real"], z["kz_c_complex"])
    assert np.array_equal(sc.pack(s)[1], kz._structure(z["kz_c_real"], z["kz_c_complex"])[1])
    with pytest.raises(AssertionError, match="negative imaginary"):
        KautzFilter(np.array([0.5 - 0.1j]), 48000)
    with pytest.raises(AssertionError, match="outside the unit circle"):
        KautzFilter(np.array([1.0 + 0j]), 48000)
    with pytest.raises(AssertionError):
        kz.set_filter_coefficients(np.ones(3), np.ones(6))


def test_kautz_pole_search_matches_the_reference(golden):
    from dsptoolbox_amd.classes.structure_filters import _optimal_poles
    z, _ = golden
    poles = _optimal_poles(6, 5, z["kz_ir"].squeeze().copy())
    want = np.concatenate([z["kz_from_ir_poles_real"], z["kz_from_ir_poles_complex"]])
    np.testing.assert_allclose(np.sort_complex(poles), np.sort_complex(want), rtol=1e-9)
    # the weights of the fit are the taps at the last sample of the reversed response: the oracle's final state gives them
    unit = so.kautz_structure(z["kz_poles"])
    taps = so.kautz_taps(unit, so.serial(unit, z["kz_ir"][::-1], dtype=np.float64)[1])[:, 0]
    np.testing.assert_allclose(taps, np.concatenate([z["kz_fit_real"], z["kz_fit_complex"]]), rtol=1e-9, atol=1e-13)


# ---- the refusals: each names its limit and none reaches the device -------------------------------------------------
def _signal(n_ch=1, n=64, fs=48000):
    return dsp.Signal(None, np.random.default_rng(0).standard_normal((n, n_ch)), fs, constrain_amplitude=False)


def test_refusals_name_their_limits(golden):
    z, meta = golden
    s = _signal()
    with pytest.raises(NotImplementedError, match="more than 64 states"):
        LatticeLadderFilter(np.full(65, 0.1), None, 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="more than 64 states"):
        WarpedFIR(np.ones(65), 0.5, 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="more than 64 states"):
        KautzFilter(0.5 * np.exp(1j * np.linspace(0.1, 3.0, 33)), 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="more than 64 states"):
        backend.sfilt_filter(np.ones((8, 1)), backend.SFILT_FIR_LATTICE, np.zeros(65), 65)
    unstable = LatticeLadderFilter(np.array([0.5, 1.0]), np.ones(3), 48000)
    with pytest.raises(NotImplementedError, match="\\|k\\| >= 1"):
        unstable.filter_signal(s)
    assert not unstable.state.any() and unstable.n_channels == 1  # (refused before any state is touched)
    with pytest.raises(NotImplementedError, match="\\|k\\| >= 1"):
        LatticeLadderFilter(np.array([[0.5, -1.5]]), np.ones((1, 3)), 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="outside the unit circle"):
        WarpedIIR(np.ones(2), np.array([1.0, -1.2]), 0.3, 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="outside the unit circle"):
        WarpedIIR(np.ones(2), np.array([1.0, -0.5]), 1.1, 48000).filter_signal(s)
    assert np.all(np.abs(WarpedIIR(z["wrp_iir_m876_b"], z["wrp_iir_m876_a"], -0.876, 48000).poles()) < 1)
    cs = dsp.Signal(None, np.ones((64, 1)) + 0.5j, 48000, constrain_amplitude=False)
    for f in (LatticeLadderFilter(np.array([0.5]), None, 48000), WarpedFIR(np.ones(3), 0.5, 48000),
              WarpedIIR(np.ones(2), np.array([1.0, -0.5]), 0.3, 48000), KautzFilter(np.array([0.5 + 0j]), 48000)):
        with pytest.raises(NotImplementedError, match="complex input"):
            f.filter_signal(cs)
        with pytest.raises(AssertionError, match="Sampling rates do not match"):
            f.filter_signal(_signal(fs=44100))
    with pytest.raises(NotImplementedError, match="complex coefficients"):
        LatticeLadderFilter(np.array([0.5 + 0.1j]), None, 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="complex coefficients"):
        WarpedFIR(np.array([1.0, 0.5j]), 0.5, 48000).filter_signal(s)
    with pytest.raises(NotImplementedError, match="complex input"):
        backend.sfilt_filter(np.ones((8, 1)) + 1j, backend.SFILT_FIR_LATTICE, np.zeros(2), 2)


def test_the_gain_limit_separates_the_golden_warped_filters(golden):
    """The Butterworth-8 warped IIR filter is accepted at lambda = 0.5 and 0 and refused at lambda = -0.876, where the
    carry gain is twice the limit (the refusal itself needs a context: tests/test_sfilt_gpu.py)."""
    z, meta = golden
    gains = {}
    for name, lam in (("iir_p50", 0.5), ("iir_zero", 0.0), ("iir_m876", -0.876)):
        w = WarpedIIR(z[f"wrp_{name}_b"], z[f"wrp_{name}_a"], lam, meta["fs"])
        _, coef, d, aux = w._structure()
        gains[name] = so.carry_gain(dict(kind="warped_iir", lam=lam, b=coef[1:1 + d], sigma=w.sigmas))
    print(gains)
    assert gains["iir_p50"] < 0.95 * sc.MAX_GAIN_WARPED_IIR and gains["iir_zero"] < 0.95 * sc.MAX_GAIN_WARPED_IIR
    assert gains["iir_m876"] > 1.5 * sc.MAX_GAIN_WARPED_IIR
    assert np.isinf(so.carry_gain(dict(kind="iir_lattice", k=np.array([0.5, 1.2]), c=np.ones(3)))) or \
        so.carry_gain(dict(kind="iir_lattice", k=np.array([0.5, 1.2]), c=np.ones(3))) > sc.MAX_GAIN


def test_a_coefficient_array_of_the_wrong_length_is_refused_before_the_entry_reads_it():
    for name in ("fir_lattice_d5_n1", "iir_lattice_d5_n1", "sos_lattice_d64_n4097_zi", "warped_fir_d5_n1", "warped_iir_d5_n1",
                 "kautz_d5_n1", "kautz_d64_n4097_zi"):
        spec = sc.CASES[name]
        kind, coef, d, aux = sc.pack(sc.structure(spec["kind"], spec["d"]))
        assert coef.shape == (backend.sfilt_coef_count(kind, d, aux),)
        for wrong in (coef[:-1], np.concatenate([coef, [0.0]])):
            with pytest.raises(AssertionError, match="packed coefficients"):
                backend.sfilt_filter(np.ones((8, 1)), kind, wrong, d, aux)
    with pytest.raises(AssertionError, match="kind or state counts"):
        backend.sfilt_filter(np.ones((8, 1)), 6, np.zeros(2), 2)
    with pytest.raises(AssertionError, match="kind or state counts"):
        backend.sfilt_filter(np.ones((8, 1)), backend.SFILT_KAUTZ, np.zeros(6), 2, 3)
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "kernels_sfilt.hpp")).read()
    body = re.search(r"inline int coef_count\(int kind, int d, int aux\) \{(.*?)\n\}", src, re.S).group(1)
    for text in ("return d;", "return 2 * d + 1;", "return 5 * (d / 2);", "return 1 + d;", "return 1 + d + aux + 1;",
                 "return 3 * aux + 6 * ((d - aux) / 2);"):
        assert text in body  # (backend.sfilt_coef_count restates these)


def test_api_surface():
    assert {"LatticeLadderFilter", "WarpedFIR", "WarpedIIR", "KautzFilter"} <= set(dsp.filterbanks.__all__)
    from dsptoolbox_amd._lib import SIGNATURES
    from dsptoolbox_amd import _build
    assert {"ds_sfilt", "ds_sfilt_dev"} <= set(SIGNATURES)
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    assert re.search(r"\bint ds_sfilt\(", header) and re.search(r"\bint ds_sfilt_dev\(", header)
    assert {"k_sfilt_group", "k_block_carry", "k_sfilt_apply"} <= set(_build.NO_SCRATCH)
    assert callable(backend.sfilt_filter) and callable(backend.sfilt_filter_device)
    from dsptoolbox_amd.classes.fir_filter_realtime import RealtimeFilter
    for cls in (LatticeLadderFilter, WarpedFIR, WarpedIIR, KautzFilter):
        assert issubclass(cls, RealtimeFilter)
        for method in ("process_sample", "reset_state", "set_n_channels", "filter_signal"):
            assert callable(getattr(cls, method))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert issubclass(WarpedIIR, WarpedFIR)
