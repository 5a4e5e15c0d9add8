"""Latency estimation without a device: the restatement of tests/latency_oracle.py reproduces the reference's results
of tests/golden/latency/cases.npz (integer lags exactly, floats to 1e-12) and the conditions the generator asserted
hold in the fixture; the host root finder follows the reference's branches, warnings included; delay; the assertions,
the guards and the entries' declarations."""

import os
import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import SIGNATURES
import latency_cases as lc
import latency_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
POS = [p for p in lc.POINTS if p > 0]


def sig_of(x, fs=lc.FS):
    return dsp.Signal(None, x.copy(), fs, constrain_amplitude=False)


def ir_of(x, fs=lc.FS):
    return dsp.ImpulseResponse(None, x.copy(), fs, constrain_amplitude=False)


def grid(key, z):
    n, step, last = z[key + "_f"]
    return np.arange(int(n)) * step


@pytest.mark.parametrize("name", list(lc.CASES))
def test_oracle_reproduces_the_reference(name):
    z, meta = lc.golden()
    in1, in2 = lc.pair_of(z, name)
    assert (in2 is None) == bool(lc.CASES[name].get("self")) and meta["signals"][name] == lc.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # condition (c)
        for p in lc.POINTS:
            lags, corr = orc.latency(in1, in2, p)
            ref = z[f"{name}_p{p}_lags"]
            if p == 0:
                assert lags.dtype.kind == "i" and ref.dtype.kind == "i" and np.array_equal(lags, ref)
            else:
                assert np.abs(lags - ref).max() <= 1e-12
            assert np.abs(corr - z[f"{name}_p{p}_corr"]).max() <= 1e-12
            info = meta["latency"][name][str(p)]
            assert info["runner_up"] <= 1 - 1e-6  # (a)
            if p > 0:
                assert info["h_floor"] >= 1e-6  # (b)
                _, d, lo, h = orc.fractional_peak(orc.xcorr(in1, in2), p, detail=True)
                assert (lo, h.shape[0], list(d)) == (info["lo"], info["m"], info["peaks"])
                assert np.abs(orc.neighbourhood(h, d - lo, p) - z[f"{name}_p{p}_near"]).max() <= 1e-12 * z[f"{name}_p{p}_hmax"]


def test_reversed_order_without_a_second_signal():
    """Channels delayed by 0, 3.3, 11.6 and 25.2 samples come back last first; the coefficients pair entry j with
    channel j + 1."""
    z, _ = lc.golden()
    assert list(z["c8_p0_lags"]) == [25, 12, 3]
    assert list(z["c8two_p0_lags"]) == [12]
    corr = z["c8_p0_corr"]
    assert abs(corr[1]) > 0.5 and abs(corr[0]) < 0.2 and abs(corr[2]) < 0.2  # only the middle entry meets its own channel


@pytest.mark.parametrize("name", list(lc.IRS))
def test_oracle_reproduces_the_impulse_response_cases(name):
    z, meta = lc.golden()
    x, e = z[name], meta["ir"][name]
    assert e["step_gap"] > 1e-3  # (d)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.abs(orc.find_ir_latency(x, True) - z[e["find_min"]]).max() <= 1e-12
        assert np.abs(orc.find_ir_latency(x, False) - z[e["find_peak"]]).max() <= 1e-12
        n_pad = 1.0 / grid(e["gd"], z)[1]  # N_padded / fs
        f, gd = orc.group_delay_latency_free(x, lc.FS)
        assert np.allclose(f, grid(e["gd"], z), rtol=1e-9) and np.abs(gd - z[e["gd"]]).max() <= 1e-12 * n_pad
        for key, analytic in ((e["egd"], False), (e["egd_analytic"], True)):
            f, gd = orc.excess_group_delay_latency_free(x, lc.FS, analytic)
            assert np.allclose(f, grid(key, z), rtol=1e-9) and np.abs(gd - z[key]).max() <= 1e-12 * n_pad


# ---- the host root finder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_root_finder_on_the_golden_neighbourhoods(name):
    z, meta = lc.golden()
    n1 = z[name + "_in1"].shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for p in POS:
            info = meta["latency"][name][str(p)]
            rows = backend.fractional_peak_rows(np.array(info["peaks"]), (info["lo"], info["m"]), z[f"{name}_p{p}_near"], p)
            assert np.array_equal(n1 - rows - 1, z[f"{name}_p{p}_lags"])


def both(near, p, d=10):
    """(value, warning texts) of the host function and of the oracle on a column that holds `near` around row d."""
    col = np.zeros(d + p + 8)
    col[d - p:d + p + 2] = near
    got = []
    for fn in (lambda: backend._fractional_index(near, p, d, 3), lambda: orc.root_of(col, d, p, 3)):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got.append((fn(), [str(x.message) for x in w]))
    return got


def test_root_finder_branches():
    # the values at d and d + 1 agree in sign, those at d - 1 and d do not: one row back, root between them
    (v, w), ref = both(np.array([-1.0, 0.5, 2.0, 3.0]), 1)
    assert (v, w) == ref and w == [] and v == pytest.approx(9 + 2 / 3, abs=1e-12)
    # still the same sign one row back: the integer row, with the reference's warning
    (v, w), ref = both(np.array([1.0, 2.0, 3.0, 4.0]), 1)
    assert (v, w) == ref and v == 10.0 and w == ["Fractional latency detection failed for channel 3. Integer latency is returned"]
    # no root in [0, 1]: both values are zero, the fitted polynomial vanishes and has no roots
    (v, w), ref = both(np.array([1.0, 0.0, 0.0, 1.0]), 1)
    assert (v, w) == ref and v == 10.0 and len(w) == 1 and "failed for channel 3" in w[0]
    # three points a side, no move: the quintic through the six values
    near = np.array([5.0, 3.5, 2.0, 0.4, -1.0, -2.2, -3.0, -3.5])
    (v, w), ref = both(near, 3)
    assert (v, w) == ref and w == [] and 10.0 < v < 11.0
    # a needed value that is not there: the peak is too close to an end of the array
    for near in (np.array([np.nan, 1.0, -1.0, 2.0]), np.array([1.0, -2.0, 3.0, np.nan])):
        with pytest.raises(ValueError, match="within 3 rows of an end"):
            backend._fractional_index(np.r_[np.nan, near, np.nan], 2, 10)
    assert backend._fractional_index(np.array([np.nan, 1.0, -1.0, np.nan]), 1, 10) == 10.5  # the two outer ones are not needed
    with pytest.raises(ValueError, match="end of the array"):
        backend._fractional_index(np.array([1.0, 1.0, np.nan, np.nan]), 1, 10)


# ---- delay -----------------------------------------------------------------------------------------------------------
def test_delay_matches_the_reference():
    z, meta = lc.golden()
    x = z["c1_in1"]
    assert len(meta["delay"]) == 4
    for case in meta["delay"]:
        sig = sig_of(x)
        out = dsp.delay(sig, case["delay_samples"], channels=case["channels"], keep_length=case["keep_length"])
        assert type(out) is dsp.Signal and out is not sig and np.array_equal(out.time_data, z[case["out"]]), case
        assert np.array_equal(sig.time_data, x)
    assert np.array_equal(z["delay_0"], x) and z["delay_1"].shape == (107, 3) and z["delay_2"].shape == (100, 3)
    assert np.array_equal(z["delay_1"][:100, 0], x[:, 0]) and np.all(z["delay_1"][100:, 0] == 0)  # padded at the end
    mb = dsp.delay(dsp.MultiBandSignal([sig_of(x), sig_of(2 * x)]), 7, channels=[1])
    assert type(mb) is dsp.MultiBandSignal and np.array_equal(mb.bands[0].time_data, z["delay_1"])
    assert np.array_equal(mb.bands[1].time_data, 2 * z["delay_1"])
    with pytest.raises(AssertionError, match="Delay too large"):
        dsp.delay(sig_of(x), 100, keep_length=True)
    with pytest.raises(AssertionError, match="invalid channel"):
        dsp.delay(sig_of(x), 3, channels=[0, 3])
    with pytest.raises(TypeError):
        dsp.delay(x, 3)
    assert dsp.delay is dsp.standard.delay and dsp.latency is dsp.standard.latency
    assert {"latency", "delay", "fractional_delay"} <= set(dsp.__all__) and "find_ir_latency" in dsp.transfer_functions.__all__


# ---- declarations, assertions and guards -------------------------------------------------------------------------------
def test_entries_are_declared():
    header = open(os.path.join(HERE, "..", "include", "dsptoolbox_amd.h")).read()
    for name, n_args in (("ds_latency", 13), ("ds_lag_pearson", 10), ("ds_group_delay_phase_lat", 8)):
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == n_args
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == n_args
    text = open(os.path.join(HERE, "..", "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert "kLatencyMaxPoints = 16;" in text and backend.LATENCY_MAX_POINTS == 16
    assert "kLatencyMaxColumns = 65535;" in text and backend.LATENCY_MAX_COLUMNS == 65535
    assert backend.LATENCY_MAX_ROWS == backend.FFT64_MAX_POW2 == 1 << 22 and "rows > kFft64MaxPow2" in text


def test_assertions_of_latency():
    x = np.random.default_rng(0).standard_normal((64, 2))
    with pytest.raises(AssertionError, match="Sampling rates must match"):
        dsp.latency(sig_of(x), sig_of(x, 44100))
    with pytest.raises(AssertionError, match="Number of channels"):
        dsp.latency(sig_of(x), sig_of(x[:, :1]))
    with pytest.raises(AssertionError, match="at least 2 channels"):
        dsp.latency(sig_of(x[:, :1]))
    with pytest.raises(AssertionError, match="Polynomial points"):
        dsp.latency(sig_of(x), sig_of(x), polynomial_points=-1)
    with pytest.raises(AssertionError, match="type Signal"):
        dsp.latency(sig_of(x), dsp.MultiBandSignal([sig_of(x)]))
    with pytest.raises(TypeError):
        dsp.latency(x, x)
    with pytest.raises(AssertionError, match="only valid for an impulse response"):
        dsp.transfer_functions.find_ir_latency(sig_of(x))
    with pytest.raises(AssertionError, match="only valid for an impulse response"):
        dsp.transfer_functions._group_delay(sig_of(x), analytic_computation=False, remove_ir_latency=True)
    # the public numerical form with remove_ir_latency keeps its refusal; the computation is _group_delay's
    for call in (lambda: dsp.transfer_functions.group_delay(ir_of(x), analytic_computation=False, remove_ir_latency=True),
                 lambda: dsp.transfer_functions.excess_group_delay(ir_of(x), remove_ir_latency=True)):
        with pytest.raises(NotImplementedError, match="not built"):
            call()


def test_non_finite_samples_and_bounds_are_refused_on_the_host():
    x = np.random.default_rng(1).standard_normal((64, 2))
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[17, 1] = bad
        for call in (lambda: dsp.latency(sig_of(y), sig_of(x)), lambda: dsp.latency(sig_of(x), sig_of(y), 2),
                     lambda: dsp.latency(sig_of(y)), lambda: dsp.transfer_functions.find_ir_latency(ir_of(y), False),
                     lambda: backend.lag_pearson(x, y, [1, 2])):
            with pytest.raises(ValueError, match="non-finite"):
                call()
    with pytest.raises(NotImplementedError, match="beyond the device kernels' bounds"):
        backend.latency_peaks(x, x, 17)
    big = np.zeros(((1 << 21) + 1, 1))
    big[5] = 1.0
    with pytest.raises(NotImplementedError, match="4194305 rows"):
        backend.latency_peaks(big, big, 0)
    with pytest.raises(ValueError, match="as many channels"):
        backend.latency_peaks(x, np.ones((64, 3)), 0)
    with pytest.raises(ValueError, match="second signal"):
        backend.latency_peaks(x, None, 1, pearson=True)
