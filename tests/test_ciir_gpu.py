"""The complex-coefficient recursion on the device (csrc/kernels_ciir.hpp through ds_iir_sos_c128): every case of
ciir_cases.py against the clongdouble oracle within the case's bound (block, group and section edges; final states from
the lane that holds the last sample), successive calls with state against one call over the joined signal, bit-identical
repeats, the guards, and the reference's golden vectors through Filter and FilterBank."""

import ctypes as C
import os
import warnings

import numpy as np
import pytest

import ciir_cases as cc
import ciir_oracle as co
import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DeviceError, get_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 8000


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "gammatone", "cases.npz"))


def run(name):
    x, zi, _, _ = cc.recursion_problem(name)
    sos = list(cc.RECURSION[name]["sos"])
    if zi is None:
        return backend.iir_sos_filter_complex(x, sos), None
    return backend.iir_sos_filter_complex(x, sos, zi=zi)


@pytest.mark.parametrize("name", list(cc.RECURSION))
def test_against_the_oracle(name):
    y, zf = run(name)
    spec = cc.RECURSION[name]
    assert y.shape == (len(spec["sos"]), spec["n"], spec["n_ch"]) and y.dtype == np.complex128
    e, tol = cc.recursion_error(name, y, zf), cc.recursion_tolerance(name)
    print(f"{name}: {e:.2e} of the peak (bound {tol:.2e}, emulation {cc.CIIR_EMULATION[name] * cc.EPS:.2e})")
    assert e <= tol, (name, e, tol)


def test_final_state_without_initial_state_and_real_part_only():
    """zf of a call that starts from rest (zi of zeros), for every length of the edge list; the real-only output equals
    the real plane of the full one bit for bit."""
    sos = cc.gammatone_sos([900, 1100], FS)
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in cc.LENGTHS:
        x = rng.standard_normal((n, 2))
        y, zf = backend.iir_sos_filter_complex(x, list(sos), zi=np.zeros((1, 4, 2, 2), dtype=np.complex128))
        y_ref, zf_ref = co.bank_ld(sos, x)
        worst = max(worst, co.stream_error(y[0], y_ref[0]), co.stream_error(zf[0].reshape(-1, 1), zf_ref[0].reshape(-1, 1)))
        re = backend.iir_sos_filter_complex(x, list(sos), real_only=True)
        assert re.dtype == np.float64 and np.array_equal(re, y.real)
    tol = cc.recursion_tolerance("gammatone23_n4097_zi")
    print(f"final states from rest over {cc.LENGTHS}: {worst:.2e} (bound {tol:.2e})")
    assert worst <= tol


@pytest.mark.parametrize("name,cut", [("two_poles_n4097_zi", cc.G + 7), ("gammatone23_n4097_zi", 31), ("max_sections_n4097_zi", cc.G)])
def test_two_calls_with_state_equal_one_joined_call(name, cut):
    x, zi, y_ref, zf_ref = cc.recursion_problem(name)
    sos = list(cc.RECURSION[name]["sos"])
    y1, z1 = backend.iir_sos_filter_complex(x[:cut], sos, zi=zi)
    y2, z2 = backend.iir_sos_filter_complex(x[cut:], sos, zi=z1)
    e = cc.recursion_error(name, np.concatenate([y1, y2], axis=1), z2)
    # two calls round the carried state twice: the bound of the joined case, once per call
    tol = 2 * cc.recursion_tolerance(name)
    print(f"{name} cut at {cut}: {e:.2e} (bound {tol:.2e})")
    assert e <= tol


def test_repeats_are_bit_identical():
    for name in ("gammatone23_n2049", "max_sections_n4097_zi"):
        (a, za), (b, zb) = run(name), run(name)
        assert np.array_equal(a, b) and (za is None or np.array_equal(za, zb))


def test_one_past_each_bound_raises_before_the_device():
    ctx = get_context()
    x = np.zeros((8, 1))
    sos = np.tile(cc.one_pole(0.5, 0.1).astype(np.complex128), (1, cc.CIIR_MAX_SEC + 1, 1))
    yr, yi = np.empty((1, 8, 1)), np.empty((1, 8, 1))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.ds_iir_sos_c128(ctx.handle, p(x), 1, 8, p(sos), 1, cc.CIIR_MAX_SEC + 1, None, p(yr), p(yi), None)
    with pytest.raises(NotImplementedError, match="16 complex second-order sections"):
        ctx.check(rc, "ds_iir_sos_c128")
    ok = np.ascontiguousarray(sos[:, :cc.CIIR_MAX_SEC])
    assert ctx.lib.ds_iir_sos_c128(ctx.handle, p(x), 1, 8, p(ok), 1, cc.CIIR_MAX_SEC, None, p(yr), p(yi), None) == 0
    for bad in (dict(n_ch=0), dict(n=0), dict(n_filt=0), dict(n_sec=0)):
        a = dict(n_ch=1, n=8, n_filt=1, n_sec=1)
        a.update(bad)
        rc = ctx.lib.ds_iir_sos_c128(ctx.handle, p(x), a["n_ch"], a["n"], p(ok), a["n_filt"], a["n_sec"], None, p(yr), p(yi), None)
        with pytest.raises((ValueError, DeviceError, RuntimeError)):
            ctx.check(rc, "ds_iir_sos_c128")
    nan = ok.copy()
    nan[0, 0, 4] = np.nan
    rc = ctx.lib.ds_iir_sos_c128(ctx.handle, p(x), 1, 8, p(nan), 1, cc.CIIR_MAX_SEC, None, p(yr), p(yi), None)
    with pytest.raises((ValueError, DeviceError, RuntimeError)):
        ctx.check(rc, "ds_iir_sos_c128")


# ---- the golden vectors through the classes -------------------------------------------------------------------------------
GOLDEN_TOL = 64 * cc.EPS  # scipy's own distance to the oracle (16 eps64, test_ciir_host.py) plus the device's: a 700-sample
                          # call is one group, whose bound is that of the n <= L B cases of a gammatone band (14.4 eps64 x 4.4)


def complex_data(sig):
    return sig.time_data + 1j * sig.time_data_imaginary


def test_golden_filterbank_parallel():
    z = golden()
    s = dsp.Signal(None, z["x"][:, :2].astype(np.float64), FS, constrain_amplitude=False)
    fb = dsp.filterbanks.auditory_filters_gammatone([700, 1500], 1, FS)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (the bank's filters have warning_if_complex off)
        out = fb.filter_signal(s, dsp.FilterBankMode.Parallel)
    assert type(out) is dsp.MultiBandSignal and len(out.bands) == len(z["par"])
    e = max(co.stream_error(complex_data(b), r) for b, r in zip(out.bands, z["par"]))
    print(f"Parallel bank against the reference: {e:.2e}")
    assert e <= GOLDEN_TOL
    fb.filters[0].warning_if_complex = True
    with pytest.warns(UserWarning, match="time_data_imaginary"):
        fb.filter_signal(s, dsp.FilterBankMode.Parallel)


def test_golden_state_single_filter_and_channel_subset():
    z = golden()
    x = z["x"].astype(np.float64)
    s2 = dsp.Signal(None, x[:, :2], FS, constrain_amplitude=False)
    fb = dsp.filterbanks.auditory_filters_gammatone([900, 1100], 1, FS)
    worst = 0.0
    for key in ("zi1", "zi2"):
        out = fb.filter_signal(s2, dsp.FilterBankMode.Parallel, activate_zi=True)
        worst = max(worst, max(co.stream_error(complex_data(b), r) for b, r in zip(out.bands, z[key])))
    assert np.iscomplexobj(fb.filters[0].zi) and np.shape(fb.filters[0].zi) == (4, 2, 2)
    f0 = dsp.filterbanks.auditory_filters_gammatone([900, 1100], 1, FS).filters[0]
    f0.warning_if_complex = True
    with pytest.warns(UserWarning, match="time_data_imaginary"):
        single = f0.filter_signal(s2)
    worst = max(worst, co.stream_error(complex_data(single), z["single"]))
    f0.warning_if_complex = False
    sub = f0.filter_signal(dsp.Signal(None, x, FS, constrain_amplitude=False), channels=1)
    worst = max(worst, co.stream_error(complex_data(sub), z["sub"]))
    assert np.array_equal(sub.time_data[:, [0, 2]], x[:, [0, 2]]) and not sub.time_data_imaginary[:, [0, 2]].any()
    print(f"state, single filter, channel subset against the reference: {worst:.2e}")
    assert worst <= GOLDEN_TOL
