"""The variable-Q transform on the device.  Every case of tests/vqt_cases.py, the edge lengths around the kernels'
tiles included, is held element by element to the longdouble oracle (tests/vqt_oracle.py) within
    |device - oracle| <= 2 c 2^-53 A
with A the element's absolute companion and c the terms summed along its chain (20 d + 1 for the first decimation, 41
per halving, L_i for the bank, 21 per interpolation stage) plus 2 per stage: the running forward bound of a chain of dot
products, whatever the summation order and with or without fused multiply-adds; the factor 2 is for the companion's own
rounding.  Then the cases with golden data against the reference within the float64 families' 1e-9 of the largest
magnitude, the resampler by itself, and the bit-level and residency properties."""

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend, transforms
from dsptoolbox_amd._lib import get_context
import vqt_cases as vc
import vqt_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-9

_golden, _device = {}, {}


def golden():
    if not _golden:
        z = np.load(vc.PATH, allow_pickle=False)
        _golden.update({k: z[k] for k in z.files})
    return _golden


def sig(name):
    return dsp.Signal(None, vc.signal(name), vc.ALL[name]["fs"])


def device(name):
    """(f, coefficients) of a case from the host-returning call, computed once"""
    if name not in _device:
        _device[name] = transforms.vqt(sig(name), **vc.ALL[name]["kw"])
    return _device[name]


def worst_ratio(got, value, a, c):
    """largest |got - value| / (2 c 2^-53 A) over every element (none is skipped: where the bound is zero the error
    must be zero too)"""
    err = np.abs(got - value).astype(np.float64)
    lim = vqt_oracle.bound(a, c)
    assert err.shape == lim.shape
    assert not err[lim == 0].any()
    return float((err / np.where(lim > 0, lim, 1.0)).max())


@pytest.mark.parametrize("name", list(vc.ALL))
def test_every_element_within_the_forward_bound(name, capsys):
    f, value, a, c = vc.expected(name)
    got_f, got = device(name)
    assert got.dtype == np.complex128 and got.shape == value.shape and np.array_equal(got_f, f)
    worst = worst_ratio(got, value, a, c)
    with capsys.disabled():
        print(f"\n{name}: worst |device - oracle| / (2 c 2^-53 A) = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(vc.CASES))
def test_against_the_reference(name, capsys):
    z = golden()
    got_f, got = device(name)
    assert np.array_equal(got_f, z[name + "_f"])
    if not vc.stored_whole(name):
        rows, samples = vc.subset(name)
        got = got[np.ix_(rows, samples)]
    worst = float(np.abs(got - z[name + "_vqt"]).max() / float(z[name + "_max"]))
    with capsys.disabled():
        print(f"\n{name}: worst |device - reference| / max|reference| = {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("up,down", vc.RATIOS)
@pytest.mark.parametrize("n", vc.RATIO_LENGTHS)
def test_resampler_within_the_forward_bound(up, down, n, capsys):
    x = vc.ratio_signal(n)
    value, a = vqt_oracle.resample_poly(x, up, down)
    got = backend.resample_int(x, up, down)
    assert got.shape == value.shape and got.dtype == np.float64
    terms = 1 if max(up, down) == 1 else (21 if down == 1 else 20 * down + 1)
    worst = worst_ratio(got, value, a, terms + 2)
    with capsys.disabled():
        print(f"\nP({up}, {down}) n = {n}: worst |device - oracle| / bound = {worst:.3g}")
    assert worst <= 1.0


def test_two_calls_give_the_same_bits():
    again = transforms.vqt(sig("default"), **vc.ALL["default"]["kw"])[1]
    assert np.array_equal(again.view(np.float64), device("default")[1].view(np.float64))


@pytest.mark.parametrize("name", ["default", "d1", "interp_2041"])
def test_result_left_on_the_device_is_the_same(name):
    f, scal = transforms.vqt(sig(name), **vc.ALL[name]["kw"], on_device=True)
    assert isinstance(scal, backend.DeviceScalogram) and scal.dtype == np.complex128
    assert scal.shape == device(name)[1].shape and np.array_equal(f, device(name)[0])
    assert np.array_equal(scal.to_host().view(np.float64), device(name)[1].view(np.float64))


@pytest.mark.parametrize("name", ["default", "kaiser", "tile_c1_771"])
def test_resident_signal_is_read_where_it_lies(name, capsys):
    """float32 planar samples in HBM: the transform of the float32-rounded samples, under the same bound"""
    f, value, a, c = vc.expected(name, f32=True)
    s = sig(name).to_device()
    got = transforms.vqt(s, **vc.ALL[name]["kw"])[1]
    worst = worst_ratio(got, value, a, c)
    with capsys.disabled():
        print(f"\n{name} resident: worst |device - oracle| / (2 c 2^-53 A) = {worst:.3g}")
    assert worst <= 1.0
    scal = transforms.vqt(s, **vc.ALL[name]["kw"], on_device=True)[1]
    assert np.array_equal(scal.to_host().view(np.float64), got.view(np.float64))


def test_launch_names():
    ctx = get_context()
    ctx.routes()
    transforms.vqt(sig("default"), **vc.ALL["default"]["kw"])
    assert ctx.routes() == {"vqt_decimate", "vqt_bank", "vqt_interp_octave", "vqt_interp"}
    s = sig("d1").to_device()
    ctx.routes()
    transforms.vqt(s, octaves=[6, 6])  # one octave: no first interpolation stage
    assert ctx.routes() == {"vqt_decimate", "vqt_bank", "vqt_interp"}
    backend.resample_int(vc.ratio_signal(21), 1, 2)
    assert ctx.routes() == {"vqt_decimate"}
    backend.resample_int(vc.ratio_signal(21), 16, 1)
    assert ctx.routes() == {"vqt_interp@real"}
