"""Frequency warping on the device.  transforms.warp and transforms.laguerre from a host Signal and from a
device-resident one on every case of tests/golden/warp/cases.npz (the reference's own outputs: float and string
factors, shift_ir on and off, total_length shorter than the signal), and the edge sweep through the ds_allpass_table
entry against the long-double table of tests/warp_oracle.py: square and rectangular shapes around the wave width and
the tile sides, channel counts around the group size, four factors.  The bound is 1e-12 of each output channel's peak:
the reference sits within 1e-14 of the long-double table on these inputs (tests/test_warp_host.py), a float64 table in
another summation order at a few 1e-15; the bound leaves two orders for the tile-order sums and the contraction into
fused multiply-adds.  A factor of 0 returns the input bit for bit, repeats are bit-identical, laguerre there and back
is held to the oracle's own round trip, and one step past each bound raises.  Every test prints the largest error it
measured."""

import ctypes as C
import json
import os

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
import warp_oracle as wo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12
_z = np.load(os.path.join(ROOT, "tests", "golden", "warp", "cases.npz"), allow_pickle=False)
META = json.loads(str(_z["meta"]))
Z = {k: _z[k] for k in _z.files if k != "meta"}
FS = META["fs"]
SHAPES = list(dict.fromkeys([(n, n) for n in wo.SQUARE_SIZES] + wo.RECT_SHAPES))


def host_signal(name):
    return dsp.ImpulseResponse(None, Z[name].astype(np.float64), FS, constrain_amplitude=False)


def resident_signal(name):
    return dsp.Signal.from_planar_f32(np.ascontiguousarray(Z[name].T), FS)


def run_warp(i, signal):
    case = META["warp"][i]
    got = dsp.transforms.warp(signal, case["factor"], case["shift_ir"], case["total_length"])
    if type(case["factor"]) is str:
        assert type(got) is tuple and got[1] == META["used"][i]
        got = got[0]
    return got


@pytest.mark.parametrize("i", range(len(META["warp"])))
@pytest.mark.parametrize("where", ["host", "resident"])
def test_warp_on_the_golden_cases(i, where):
    s = host_signal(META["warp"][i]["sig"]) if where == "host" else resident_signal(META["warp"][i]["sig"])
    assert s.on_device == (where == "resident")
    got = run_warp(i, s)
    assert type(got) is type(s) and got.sampling_rate_hz == FS and got.time_data.dtype == np.float64
    e = wo.channel_error(got.time_data, Z[f"warp_{i}"])
    print(f"warp {where} case {i} {META['warp'][i]}: {e:.2e}")
    assert e <= BOUND


@pytest.mark.parametrize("i", range(len(META["laguerre"])))
@pytest.mark.parametrize("where", ["host", "resident"])
def test_laguerre_on_the_golden_cases(i, where):
    case = META["laguerre"][i]
    s = host_signal(case["sig"]) if where == "host" else resident_signal(case["sig"])
    got = dsp.transforms.laguerre(s, case["factor"])
    assert type(got) is type(s) and len(got) == len(s)
    e = wo.channel_error(got.time_data, Z[f"laguerre_{i}"])
    print(f"laguerre {where} case {i} {case}: {e:.2e}")
    assert e <= BOUND


@pytest.mark.parametrize("n_in,n_out", SHAPES)
def test_edge_sweep_against_the_long_double_table(n_in, n_out):
    worst = 0.0
    for lam in wo.LAMBDAS:
        x, (p, q, row0, col0), want = wo.sweep_reference(n_in, n_out, lam)
        for n_ch in wo.CHANNELS:
            got = backend.allpass_table(x[:, :n_ch], p, q, row0, col0)
            assert got.shape == (n_out, n_ch) and got.dtype == np.float64
            e = wo.channel_error(got, want[:, :n_ch])
            worst = max(worst, e)
            assert e <= BOUND, (n_in, n_out, lam, n_ch, e)
    print(f"allpass_table {n_in} x {n_out}: {worst:.2e}")


def test_edge_sweep_from_device_resident_samples():
    from dsptoolbox_amd._lib import DevicePlanar, get_context
    worst = 0.0
    for n_in, n_out in ((wo.TJ + 1, wo.TJ + 1), (2 * wo.TI + 1, 2 * wo.TJ + 1), (3 * wo.TI, wo.TJ - 1)):
        x, (p, q, row0, col0), want = wo.sweep_reference(n_in, n_out, -0.876)
        planar = np.zeros((wo.G + 1, n_in + 7), dtype=np.float32)  # a leading dimension beyond the samples
        planar[:, :n_in] = x.T  # (the samples are float32 values)
        whole = DevicePlanar.from_planar(get_context(), planar)
        dev = DevicePlanar(whole.owner, wo.G + 1, n_in, n_in + 7)
        worst = max(worst, wo.channel_error(backend.allpass_table(dev, p, q, row0, col0), want))
    print(f"allpass_table from resident samples: {worst:.2e}")
    assert worst <= BOUND


def test_factor_zero_returns_the_input_bit_for_bit():
    for name in ("n300c2", "n2500c2"):
        x = Z[name].astype(np.float64)
        for s in (host_signal(name), resident_signal(name)):
            assert np.array_equal(dsp.transforms.warp(s, 0.0, False).time_data, x)
            assert np.array_equal(dsp.transforms.laguerre(s, 0.0).time_data, x)
    for n_in, n_out in wo.RECT_SHAPES:
        x, (p, q, row0, col0), _ = wo.sweep_reference(n_in, n_out, 0.0)
        got = backend.allpass_table(x, p, q, row0, col0)
        m = min(n_in, n_out)
        assert np.array_equal(got[:m], x[:m]) and not got[m:].any()
    # every launch of the longest table: 128 x 512 tiles, 639 anti-diagonals
    n = backend.WARP_MAX_SIDE
    x = wo.decaying_noise(n, 1, 17).astype(np.float64)
    assert np.array_equal(backend.warp_time_series(x, 0.0), x)


def test_laguerre_there_and_back():
    name, f = "n1030c3", 0.6
    s = host_signal(name)
    back = dsp.transforms.laguerre(dsp.transforms.laguerre(s, f), -f).time_data
    x = Z[name].astype(np.float64)
    want = wo.laguerre(wo.laguerre(x, f), -f)
    e, off = wo.channel_error(back, want), wo.channel_error(want, x)
    print(f"laguerre({f}) then laguerre({-f}) on {name}: {e:.2e} from the oracle's round trip, which is {off:.2e} from the input")
    assert e <= BOUND and off > BOUND  # (not the identity on a truncated signal)


def test_repeats_are_bit_identical():
    s = host_signal("n2500c2")
    for run in (lambda: dsp.transforms.warp(s, -0.7, True).time_data, lambda: dsp.transforms.laguerre(s, 0.9).time_data):
        assert np.array_equal(run(), run())
    x, (p, q, row0, col0), _ = wo.sweep_reference(2 * wo.TI + 1, 2 * wo.TJ + 1, 0.99)
    assert np.array_equal(backend.allpass_table(x, p, q, row0, col0), backend.allpass_table(x, p, q, row0, col0))


def test_one_step_past_each_bound():
    side = backend.WARP_MAX_SIDE
    long = dsp.Signal(None, np.zeros((side + 1, 1)), FS)
    with pytest.raises(NotImplementedError):
        dsp.transforms.warp(long, -0.5, False)
    with pytest.raises(NotImplementedError):
        dsp.transforms.laguerre(long, 0.5)
    with pytest.raises(NotImplementedError):
        dsp.transforms.warp(dsp.Signal.from_planar_f32(np.zeros((1, side + 1), dtype=np.float32), FS), -0.5, False)
    with pytest.raises(NotImplementedError):
        backend._warp_check(10, 10, backend.WARP_MAX_CHANNELS + 1)
    groups_over = int(backend.WARP_MAX_WORK / (side * side)) + 1
    with pytest.raises(NotImplementedError):
        backend._warp_check(side, side, (groups_over - 1) * wo.G + 1)
    # the C entries answer alike, with a context at hand
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    p = backend._ptr
    x, row0, col0, out = np.zeros((10, 1)), np.zeros(10), np.zeros(10), np.zeros((10, 1))
    call = ctx.lib.ds_allpass_table
    assert call(ctx.handle, p(x), 10, 1, -0.5, 0.5, p(row0), p(col0), 10, p(out)) == 0
    assert call(ctx.handle, p(x), side + 1, 1, -0.5, 0.5, p(row0), p(col0), 10, p(out)) == -2
    assert call(ctx.handle, p(x), 10, 1, -0.5, 0.5, p(row0), p(col0), side + 1, p(out)) == -2
    assert call(ctx.handle, p(x), 10, backend.WARP_MAX_CHANNELS + 1, -0.5, 0.5, p(row0), p(col0), 10, p(out)) == -2
    assert call(ctx.handle, p(x), side, (groups_over - 1) * wo.G + 1, -0.5, 0.5, p(row0), p(col0), side, p(out)) == -2
    assert call(ctx.handle, p(x), 10, 1, float("nan"), 0.5, p(row0), p(col0), 10, p(out)) == -1
    assert call(ctx.handle, p(x), 0, 1, -0.5, 0.5, p(row0), p(col0), 10, p(out)) == -1
    assert ctx.lib.ds_allpass_table_dev(ctx.handle, C.c_void_p(16), 1, 9, 10, -0.5, 0.5, p(row0), p(col0), 10, p(out)) == -1  # ldx


def test_factors_outside_the_unit_interval_are_assertion_errors():
    s = host_signal("n65c1")
    for bad in (1.0, -1.0, 1.5):
        with pytest.raises(AssertionError):
            dsp.transforms.warp(s, bad, False)
        with pytest.raises(AssertionError):
            dsp.transforms.laguerre(s, bad)
