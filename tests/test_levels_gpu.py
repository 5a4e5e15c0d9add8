"""Levels and loudness on the device (csrc/kernels_level.hpp through standard.normalize, rms, crest_factor, fade,
apply_gain, detrend, envelope, lufs_integrated and the backend's ndarray functions): the reference's recorded outputs
(tests/golden/levels/cases.npz), the long-double oracle of tests/levels_oracle.py at the shapes where a kernel changes
path, and device-resident signals against host ones."""

import functools
import json
import os
import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import fft64_cases as f64c
import levels_cases as lc
import levels_oracle as lo
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context
from dsptoolbox_amd.standard import gain_and_level as gl
from test_iir_gpu import EDGE_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = lc.U
FLOOR = 64 * U          # detrend and the boxcar envelope: the nine-term recurrence and the subtraction
F32 = 2.0 ** -24        # the float32 store of a resident result, of the channel's peak
LD = lo.LD


@functools.lru_cache(maxsize=None)
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "levels", "cases.npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z


def host(x, fs=lc.FS):
    return dsp.Signal(None, x.copy(), fs, constrain_amplitude=False)


def resident(x, fs=lc.FS):
    return dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), fs)


def sum_bound(n):
    return 4 * lo.reduction_depth(n) * U


# ---- golden through the public functions -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["peak_all", "peak_each"])
def test_normalize_peak_equals_the_reference(name):
    seed, n, n_ch, dbfs, pk, each = lc.NORMALIZE[name]
    got = dsp.normalize(host(lc.noise(seed, n, n_ch)), dbfs, pk, each).time_data
    assert np.array_equal(got, gold()[1][f"normalize_{name}"])


@pytest.mark.parametrize("name", list(lc.GAIN))
def test_apply_gain_equals_the_reference(name):
    seed, n, n_ch, g = lc.GAIN[name]
    got = dsp.apply_gain(host(lc.noise(seed, n, n_ch)), np.asarray(g) if isinstance(g, list) else g).time_data
    assert np.array_equal(got, gold()[1][f"gain_{name}"])


@pytest.mark.parametrize("name", list(lc.FADE))
def test_fade_equals_the_reference(name):
    seed, n, n_ch, kind, l_s, a, b = lc.FADE[name]
    x = lc.noise(seed, n, n_ch)
    got = dsp.fade(host(x), getattr(dsp.FadeType, kind), lc.fade_seconds(l_s), a, b)
    assert np.array_equal(got.time_data, gold()[1][f"fade_{name}"])
    if kind == "NoFade":
        assert np.array_equal(got.time_data, x) and got.time_data is not x


@pytest.mark.parametrize("name", list(lc.NORMALIZE))
def test_rms_crest_and_rms_normalisation(name):
    seed, n, n_ch, dbfs, pk, each = lc.NORMALIZE[name]
    x = lc.noise(seed, n, n_ch)
    want, bound = lo.rms(x), sum_bound(n)
    got = dsp.rms(host(x), in_dbfs=False)
    e = float(np.max(np.abs(got - want) / want))
    crest = dsp.crest_factor(host(x), in_db=False)
    e_c = float(np.max(np.abs(crest - lo.peak(x) / want) / (lo.peak(x) / want)))
    print(f"{name}: rms {e:.2e}, crest {e_c:.2e}, bound {bound:.2e}")
    assert got.shape == (n_ch,) and e <= bound and e_c <= bound
    assert np.allclose(dsp.rms(host(x)), 20 * np.log10(got), rtol=0, atol=1e-12)
    assert np.allclose(dsp.crest_factor(host(x)), 20 * np.log10(crest), rtol=0, atol=1e-12)
    assert np.array_equal(backend.level_stats(x), backend.level_stats(x))  # the same bits on every call
    if not pk:
        y = dsp.normalize(host(x), dbfs, pk, each).time_data
        want_y = lo.normalize(x, dbfs, pk, each)
        e_n = float(np.max(np.abs(y.astype(LD) - want_y) / np.abs(want_y)))  # per sample: the gain's error and one product
        print(f"{name}: rms-normalised {e_n:.2e} of each sample")
        assert e_n <= bound


def test_silent_channel_and_constrained_amplitude():
    x = lc.noise(5, 300, 2)
    x[:, 1] = 0.0
    with np.errstate(all="ignore"):
        y = dsp.normalize(host(x), -3.0, True, True).time_data
    assert np.isfinite(y[:, 0]).all() and np.isnan(y[:, 1]).all()  # 0 * inf, as numpy gives
    s = dsp.Signal(None, lc.noise(6, 300, 2), lc.FS, constrain_amplitude=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loud = dsp.apply_gain(s, 40.0)
    assert np.max(np.abs(loud.time_data)) == pytest.approx(1.0, abs=1e-15) and loud.constrain_amplitude


# ---- detrend and the envelopes against the oracle, bounds from the reference's own error -------------------------------
@pytest.mark.parametrize("order", lc.DETREND_ORDERS)
def test_detrend_orders(order):
    meta, z = gold()
    x = lc.detrend_input()
    got = dsp.detrend(host(x), order).time_data
    e = lo.relative_to_peak(got, lo.detrend(x, order))
    bound = max(4 * meta["measured"]["detrend"][str(order)], FLOOR)
    print(f"order {order}: {e:.2e} of the peak, bound {bound:.2e}, against the reference {lo.relative_to_peak(got, z[f'detrend_{order}'].astype(LD)):.2e}")
    assert e <= bound


@pytest.mark.parametrize("name", list(lc.ENVELOPE_BOXCAR))
def test_boxcar_envelope(name):
    meta, _ = gold()
    _, _, _, w, _ = lc.ENVELOPE_BOXCAR[name]
    x = lc.boxcar_input(name)
    got = dsp.envelope(host(x), analytic=False, window_length_samples=w)
    want = lo.moving_mean_square(x, w)
    e = float(np.max(np.max(np.abs(got.astype(LD) ** 2 - want), axis=0) / np.max(want, axis=0)))
    bound = max(4 * meta["measured"]["env_boxcar"][name], FLOOR)
    print(f"{name}: {e:.2e} of the peak mean square, bound {bound:.2e}")
    assert got.shape == x.shape and np.isfinite(got).all() and (got >= 0).all() and e <= bound


@pytest.mark.parametrize("name", list(lc.ENVELOPE_ANALYTIC))
def test_analytic_envelope(name):
    meta, _ = gold()
    seed, n, n_ch = lc.ENVELOPE_ANALYTIC[name]
    x = lc.noise(seed, n, n_ch)
    got = dsp.envelope(host(x))
    d = lo.detrend(x, 1)
    ref = f64c.oracle_hilbert(d)
    err = np.max(np.abs(got.astype(LD) - np.abs(ref)), axis=0)
    pk = np.max(np.abs(ref), axis=0)
    scale = np.sqrt(np.mean(np.abs(ref) ** 2, axis=0))
    floor = f64c.tolerance(("hilbert", f64c.plan(n)[1])) * scale  # what fft64_cases holds ds_hilbert to at this length
    bound = np.maximum(4 * meta["measured"]["env_analytic"][name] * pk, floor)
    print(f"{name}: {float(np.max(err / pk)):.2e} of the peak, bound {float(np.min(bound / pk)):.2e}")
    assert got.shape == x.shape and (err <= bound).all()


# ---- loudness ----------------------------------------------------------------------------------------------------------
def check_blocks(x, fs, blocks):
    zo, pk = lo.lufs_blocks(x, fs)
    assert blocks.shape == zo.shape
    if zo.size:
        rel = np.abs(blocks.astype(LD) - zo) / zo
        bound = 2 * 2 * EDGE_TOL * pk * pk / zo
        print(f"blocks {zo.shape}: worst {float(np.max(rel / bound)):.2e} of the bound, {float(np.max(rel)):.2e} relative")
        assert (rel <= bound).all()
    return zo


@pytest.mark.parametrize("name", list(lc.LUFS))
def test_lufs_integrated(name):
    _, z = gold()
    x, fs = lc.lufs_input(name)
    tg, step = lc.lufs_blocks(fs)
    blocks = backend.loudness_blocks(x, gl._k_weighting_sos(fs), tg, step)
    check_blocks(x, fs, blocks)
    value, want = dsp.lufs_integrated(host(x, fs)), float(z[f"lufs_{name}"])
    if np.isnan(want):
        assert np.isnan(value) and blocks.shape[0] == 0
        return
    assert np.array_equal(lo.lufs_gating(blocks)[3], z[f"lufs_{name}_gated"])
    print(f"{name}: {value:.9f} LUFS, golden {want:.9f}")
    assert abs(value - want) <= 1e-7


@pytest.mark.parametrize("fs,extra", [(8000, 2047), (8000, 2048), (8000, 2049), (8000, 4097), (11025, 2049), (11025, 4097)])
def test_lufs_blocks_around_the_carry_groups(fs, extra):
    """Lengths one and two carry groups of the section runner (2048 samples) beyond one block."""
    tg, step = lc.lufs_blocks(fs)
    x = lc.programme(90, fs, 2, [(tg + extra - 1500, "tone", 0.4), (1500, "noise", 0.05)])
    check_blocks(x, fs, backend.loudness_blocks(x, gl._k_weighting_sos(fs), tg, step))
    xr = DevicePlanar.from_planar(get_context(), x.T.astype(np.float32))
    assert np.array_equal(backend.loudness_blocks(xr, gl._k_weighting_sos(fs), tg, step),
                          backend.loudness_blocks(x, gl._k_weighting_sos(fs), tg, step))


# ---- shape edges against the oracle ------------------------------------------------------------------------------------
REDUCTIONS = ([(n, c) for n in (1, 2, lc.SPAN - 1, lc.SPAN, lc.SPAN + 1, 2 * lc.SPAN + 1) for c in (1, 3)]
              + [(lc.SPAN + 1, 65), (lc.NT * lc.SPAN + 1, 1)])


@pytest.mark.parametrize("n,n_ch", REDUCTIONS)
def test_reduction_lengths(n, n_ch):
    """The projection (order 2 where the length allows) and the residual statistics: one workgroup, its edge, several,
    and the second round of the final kernel's lanes."""
    x = lc.noise(100 + n % 97, n, n_ch)
    order = min(2, n - 1)
    P = lo.gram_basis(n, order)
    got = backend.level_project(x, order)
    want = P @ x.astype(LD)
    weight = np.abs(P) @ np.abs(x).astype(LD)  # sum |x P_k|: what a sum's rounding is relative to
    depth = lo.reduction_depth(n)
    e = float(np.max(np.abs(got[:, :order + 1].T - want) / weight))
    print(f"n={n}, {n_ch} ch: coefficients {e / U:.1f} u of sum |x P|, depth {depth}")
    assert got.shape == (n_ch, 10) and e <= (4 * depth + 64) * U  # the sum's depth, and the recurrence's 64 u per term
    assert np.array_equal(got[:, 9], np.max(np.abs(x), axis=0)) and not got[:, order + 1:9].any()
    st = backend.level_stats(x, 0)
    d = x.astype(LD) - np.mean(x.astype(LD), axis=0)
    ss = np.sum(d * d, axis=0)
    assert np.array_equal(st[:, 2], np.max(np.abs(x), axis=0))
    if n > 1:
        # the mean carries an error of up to depth u max |x|, and so does every deviation (a short signal's deviations
        # may be far smaller than its samples); in the sum of squares that common shift cancels to first order
        shift = 4 * depth * U * np.max(np.abs(x), axis=0)
        assert (np.abs(st[:, 0] - ss) <= 4 * depth * U * ss + n * shift ** 2).all()
        assert (np.abs(st[:, 1] - np.max(np.abs(d), axis=0)) <= shift).all()
    common = backend.level_stats(x, 0, common=True)
    dc = x.astype(LD) - np.mean(x.astype(LD))
    assert float(np.abs(np.sum(common[:, 0]) - np.sum(dc * dc))) <= 4 * (depth + n_ch) * U * float(np.sum(dc * dc)) + 1e-300


def expected_apply(x, gain, table, at_start, at_end):
    """The kernel's operations in numpy, one rounding each: gain, fade in, fade out."""
    y = x * gain[None, :]
    l = len(table)
    if at_start:
        y[:l] = y[:l] * table[:, None]
    if at_end:
        y[len(y) - l:] = y[len(y) - l:] * table[::-1, None]
    return y


@pytest.mark.parametrize("n", list(range(1, 10)) + [1003])
def test_apply_lengths_and_strides(n):
    """Host (double2 pairs, the odd last value) and resident rows: dense (float4 body, scalar head and tail, the head
    changing from row to row), and with a pitch and a start that are no multiple of the vector (scalar rows)."""
    n_ch = 3
    x = lc.noise(200 + n, n, n_ch)
    gain = np.array([0.5, -1.25, 3.0])
    table = np.linspace(0.1, 0.9, min(n, 3))
    want = expected_apply(x.copy(), gain, table, True, True)
    assert np.array_equal(backend.level_apply(x, gain=gain, fade=table, at_start=True, at_end=True), want)
    assert np.array_equal(backend.level_apply(x), x)
    want32 = want.astype(np.float32).T
    ctx = get_context()
    dense = DevicePlanar.from_planar(ctx, x.T.astype(np.float32))
    y = backend.level_apply(dense, gain=gain, fade=table, at_start=True, at_end=True)
    assert isinstance(y, DevicePlanar) and np.array_equal(y.to_planar(), want32)
    ld = n + 1 if (n + 1) % 4 else n + 2  # a pitch that is no multiple of four samples, from a start that is none either
    padded = np.full((n_ch, ld), 7.0, dtype=np.float32)
    padded[:, :n] = x.T
    buf = DeviceBuffer.from_array(ctx, np.concatenate([np.zeros(1, np.float32), padded.ravel()]))
    odd = DevicePlanar(buf, n_ch, n, ld, 4)
    assert ld % 4 != 0
    assert np.array_equal(backend.level_apply(odd, gain=gain, fade=table, at_start=True, at_end=True).to_planar(), want32)
    assert np.array_equal(backend.level_stats(odd), backend.level_stats(dense))


MOVING = [(n, w) for n in (2 * lc.TILE, 2 * lc.TILE + 3) for w in (1, 2, lc.TILE - 1, lc.TILE, lc.TILE + 1, n, n + 5)]


@pytest.mark.parametrize("n,w", MOVING)
def test_moving_window_edges(n, w):
    x = lc.noise(300 + w % 89, n, 2)
    got = backend.moving_rms(x, w)
    want = lo.moving_mean_square(x, w)
    e = float(np.max(np.max(np.abs(got.astype(LD) ** 2 - want), axis=0) / np.max(want, axis=0)))
    print(f"n={n}, w={w}: {e / U:.1f} u of the peak mean square")
    assert np.isfinite(got).all() and (got >= 0).all() and e <= FLOOR


def test_moving_window_long_stream_last_tile():
    """2^20 samples: an error that grew along the signal would show in the last tile."""
    n, w = 1 << 20, 1000
    x = lc.noise(400, n, 1)
    got = backend.moving_rms(x, w)[n - lc.TILE:]
    d = lo.detrend(x, 1)[n - lc.TILE - w:]
    cs = np.concatenate([np.zeros((1, 1), LD), np.cumsum(d * d, axis=0)])
    want = (cs[w + 1:] - cs[1:lc.TILE + 1]) / w
    e = float(np.max(np.abs(got.astype(LD) ** 2 - want)) / np.max(want))
    print(f"last tile of 2^20: {e / U:.1f} u of the peak mean square")
    assert want.shape == got.shape and e <= FLOOR


# ---- resident against host ---------------------------------------------------------------------------------------------
def test_resident_results_stay_resident():
    n, n_ch = 5003, 3
    x = lc.noise(500, n, n_ch, curve=0.4)
    h, r = host(x), resident(x)
    calls = {
        "normalize": lambda s: dsp.normalize(s, -3.0, True, False),
        "normalize_rms": lambda s: dsp.normalize(s, -20.0, False, True),
        "fade": lambda s: dsp.fade(s, dsp.FadeType.Logarithmic, 0.1),
        "no_fade": lambda s: dsp.fade(s, dsp.FadeType.NoFade),
        "apply_gain": lambda s: dsp.apply_gain(s, [1.0, -2.0, 3.0]),
        "detrend": lambda s: dsp.detrend(s, 3),
    }
    for name, f in calls.items():
        out, ref = f(r), f(h).time_data
        assert out.on_device and not out._has_host_copy and not out.constrain_amplitude, name
        e = float(np.max(np.max(np.abs(out.time_data - ref), axis=0) / np.max(np.abs(ref), axis=0)))
        print(f"{name}: resident against host {e / F32:.2f} x 2^-24 of the peak")
        assert e <= F32, name
    assert r.on_device and not r._has_host_copy  # nothing was downloaded from the input


def test_resident_measures_equal_host_measures():
    n, n_ch = 5003, 2
    x = lc.noise(501, n, n_ch)
    h, r = host(x), resident(x)
    bound = sum_bound(n)
    assert np.max(np.abs(dsp.rms(r, False) - dsp.rms(h, False)) / dsp.rms(h, False)) <= bound
    assert np.max(np.abs(dsp.crest_factor(r, False) - dsp.crest_factor(h, False)) / dsp.crest_factor(h, False)) <= bound
    env_h, env_r = dsp.envelope(h, False, 100), dsp.envelope(r, False, 100)
    assert np.max(np.abs(env_r ** 2 - env_h ** 2)) <= FLOOR * np.max(env_h ** 2)
    a_h, a_r = dsp.envelope(h), dsp.envelope(r)
    tol = f64c.tolerance(("hilbert", f64c.plan(n)[1])) * np.sqrt(np.mean(a_h ** 2, axis=0))  # of the column's rms, as ds_hilbert is held
    assert (np.max(np.abs(a_r - a_h), axis=0) <= tol).all()
    xl, fs = lc.lufs_input("programme_8000")
    assert abs(dsp.lufs_integrated(resident(xl, fs)) - dsp.lufs_integrated(host(xl, fs))) <= 1e-7
    assert np.isnan(dsp.lufs_integrated(resident(*lc.lufs_input("edge_3200_2ch"))))
    assert r.on_device and not r._has_host_copy


def test_multiband_shapes():
    x = lc.noise(502, 700, 2)
    mb = dsp.MultiBandSignal([host(x), host(0.5 * x)])
    assert dsp.rms(mb).shape == (2, 2) and dsp.crest_factor(mb).shape == (2, 2)
    # kept from the reference: the bands' crest factors in dB are converted to dB once more
    assert np.array_equal(dsp.crest_factor(mb)[0], dsp.tools.to_db(dsp.crest_factor(host(x)), True))
    assert np.array_equal(dsp.crest_factor(mb, in_db=False)[0], dsp.crest_factor(host(x), in_db=False))
    assert np.allclose(dsp.rms(mb, False)[1], 0.5 * dsp.rms(mb, False)[0], rtol=1e-14)
    assert dsp.envelope(mb).shape == (700, 2, 2) and dsp.envelope(mb, False, 10).shape == (700, 2, 2)
    out = dsp.normalize(mb, -6.0, True, True)
    assert isinstance(out, dsp.MultiBandSignal) and np.array_equal(out.bands[0].time_data, out.bands[1].time_data)
    assert np.array_equal(dsp.detrend(mb, 1).bands[0].time_data, dsp.detrend(host(x), 1).time_data)
    assert np.array_equal(dsp.apply_gain(mb, 6.0).bands[1].time_data, dsp.apply_gain(host(0.5 * x), 6.0).time_data)
