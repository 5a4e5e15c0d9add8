"""Spectral subtraction on the device (csrc/kernels_specsub.hpp through ds_fx_specsub): every golden case of the reference
through the class, held to max(4 x the reference's own error on that case, FLOOR) with the reference's output in the
oracle's place; generated shapes -- windows of 4 to 16384 samples, lengths on either side of a frame boundary, frame
counts and lengths on either side of the tiles of k_ss_track and k_ss_ola -- against the long-double oracle of
specsub_oracle.py within FLOOR alone; a resident signal against the host path within float32 store rounding; two calls
bit for bit; the refusals with no launch."""

import functools
import json
import os
import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import specsub_cases as sc
import specsub_oracle as so
from dsptoolbox_amd import backend, effects
from dsptoolbox_amd.effects.spectral import SpectralSubtractor
from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_LENGTHS = sc.tile_lengths(backend.SS_TRACK_TILE, backend.SS_OLA_TILE)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "specsub", "cases.npz"))
    return z, json.loads(str(z["meta"]))["cases"]


def signal(x):
    return dsp.Signal(None, x, sc.FS, constrain_amplitude=False)


def judge(what, got, want, window, reference_error=0.0):
    e, b = so.stream_error(got, want), so.bound(window, reference_error)
    print(f"{what}: {e:.2e} of the peak, {e / so.floor(window):.3f} of the floor {so.floor(window):.2e}"
          + (f", {e / reference_error:.2f} of the reference's own error" if reference_error else "") + f" (bound {b:.2e})")
    assert e <= b, (what, e, b)


def apply(ctor, adv, s):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return sc.effect(effects.spectral, dsp, ctor, adv).apply(s)


# ---- the reference's golden vectors through the class ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.GOLDEN))
def test_golden(golden, name, capfd):
    _, n, n_ch, ctor, adv = sc.GOLDEN[name]
    y = apply(ctor, adv, signal(sc.samples(name))).time_data
    assert capfd.readouterr().out == ""  # nothing is printed
    assert y.shape == (n, n_ch) and y.dtype == np.float64
    if name == "silence":
        assert np.isnan(y[:, 1]).all()
    judge(name, y, golden[0][f"out_{name}"], sc.W, golden[1][name]["error"])


def test_golden_bands(golden):
    seeds, n, n_ch, ctor, adv = sc.MULTIBAND["bands"]
    ctx = get_context()
    ctx.profile_enable(True)
    ctx.profile_report()
    out = apply(ctor, adv, dsp.MultiBandSignal([signal(sc.burst(seed, n, n_ch)) for seed in seeds]))
    launches = ctx.profile_report()
    ctx.profile_enable(False)
    assert type(out) is dsp.MultiBandSignal and out.number_of_bands == 2
    assert launches["ss_track"][1] == 1  # adaptive mode: the bands are streams of one call
    for i in range(2):
        judge(f"band {i}", out.bands[i].time_data, golden[0][f"out_bands_{i}"], sc.W, golden[1][f"bands_{i}"]["error"])


def test_no_gate_returns_the_input():
    x = sc.samples("no_gate")
    _, _, _, ctor, adv = sc.GOLDEN["no_gate"]
    judge("no_gate against its input", apply(ctor, adv, signal(x)).time_data, x, sc.W)


# ---- generated shapes against the oracle -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(window, n, mode):
    x, w, step = sc.generated(window, n)
    kw = dict(env_floor=1e-4) if mode == "adaptive" else dict(table=sc.given_spectrum(93) ** 0.5)
    y, gates, clips = so.subtract(x, w, step, mode, **kw)
    sc.conditions(gates, clips, adaptive=mode == "adaptive")  # (a condition of the case, never a skip)
    return y


@pytest.mark.parametrize("window", sc.WINDOWS)
def test_windows_and_frame_boundaries(window):
    for n in sc.edge_lengths(window):
        x, _, step = sc.generated(window, n)
        assert n % step in (0, 1, step - 1) and 5 <= backend.specsub_frames(n, window, step) <= 6
        y = backend.fx_specsub(x, "hann", window, step, "adaptive", env_floor=1e-4)
        assert y.shape == x.shape and y.dtype == np.float64
        judge(f"W={window} n={n}", y, reference(window, n, "adaptive"), window)


@pytest.mark.parametrize("mode", ["adaptive", "static"])
@pytest.mark.parametrize("n", TILE_LENGTHS)
def test_tile_edges(n, mode):
    x, _, step = sc.generated(sc.W, n)
    kw = dict(env_floor=1e-4) if mode == "adaptive" else dict(noise_table=sc.given_spectrum(93) ** 0.5)
    y = backend.fx_specsub(x, "hann", sc.W, step, mode, **kw)
    judge(f"{mode} n={n} frames={backend.specsub_frames(n, sc.W, step)}", y, reference(sc.W, n, mode), sc.W)


def test_a_table_per_stream():
    n = 300
    x, w, step = sc.generated(sc.W, n)
    table = np.stack([sc.given_spectrum(94) ** 0.5, sc.given_spectrum(95, 3.0) ** 0.5])
    y = backend.fx_specsub(x, "hann", sc.W, step, "static", noise_table=table)
    want, gates, clips = so.subtract(x, w, step, "static", table=table)
    sc.conditions(gates, clips, adaptive=False)
    judge("two tables", y, want, sc.W)


# ---- device-resident signals, repeatability ------------------------------------------------------------------------------------
def resident(x):
    return dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), sc.FS)


@pytest.mark.parametrize("name", ["default", "static_given", "static_detector"])
def test_resident_signal_equals_the_host_path_and_stays_resident(name):
    _, n, n_ch, ctor, adv = sc.GOLDEN[name]
    x = sc.samples(name)
    host = apply(ctor, adv, signal(x)).time_data
    out = apply(ctor, adv, resident(x))
    assert out.on_device and out.device_samples.n_samples == n
    e = so.stream_error(out.time_data, host)
    print(f"{name}: {e:.2e} of the peak (float32 store rounding {2.0 ** -24:.2e})")
    assert e <= 2.0 ** -24


def test_resident_bands_are_streams_of_one_call():
    n, n_ch, n_bands = 300, 2, 3
    x = [sc.burst(820 + b, n, n_ch) for b in range(n_bands)]
    ctx = get_context()
    owner = DeviceBuffer.from_array(ctx, np.concatenate([np.ascontiguousarray(b.T, dtype=np.float32) for b in x]))
    bands = [dsp.Signal.from_planar_f32(DevicePlanar(owner, n_ch, n, n, 4 * b * n_ch * n), sc.FS) for b in range(n_bands)]
    e = SpectralSubtractor(block_length_s=sc.BLOCK_S)
    ctx.profile_enable(True)
    ctx.profile_report()
    out = e.apply(dsp.MultiBandSignal(bands))
    launches = ctx.profile_report()
    ctx.profile_enable(False)
    assert launches["ss_analyze"][1] == 1 and out.on_device
    for b in range(n_bands):
        err = so.stream_error(out.bands[b].time_data, e.apply(signal(x[b])).time_data)
        assert err <= 2.0 ** -24, (b, err)


@pytest.mark.parametrize("mode", ["adaptive", "static"])
def test_two_calls_give_identical_bits(mode):
    x, _, step = sc.generated(256, 1000)
    kw = dict(env_floor=1e-4) if mode == "adaptive" else dict(noise_table=np.full(129, 0.05))
    a = backend.fx_specsub(x, "hann", 256, step, mode, exponent=1.5, **kw)
    b = backend.fx_specsub(x, "hann", 256, step, mode, exponent=1.5, **kw)
    assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_each_refusal_raises_before_a_launch():
    ctx = get_context()
    x = sc.burst(830, 200, 2)
    ctx.routes()
    for call, error in ((lambda: backend.fx_specsub(x, "hann", 32768, 16384), NotImplementedError),
                        (lambda: backend.fx_specsub(x, "hann", 2, 1), NotImplementedError),
                        (lambda: backend.fx_specsub(x.astype(complex), "hann", 64, 32), NotImplementedError),
                        (lambda: backend.fx_specsub(x, "hann", 48, 24), ValueError),
                        (lambda: backend.fx_specsub(x, "hann", 64, 0), ValueError),
                        (lambda: SpectralSubtractor().apply(dsp.Signal(None, x, 400_000)), NotImplementedError),
                        (lambda: SpectralSubtractor(adaptive_mode=False).apply(dsp.Signal(None, x, 400_000)),
                         NotImplementedError)):
        with pytest.raises(error):
            call()
    assert not ctx.routes()  # nothing was launched
    # the library's own answers, past the Python guards: DS_ERR_UNSUP = -2 before anything is allocated
    import ctypes as C
    w, y = np.ones(32768), np.zeros_like(x)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = ctx.lib.ds_fx_specsub(ctx.handle, p(x), 0, 2, 200, 200, p(w), p(w), 32768, 16384, 0, -40.0, 0.9, 2.0, 2.0, None, 1e-4,
                               p(y), 200)
    assert rc == -2 and not ctx.routes()
