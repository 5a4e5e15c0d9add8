"""The audio effects on the device (csrc/kernels_fx.hpp through ds_fx_*): every golden case of the reference through the
classes, and generated shapes -- lengths around the follower's tile, every delay at which the comb changes shape, bands
as streams of one call -- against the long-double oracle of fx_oracle.py, all within BOUND = 1e-12 of each channel's
peak; the detector's mask exactly; device-resident signals against the host path within float32 store rounding."""

import functools
import json
import os
import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import fx_cases as fc
import fx_oracle as fo
from dsptoolbox_amd import backend, effects
from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = backend.FX_FOLLOW_TILE
LENGTHS = fc.follower_lengths(TILE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fx", "cases.npz"))


def signal(seed, n, n_ch):
    return dsp.Signal(None, fc.burst(seed, n, n_ch), fc.FS, constrain_amplitude=False)


def judge(what, got, want, bound=fo.BOUND):
    e = fo.stream_error(got, want)
    print(f"{what}: {e:.2e} of the peak (bound {bound:.1e})")
    assert e <= bound, (what, e)


# ---- the reference's golden vectors through the classes ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.COMPRESSOR))
def test_compressor_golden(golden, name):
    seed, n, n_ch, p = fc.COMPRESSOR[name]
    judge(name, fc.compressor(effects, p).apply(signal(seed, n, n_ch)).time_data, golden[f"compressor_{name}"])


@pytest.mark.parametrize("name", list(fc.DETECTOR))
def test_detector_golden(golden, name):
    seed, n, n_ch, p = fc.DETECTOR[name]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        det, others = dsp.activity_detector(signal(seed, n, n_ch), p["threshold_dbfs"], 0, p["relative"], None, 1,
                                            p["release_time_ms"])
    assert np.array_equal(others["signal_indices"], golden[f"detector_{name}"])  # every sample, none left out
    assert np.array_equal(others["noise_indices"], ~golden[f"detector_{name}"]) and not others["signal_indices"][0]
    assert np.array_equal(others["noise"].time_data, golden[f"detector_{name}_noise"])
    if name == "empty":  # (the reference's fallback for a selection its numpy refuses: a warning and 500 zeros)
        assert det.time_data.shape == (500, 1) and not det.time_data.any() and any("No detected activity" in str(i.message) for i in w)
    else:
        assert np.array_equal(det.time_data, golden[f"detector_{name}_signal"])


@pytest.mark.parametrize("name", list(fc.DELAY))
def test_delay_golden(golden, name):
    seed, n, n_ch, p = fc.DELAY[name]
    y = fc.delay(effects, p).apply(signal(seed, n, n_ch)).time_data
    assert y.shape == golden[f"delay_{name}"].shape  # the reference's padding
    judge(name, y, golden[f"delay_{name}"])


@pytest.mark.parametrize("name", list(fc.CHORUS))
def test_chorus_golden(golden, name):
    seed, n, n_ch, p = fc.CHORUS[name]
    np.random.seed(p["seed"])
    judge(name, fc.chorus(effects, p).apply(signal(seed, n, n_ch)).time_data, golden[f"chorus_{name}"])


@pytest.mark.parametrize("name", list(fc.DISTORTION))
def test_distortion_golden(golden, name):
    seed, n, n_ch, p = fc.DISTORTION[name]
    judge(name, fc.distortion(effects, p).apply(signal(seed, n, n_ch)).time_data, golden[f"distortion_{name}"])


@pytest.mark.parametrize("name", list(fc.TREMOLO))
def test_tremolo_golden(golden, name):
    seed, n, n_ch, p = fc.TREMOLO[name]
    np.random.seed(p["seed"])
    judge(name, fc.tremolo(effects, p).apply(signal(seed, n, n_ch)).time_data, golden[f"tremolo_{name}"])


# ---- the follower over lengths around its tile ------------------------------------------------------------------------
# both directions, knee 0 and above, attack_samples = 0, the threshold relative and absolute, make-up gain on and off
FOLLOW = {"down_hard_rel_makeup": dict(threshold_dbfs=-10, attack_time_ms=0.5, release_time_ms=20, ratio=3),
          "up_knee_abs": dict(threshold_dbfs=-16, attack_time_ms=1.0, release_time_ms=12, ratio=4, relative=False, knee_db=5,
                              make_up=False, downward=False),
          "down_knee_attack0_gain": dict(threshold_dbfs=-12, attack_time_ms=0.0, release_time_ms=40, ratio=8, knee_db=3,
                                         pre_gain_db=2.5),
          "up_hard_rel": dict(threshold_dbfs=-22, attack_time_ms=2.0, release_time_ms=8, ratio=2, downward=False, make_up=False)}


@functools.lru_cache(maxsize=None)
def follow_reference(config, n, n_ch):
    want, nearest = fo.compress(fc.burst(100 + n % 97 + n_ch, n, n_ch), fc.FS, **FOLLOW[config])
    assert FOLLOW[config].get("knee_db", 0) > 0 or nearest > 1e-9, (config, n, nearest)  # (a condition of the case)
    return want


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("config", list(FOLLOW))
def test_follower_lengths(config, n):
    p = FOLLOW[config]
    for n_ch in (1, 3):
        x = fc.burst(100 + n % 97 + n_ch, n, n_ch)
        gain = 10 ** (p.get("pre_gain_db", 0) / 20)
        y = backend.fx_compress(x, p["threshold_dbfs"], p["ratio"], p.get("knee_db", 0), int(p["attack_time_ms"] * 1e-3 * fc.FS),
                                int(p["release_time_ms"] * 1e-3 * fc.FS), pre_gain=gain, final_gain=gain,
                                downward=p.get("downward", True), relative=p.get("relative", True), make_up=p.get("make_up", True))
        assert y.shape == (n, n_ch) and y.dtype == np.float64
        with np.errstate(invalid="ignore"):
            judge(f"{config} n={n} ch={n_ch}", y, follow_reference(config, n, n_ch))


def test_eight_bands_of_two_channels_are_streams_of_one_call():
    n, p = TILE + 1, FOLLOW["down_knee_attack0_gain"]
    bands = [signal(200 + b, n, 2) for b in range(8)]
    ctx = get_context()
    ctx.profile_enable(True)
    ctx.profile_report()
    out = fc.compressor(effects, p).apply(dsp.MultiBandSignal(bands))
    launches = ctx.profile_report()
    ctx.profile_enable(False)
    assert launches["fx_follow"][1] == 1 and type(out) is dsp.MultiBandSignal and out.number_of_bands == 8
    for b in range(8):
        judge(f"band {b}", out.bands[b].time_data, fo.compress(bands[b].time_data, fc.FS, **p)[0])


@pytest.mark.parametrize("n", LENGTHS)
def test_detector_lengths(n):
    x = fc.burst(300 + n % 89, n, 3)
    for relative, thr, ms in ((True, -18.0, 25), (False, -27.0, 4)):
        got = backend.fx_detect(x, thr, fo.detector_coefficient(ms, fc.FS), relative)
        assert got.shape == (n, 3) and got.dtype == bool
        for c in range(3):
            want, nearest = fo.detect(x[:, c], fc.FS, thr, relative, ms)
            assert nearest > 1e-9, (n, c, nearest)  # (a condition of the case: the mask is then decided)
            assert np.array_equal(got[:, c], want), (n, relative, c, int(np.sum(got[:, c] != want)))


# ---- comb ---------------------------------------------------------------------------------------------------------------
N_COMB = 300


@pytest.mark.parametrize("saturation", ["digital", "arctan"])
@pytest.mark.parametrize("d", fc.comb_delays(N_COMB))
def test_comb_delays(d, saturation):
    x = fc.burst(400 + d % 83, N_COMB, 2)
    for fb in (0.0, 0.4):
        pad = int(d * (1 + fb * 15))
        y = backend.fx_delay(x, d, pad, fb, saturation)
        assert y.shape == (N_COMB + pad, 2)
        judge(f"d={d} fb={fb} {saturation}", y, fo.delay_samples(x, d, pad, fb, saturation))


# ---- shape: what IEEE arithmetic gives for a silent channel ---------------------------------------------------------------
def test_a_silent_channel_keeps_its_nans():
    x = fc.burst(500, 200, 2)
    x[:, 1] = 0.0
    p = fc.DISTORTION["combined"][3]
    with np.errstate(all="ignore"):
        y = fc.distortion(effects, p).apply(dsp.Signal(None, x, fc.FS, constrain_amplitude=False)).time_data
        want = fo.distort(x, *fc.distortion_lists(p), p["post"])
    assert np.isnan(y[:, 1]).all()
    judge("silent channel", y, want)


# ---- device-resident signals ------------------------------------------------------------------------------------------------
def resident(x):
    return dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), fc.FS)


def held_to_store_rounding(what, got, want):
    e = fo.stream_error(got, want)
    print(f"{what}: {e:.2e} of the peak (float32 store rounding {2.0 ** -24:.2e})")
    assert e <= 2.0 ** -24, (what, e)


@pytest.mark.parametrize("what", ["compressor", "delay", "chorus", "distortion", "tremolo"])
def test_resident_signal_equals_the_host_path_and_stays_resident(what):
    cases = {"compressor": (fc.COMPRESSOR, "knee_up_abs", fc.compressor), "delay": (fc.DELAY, "arctan", fc.delay),
             "chorus": (fc.CHORUS, "three", fc.chorus), "distortion": (fc.DISTORTION, "combined", fc.distortion),
             "tremolo": (fc.TREMOLO, "sawtooth_smooth", fc.tremolo)}
    table, name, make = cases[what]
    seed, n, n_ch, p = table[name]
    x = fc.burst(seed, n, n_ch)
    np.random.seed(p.get("seed", 0))
    host = make(effects, p).apply(dsp.Signal(None, x, fc.FS, constrain_amplitude=False)).time_data
    np.random.seed(p.get("seed", 0))
    out = make(effects, p).apply(resident(x))
    assert out.on_device and out.device_samples.n_samples == host.shape[0]
    held_to_store_rounding(what, out.time_data, host)


def test_resident_bands_and_the_resident_detector():
    n, n_ch, n_bands = TILE + 7, 2, 3
    x = [fc.burst(600 + b, n, n_ch) for b in range(n_bands)]
    ctx = get_context()
    owner = DeviceBuffer.from_array(ctx, np.concatenate([np.ascontiguousarray(b.T, dtype=np.float32) for b in x]))
    bands = [dsp.Signal.from_planar_f32(DevicePlanar(owner, n_ch, n, n, 4 * b * n_ch * n), fc.FS) for b in range(n_bands)]
    comp = fc.compressor(effects, FOLLOW["up_knee_abs"])
    ctx.profile_enable(True)
    ctx.profile_report()
    out = comp.apply(dsp.MultiBandSignal(bands))
    launches = ctx.profile_report()
    ctx.profile_enable(False)
    assert launches["fx_follow"][1] == 1 and out.on_device
    for b in range(n_bands):
        host = comp.apply(dsp.Signal(None, x[b], fc.FS, constrain_amplitude=False)).time_data
        held_to_store_rounding(f"band {b}", out.bands[b].time_data, host)
    _, others = dsp.activity_detector(bands[1], -20, 1)
    want, nearest = fo.detect(x[1][:, 1], fc.FS, -20, True, 25)
    assert nearest > 1e-9 and np.array_equal(others["signal_indices"], want)


def test_detector_pre_filter_gates_on_the_filtered_samples():
    s = signal(700, 600, 2)
    f = dsp.Filter.iir_filter(4, [300.0, 900.0], dsp.FilterPassType.Bandpass, fc.FS)
    det, others = dsp.activity_detector(s, -25, 1, True, f)
    filtered = f.filter_signal(s.get_channels(1), zero_phase=True).time_data[:, 0]
    want, nearest = fo.detect(filtered, fc.FS, -25, True, 25)
    assert nearest > 1e-9 and np.array_equal(others["signal_indices"], want)
    assert np.array_equal(det.time_data[:, 0], s.time_data[want, 1])  # (the unfiltered samples are what is returned)
