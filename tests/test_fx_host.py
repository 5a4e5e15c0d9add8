"""The audio effects on the CPU: the long-double oracle against every golden array of the reference, the exported names,
constructor and setter assertions, the reference's quirks that raise, the musical-rhythm helpers, LFO waveforms and
seeded phases bit for bit, the chorus index table, the work-bound refusals and the library's new symbols.  No sample is
computed here by the package: that is the device's work (test_fx_gpu.py)."""

import json
import os
import re

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import fx_cases as fc
import fx_oracle as fo
from dsptoolbox_amd import backend, effects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fx", "cases.npz"))
    return z, json.loads(str(z["meta"]))


def judge(what, got, want):
    e = fo.stream_error(got, want)
    print(f"{what}: {e:.2e} of the peak (bound {fo.BOUND:.0e})")
    assert e <= fo.BOUND, (what, e)


# ---- the oracle against the reference's outputs --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.COMPRESSOR))
def test_oracle_compressor(golden, name):
    seed, n, n_ch, p = fc.COMPRESSOR[name]
    judge(name, fo.compress(fc.burst(seed, n, n_ch), fc.FS, **p)[0], golden[0][f"compressor_{name}"])


@pytest.mark.parametrize("wrong", list(fc.WRONG_ORACLES))
def test_a_wrong_oracle_misses_the_bound_widely(golden, wrong):
    name = fc.WRONG_ORACLES[wrong]
    seed, n, n_ch, p = fc.COMPRESSOR[name]
    e = fo.stream_error(fo.compress(fc.burst(seed, n, n_ch), fc.FS, wrong=wrong, **p)[0], golden[0][f"compressor_{name}"])
    print(f"{wrong}: {e:.2e}")
    assert e > 1e6 * fo.BOUND


@pytest.mark.parametrize("name", list(fc.DETECTOR))
def test_oracle_detector(golden, name):
    seed, n, n_ch, p = fc.DETECTOR[name]
    mask, nearest = fo.detect(fc.burst(seed, n, n_ch)[:, 0], fc.FS, **p)
    assert nearest > 1e-9 and np.array_equal(mask, golden[0][f"detector_{name}"]) and not mask[0]


@pytest.mark.parametrize("name", list(fc.DELAY))
def test_oracle_delay(golden, name):
    seed, n, n_ch, p = fc.DELAY[name]
    want = golden[0][f"delay_{name}"]
    assert want.shape[0] == n + fo.delay_lengths(fc.FS, p["delay_ms"], p["feedback"])[1]
    judge(name, fo.delay(fc.burst(seed, n, n_ch), fc.FS, **p), want)


@pytest.mark.parametrize("name", list(fc.CHORUS))
def test_oracle_chorus_and_the_index_table(golden, name):
    seed, n, n_ch, p = fc.CHORUS[name]
    np.random.seed(p["seed"])
    table, half = fc.chorus_table(fc.chorus(effects, p), n)
    assert half > 1e-6 and np.array_equal(table, golden[0][f"chorus_{name}_table"])
    np.random.seed(p["seed"])
    assert np.array_equal(fc.chorus(effects, p)._delay_table(fc.FS, n), table)
    judge(name, fo.chorus(fc.burst(seed, n, n_ch), table, p["mix_percent"] / 100), golden[0][f"chorus_{name}"])


@pytest.mark.parametrize("name", list(fc.DISTORTION))
def test_oracle_distortion(golden, name):
    seed, n, n_ch, p = fc.DISTORTION[name]
    judge(name, fo.distort(fc.burst(seed, n, n_ch), *fc.distortion_lists(p), p["post"]), golden[0][f"distortion_{name}"])


@pytest.mark.parametrize("name", list(fc.TREMOLO))
def test_oracle_tremolo_and_the_modulator(golden, name):
    seed, n, n_ch, p = fc.TREMOLO[name]
    e = fc.tremolo(effects, p)
    np.random.seed(p["seed"])
    mod = np.abs(e.modulator.get_waveform(fc.FS, n) * e.depth + 1)
    assert np.array_equal(mod, golden[0][f"tremolo_{name}_mod"])
    judge(name, fo.tremolo(fc.burst(seed, n, n_ch), mod), golden[0][f"tremolo_{name}"])


def test_the_cases_keep_the_coefficient_floor():
    for _, _, _, p in fc.COMPRESSOR.values():
        for ms in (p.get("attack_time_ms", 0.5), p.get("release_time_ms", 20)):
            assert fo.coefficient(int(ms * 1e-3 * fc.FS)) >= fo.C_MIN
    assert fo.coefficient(0) == 1.0 == backend.fx_follower_coefficient(0)
    assert backend.fx_follower_coefficient(160) == fo.coefficient(160) == 1 - np.exp(np.log(1 - 0.95) / 160)


# ---- tables the host builds ------------------------------------------------------------------------------------------
def test_lfo_waveforms_and_seeded_phases_bit_for_bit(golden):
    for i, (freq, waveform, random_phase, smooth, length, seed) in enumerate(fc.LFOS):
        np.random.seed(seed)
        w = effects.LFO(freq, waveform, random_phase, smooth).get_waveform(fc.FS, length)
        assert np.array_equal(w, golden[0][f"lfo_{i}"]), (i, waveform)
    lfo = effects.LFO(3, "square")
    lfo.set_parameters(waveform="Triangle", smooth=2)
    assert lfo.frequency_hz == 3 and lfo.smooth == 2 and lfo.oscillator is effects.LFO(1, "triangle").oscillator
    with pytest.raises(ValueError):
        effects.LFO(1, "noise")
    with pytest.raises(TypeError):
        effects.LFO("fast")
    with pytest.raises(AssertionError):
        effects.LFO(("quarter", 60, 1))
    with pytest.raises(NotImplementedError):
        lfo.plot_waveform()


def test_musical_rhythm_helpers(golden):
    got = np.array([effects.get_frequency_from_musical_rhythm(n, b) for n, b in fc.RHYTHMS])
    assert np.array_equal(got, golden[0]["rhythm"])
    assert effects.get_time_period_from_musical_rhythm("quarter", 120) == 1 / got[0]
    with pytest.raises(ValueError):
        effects.get_frequency_from_musical_rhythm("breve", 100)
    with pytest.raises(AssertionError):
        effects.get_frequency_from_musical_rhythm("quarter", "100")


# ---- the API surface ------------------------------------------------------------------------------------------------------
def test_exported_names():
    assert effects.__all__ == ["AudioEffect", "Compressor", "Distortion", "DistortionType", "Tremolo", "Chorus",
                               "DigitalDelay", "LFO", "get_frequency_from_musical_rhythm",
                               "get_time_period_from_musical_rhythm"]
    assert all(hasattr(effects, n) for n in effects.__all__) and not hasattr(effects, "SpectralSubtractor")
    assert dsp.effects is effects and "effects" in dsp.__all__
    assert dsp.activity_detector is dsp.standard.activity_detector and "activity_detector" in dsp.__all__
    assert "activity_detector" in dsp.standard.__all__
    assert [t.name for t in effects.DistortionType] == ["Arctan", "HardClip", "SoftClip", "NoDistortion"]


def test_compressor_parameters():
    c = effects.Compressor()
    assert (c.threshold_dbfs, c.attack_time_ms, c.release_time_ms, c.ratio, c.relative_to_peak_level) == (-10, 0.5, 20, 3, True)
    assert (c.knee_factor_db, c.pre_gain_db, c.post_gain_db, c.mix, c.automatic_make_up_gain, c.downward_compression) == \
        (0, 0, 0, 1.0, True, True)
    c.set_parameters(ratio=5)
    assert c.ratio == 5 and c.threshold_dbfs == -10
    with pytest.warns(UserWarning):
        effects.Compressor(threshold_dbfs=3)
    for bad in (dict(attack_time_ms=-1), dict(release_time_ms=-1), dict(ratio=0.5)):
        with pytest.raises(AssertionError):
            effects.Compressor(**bad)
    for bad in (dict(knee_factor_db=-1), dict(mix_percent=0), dict(mix_percent=101)):
        with pytest.raises(AssertionError):
            c.set_advanced_parameters(**bad)
    with pytest.raises(NotImplementedError):
        c.show_compression()
    with pytest.raises(TypeError):
        c.apply(np.zeros(10))


def test_distortion_parameters():
    d = effects.Distortion()
    assert np.array_equal(d.mix, [1.0, 0.0]) and np.array_equal(d.distortion_levels, [20, 0]) and d.post_gain_db == 0
    assert d.offset_db[0] == -np.inf and d.offset_db[1] == -np.inf
    T = effects.DistortionType
    with pytest.raises(AssertionError):
        d.set_advanced_parameters(mix_percent=120)
    with pytest.raises(AssertionError):
        d.set_advanced_parameters([T.Arctan, T.HardClip], np.array([1, 2]), np.array([50, 40]), np.array([-np.inf, -np.inf]))
    with pytest.raises(AssertionError):
        d.set_advanced_parameters([T.Arctan, T.HardClip], np.array([1, 2, 3]), np.array([50, 50]), np.array([-np.inf, -np.inf]))
    with pytest.raises(ValueError):
        d.set_advanced_parameters("arctan")


def test_tremolo_and_chorus_parameters():
    t = effects.Tremolo()
    assert t.depth == 0.5 and type(t.modulator) is effects.LFO and t.modulator.frequency_hz == 1
    with pytest.raises(AssertionError):  # an ndarray modulator never passes the reference's type check
        effects.Tremolo(0.5, np.ones(100))
    for depth in (0, 1.5):
        with pytest.raises(AssertionError):
            effects.Tremolo(depth)
    c = effects.Chorus()
    assert c.number_of_voices == 1 and c.mix == 1.0 and c.modulators[0].frequency_hz == 2 and c.modulators[0].random_phase
    assert np.array_equal(c.depths_ms, [5]) and np.array_equal(c.base_delays_ms, [15])
    c3 = effects.Chorus([1, 2, 3])
    assert c3.number_of_voices == 3 and len(c3.modulators) == 3 and np.array_equal(c3.base_delays_ms, [15, 15, 15])
    with pytest.raises(AssertionError):
        effects.Chorus(modulators=np.ones((100, 1)))
    with pytest.raises(AssertionError):
        effects.Chorus(base_delays_ms=0)
    with pytest.raises(AssertionError):
        effects.Chorus([1, 2, 3], [1, 2])
    with pytest.raises(AssertionError):
        effects.Chorus(modulators=[effects.LFO(1), "lfo"])
    with pytest.raises(AssertionError):
        effects.Chorus(mix_percent=0)


def test_delay_parameters():
    d = effects.DigitalDelay()
    assert (d.delay_ms, d.feedback, d.saturation) == (300, 0.1, "digital")
    d.set_advanced_parameters("ArcTan")
    assert d.saturation == "arctan"
    with pytest.raises(AttributeError):  # a callable ends at .lower() before it is ever used
        d.set_advanced_parameters(lambda v: v)
    with pytest.raises(AssertionError):
        effects.DigitalDelay(0)
    with pytest.raises(AssertionError):
        effects.DigitalDelay(10, 0)
    with pytest.raises(NotImplementedError):
        d.plot_delay()


def test_activity_detector_assertions():
    s = dsp.Signal(None, fc.burst(1, 100, 2), fc.FS)
    for bad in (dict(channel=[0]), dict(channel=0.0), dict(threshold_dbfs=0), dict(release_time_ms=-1), dict(attack_time_ms=-1),
                dict(pre_filter="lowpass")):
        with pytest.raises(AssertionError):
            dsp.activity_detector(s, **bad)


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def test_work_bounds_refuse_before_the_device():
    guards = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    for name, value in (("kFxMaxStreams", backend.FX_MAX_STREAMS), ("kFxMaxCurves", backend.FX_MAX_CURVES),
                        ("kFxMaxVoices", backend.FX_MAX_VOICES)):
        assert int(re.search(rf"{name} = (\d+);", guards).group(1)) == value
    for name, value in (("kFxMaxSamples", backend.FX_MAX_SAMPLES), ("kFxMaxElements", backend.FX_MAX_ELEMENTS)):
        assert 1 << int(re.search(rf"{name} = \(int64_t\)1 << (\d+);", guards).group(1)) == value
    kernels = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "kernels_fx.hpp")).read()
    assert int(re.search(r"FOLLOW_TILE = (\d+);", kernels).group(1)) == backend.FX_FOLLOW_TILE
    assert int(re.search(r"constexpr int NT = (\d+);", kernels).group(1)) == backend.FX_THREADS
    for args, word in (((backend.FX_MAX_STREAMS + 1, 10), "FX_MAX_STREAMS"), ((1, backend.FX_MAX_SAMPLES + 1), "FX_MAX_SAMPLES"),
                       ((1 << 12, 1 << 20), "FX_MAX_ELEMENTS")):
        with pytest.raises(NotImplementedError, match=word):
            backend._fx_guard(*args)
    with pytest.raises(NotImplementedError, match="FX_MAX_VOICES"):
        backend.fx_chorus(np.zeros((4, 1)), np.ones((4, backend.FX_MAX_VOICES + 1), dtype=int), 1.0)
    with pytest.raises(NotImplementedError, match="FX_MAX_CURVES"):
        backend.fx_distort(np.zeros((4, 1)), [0] * 9, [1.0] * 9, [0.0] * 9, [1 / 9] * 9)
    with pytest.raises(NotImplementedError, match="complex"):
        backend.fx_tremolo(np.zeros((4, 1), dtype=complex), np.ones(4))
    many = dsp.Signal(None, np.zeros((70000, 2)), fc.FS)
    with pytest.raises(NotImplementedError, match="FX_MAX_SAMPLES"):
        effects.DigitalDelay(40e6, 0.5).apply(many)  # the repetitions' padding alone is beyond the bound


def test_library_exports_the_new_symbols():
    from dsptoolbox_amd import _build
    from dsptoolbox_amd._lib import SIGNATURES, load_library
    lib = load_library(_build.build_library())
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    for name in ("ds_fx_compress", "ds_fx_detect", "ds_fx_delay", "ds_fx_chorus", "ds_fx_distort", "ds_fx_tremolo"):
        decl = re.search(rf"int {name}\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(SIGNATURES[name][1]) and hasattr(lib, name)
        assert "x_on_device" in decl
    for k in ("k_fx_stats", "k_fx_follow", "k_fx_comb", "k_fx_voices", "k_fx_curve_peak", "k_fx_shape", "k_fx_tremolo",
              "k_fx_scale"):
        assert k in _build.NO_SCRATCH
