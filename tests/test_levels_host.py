"""Levels and loudness without a device: the long-double oracle against the reference's recorded outputs
(tests/golden/levels/cases.npz, tools/gen_golden_levels.py), the public interface's signatures, assertions and refusals
(none of which reaches the device), and the host helpers merge_filters, to_db / from_db, FadeType and the fade tables."""

import inspect
import json
import os
import re

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import fft64_cases as f64c
import levels_cases as lc
import levels_oracle as lo
from dsptoolbox_amd import backend, standard
from dsptoolbox_amd.standard import gain_and_level as gl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITY = 1e-9  # the generator's bound on the reference against the oracle, of the peak


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "levels", "cases.npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z


def sig(n=64, n_ch=2, fs=lc.FS):
    return dsp.Signal(None, lc.noise(1, n, n_ch), fs, constrain_amplitude=False)


# ---- the oracle against the golden file ----------------------------------------------------------------------------
def test_oracle_normalize_gain_fade(gold):
    _, z = gold
    for name, (seed, n, n_ch, dbfs, pk, each) in lc.NORMALIZE.items():
        x = lc.noise(seed, n, n_ch)
        assert lo.relative_to_peak(z[f"normalize_{name}"], lo.normalize(x, dbfs, pk, each)) <= SANITY, name
        bound = 4 * lo.reduction_depth(n) * lc.U
        assert np.max(np.abs(z[f"rms_{name}"] - lo.rms(x)) / lo.rms(x)) <= bound, name
        assert np.allclose(z[f"rms_db_{name}"], 20 * np.log10(z[f"rms_{name}"]), rtol=0, atol=1e-12)
        assert np.max(np.abs(z[f"crest_{name}"] - lo.peak(x) / lo.rms(x))) <= 1e-12, name
    for name, (seed, n, n_ch, g) in lc.GAIN.items():
        assert lo.relative_to_peak(z[f"gain_{name}"], lo.gain(lc.noise(seed, n, n_ch), g)) <= SANITY, name
    for name, (seed, n, n_ch, kind, l_s, a, b) in lc.FADE.items():
        l_eff = int(n / lc.FS * 0.025 * lc.FS) if l_s is None else l_s
        assert lo.relative_to_peak(z[f"fade_{name}"], lo.fade(lc.noise(seed, n, n_ch), kind, l_eff, a, b)) <= 1e-14, name


def test_oracle_detrend_and_envelopes(gold):
    meta, z = gold
    x = lc.detrend_input()
    for order in lc.DETREND_ORDERS:
        e = lo.relative_to_peak(z[f"detrend_{order}"], lo.detrend(x, order))
        assert e <= SANITY and e == pytest.approx(meta["measured"]["detrend"][str(order)], rel=1e-6, abs=1e-18), order
    for name, (seed, n, n_ch) in lc.ENVELOPE_ANALYTIC.items():
        assert lo.relative_to_peak(z[f"env_analytic_{name}"], lo.envelope_analytic(lc.noise(seed, n, n_ch))) <= SANITY, name
    for name, (_, _, _, w, _) in lc.ENVELOPE_BOXCAR.items():
        want = lo.moving_mean_square(lc.boxcar_input(name), w)
        got = np.nan_to_num(z[f"env_boxcar_{name}"], nan=0.0) ** 2
        assert np.max(np.max(np.abs(got - want), axis=0) / np.max(want, axis=0)) <= SANITY, name


@pytest.mark.parametrize("name", list(lc.LUFS))
def test_oracle_lufs(gold, name):
    _, z = gold
    x, fs = lc.lufs_input(name)
    zo, _ = lo.lufs_blocks(x, fs)
    value, _, _, both, _ = lo.lufs_gating(zo)
    assert zo.shape == z[f"lufs_{name}_z"].shape
    if zo.shape[0] == 0:
        assert np.isnan(value) and np.isnan(z[f"lufs_{name}"])
        return
    assert np.max(np.abs(z[f"lufs_{name}_z"] - zo) / zo) <= SANITY
    assert np.array_equal(both, z[f"lufs_{name}_gated"]) and abs(value - float(z[f"lufs_{name}"])) <= SANITY


def test_golden_case_conditions(gold):
    meta, z = gold
    m = meta["measured"]
    assert min(meta["seen"].values()) >= 1, meta["seen"]
    for name, rec in m["lufs"].items():
        assert min(rec["margin_absolute"], rec["margin_relative"]) > meta["gate_margin_lu"], name
    tg, step = lc.lufs_blocks(8000)
    assert lc.LUFS_EDGE_LENGTHS == (tg - 1, tg, tg + 1, tg + step, tg + step + 1) and lc.lufs_blocks(11025) == (4410, 1103)
    for n_ch in (2, 5):
        vals = [float(z[f"lufs_edge_{n}_{n_ch}ch"]) for n in lc.LUFS_EDGE_LENGTHS]
        assert np.isnan(vals[:2]).all() and np.isfinite(vals[2:]).all(), vals
        assert vals[2] == vals[3] != vals[4]  # tg + step samples: the second full block is lost to the ceil
    # the wrong oracles miss their bounds by orders of magnitude
    assert set(meta["wrong_oracles"]) == set(lc.WRONG_ORACLES)
    assert m["wrong_rms"] > 1e3 * 4 * lo.reduction_depth(1001) * lc.U
    assert m["wrong_fade"] > 1e3 * 1e-14 and m["wrong_lufs"] > 1e3 * meta["lufs_tol"]
    assert m["wrong_envelope"] > 1e3 * f64c.tolerance(("hilbert", 8192))


# ---- constants, basis, ABI -----------------------------------------------------------------------------------------
def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "kernels_level.hpp")).read()

    def const(name):
        return re.search(rf"constexpr int {name} = ([^;]+);", src).group(1)

    assert int(const("NT")) == lc.NT == backend.LEVEL_NT
    assert int(const("PER_LANE")) == lc.PER_LANE == backend.LEVEL_PER_LANE
    assert const("SPAN") == "NT * PER_LANE" and lc.SPAN == backend.LEVEL_SPAN == lc.NT * lc.PER_LANE
    assert const("TILE") == "NT * TILE_PER_LANE" and int(const("TILE_PER_LANE")) * lc.NT == lc.TILE == backend.LEVEL_TILE
    assert int(const("VEC_BYTES")) == lc.VEC_BYTES == backend.LEVEL_VEC_BYTES
    assert int(const("MAX_ORDER")) == lc.MAX_ORDER == backend.LEVEL_MAX_ORDER
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    for name, value in backend.LEVEL_NORMS.items():
        assert re.search(rf"#define DS_LEVEL_NORM_{name.upper()} {value}\b", header), name
    guards = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert f"kLevelMaxChannels = {backend.LEVEL_MAX_CHANNELS};" in guards and "kLevelMovingMaxWork = 1e12;" in guards
    assert backend.LEVEL_MAX_SAMPLES == (1 << 31) - 1 and backend.LEVEL_MAX_ELEMENTS == 1 << 33


@pytest.mark.parametrize("n", [1, 2, 9, 10, 1000, lc.SPAN + 1, 1 << 20])
def test_basis_is_orthonormal_and_matches_the_oracle(n):
    order = min(lc.MAX_ORDER, n - 1)
    b = backend.level_basis(n, order)
    assert b.shape == (18,) and b[0] == (n - 1) / 2
    t = np.arange(n) - b[0]
    P = [np.full(n, b[1])]
    for k in range(order):
        P.append(b[2 + k] * t * P[k] - (b[10 + k] * P[k - 1] if k else 0.0))
    P = np.array(P)
    assert np.max(np.abs(P @ P.T - np.eye(order + 1))) <= 64 * n ** 0.5 * lc.U + 1e-14
    assert np.max(np.abs(P - lo.gram_basis(n, order))) <= 1e-12
    with pytest.raises(AssertionError):
        backend.level_basis(n, n)


def test_entries_are_declared():
    from dsptoolbox_amd._lib import SIGNATURES
    assert {"ds_level_project", "ds_level_stats", "ds_level_apply", "ds_moving_rms", "ds_loudness_blocks",
            "ds_envelope_analytic"} <= set(SIGNATURES)
    build = open(os.path.join(ROOT, "dsptoolbox_amd", "_build.py")).read()
    for kernel in ("k_level_project", "k_level_final", "k_level_stats", "k_level_apply", "k_level_moving", "k_level_blocks", "k_level_mag"):
        assert f'"{kernel}"' in build, kernel  # the no-spill gate covers the new kernels


# ---- the public interface ------------------------------------------------------------------------------------------
def test_exports_and_signatures():
    names = ["normalize", "rms", "crest_factor", "fade", "apply_gain", "lufs_integrated", "detrend", "envelope", "merge_filters"]
    for name in names:
        assert name in standard.__all__ and name in dsp.__all__ and getattr(dsp, name) is getattr(standard, name), name
    assert "FadeType" in dsp.__all__ and dsp.FadeType is standard.enums.FadeType
    assert [m.name for m in dsp.FadeType] == ["Linear", "Exponential", "Logarithmic", "NoFade"]

    def pars(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert pars(dsp.normalize) == [("sig", E), ("norm_dbfs", E), ("peak_normalization", True), ("each_channel", False)]
    assert pars(dsp.rms) == [("sig", E), ("in_dbfs", True)]
    assert pars(dsp.crest_factor) == [("sig", E), ("in_db", True), ("use_true_peak", False)]
    assert pars(dsp.fade) == [("sig", E), ("fade_type", E), ("length_fade_seconds", None), ("at_start", True), ("at_end", True)]
    assert pars(dsp.apply_gain) == [("target", E), ("gain_db", E)]
    assert pars(dsp.detrend) == [("sig", E), ("polynomial_order", 0)]
    assert pars(dsp.envelope) == [("signal", E), ("analytic", True), ("window_length_samples", None)]
    assert pars(dsp.lufs_integrated) == [("s", E)]
    assert pars(dsp.merge_filters) == [("filters", E)]
    assert pars(dsp.tools.to_db)[:3] == [("x", E), ("amplitude_input", E), ("dynamic_range_db", None)]
    assert pars(dsp.tools.from_db) == [("x", E), ("amplitude_output", E)]


def test_refusals_reach_no_device(monkeypatch):
    def no_device(*a, **k):
        raise RuntimeError("the device was called")

    monkeypatch.setattr(backend, "get_context", no_device)
    s = sig()
    for call in (lambda: dsp.normalize(np.zeros(4), -3), lambda: dsp.rms("x"), lambda: dsp.crest_factor(3.0),
                 lambda: dsp.apply_gain([1.0], 3), lambda: dsp.detrend(np.zeros(4)), lambda: dsp.envelope(None)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(NotImplementedError, match="resampl"):
        dsp.crest_factor(s, use_true_peak=True)
    with pytest.raises(AssertionError):
        dsp.detrend(s, -1)
    with pytest.raises(NotImplementedError, match="up to 8"):
        dsp.detrend(s, 9)
    with pytest.raises(AssertionError):
        dsp.envelope(s, analytic=False)
    with pytest.raises(AssertionError):
        dsp.envelope(s, analytic=False, window_length_samples=0)
    with pytest.raises(AssertionError):
        dsp.fade(s, dsp.FadeType.Linear, at_start=False, at_end=False)
    with pytest.raises(AssertionError):
        dsp.fade(s, dsp.FadeType.Linear, length_fade_seconds=1.0)  # longer than the signal
    with pytest.raises(AssertionError):
        dsp.fade(s, dsp.FadeType.Linear, length_fade_seconds=-1.0)
    with pytest.raises(ValueError):
        dsp.fade(s, "Linear", length_fade_seconds=0.002)
    with pytest.raises(AssertionError):
        dsp.lufs_integrated(sig(64, 6))
    with pytest.raises(ValueError):
        dsp.apply_gain(s, [1.0, 2.0, 3.0])
    long = dsp.Signal(None, np.zeros(((1 << 22) + 2, 1)), 48000, constrain_amplitude=False)
    with pytest.raises(NotImplementedError, match="transform"):
        dsp.envelope(long)
    with pytest.raises(AssertionError):
        backend.loudness_blocks(np.zeros((4000, 1)), np.zeros((0, 6)), 3200, 800)
    with pytest.raises(NotImplementedError, match="32"):
        backend.loudness_blocks(np.zeros((4000, 1)), np.tile([1.0, 0, 0, 1, 0, 0], (33, 1)), 3200, 800)
    with pytest.raises(NotImplementedError, match="LEVEL_MOVING_MAX_WORK"):
        backend.moving_rms(np.zeros((1 << 22, 64)), 1 << 22)
    with pytest.raises(AssertionError):
        dsp.envelope(dsp.MultiBandSignal([s, sig(fs=4000)], same_sampling_rate=False))


# ---- host helpers ----------------------------------------------------------------------------------------------------
def test_db_conversions(gold):
    _, z = gold
    v = z["db_in"]
    with np.errstate(divide="ignore"):
        assert np.array_equal(dsp.tools.to_db(v, True), z["to_db_amp"]) and np.array_equal(dsp.tools.to_db(v, False), z["to_db_pow"])
        assert np.array_equal(dsp.tools.to_db(v, True, dynamic_range_db=40.0), z["to_db_range"])
        assert np.array_equal(dsp.tools.to_db(v[:3], False, None, None), z["to_db_noclip"])
    assert np.array_equal(dsp.tools.from_db(np.array([-6.0, 0.0, 3.0]), True), z["from_db_amp"])
    assert np.array_equal(dsp.tools.from_db(np.array([-6.0, 0.0, 3.0]), False), z["from_db_pow"])
    assert dsp.tools.to_db(0.0, True) == 20 * np.log10(np.finfo(np.float64).smallest_normal)


def test_fade_tables(gold):
    _, z = gold
    for kind in ("Linear", "Exponential", "Logarithmic"):
        assert np.array_equal(gl._fade_table(getattr(dsp.FadeType, kind), 300), z[f"fadetable_{kind}"]), kind
        assert np.max(np.abs(z[f"fadetable_{kind}"] - lo.fade_table(kind, 300))) <= 1e-14
    with pytest.raises(ValueError):
        gl._fade_table(dsp.FadeType.NoFade, 10)


def test_merge_filters_and_filter_gain(gold):
    _, z = gold
    iir = [dsp.Filter.biquad(dsp.BiquadEqType.Highshelf, 1500, 4.0, 2**0.5 / 2.0, 48000),
           dsp.Filter.biquad(dsp.BiquadEqType.Highpass, 38.1, 0.0, 0.5, 48000)]
    merged = dsp.merge_filters(iir)
    assert np.allclose(merged.sos, z["merge_sos"], rtol=1e-13, atol=0) and merged.sampling_rate_hz == 48000
    assert np.array_equal(dsp.merge_filters(dsp.FilterBank(iir)).sos, merged.sos)
    assert np.allclose(gl._k_weighting_sos(48000), z["merge_sos"], rtol=1e-13, atol=0)
    for k, s in enumerate(lo.k_weighting(48000)):  # the oracle's own biquads
        assert np.allclose(merged.sos[k], (s / s[3]).astype(float), rtol=1e-12, atol=0)
    fir = [dsp.Filter.from_ba(np.array([1.0, 0.5, 0.25]), [1.0], 48000), dsp.Filter.from_ba(np.array([0.5, -0.25]), [1.0], 48000)]
    assert np.allclose(dsp.merge_filters(fir).ba[0], z["merge_fir"], rtol=1e-15, atol=1e-17)
    with pytest.raises(AssertionError):
        dsp.merge_filters(fir[:1])
    with pytest.raises(AssertionError):
        dsp.merge_filters([fir[0], iir[0]])
    with pytest.raises(AssertionError):
        dsp.merge_filters([fir[0], dsp.Filter.from_ba(np.array([1.0]), [1.0], 44100)])
    # apply_gain on coefficients is host arithmetic
    g = 10 ** (6.0 / 20)
    assert np.allclose(dsp.apply_gain(fir[0], 6.0).ba[0], fir[0].ba[0] * g, rtol=1e-15)
    assert np.allclose(dsp.apply_gain(merged, 6.0).sos[-1, :3], merged.sos[-1, :3] * g, rtol=1e-15)
    assert np.array_equal(dsp.apply_gain(merged, 6.0).sos[0], merged.sos[0])
    bank = dsp.apply_gain(dsp.FilterBank(fir), [0.0, 6.0])
    assert np.array_equal(bank.filters[0].ba[0], fir[0].ba[0]) and np.allclose(bank.filters[1].ba[0], fir[1].ba[0] * g, rtol=1e-15)
    with pytest.raises(AssertionError):
        dsp.apply_gain(dsp.FilterBank(fir), [1.0, 2.0, 3.0])


def test_lufs_gating_on_the_reference_blocks(gold):
    """The four host lines of lufs_integrated on the block mean squares the reference formed."""
    _, z = gold
    for name in lc.LUFS:
        got, want = gl._lufs_gating(z[f"lufs_{name}_z"]), float(z[f"lufs_{name}"])
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-12, name
    assert gl._lufs_blocks(11025) == (4410, 1103) and backend.loudness_block_count(3200, 3200, 800) == 0
    assert backend.loudness_block_count(3201, 3200, 800) == 1 and backend.loudness_block_count(4001, 3200, 800) == 2
