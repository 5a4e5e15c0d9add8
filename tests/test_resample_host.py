"""Rational-ratio resampling without a device.  The long-double direct sum of tests/resample_oracle.py is held to
scipy.signal.resample_poly on every ratio and length of tests/resample_cases.py within twice the forward bound (scipy's own
float64 sum is held to the same bound as the device's); the plan's constants, the C signatures and the exports to the
sources; every refusal of the Python layer and of the C entries to its answer before any device is touched;
resample_filter to the coefficients the reference produced (tests/golden/resample/cases.npz, tools/gen_golden_resample.py);
and the tile plan with the kernel's index arithmetic emulated in a stand-alone C++ program under AddressSanitizer and
UBSan (tests/host_san/resample_plan_san.cpp)."""

import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.signal import resample_poly

import dsptoolbox_amd as dsp
import resample_cases as rc
import resample_oracle as ro
from dsptoolbox_amd import backend, standard
from dsptoolbox_amd._lib import SIGNATURES, load_library

ROOT = rc.ROOT


@pytest.fixture(scope="module")
def gold():
    z = np.load(rc.PATH, allow_pickle=False)
    return json.loads(str(z["meta"])), z


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", rc.RATIOS)
def test_oracle_against_scipy(up, down, capsys):
    worst = 0.0
    for n in rc.all_lengths(up, down):
        x = rc.signal(n)
        value, a = ro.resample_poly(x, up, down)
        want = resample_poly(x, up, down, axis=0)
        assert want.shape == value.shape == (rc.n_out(n, up, down), 5)
        worst = max(worst, ro.worst_ratio(want, value, 2 * ro.bound(a, up, down)))
    with capsys.disabled():
        print(f"\nP({up}, {down}): worst |scipy - oracle| / (2 x bound) = {worst:.3g}")
    assert worst <= 1.0


def test_oracle_scale_is_folded_into_the_taps():
    x = rc.signal(257, 2)
    value, a = ro.resample_poly(x, 160, 147, 147 / 160)
    plain, _ = ro.resample_poly(x, 160, 147)
    lim = 2 * ro.bound(a, 160, 147)  # one rounding per tap: within the bound of the sum
    assert ro.worst_ratio((plain * ro.LD(147 / 160)).astype(np.float64), value, lim) <= 1.0
    assert np.array_equal(backend._resample_taps(160, 147), ro.taps(160, 147))


def test_term_counts_of_the_issue():
    assert [rc.terms(*r) for r in ((160, 147), (147, 160), (2, 3), (80, 441), (147, 640))] == [21, 22, 31, 111, 88]
    assert rc.terms(640, 147) * 640 * 8 <= 110 * 1024  # 12801 taps, padded to 21 per phase


# ---- plan, constants, ABI --------------------------------------------------------------------------------------------
def test_plan_constants_match_the_header():
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "resample_plan.hpp")).read()

    def const(name):
        return re.search(rf"constexpr int {name} = ([^;]+);", src).group(1)

    assert int(const("NT")) == rc.NT == backend.RESAMPLE_NT
    assert int(const("PASSES")) == rc.PASSES == backend.RESAMPLE_PASSES
    assert const("LDS_DOUBLES") == "160 * 1024 / 8" and rc.LDS_DOUBLES == backend.RESAMPLE_LDS_DOUBLES == 160 * 1024 // 8
    assert int(const("MAX_RATE")) == rc.MAX_RATE == backend.RESAMPLE_MAX_RATE >= 640
    guards = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert f"kResampleMaxRate = {backend.RESAMPLE_MAX_RATE};" in guards
    assert "kResampleMaxSamples = (int64_t)1 << 31;" in guards and backend.RESAMPLE_MAX_SAMPLES == 1 << 31
    assert f"kResampleMaxChannels = {backend.RESAMPLE_MAX_CHANNELS};" in guards
    # the backend's restatement of the plan is the cases' one, and every plan fits the LDS
    for up, down in rc.RATIOS + [(640, 639), (639, 640), (2, 639)]:
        for n_ch in rc.CHANNELS:
            p = rc.plan(up, down, n_ch)
            assert backend._resample_tile(up, down, n_ch) == (p["tile"], p["chunks"], p["span"], p["lds_bytes"])
            assert p["lds_bytes"] <= 160 * 1024 and p["tile"] >= 1 and p["jc"] >= 1 and p["tile"] * p["cg"] <= rc.PASSES * rc.NT
    assert rc.plan(1, 640, 5)["chunks"] > 1 and all(rc.plan(u, d, c)["chunks"] == 1 for u, d in rc.RATIOS[:-1] for c in rc.CHANNELS)
    from dsptoolbox_amd._build import NO_SCRATCH
    assert "k_resample_poly" in NO_SCRATCH


def test_edge_lengths_straddle_the_tile():
    for up, down in rc.RATIOS:
        for n_ch in rc.CHANNELS:
            tile = rc.plan(up, down, n_ch)["tile"]
            outs = [rc.n_out(n, up, down) for n in rc.edge_lengths(up, down, n_ch)]
            assert any(o >= tile for o in outs) and any(o > tile for o in outs), (up, down, n_ch, outs)
            assert tile == 1 or any(o < tile for o in outs), (up, down, n_ch, outs)
            if up <= down:  # every output length exists
                assert outs == [tile - 1, tile, tile + 1][3 - len(outs):], (up, down, n_ch, outs)


def test_signatures_and_exports():
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    lib = load_library()
    for name, n_args in (("ds_resample_poly", 8), ("ds_resample_poly_dev", 10)):
        assert hasattr(lib, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args == len(SIGNATURES[name][1])
    for name in ("resample", "resample_filter"):
        assert name in standard.__all__ and callable(getattr(standard, name))
    assert "resample" in dsp.__all__ and dsp.resample is dsp.standard.resample
    E = inspect.Parameter.empty

    def pars(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    assert pars(dsp.resample) == [("sig", E), ("desired_sampling_rate_hz", E), ("rescaling", False)]
    assert pars(standard.resample_filter) == [("filter", E), ("new_sampling_rate_hz", E)]
    assert callable(backend.resample_poly) and callable(backend.resample_poly_device)


# ---- nothing here reaches the device -----------------------------------------------------------------------------------
def test_decided_without_a_device(monkeypatch):
    def no_device(*a, **k):
        raise RuntimeError("the device was called")

    monkeypatch.setattr(backend, "get_context", no_device)
    x = rc.signal(64, 2)
    s = dsp.Signal(None, x, 44100)
    # a rate of 1 / 1
    same = dsp.resample(s, 44100)
    assert same is not s and np.array_equal(same.time_data, x) and same.sampling_rate_hz == 44100
    copy = backend.resample_poly(x, 3, 3)
    assert np.array_equal(copy, x) and copy is not x and not np.shares_memory(copy, x)
    assert np.array_equal(backend.resample_poly(x, 7, 7, 0.5), x * 0.5)
    # a bad ratio, no samples
    for up, down in ((0, 1), (1, 0), (-2, 3), (1.5, 1)):
        with pytest.raises(ValueError):
            backend.resample_poly(x, up, down)
    with pytest.raises(ValueError):
        backend.resample_poly(np.zeros((0, 2)), 3, 2)
    # beyond the bounds, each named
    with pytest.raises(NotImplementedError, match="RESAMPLE_MAX_RATE"):
        dsp.resample(s, 44101)
    with pytest.raises(NotImplementedError, match="RESAMPLE_MAX_RATE"):
        backend.resample_poly(x, 641, 640)
    backend._resample_ratio("resample_poly", 1280, 2, 64, 2)  # reduced first: 640 / 1 is inside
    with pytest.raises(NotImplementedError, match="RESAMPLE_MAX_SAMPLES"):
        backend.resample_poly(np.zeros((1 << 25, 1)), 100, 1)  # 3.4e9 output samples (the zeros are never touched)
    with pytest.raises(NotImplementedError, match="RESAMPLE_MAX_SAMPLES"):
        backend._resample_ratio("resample_poly", 1, 100, (1 << 31) + 1, 1)  # the input counts as well
    backend._resample_ratio("resample_poly", 2, 1, 1 << 30, 1)  # 2^31 output samples: the bound itself is inside
    with pytest.raises(NotImplementedError, match="RESAMPLE_MAX_CHANNELS"):
        backend._resample_ratio("resample_poly", 3, 2, 10, 65536)
    # complex signals
    c = dsp.Signal(None, x + 1j * x, 44100)
    assert c.is_complex_signal
    with pytest.raises(NotImplementedError, match="imaginary"):
        dsp.resample(c, 48000)
    with pytest.raises(NotImplementedError, match="complex"):
        backend.resample_poly(x + 1j * x, 3, 2)
    # the true peak keeps its refusal
    with pytest.raises(NotImplementedError):
        dsp.crest_factor(s, use_true_peak=True)


def test_entries_check_their_arguments():
    lib = load_library()
    p = backend._ptr
    x, taps, out = np.zeros((10, 2)), np.zeros(61), np.zeros((15, 2))
    ok = (p(x), 10, 2, 3, 2, p(taps), p(out))
    assert lib.ds_resample_poly(None, *ok) == -1                                           # no context
    assert lib.ds_resample_poly(None, None, *ok[1:]) == -1                                 # null samples
    assert lib.ds_resample_poly(None, p(x), 0, 2, 3, 2, p(taps), p(out)) == -1             # no samples
    assert lib.ds_resample_poly(None, p(x), 10, 0, 3, 2, p(taps), p(out)) == -1            # no channels
    assert lib.ds_resample_poly(None, p(x), 10, 2, 1, 1, p(taps), p(out)) == -1            # 1 / 1 is the caller's copy
    assert lib.ds_resample_poly(None, p(x), 10, 2, 6, 4, p(taps), p(out)) == -1            # not reduced
    assert lib.ds_resample_poly(None, p(x), 10, 2, 641, 640, p(taps), p(out)) == -2        # one step past each bound
    assert lib.ds_resample_poly(None, p(x), 10, 2, 1, 641, p(taps), p(out)) == -2
    assert lib.ds_resample_poly(None, p(x), (1 << 30) + 1, 2, 2, 3, p(taps), p(out)) == -2
    assert lib.ds_resample_poly(None, p(x), 1 << 30, 1, 3, 1, p(taps), p(out)) == -2
    assert lib.ds_resample_poly(None, p(x), 10, 65536, 3, 2, p(taps), p(out)) == -2
    assert lib.ds_resample_poly(None, p(x), 1 << 30, 2, 2, 3, p(taps), p(out)) == -1        # inside: the null context
    assert lib.ds_resample_poly_dev(None, p(x), 10, 10, 2, 3, 2, p(taps), p(out), 15) == -1
    assert lib.ds_resample_poly_dev(None, p(x), 10, 10, 2, 641, 640, p(taps), p(out), 15) == -2


# ---- resample_filter -------------------------------------------------------------------------------------------------
def test_resample_filter_against_the_reference(gold, capsys):
    meta, z = gold
    assert [(f["kind"], f["fs"], f["new_fs"]) for f in meta["filters"]] == [
        ("butter4", 48000, 44100), ("butter4", 44100, 96000), ("peaking", 48000, 44100), ("peaking", 44100, 96000)]
    worst = 0.0
    for i, f in enumerate(meta["filters"]):
        filt = dsp.Filter.from_zpk(z[f"filt_{i}_z"], z[f"filt_{i}_p"], float(z[f"filt_{i}_k"]), f["fs"])
        new = standard.resample_filter(filt, f["new_fs"])
        assert type(new) is dsp.Filter and new.sampling_rate_hz == f["new_fs"] and filt.sampling_rate_hz == f["fs"]
        nz, np_, nk = new.get_coefficients(dsp.FilterCoefficientsType.Zpk)
        for got, want in ((nz, z[f"filt_{i}_rz"]), (np_, z[f"filt_{i}_rp"])):
            got, want = np.sort_complex(np.asarray(got, dtype=complex)), np.sort_complex(want)
            assert got.shape == want.shape
            worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
            assert np.allclose(got, want, rtol=1e-12, atol=0)
        assert np.isclose(nk, float(z[f"filt_{i}_rk"]), rtol=1e-12, atol=0)
        worst = max(worst, abs(nk / float(z[f"filt_{i}_rk"]) - 1))
    with capsys.disabled():
        print(f"\nresample_filter: largest relative difference of a zero, pole or gain {worst:.2e}")


def test_golden_signals_are_rebuilt(gold):
    meta, z = gold
    assert list(meta["cases"]) == list(rc.GOLDEN)
    for name in rc.GOLDEN:
        x = rc.golden_signal(name)
        assert x.shape == (rc.GOLDEN_N, rc.GOLDEN_CH) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
        assert np.array_equal(z[name + "_probe"], np.concatenate([x[:16, 0], [x.sum()]])), name
    assert meta["cases"]["overshoot_44100_48000"]["scale_factor"] < 1.0 and np.abs(rc.golden_signal("overshoot_44100_48000")).max() < 1.0
    assert meta["cases"]["ir_48000_44100"]["type"] == "ImpulseResponse"


# ---- the plan under the sanitizers -----------------------------------------------------------------------------------
def test_plan_and_index_arithmetic_under_sanitizers(tmp_path):
    """tests/host_san/resample_plan_san.cpp: csrc/resample_plan.hpp followed tile by tile and chunk by chunk for every
    ratio, length and channel count of resample_cases, in both layouts: every LDS read inside the staged span, every tap
    inside the padded table, every output written once, the sums equal to the definition."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = os.path.join(ROOT, "tests", "host_san", "resample_plan_san.cpp")
    exe, cases = str(tmp_path / "resample_plan_san"), tmp_path / "cases.txt"
    lines = [f"{u} {d} {c} {n}" for u, d in rc.RATIOS for c in rc.CHANNELS for n in rc.lengths(u, d, c)]
    cases.write_text("\n".join(lines) + "\n")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"resample_plan_san: ok ({len(lines)} cases, both layouts)" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    for u, d in rc.RATIOS:
        for c in rc.CHANNELS:
            p = rc.plan(u, d, c)
            for n in rc.lengths(u, d, c):
                for layout in ("interleaved", "planar"):
                    assert (f"up {u} down {d} ch {c} n {n} {layout}: tile {p['tile']} chunks {p['chunks']} span {p['span']} "
                            f"lds {p['lds_bytes']} bytes, n_out {rc.n_out(n, u, d)},") in r.stdout
