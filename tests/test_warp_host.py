"""Frequency warping without a GPU.  The long-double table of tests/warp_oracle.py is held to every case of
tests/golden/warp/cases.npz, which tools/gen_golden_warp.py made by running the reference, within 1e-13 of each
channel's peak -- the generator's own assertion (measured there: 3.2e-15 for warp, 1.0e-14 for laguerre) -- and a float64
evaluation of the same table within the 1e-12 the device is held to.  With a factor of 0 the table is the identity and the
output is the input bit for bit.  Then _get_warping_factor's answers, warp_filter against the reference's zpk, the
bounds of the Python layer and of the C entries (all answer before any device is touched), the agreement of the header,
the ctypes signatures and the Python constants with the sources, and the tile schedule with the kernel's arrangement
emulated in a stand-alone C++ program under AddressSanitizer and UBSan (tests/host_san/warp_plan_san.cpp).
Every test prints the largest error it measured."""

import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import SIGNATURES, DeviceError, load_library
from dsptoolbox_amd.transforms import _find_ir_start, _get_warping_factor
import warp_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_z = np.load(os.path.join(ROOT, "tests", "golden", "warp", "cases.npz"), allow_pickle=False)
META = json.loads(str(_z["meta"]))
Z = {k: _z[k] for k in _z.files if k != "meta"}
FS = META["fs"]


def warp_input(case):
    """the samples the reference's warp hands to its table: rolled to the onset, then truncated"""
    td = Z[case["sig"]].astype(np.float64)
    if case["shift_ir"]:
        for ch in range(td.shape[1]):
            td[:, ch] = np.roll(td[:, ch], -_find_ir_start(td[:, ch], -20))
    return td[:case["total_length"]]


def test_new_names_exist():
    for name in ("warp", "laguerre", "warp_filter"):
        assert callable(getattr(dsp.transforms, name)) and name in dsp.transforms.__all__
    for name in ("allpass_table", "warp_time_series", "laguerre_transform"):
        assert callable(getattr(backend, name))
    lib = load_library()
    assert hasattr(lib, "ds_allpass_table") and hasattr(lib, "ds_allpass_table_dev")


def test_header_signatures_and_constants_agree_with_the_sources():
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    for name, n_args in (("ds_allpass_table", 10), ("ds_allpass_table_dev", 11)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args == len(SIGNATURES[name][1])
    guards = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert "kWarpMaxSide = (int64_t)1 << 17;" in guards and backend.WARP_MAX_SIDE == 1 << 17
    assert int(re.search(r"kWarpMaxChannels = (\d+);", guards).group(1)) == backend.WARP_MAX_CHANNELS
    assert float(re.search(r"kWarpMaxWork = ([0-9.e+]+);", guards).group(1)) == backend.WARP_MAX_WORK
    assert wo.G == backend.WARP_GROUP and wo.TJ == wo.WAVE * wo.K["WAVES"]
    assert wo.K["STAGGER"] >= 2 * wo.WAVE - 1  # a column value is read at least 64 steps, one barrier, after it was written
    # the LDS a workgroup declares stays within 160 KiB; the groups fit grid.y
    assert ((wo.K["WAVES"] + 1) * wo.TI + wo.TI * wo.G) * 8 <= 160 * 1024
    assert -(-backend.WARP_MAX_CHANNELS // wo.G) <= 65535
    from dsptoolbox_amd._build import NO_SCRATCH
    assert any("k_allpass_tile" in k for k in NO_SCRATCH)


def test_oracle_reproduces_the_golden_vectors():
    worst = dict(warp=0.0, laguerre=0.0, warp64=0.0, laguerre64=0.0)
    for i, case in enumerate(META["warp"]):
        x, ref = warp_input(case), Z[f"warp_{i}"]
        assert ref.shape == x.shape and ref.dtype == np.float64
        worst["warp"] = max(worst["warp"], wo.channel_error(ref, wo.warp(x, META["used"][i])))
        if len(x) <= 1100:
            worst["warp64"] = max(worst["warp64"], wo.channel_error(wo.warp(x, META["used"][i], np.float64), ref))
    for i, case in enumerate(META["laguerre"]):
        x, ref = Z[case["sig"]].astype(np.float64), Z[f"laguerre_{i}"]
        worst["laguerre"] = max(worst["laguerre"], wo.channel_error(ref, wo.laguerre(x, case["factor"])))
        if len(x) <= 1100:
            worst["laguerre64"] = max(worst["laguerre64"], wo.channel_error(wo.laguerre(x, case["factor"], np.float64), ref))
    print("worst error of the reference against the long-double table, and of a float64 table against the reference:", worst)
    assert worst["warp"] <= 1e-13 and worst["laguerre"] <= 1e-13
    assert worst["warp64"] <= 1e-12 and worst["laguerre64"] <= 1e-12


def test_factor_zero_is_the_identity():
    x = Z["n300c2"].astype(np.float64)
    for dtype in (np.float64, wo.LD):
        assert np.array_equal(wo.warp(x, 0.0, dtype), x) and np.array_equal(wo.laguerre(x, 0.0, dtype), x)
    assert np.array_equal(Z["warp_3"], x)  # the reference's own answer
    # rectangular: the leading samples, zeros behind them
    p, q, row0, col0 = wo.warp_tables(0.0, 300, 310)
    out = wo.allpass_table(x, p, q, row0, col0)
    assert np.array_equal(out[:300], x) and not out[300:].any()


def test_get_warping_factor_answers_like_the_reference():
    for name, value in META["factors"].items():
        got = _get_warping_factor(name, FS)
        assert got == value and _get_warping_factor(name.upper(), FS) == value, (name, got, value)
    assert abs(META["factors"]["bark"] + 0.876) < 1e-3  # the rate goes in in Hz: the same factor at every audio rate
    assert abs(_get_warping_factor("bark", 8000) - _get_warping_factor("bark", 96000)) < 1e-3
    assert _get_warping_factor(-0.5, FS) == -0.5 and _get_warping_factor(0.0, FS) == 0.0
    for bad in (1.0, -1.0, 1.5):
        with pytest.raises(AssertionError):
            _get_warping_factor(bad, FS)
    for bad in (1, np.float64(0.5), None, [0.5]):
        with pytest.raises(TypeError):
            _get_warping_factor(bad, FS)
    for bad in ("mel", "bar", ""):
        with pytest.raises(ValueError):
            _get_warping_factor(bad, FS)


def test_find_ir_start():
    x = np.array([0.0, 0.01, 0.05, 0.2, 1.0, 0.5])
    assert _find_ir_start(x, -20) == 2           # 0.05 < 0.1 <= 0.2
    assert _find_ir_start(x[::-1].copy(), -20) == 0 and _find_ir_start(np.ones(4), -20) == 0
    assert _find_ir_start(-x, 20) == 2           # magnitudes; the sign of the threshold does not matter


def test_warp_filter_matches_the_reference():
    worst = 0.0
    for i, f in enumerate(META["filters"]):
        if f["kind"] == "zpk":
            filt = dsp.Filter.from_zpk(Z[f"filt_{i}_z"], Z[f"filt_{i}_p"], float(Z[f"filt_{i}_k"]), FS)
        else:
            filt = dsp.Filter.from_ba(Z[f"filt_{i}_b"], Z[f"filt_{i}_a"], FS)
        warped = dsp.transforms.warp_filter(filt, f["factor"])
        assert type(warped) is dsp.Filter and warped.sampling_rate_hz == FS
        z, p, k = warped.get_coefficients(dsp.FilterCoefficientsType.Zpk)
        wz, wp, wk = Z[f"filt_{i}_wz"], Z[f"filt_{i}_wp"], Z[f"filt_{i}_wk"]
        assert len(z) == len(p) == len(wz) == len(wp)
        for got, want in ((z, wz), (p, wp)):
            e = np.abs(np.sort_complex(np.asarray(got, dtype=complex)) - np.sort_complex(want.astype(complex))).max()
            worst = max(worst, float(e))
        assert np.isclose(k, wk, rtol=1e-14)
    print(f"warp_filter: largest pole / zero difference {worst:.2e}")
    assert worst <= 1e-12
    with pytest.raises(AssertionError):
        dsp.transforms.warp_filter(filt, 1.0)
    # the map keeps the unit disc, so a warped stable filter is stable: every stored pole passed Filter's stable-poles rule
    assert all(np.abs(Z[f"filt_{i}_wp"]).max() < 1.0 for i in range(len(META["filters"])))


def test_bounds_raise_without_a_device():
    side, ch, work = backend.WARP_MAX_SIDE, backend.WARP_MAX_CHANNELS, backend.WARP_MAX_WORK
    backend._warp_check(side, side, 2)  # the largest two-channel call is inside
    for bad in ((side + 1, 10, 1), (10, side + 1, 1), (10, 10, ch + 1)):
        with pytest.raises(NotImplementedError, match="bounds"):
            backend._warp_check(*bad)
    groups_over = int(work / (side * side)) + 1
    backend._warp_check(side, side, (groups_over - 1) * wo.G)
    with pytest.raises(NotImplementedError, match="work"):
        backend._warp_check(side, side, (groups_over - 1) * wo.G + 1)
    for bad in ((0, 10, 1), (10, 0, 1), (10, 10, 0)):
        with pytest.raises(ValueError):
            backend._warp_check(*bad)
    long = dsp.Signal(None, np.zeros((side + 1, 1)), FS)
    with pytest.raises(NotImplementedError):
        dsp.transforms.warp(long, -0.5, False)
    with pytest.raises(NotImplementedError):
        dsp.transforms.warp(long, "bark", True)
    with pytest.raises(NotImplementedError):
        dsp.transforms.laguerre(long, 0.5)
    with pytest.raises(NotImplementedError):
        backend.allpass_table(np.zeros((10, 1)), 0.5, -0.5, np.zeros(side + 1), np.zeros(10))
    s = dsp.Signal(None, np.zeros((100, 1)), FS)
    for bad in (1.0, -1.0, 2.0):
        with pytest.raises(AssertionError):
            dsp.transforms.warp(s, bad, False)
        with pytest.raises(AssertionError):
            dsp.transforms.laguerre(s, bad)
    with pytest.raises(TypeError):
        dsp.transforms.warp(s, 1, False)
    with pytest.raises(ValueError):
        dsp.transforms.warp(s, "mel", False)
    with pytest.raises(ValueError):
        backend.allpass_table(np.zeros((10, 1)), np.nan, 0.0, np.zeros(10), np.zeros(10))


def test_entries_check_their_arguments():
    lib = load_library()
    p = backend._ptr
    x, row0, col0, out = np.zeros((10, 2)), np.zeros(12), np.zeros(10), np.zeros((12, 2))
    side = backend.WARP_MAX_SIDE
    ok = (p(x), 10, 2, -0.5, 0.5, p(row0), p(col0), 12, p(out))
    assert lib.ds_allpass_table(None, *ok) == -1                                                  # no context
    assert lib.ds_allpass_table(None, None, *ok[1:]) == -1                                        # null samples
    assert lib.ds_allpass_table(None, p(x), 0, 2, *ok[3:]) == -1                                  # no input samples
    assert lib.ds_allpass_table(None, p(x), 10, 0, *ok[3:]) == -1                                 # no channels
    assert lib.ds_allpass_table(None, p(x), 10, 2, -0.5, 0.5, p(row0), p(col0), 0, p(out)) == -1  # no output samples
    assert lib.ds_allpass_table(None, p(x), 10, 2, float("nan"), 0.5, *ok[5:]) == -1
    assert lib.ds_allpass_table(None, p(x), 10, 2, -0.5, float("inf"), *ok[5:]) == -1
    assert lib.ds_allpass_table(None, p(x), side + 1, 2, *ok[3:]) == -2                           # one step past each bound
    assert lib.ds_allpass_table(None, p(x), 10, 2, -0.5, 0.5, p(row0), p(col0), side + 1, p(out)) == -2
    assert lib.ds_allpass_table(None, p(x), 10, backend.WARP_MAX_CHANNELS + 1, *ok[3:]) == -2
    groups_over = int(backend.WARP_MAX_WORK / (side * side)) + 1
    over = (-0.5, 0.5, p(row0), p(col0), side, p(out))
    assert lib.ds_allpass_table(None, p(x), side, (groups_over - 1) * wo.G + 1, *over) == -2
    assert lib.ds_allpass_table(None, p(x), side, (groups_over - 1) * wo.G, *over) == -1         # inside: the null context
    assert lib.ds_allpass_table_dev(None, None, 2, 10, 10, *ok[3:]) == -1
    assert lib.ds_allpass_table_dev(None, None, 2, side + 1, side + 1, *ok[3:]) == -2


def test_no_gpu_means_device_error():
    if load_library().ds_device_count() > 0:
        pytest.skip("GPU present")
    s = dsp.Signal(None, Z["n65c1"].astype(np.float64), FS)
    with pytest.raises(DeviceError):
        dsp.transforms.warp(s, -0.5, False)
    with pytest.raises(DeviceError):
        dsp.transforms.laguerre(s, 0.5)


def test_tile_schedule_and_kernel_arrangement_under_sanitizers(tmp_path):
    """tests/host_san/warp_plan_san.cpp: csrc/warp_plan.hpp followed launch by launch with the tile kernel emulated lane
    by lane, on the issue's rectangular shapes (1, 1), (TI + 1, 5), (5, TJ + 1), (2 TI + 1, 2 TJ + 1), (3 TI, TJ - 1) and
    a few more; out against the table cell by cell within 1e-13, every boundary slot read from the tile that should have
    written it, every cross-wave value read a barrier after it was written."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = os.path.join(ROOT, "tests", "host_san", "warp_plan_san.cpp")
    exe = str(tmp_path / "warp_plan_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "warp_plan_san: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    ti, tj = wo.TI, wo.TJ
    for n_in, n_out in wo.RECT_SHAPES:
        assert f"n_in {n_in} n_out {n_out} " in r.stdout
