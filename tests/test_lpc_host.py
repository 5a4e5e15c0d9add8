"""Linear prediction without a GPU.  The numpy restatements of tests/lpc_oracle.py (framing, Yule-Walker, Burg, the
all-pole filters and the overlap-add) are held to every case of tests/golden/lpc/cases.npz, which
tools/gen_golden_lpc.py made by running the reference: in float64 within 1e-9 -- the bound the device is held to; two
float64 evaluations that add in different orders differ by what either differs from the truth, measured 4.7e-11 at most,
at order = L - 1 -- and in long double within 1e-11, the generator's own assertion (measured: 7.0e-12 for Yule-Walker at
order = L - 1, 1.5e-13 / 4.4e-13 for Burg's a / den, 1.9e-15 for the synthesis).  The arrangements the kernels use --
Burg's two error rows updated in place, the transposed direct form II with four states per lane, the overlap-add
gathered per output sample -- are restated too and agree with the plain forms.  Then the reference's quirks (Burg's
L + 1 rows, NaN and zero patterns of silent frames), the argument checks and bounds of the Python layer and of the C
entries, all of which answer before any device is touched."""

import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.signal import get_window, lfilter

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DeviceError, load_library
from lpc_oracle import (all_pole, burg, channel_error, coefficient_error, levinson, overlap_add, synthesize,
                        variance_error, windowed_frames, yule_walker)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
_cache = {}


def golden():
    if not _cache:
        z = np.load(os.path.join(ROOT, "tests", "golden", "lpc", "cases.npz"), allow_pickle=False)
        import json
        _cache["z"], _cache["meta"] = {k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"]))
    return _cache["z"], _cache["meta"]


def frames_of_case(z, case):
    window = get_window("hann", case["L"], fftbins=True)
    return windowed_frames(z[case["sig"]], window, case["hop"]), window


def estimate(td, order, method, dtype):
    if method == "yw":
        a, var, singular = yule_walker(td, order, dtype)
        assert not singular
        return a, var
    return burg(td, order, dtype)


def test_new_names_exist():
    assert callable(dsp.transforms.lpc) and "lpc" in dsp.transforms.__all__
    assert callable(backend.lpc) and callable(backend.levinson_durbin) and callable(backend.lpc_synthesize)
    lib = load_library()
    for name in ("ds_lpc", "ds_lpc_dev", "ds_levinson", "ds_lpc_synth"):
        assert hasattr(lib, name)


def test_python_bounds_are_the_sources():
    text = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert int(re.search(r"kLpcMaxWindow = (\d+);", text).group(1)) == backend.LPC_MAX_WINDOW
    assert int(re.search(r"kLpcMaxOrder = (\d+);", text).group(1)) == backend.LPC_MAX_ORDER
    assert float(re.search(r"kLpcMaxWork = ([0-9.e+]+);", text).group(1)) == backend.LPC_MAX_WORK
    assert "kLpcMaxPairs = ((int64_t)1 << 31) - 1;" in text and backend.LPC_MAX_PAIRS == 2 ** 31 - 1
    kernels = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "kernels_lpc.hpp")).read()
    assert int(re.search(r"MAX_LAGS = (\d+);", kernels).group(1)) == backend.LPC_MAX_ORDER + 1
    # the LDS a workgroup declares at the largest window stays within 160 KiB
    L = backend.LPC_MAX_WINDOW
    assert (2 * L + 2 * 256 + 8) * 8 <= 160 * 1024 and (L + 260 + 2 * 256) * 8 <= 160 * 1024


def test_estimators_match_the_reference_and_the_long_double_oracle():
    z, meta = golden()
    worst = {}
    for i, case in enumerate(meta["cases"]):
        td, _ = frames_of_case(z, case)
        assert td.shape[1] == -(-len(z[case["sig"]]) // case["hop"])
        for method in case["methods"]:
            ref_a, ref_var = z[f"{method}_{i}_a"], z[f"{method}_{i}_var"]
            if method == "burg":  # the reference's L + 1 rows, zeros after row `order`
                assert ref_a.shape[0] == case["L"] + 1 and not ref_a[case["order"] + 1:].any()
                ref_a = ref_a[:case["order"] + 1]
            assert ref_a.shape == (case["order"] + 1,) + td.shape[1:] and ref_var.shape == td.shape[1:]
            for dtype, bound in ((np.float64, 1e-9), (LD, 1e-11)):
                a, var = estimate(td, case["order"], method, dtype)
                ea, ev = coefficient_error(a, ref_a), variance_error(var, ref_var)
                key = (method, dtype.__name__)
                worst[key] = tuple(max(p) for p in zip(worst.get(key, (0.0, 0.0)), (ea, ev)))
                assert ea <= bound and ev <= bound, (case, method, dtype, ea, ev)
    print("worst (a, var) error against the fixtures:", worst)


def test_silent_frames_follow_ieee():
    z, meta = golden()
    for i, n_silent in ((9, 1), (10, 1)):  # N % hop == 1; hop = 1: the last frame starts on the signal's last sample
        case = meta["cases"][i]
        td, _ = frames_of_case(z, case)
        silent = ~td.any(axis=(0, 2))
        assert silent.sum() == n_silent and silent[-1]
        a, var = z[f"yw_{i}_a"], z[f"yw_{i}_var"]
        assert np.isnan(a[1:, silent]).all() and (a[0] == 1).all() and np.isnan(var[silent]).all()
        assert np.isfinite(a[:, ~silent]).all() and np.isfinite(var[~silent]).all()
        a, var = z[f"burg_{i}_a"], z[f"burg_{i}_var"]
        assert (a[0, silent] == 1).all() and not a[1:, silent].any() and not var[silent].any()
        # the restatement gives the same patterns (coefficient_error and variance_error assert them)
        for method in ("yw", "burg"):
            got_a, got_var = estimate(td, case["order"], method, np.float64)
            coefficient_error(got_a, z[f"{method}_{i}_a"][:case["order"] + 1])
            variance_error(got_var, z[f"{method}_{i}_var"])


def test_levinson_on_the_stored_autocorrelations_and_the_singular_case():
    z, meta = golden()
    for i in meta["levinson"]:
        a, var, singular = levinson(z[f"r_{i}"])
        assert not singular
        assert coefficient_error(a, z[f"yw_{i}_a"]) <= 1e-9 and variance_error(var, z[f"yw_{i}_var"]) <= 1e-9
    a, var, singular = levinson(np.array([[1.0, 1.0], [1.0, 0.5]]))
    assert singular and var[0] == 0.0 and a[1, 0] == -1.0 and var[1] == 0.75


def test_synthesis_chain_matches_the_reference():
    z, meta = golden()
    for j, case in enumerate(meta["synthesis"]):
        window = get_window("hann", case["L"], fftbins=True)
        a, var, src, out = (z[f"syn_{j}_{k}"] for k in ("a", "var", "sources", "out"))
        np.random.seed(case["seed"])  # the draws line up: channel outer, frame inner
        for c in range(var.shape[1]):
            for f in range(var.shape[0]):
                assert np.array_equal(np.random.normal(0.0, var[f, c] ** 0.5, case["L"]), src[:, f, c])
        assert out.shape == z[case["sig"]].shape
        e64 = channel_error(synthesize(a, src, window, case["hop"], len(out)), out)
        eld = channel_error(synthesize(a, src, window, case["hop"], len(out), LD), out)
        print(f"synthesis {j}: float64 restatement {e64:.2e}, long double {eld:.2e}")
        assert e64 <= 1e-9 and eld <= 1e-11
        filtered = all_pole(a, src)
        for f, c in ((0, 0), (var.shape[0] - 1, var.shape[1] - 1)):
            assert np.allclose(filtered[:, f, c], lfilter([1.0], a[:, f, c], src[:, f, c]), rtol=0, atol=1e-12 * np.abs(filtered[:, f, c]).max())


# ---- the arrangements of csrc/kernels_lpc.hpp ------------------------------------------------------------------------
def burg_in_place(x, order):
    """k_lpc_burg for one frame: pass i's forward error j at EF[j + i], its backward error j at EB[j]."""
    L = len(x)
    EB, EF = x.copy(), np.concatenate([x[1:], [0.0]])
    M = L - 1
    den = np.sum(EF[:M] ** 2 + EB[:M] ** 2)
    cur, prev = np.zeros(order + 1), np.zeros(order + 1)
    cur[0] = prev[0] = 1.0
    for i in range(order):
        n = M - i
        rc = -2.0 * np.sum(EB[:n] * EF[i:i + n]) / (den + np.finfo(np.float64).eps)
        cur, prev = prev, cur
        for t in range(1, i + 2):
            cur[t] = prev[t] + rc * prev[i - t + 1]
        fe, be = EF[i:i + n].copy(), EB[:n].copy()
        EF[i:i + n], EB[:n] = fe + rc * be, be + rc * fe
        den = (1.0 - rc * rc) * den - EB[n - 1] ** 2 - EF[i] ** 2
    return cur, den


def df2t_blocked(a, x, taps=4, lanes=64):
    """k_lpc_filter for one pair: state z[k] in lane k // taps, slot k % taps; z[k] <- z[k + 1] - a[k + 1] y."""
    order = len(a) - 1
    ak = np.zeros((lanes, taps))
    live = np.zeros((lanes, taps), dtype=bool)
    for k in range(order):
        ak[k // taps, k % taps], live[k // taps, k % taps] = a[k + 1] / a[0], True
    z = np.zeros((lanes, taps))
    y = np.empty(len(x))
    for n in range(len(x)):
        y[n] = z[0, 0] + x[n] / a[0]
        up = np.concatenate([z[1:, 0], [0.0]])  # lane l receives z[taps (l + 1)], the last lane nothing
        for q in range(taps):
            nxt = z[:, q + 1] if q + 1 < taps else up
            z[:, q] = np.where(live[:, q], nxt - ak[:, q] * y[n], 0.0)
    return y


def ola_gather(frames, window, hop, n_out):
    """k_lpc_ola: per output sample the covering frames in frame order."""
    L, n_frames, n_ch = frames.shape
    out = np.zeros((n_out, n_ch))
    for n in range(n_out):
        f_lo = (n - L) // hop + 1 if n >= L else 0
        f_hi = min(n_frames - 1, n // hop)
        s, env = np.zeros(n_ch), 0.0
        for f in range(f_lo, f_hi + 1):
            m = n - f * hop
            assert 0 <= m < L
            s += frames[m, f] * window[m]
            env += window[m] * window[m]
        out[n] = s / max(env, 1e-4)
    return out


def test_kernel_arrangements_agree_with_the_plain_forms():
    z, meta = golden()
    case = meta["cases"][3]  # L = 250, hop = 100, order = 32
    td, window = frames_of_case(z, case)
    a, den = burg(td, case["order"])
    for f, c in ((0, 0), (4, 1), (td.shape[1] - 1, 2)):
        a1, den1 = burg_in_place(td[:, f, c], case["order"])
        assert np.allclose(a1, a[:, f, c], rtol=0, atol=1e-12 * np.abs(a[:, f, c]).max())
        assert abs(den1 - den[f, c]) <= 1e-11 * abs(den[f, c])
    sa, src = z["syn_1_a"], z["syn_1_sources"]
    for order_cut in (32, 5, 3):  # a full lane, two lanes, less than one
        coeffs = sa[:order_cut + 1, 2, 1]
        want = lfilter([1.0], coeffs, src[:, 2, 1])
        assert np.allclose(df2t_blocked(coeffs, src[:, 2, 1]), want, rtol=0, atol=1e-12 * np.abs(want).max())
    frames = all_pole(sa, src)
    for hop, n_out in ((100, 1000), (100, 1200), (300, 1000), (1, 300)):  # padded; hop > L; hop = 1
        fr = frames[:, :5] if hop != 100 else frames
        want = overlap_add(fr, window, hop, n_out)
        assert np.allclose(ola_gather(fr, window, hop, n_out), want, rtol=0, atol=1e-13 * np.abs(want).max())


# ---- the Python layer and the C entries answer before any device -----------------------------------------------------
def test_validation_and_guards_raise_without_a_device():
    fs = 48000
    s = dsp.Signal(None, np.random.default_rng(0).standard_normal((400, 2)), fs)
    for kw in (dict(order=0, window_length_samples=64), dict(order=64, window_length_samples=64),
               dict(order=70, window_length_samples=64), dict(order=4, window_length_samples=64, hop_size_samples=0),
               dict(order=1, window_length_samples=1)):
        with pytest.raises(ValueError):
            dsp.transforms.lpc(s, **kw)
    cplx = dsp.Signal(None, np.ones((400, 1)) + 1j * np.ones((400, 1)), fs)
    with pytest.raises(ValueError, match="real"):
        dsp.transforms.lpc(cplx, 4, 64)
    with pytest.raises(ValueError, match="real"):
        backend.lpc(np.ones((400, 1), dtype=np.complex128), 4, np.ones(64), 32)
    long = dsp.Signal(None, np.zeros((20000, 1)), fs)
    with pytest.raises(NotImplementedError, match="bounds"):
        dsp.transforms.lpc(long, 4, backend.LPC_MAX_WINDOW + 1)
    with pytest.raises(NotImplementedError, match="bounds"):
        dsp.transforms.lpc(long, backend.LPC_MAX_ORDER + 1, 1024, use_burg_method=True)
    n_over = int(backend.LPC_MAX_WORK / (backend.LPC_MAX_WINDOW * (backend.LPC_MAX_ORDER + 1))) + 2
    with pytest.raises(NotImplementedError, match="work"):
        dsp.transforms.lpc(dsp.Signal(None, np.zeros((n_over, 1)), fs), backend.LPC_MAX_ORDER, backend.LPC_MAX_WINDOW,
                           hop_size_samples=1)
    backend._lpc_guard(2048 * 64, 1, 1024, 32)  # the shape the timing tool runs (64 channels x 2^20 samples)
    backend._lpc_guard(1, 1, backend.LPC_MAX_WINDOW, backend.LPC_MAX_ORDER)
    with pytest.raises(NotImplementedError):
        backend._lpc_guard(2 ** 31, 1, 64, 4)
    with pytest.raises(NotImplementedError):
        backend.levinson_durbin(np.ones((backend.LPC_MAX_ORDER + 2, 1)))
    with pytest.raises(ValueError):
        backend.levinson_durbin(np.ones((1, 3)))
    with pytest.raises(NotImplementedError):
        backend.lpc_synthesize(np.ones((5, 2, 1)), np.ones((backend.LPC_MAX_WINDOW + 1, 2, 1)),
                               np.ones(backend.LPC_MAX_WINDOW + 1), 32, 100)


def test_no_gpu_means_device_error():
    if load_library().ds_device_count() > 0:
        pytest.skip("GPU present")
    s = dsp.Signal(None, np.random.default_rng(0).standard_normal((400, 2)), 48000)
    for burg_method in (False, True):
        with pytest.raises(DeviceError):
            dsp.transforms.lpc(s, 4, 64, use_burg_method=burg_method)
    with pytest.raises(DeviceError):
        backend.levinson_durbin(np.array([[1.0], [0.5]]))


def test_entries_check_their_arguments():
    lib = load_library()
    x, w = np.zeros((100, 2)), np.ones(16)
    a, var, flag = np.zeros((5, 13, 2)), np.zeros((13, 2)), C.c_int(0)
    p = backend._ptr
    ok = (p(x), 100, 2, p(w), 16, 8, 4, 0, p(a), p(var), C.byref(flag))
    assert lib.ds_lpc(None, *ok) == -1                                       # no context
    assert lib.ds_lpc(None, None, *ok[1:]) == -1                             # null samples
    assert lib.ds_lpc(None, p(x), 100, 2, p(w), 16, 8, 16, 0, *ok[8:]) == -1   # order >= window length
    assert lib.ds_lpc(None, p(x), 100, 2, p(w), 16, 0, 4, 0, *ok[8:]) == -1    # hop < 1
    assert lib.ds_lpc(None, p(x), 100, 2, p(w), 16, 8, 4, 2, *ok[8:]) == -1    # unknown method
    assert lib.ds_lpc(None, p(x), 100, 2, p(w), 8193, 8, 4, 0, *ok[8:]) == -2  # beyond the window bound
    assert lib.ds_lpc(None, p(x), 100, 2, p(w), 1024, 8, 256, 1, *ok[8:]) == -2  # beyond the order bound
    assert lib.ds_lpc(None, p(x), 10 ** 9, 2, p(w), 8192, 1, 255, 0, *ok[8:]) == -2  # beyond the work bound
    assert lib.ds_lpc_dev(None, None, 2, 100, 100, *ok[3:]) == -1
    assert lib.ds_lpc_dev(None, None, 2, 100, 100, p(w), 8193, 8, 4, 0, *ok[8:]) == -2
    assert lib.ds_levinson(None, None, 4, 3, None, None, None) == -1
    assert lib.ds_levinson(None, None, 0, 3, None, None, None) == -1
    assert lib.ds_levinson(None, None, 256, 3, None, None, None) == -2
    assert lib.ds_lpc_synth(None, None, None, None, 16, 13, 2, 8, 4, 100, None) == -1
    assert lib.ds_lpc_synth(None, None, None, None, 16, 13, 2, 8, 16, 100, None) == -1
    assert lib.ds_lpc_synth(None, None, None, None, 8193, 13, 2, 8, 4, 100, None) == -2
