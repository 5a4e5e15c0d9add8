"""ds_rfft / ds_rfft_dev and ds_deconv / ds_deconv_dev on the device at every four-step length 2^15 ... 2^24 and on every
Bluestein M from 2^15 to 2^24 (tests/xform_cases.py: all ten k_big_rows kernels, the fullest and emptiest length of an
M, odd, prime and even lengths, the largest length the library takes), every output judged per element against the
float64 oracle at a bound of four times what a float32 emulation achieves on the CPU (1e-6 ... 1.5e-5 of the row's
rms).  Every call asserts the kernels that ran.  Then: a repeated call returns the same bits; the lengths the library
does not take are refused with xform_check's words before anything is launched or written; and a device input whose
row stride exceeds n_samples is read up to n_samples and no further (the tails are NaN).

On an MI355X (2026-10-21), worst error / bound over all lengths, calls and both entries of a family: four-step rfft
0.247 (2^19; 0.242 at 2^24, 0.234 at 2^23), Bluestein rfft 0.269 (1001; 0.253 at 65535, 0.231 at 8388607), four-step
deconv 0.287 (2^21; 0.251 at 2^24), Bluestein deconv 0.289 (1572864; 0.270 at 8388607); the pitched device rows 0.213 ...
0.236.  That is the float32 emulation's own error, 1.0 ... 1.2 times over: no case came near its bound and nothing had to be
fixed in the kernels.  The largest cases take: rfft 2^24 2.2 s (0.8 s of it the oracles), deconv 2^24 4.1 s (1.8 s),
rfft 8388607 3.2 s (2.6 s), deconv 8388607 6.0 s (4.8 s); every other case under 2.1 s, the whole file 31 s.
"""

import ctypes as C
import time

import numpy as np
import pytest

import route_oracles as ros
import xform_cases as xc
from xform_calls import deconv_route_case, rfft_route_case, route_call

pytestmark = pytest.mark.gpu

FOUR_STEP = {"bigfft_cols", "bigfft_rows"}
ROUTES = {("rfft", True): FOUR_STEP | {"bigfft_unpack"}, ("deconv", True): FOUR_STEP | {"bigfft_mul", "bigfft_store"},
          ("rfft", False): FOUR_STEP | {"blue_pre"}, ("deconv", False): FOUR_STEP | {"blue_pre"}}
ENTRY_NAMES = {"rfft": "ds_rfft", "rfft_dev": "ds_rfft_dev", "deconv": "ds_deconv", "deconv_dev": "ds_deconv_dev"}


def expected_routes(family, n_fft):
    """the launch names of one call: the four-step pair and the pair (un)packing kernels for a power of two (cols and
    rows twice in a deconvolution); blue_pre and the four-step pair for Bluestein, twice in a spectrum and four times in
    a deconvolution (and once more where the call builds the chirp filter) -- never `rfft` / `deconv@...`, the LDS
    routes.  ctx.routes() reports names, not counts."""
    return sorted(ROUTES[(family, n_fft & (n_fft - 1) == 0)])


def call(family, entry, p, n_out=None):
    if family == "rfft":
        return rfft_route_case(entry, p)
    return deconv_route_case(entry, dict(p, n_out=n_out))


def sweep(family, n_fft):
    """every call of one length: the launch names, then the values; all calls are judged before the case fails"""
    t0, o0 = time.perf_counter(), ros.seconds["oracle"]
    worst, at, failed, n = 0.0, None, [], 0
    for key, entry, (fam, spec), n_out in xc.calls(family, n_fft):
        p = xc.problem(fam, spec)
        out, routes = call(family, entry, p, n_out)
        assert routes == expected_routes(family, n_fft), (key, routes)
        try:
            frac = xc.judge_call(key, p, out, n_out)
        except AssertionError as e:
            failed.append(e)
            print(f"xform {key}: FAILED {e}")
            continue
        n += 1
        if frac >= worst:
            worst, at = frac, key
    tol = xc.tolerance((family, n_fft))
    print(f"xform {family} {n_fft}: {n} outputs judged, worst error / bound {worst:.3f} at {at} (bound {tol:.3g} of the rms); "
          f"{time.perf_counter() - t0:.1f} s, {ros.seconds['oracle'] - o0:.1f} s of them the oracles")
    assert not failed, failed


@pytest.mark.parametrize("N", xc.FOUR)
def test_four_step_rfft(N):
    sweep("rfft", N)


@pytest.mark.parametrize("L", list(xc.BLUE))
def test_bluestein_rfft(L):
    sweep("rfft", L)


@pytest.mark.parametrize("N", xc.FOUR)
def test_four_step_deconv(N):
    sweep("deconv", N)


@pytest.mark.parametrize("L", xc.BLUE_DECONV)
def test_bluestein_deconv(L):
    sweep("deconv", L)


@pytest.mark.parametrize("n_fft", [1 << 16, 16385])
def test_a_repeated_call_returns_the_same_bits(n_fft):
    """Neither path has atomics, and a cached chirp filter is the one the first call built."""
    for family, spec in (("rfft", (n_fft, xc.short(n_fft), 3)), ("deconv", (n_fft, n_fft, 1, 2, 3))):
        p = xc.problem(family, spec)
        for entry in xc.ENTRIES[family]:
            first, _ = call(family, entry, p, n_fft // 2 + 3)
            again, routes = call(family, entry, p, n_fft // 2 + 3)
            assert routes == expected_routes(family, n_fft), (entry, routes)
            assert first.any() and first.tobytes() == again.tobytes(), (entry, n_fft)


@pytest.mark.parametrize("n_fft", xc.REFUSED)
def test_lengths_beyond_the_transforms_are_refused(n_fft):
    """DS_ERR_UNSUP with xform_check's words, no launch, the host arrays still zero.  Eight samples of two channels."""
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    problems = {"rfft": xc.rfft_problem(n_fft, 8, 2), "deconv": xc.deconv_problem(n_fft, 8, 0, 1, 2)}
    for family, p in problems.items():
        for entry in xc.ENTRIES[family]:
            out, routes = call(family, entry, p, 8)
            assert routes == [f"ERR{xc.DS_ERR_UNSUP}"], (entry, n_fft, routes)
            assert ctx.last_error() == f"{ENTRY_NAMES[entry]} n_fft: {xc.refusal(n_fft)}", (entry, ctx.last_error())
            assert ctx.routes() == set(), entry
            ros.judge_rejected(f"{entry}|{n_fft}", entry, out)


@pytest.mark.parametrize("n_fft", [1 << 16, 16385])
def test_a_device_row_is_read_up_to_n_samples_only(n_fft):
    """ds_rfft_dev and ds_deconv_dev on rows ld = n_samples + 37 apart whose last 37 samples are NaN (the ragged signal
    length: the transform pads from n_samples on): the outputs are finite and within the bound."""
    from dsptoolbox_amd._lib import DeviceBuffer, get_context
    ctx = get_context()
    n, pad = xc.short(n_fft), 37
    for family, spec in (("rfft", (n_fft, n, 3)), ("deconv", (n_fft, n, 1, 1, 3))):
        p = xc.problem(family, spec)
        rows = p["xp"] if family == "rfft" else p["yp"]
        pitched = np.full((len(rows), n + pad), np.nan, np.float32)
        pitched[:, :n] = rows
        dx = DeviceBuffer.from_array(ctx, pitched)
        ctx.routes()
        if family == "rfft":
            do = DeviceBuffer(ctx, p["B"] * 3 * 8)
            routes = route_call(ctx, ctx.lib.ds_rfft_dev, (C.c_void_p(dx.ptr), 3, n + pad, n, n_fft, C.c_float(p["scale"]),
                                                           C.c_void_p(do.ptr)))
            out, bufs = do.to_array((p["B"], 3), np.complex64), (dx, do)
        else:
            dr, do = DeviceBuffer.from_array(ctx, p["r"]), DeviceBuffer(ctx, 3 * n_fft * 4)
            routes = route_call(ctx, ctx.lib.ds_deconv_dev, (C.c_void_p(dx.ptr), 1, 3, n + pad, n, n_fft, C.c_void_p(dr.ptr), 1,
                                                             n_fft, n_fft, C.c_void_p(do.ptr)))
            out, bufs = do.to_array((1, 3, n_fft), np.float32), (dx, dr, do)
        for b in bufs:
            b.free()
        assert routes == expected_routes(family, n_fft), (family, routes)
        frac = xc.judge_call(f"{family}_dev|{n_fft}|ld={n + pad}", p, out, n_fft if family == "deconv" else None)
        print(f"xform {family}_dev {n_fft}, rows {n + pad} apart: worst error / bound {frac:.3f}")
