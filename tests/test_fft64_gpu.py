"""ds_fft_c128 and ds_hilbert on the device against a long-double oracle, at a bound of four times what a float64
emulation of the same algorithm achieves on the CPU and never above 1e-13 of the column rms: the cases of
tests/fft64_cases.py, one per edge of the three routes of csrc/kernels_fft64.hpp (one workgroup in LDS, four-step up to
2^22, Bluestein up to 2^21 - 1), with up to 4096 columns.  Every case asserts the kernels that ran and prints its worst
error / bound.  Then: scaling the input by 2^+-200 scales the output bit for bit, and a chirp table that the cache's
least-recently-used eviction pushed out is rebuilt to the same bits."""

import os
import re

import numpy as np
import pytest

import fft64_cases as fc
from dsptoolbox_amd import backend

pytestmark = pytest.mark.gpu

IO = {"fft64_load", "fft64_store"}
BLUE = {"fft64_blue", "fft64_lds", "fft64_lds@inv"}


def routes(n, inverse=False, first=None):
    """the launch names ctx.routes() has to report after one call of ds_fft_c128 at n points; first: whether the chirp
    tables are built by this call (None: either)"""
    route, M, _ = fc.plan(n)
    if route != "blue":
        names = IO | ({"fft64_lds@inv" if inverse else "fft64_lds"} if n > 1 else set())
        return [names | ({"fft64_transpose"} if route == "four" else set())]
    names = IO | BLUE | ({"fft64_transpose"} if M > fc.LDS_MAX else set())
    return [names | {"fft64_chirp"}] if first else [names] if first is False else [names, names | {"fft64_chirp"}]


@pytest.mark.parametrize("ident", fc.IDENTS)
def test_float64_transform_route_matrix(ident):
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    c = fc.case(ident)
    failed, worst = [], 0.0
    for i, q in enumerate(c["calls"]):
        x = fc.call_input(c, i)
        ctx.routes()
        if c["fn"] == "hilbert":
            out = backend.hilbert(x)
            assert ctx.routes() - {"fft64_chirp"} == (routes(c["n"])[0] | routes(c["n"], True)[0] | {"fft64_point"}), ident
        else:
            out = backend.fft_c128(x, c["n"], inverse=q["inverse"])
            assert ctx.routes() in routes(c["n"], q["inverse"]), (fc.call_name(c, i), ctx.routes())
        try:
            worst = max(worst, fc.judge_call(c, i, out, fc.oracle(c, i, x)))
        except AssertionError as e:  # (judge every call of the case before failing it)
            failed.append(e)
            print(f"fft64 {fc.call_name(c, i)}: FAILED {e}")
    tol = fc.tolerance(c["key"])
    print(f"fft64 {ident}: worst error / bound {worst:.3f} = {worst * tol / fc.EPS:.3g} eps of the column rms "
          f"(bound {tol:.3g}, {len(c['calls'])} calls)")
    assert not failed, failed


@pytest.mark.parametrize("n", [8192, 1 << 15, 4097])
def test_a_power_of_two_scales_the_result_exactly(n):
    """The algorithm is linear, and nothing overflows or goes subnormal at 2^+-200: fft(x 2^k) = fft(x) 2^k bit for bit,
    forward and inverse, real and complex, on the LDS route, the four-step and Bluestein."""
    rng = np.random.default_rng(64000 + n)
    real = rng.standard_normal((n, 2))
    real[:, 1] *= 1e-3
    for x in (real, real + 1j * rng.standard_normal((n, 2))):
        for inverse in (False, True):
            base = backend.fft_c128(x, inverse=inverse)
            assert np.all(np.isfinite(base)) and base.any()
            for k in (200, -200):
                out = backend.fft_c128(x * 2.0 ** k, inverse=inverse)
                assert np.array_equal(out, base * 2.0 ** k), (n, x.dtype, inverse, k)


def test_an_evicted_chirp_table_is_rebuilt_to_the_same_bits():
    """Seven lengths just above 600000 (M = 2^21, one channel): each table is (n + 2^21) x 16 B = 43.2e6 B, six are 258.9e6
    of the cap's 268.4e6 (256 MiB) and seven 302.1e6: whatever the cache held before is older and goes first, so building
    the seventh pushes the first length's table out and the last six stay.  The first length again: its tables are built again
    (fft64_chirp runs), the result is bit-identical to the first call's and within the oracle bound.  The last length
    again: no table is built, the same bits."""
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    api = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dsptoolbox_amd", "csrc", "api.hip")).read()
    (mb,) = re.findall(r"kBlue64CapBytes = \(size_t\)(\d+) << 20;", api)
    cap = int(mb) << 20
    lengths = [600001 + 2 * k for k in range(7)]
    table = lambda n: (n + fc.plan(n)[1]) * 16
    assert all(fc.plan(n)[:2] == ("blue", 1 << 21) for n in lengths)
    assert sum(table(n) for n in lengths[1:]) <= cap < sum(table(n) for n in lengths)  # the first is pushed out, six stay
    rng = np.random.default_rng(600001)
    xs = [rng.standard_normal((n, 1)) + 1j * rng.standard_normal((n, 1)) for n in lengths]
    outs = []
    for n, x in zip(lengths, xs):
        ctx.routes()
        outs.append(backend.fft_c128(x))
        if n != lengths[0]:  # (another test may have left the first length's table behind)
            assert ctx.routes() in routes(n, first=True), (n, ctx.routes())
    ctx.routes()
    again = backend.fft_c128(xs[0])
    assert ctx.routes() in routes(lengths[0], first=True), "the first length's table was not evicted"
    assert np.array_equal(again, outs[0])
    c = fc.adhoc(lengths[0], [fc.call_spec(1, lengths[0], True, False)])
    worst = fc.judge_call(c, 0, again, fc.oracle_fft(xs[0], lengths[0], False))
    print(f"fft64 after eviction, n = {lengths[0]}: worst error / bound {worst:.3f}")
    ctx.routes()
    assert np.array_equal(backend.fft_c128(xs[-1]), outs[-1])
    assert ctx.routes() in routes(lengths[-1], first=False), "the last length's table did not stay"
