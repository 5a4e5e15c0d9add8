"""The cases, oracle, emulation and bound of the float64 any-length transform (fft64_cases.py) without a GPU: the
constants it mirrors are the sources'; every Bluestein length runs on the M the case list claims; the long-double oracle
agrees with the direct sum of test_phase_host.longdouble_dft up to 1024 points; the float64 emulation stays within the
recorded table (re-measured here for every case whose power-of-two transform has at most 2^18 points -- the larger
entries are measured by tools/measure_fft64_emulation.py, which prints the whole table) and every entry within a
quarter of the 1e-13 cap; five deliberately wrong emulations each exceed their case's bound at least ten times over; and
numpy.fft, judged by the same rule, stays within the cap."""

import functools
import os
import re

import numpy as np
import pytest

import fft64_cases as fc
import route_oracles as ros
from test_phase_host import longdouble_dft

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsptoolbox_amd", "csrc")
HOST_POINTS = 1 << 18
HOST = [i for i in fc.IDENTS if fc.case(i)["key"][1] <= HOST_POINTS]


def test_the_constants_are_the_sources():
    hpp = open(os.path.join(CSRC, "kernels_fft64.hpp")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()
    guards = open(os.path.join(CSRC, "size_guards.hpp")).read()

    def one(text, pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    assert one(hpp, r"constexpr int NT = (\d+);") == fc.NT
    assert one(hpp, r"constexpr int LDS_MAX = (\d+), LDS_MAX_LG = 13;") == fc.LDS_MAX == 1 << 13
    assert one(hpp, r"__shared__ double2 tile\[(\d+)\]\[33\];") == fc.TRANSPOSE_TILE
    assert "dim3((unsigned)(cols / 32), (unsigned)(rows / 32), (unsigned)n_cols)" in api
    assert 1 << one(guards, r"kFft64MaxPow2 = \(int64_t\)1 << (\d+);") == fc.MAX_POW2
    assert 1 << one(guards, r"kFft64MaxAny = \(int64_t\)1 << (\d+);") == fc.MAX_ANY
    assert one(api, r"kBlue64CapBytes = \(size_t\)(\d+) << 20;") << 20 == fc.BLUE_CAP_BYTES
    # what the emulation restates
    assert "if (n <= LDS_MAX) return n > 1 ? lds(x, (int)n, lg, 1, 0) : DS_OK;" in api
    assert "const int lg1 = lg / 2, lg2 = lg - lg1, n1 = 1 << lg1, n2 = 1 << lg2;" in api
    assert "while (M < (pl->blue ? 2 * n - 1 : n)) M <<= 1, ++lg;" in api
    assert "const int64_t r = (j * j) % (2 * n);" in hpp and "const int64_t r = (b * k) % p.twid_n;" in hpp


def test_every_case_runs_the_route_it_names():
    for n, M in fc.BLUE_CASES.items():
        assert fc.plan(n)[:2] == ("blue", M) and M // 2 < 2 * n - 1 <= M, n
        assert fc.case(f"blue|{n}")["key"] == ("blue", M)
    tops, bottoms = {}, {}
    for n, M in fc.BLUE_CASES.items():
        tops[M], bottoms[M] = max(tops.get(M, 0), n), min(bottoms.get(M, n), n)
    for M in (512, 8192, 16384):  # bottom and top of an M: 2 n - 1 = M / 2 + 1, and the last length below the power of two M / 2
        assert 2 * bottoms[M] - 1 == M // 2 + 1 and tops[M] == M // 2 - 1, M
    assert 2 * bottoms[1 << 22] - 1 == (1 << 21) + 1 and tops[1 << 22] == fc.MAX_ANY - 1
    assert fc.BLUE_CASES[4095] == fc.LDS_MAX and fc.BLUE_CASES[4097] == 2 * fc.LDS_MAX
    assert 46340 ** 2 < 1 << 31 < 46341 ** 2
    for n in (65537, 1048573):
        assert all(n % d for d in range(2, int(n ** 0.5) + 1)), n
    for n in (3, 5):
        assert fc.BLUE_CASES[n] < fc.NT
    assert all(fc.plan(n)[0] == "lds" for n in fc.LDS_CASES) and max(fc.LDS_CASES) == fc.LDS_MAX
    assert all(fc.plan(n)[0] == "four" for n in fc.FOUR_CASES)
    assert min(fc.FOUR_CASES) == 2 * fc.LDS_MAX and max(fc.FOUR_CASES) == fc.MAX_POW2
    assert {(fc.plan(n)[2] // 2, fc.plan(n)[2] - fc.plan(n)[2] // 2) for n in fc.FOUR_CASES} == {(7, 7), (7, 8), (8, 8), (9, 10),
                                                                                                (10, 11), (11, 11)}
    assert [fc.plan(n)[:2] for n in fc.HILBERT_CASES] == [("four", 1 << 15), ("blue", 16384), ("blue", 16384), ("blue", 8192)]
    for n, C in fc.COLUMN_CASES:
        assert fc.case(f"cols|{n}x{C}")["calls"][0]["n_ch"] == C
    assert (1 << 14) // fc.TRANSPOSE_TILE ** 2 * 33 > 32 and 1000 & 999 and 300 & 299
    # the cross below a transform of 2^20 points: 24 calls, 16 at one point; two calls from there on
    assert len(fc.case("lds|8192")["calls"]) == 24 and len(fc.case("lds|1")["calls"]) == 16
    for i in fc.IDENTS:
        c = fc.case(i)
        if c["fn"] == "fft" and c["key"][1] >= fc.BIG:
            assert [(q["n_ch"], q["n_in"], q["cplx"], q["inverse"], q["impulse"]) for q in c["calls"]] == \
                [(2, c["n"], True, False, None), (2, c["n"] - 7, False, True, 1)], i
    assert set(fc.FFT64_EMULATION) == {fc.case(i)["key"] for i in fc.IDENTS}


def test_inputs_are_what_the_docstring_says():
    c = fc.case("blue|255")
    for i, q in enumerate(c["calls"]):
        x = fc.call_input(c, i)
        assert x.shape == (q["n_in"], q["n_ch"]) and x.dtype == (np.complex128 if q["cplx"] else np.float64)
        assert x.flags.c_contiguous and np.array_equal(x, fc.call_input(c, i))
        if q["n_ch"] == 3:
            kept = min(q["n_in"], 255)
            assert np.count_nonzero(x[:, 1]) == 1 and abs(x[kept - 1, 1]) == 1.0
            assert 2e-4 < np.sqrt(np.mean(np.abs(x[:, 2]) ** 2)) < 3e-3 < 0.5 < np.sqrt(np.mean(np.abs(x[:, 0]) ** 2))
    c = fc.case("cols|1000x300")
    assert not fc.call_input(c, 0)[:, 2].any()
    ref = fc.oracle(c, 0, fc.call_input(c, 0))
    assert not ref[:, 2].any() and np.count_nonzero(ros._rms(ref, 0) == 0) == 1
    with pytest.raises(AssertionError, match="must be zero"):  # the judge holds a zero column to exactly zero
        out = ref.astype(np.complex128)
        out[17, 2] = 1e-300
        fc.judge_call(c, 0, out, ref)


def test_the_oracle_agrees_with_the_direct_sum():
    """scipy's long-double transform against the direct long-double sum with integer-reduced phases, at every case
    length up to 1024: 0.1 eps64 of the column rms.  The direct sum's own error walks to about sqrt(n) eps_ld = 3.5e-18
    at 1024 points; the bound is 2.2e-17, forty times below the tightest bound the cases assert (4 x 0.5 x 1.1 eps64)."""
    seen = set()
    for ident in fc.IDENTS:
        c = fc.case(ident)
        if c["n"] > 1024 or c["fn"] != "fft":
            continue
        for i, q in enumerate(c["calls"]):
            if q["n_ch"] > 3 and i > 1:
                continue
            x = fc.call_input(c, i)[:, :8]
            ref = fc.oracle(c, i, x)
            direct = longdouble_dft(x, c["n"], inverse=q["inverse"])
            worst = fc.fraction(direct, ref)  # (both long double: nothing is rounded to float64)
            assert worst <= 0.1, (fc.call_name(c, i), worst)
        seen.add(c["n"])
    assert seen == {1, 2, 3, 4, 5, 8, 129, 255, 256, 512, 1000, 1024}


@functools.lru_cache(maxsize=None)
def _sweep():
    """{ident: the emulation's worst error / (eps scale)} of every host-sized case, measured once"""
    return {ident: fc.emulation_fraction(fc.case(ident)) for ident in HOST}


def test_float64_emulation_stays_within_the_recorded_table():
    worst = {}
    for ident, frac in _sweep().items():
        key = fc.case(ident)["key"]
        if frac >= worst.get(key, (0.0, None))[0]:
            worst[key] = (frac, ident)
    assert set(worst) == {k for k in fc.FFT64_EMULATION if k[1] <= HOST_POINTS}
    for key, (frac, ident) in sorted(worst.items()):
        print(f"float64 emulation {key}: worst error / (eps scale) {frac:.3g} at {ident}; bound {fc.tolerance(key):.3g}")
        assert frac <= fc.FFT64_EMULATION[key] * fc.HOST_MARGIN, (key, ident, frac)


def test_every_bound_is_within_the_cap_and_the_emulation_within_a_quarter_of_it():
    for key, frac in fc.FFT64_EMULATION.items():
        assert fc.tolerance(key) <= fc.CAP, (key, fc.tolerance(key))
        assert frac * fc.HOST_MARGIN * fc.EPS <= fc.CAP / 4, (key, frac)
        assert 4.0 * frac * fc.HOST_MARGIN * fc.EPS <= fc.tolerance(key)


# ---- the bound bites -------------------------------------------------------------------------------------------------------------
def _at_50000():
    return fc.adhoc(50000, [fc.call_spec(3, 50000, True, False, impulse=1, small=2), fc.call_spec(1, 49993, False, True)])


WRONG = [
    # (a) the chirp phase as the double quotient k^2 / n, without the integer reduction
    ("chirp_float", _at_50000, None), ("chirp_float", lambda: fc.case("blue|46341"), (18, 17)),
    # (b) the four-step twiddle's phase formed in float32
    ("twiddle_f32_phase", lambda: fc.case("four|32768"), (18, 17)),
    # (c) the twiddle table rounded through float32
    ("table_f32", lambda: fc.case("lds|8192"), (18, 17)),
    # (d) the 1 / M left out of one column
    ("scale_one_column", lambda: fc.case("blue|129"), (18, 17)),
    # (e) the mirrored half of the filter one place off
    ("filter_shift", lambda: fc.case("blue|255"), (18, 17)),
]


@pytest.mark.parametrize("perturb,make,calls", WRONG, ids=[f"{w[0]}-{k}" for k, w in enumerate(WRONG)])
def test_the_bound_rejects_a_subtly_wrong_transform(perturb, make, calls):
    """Each wrong emulation exceeds its case's bound at least ten times over on every call tried (a forward complex and
    an inverse real call of three channels: n_in = n: indices 18 and 17 of the cross), and the judge raises on it; the emulation
    as the device does it passes the same calls within a quarter of the bound.  (b): float32(j2 k1) / n itself is exact
    below 2^24 with n a power of two, so the defect restated is the one that rounds -- the phase 2 pi j2 k1 / n in
    radians held in float32, as a kernel calling a float sincos would form it.  Measured: (a) 2900 to 3300 times
    the bound at 50000 and 46341, (b) and (c) 5e7, (d) 1e17, (e) 4e14."""
    c = make()
    good, wrong = fc.Emulation(), fc.Emulation(perturb)
    for i in (range(len(c["calls"])) if calls is None else calls):
        x = fc.call_input(c, i)
        ref = fc.oracle(c, i, x)
        ratio = fc.fraction(wrong.run(c, i, x), ref) * fc.EPS / fc.tolerance(c["key"])
        print(f"{perturb} {fc.call_name(c, i)}: {ratio:.3g} times the bound")
        assert ratio >= 10.0, (perturb, fc.call_name(c, i), ratio)
        with pytest.raises(AssertionError):
            fc.judge_call(c, i, wrong.run(c, i, x), ref)
        assert fc.judge_call(c, i, good.run(c, i, x), ref) <= 0.25 * fc.HOST_MARGIN + 1e-9


def test_numpy_fft_stays_within_the_cap():
    """numpy.fft (float64) on every host-sized case by the same rule, with the cap as the bound: the rule is not tighter
    than a good float64 transform can meet."""
    worst = (0.0, "")
    for ident in HOST:
        c = fc.case(ident)
        if c["fn"] != "fft":
            continue
        for i, q in enumerate(c["calls"]):
            x = fc.call_input(c, i)
            out = (np.fft.ifft if q["inverse"] else np.fft.fft)(x, c["n"], axis=0)
            worst = max(worst, (fc.judge_call(c, i, out, fc.oracle(c, i, x), fc.CAP), fc.call_name(c, i)))
    print(f"numpy.fft: at worst {worst[0]:.3g} of the cap ({worst[1]})")
