"""The cases, plan restatement, emulations and bounds of the float32 whole-signal transform sweep (xform_cases.py)
without a GPU: the restated plan is the sources'; every Bluestein length runs on the M the list claims and the ten
four-step lengths cover every rows kernel; every recorded emulation figure is measured again; the float32 chirp-z
restatement keeps a quarter of its own bound at every Bluestein length; four deliberately wrong float64 restatements
(xform_cases.WRONG) each miss the bound at least ten times over, on a small and on a large length; and the cases are
what the docstring says (no row of scale 0, ragged signals leave a zero tail, the (L - k) % L partner of every bin)."""

import functools
import os
import re

import numpy as np
import pytest

import route_oracles as ros
import xform_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsptoolbox_amd", "csrc")
LENGTHS = {"rfft": xc.FOUR + tuple(xc.BLUE), "deconv": xc.FOUR + xc.BLUE_DECONV}


def test_the_plan_restated_is_the_sources():
    api = open(os.path.join(CSRC, "api.hip")).read()
    big = open(os.path.join(CSRC, "kernels_bigfft.hpp")).read()
    lds = open(os.path.join(CSRC, "fft_lds.hpp")).read()
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()

    def one(text, pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    assert one(api, r"static const int kMaxFft = (\d+), kMinFft = 8;") == xc.MAX_FFT
    assert 1 << one(api, r"kMaxBigFft = \(int64_t\)1 << (\d+);") == xc.MAX_BIG
    assert one(header, r"#define DS_ERR_UNSUP\s+(-\d+)") == xc.DS_ERR_UNSUP
    # blue_len: the smallest M is the smallest four-step length
    assert 1 << one(api, r"int64_t m = \(int64_t\)1 << (\d+);  // smallest four-step length") == xc.BLUE_MIN == 2 * xc.MAX_FFT
    assert "while (m < 2 * L - 1) m <<= 1;" in api
    # lds_len, ch_stride, threads_for, big_rows_ct
    assert "constexpr int lds_len() { return N + N / 16 + 2; }" in lds
    assert "constexpr int threads_for(int n) { return cmax(64, cmin(512, n / 16)); }" in lds
    assert "constexpr int ch_stride() { return ((lds_len<N>() + 30) / 32) * 32 + 1; }" in big
    assert "size_t per = (size_t)(((n2 + n2 / 16 + 2 + 30) / 32) * 32 + 1) * sizeof(float2);" in api
    assert "int ct = std::min<int>({16, 1024 / nt, std::max<int>(1, (int)((70 * 1024) / per))});" in api
    assert "while (ct & (ct - 1)) ct &= ct - 1;  // power of two: must divide N1" in api
    assert xc.LDS_BUDGET == 70 * 1024
    # the two launches of a transform
    assert api.count("constexpr int N1 = 1024;") >= 2 and xc.N1 == 1024
    assert "a.ct = std::min(8, a.n2);" in api
    assert "const size_t lds = (size_t)a.ct * dsbig::ch_stride<N1>() * sizeof(float2);" in api
    assert "DISPATCH_N(n2, lds = (size_t)ct * dsbig::ch_stride<NN>() * sizeof(float2));" in api
    assert "dim3(N1 / ct, batch), ct * Cfg<NN>::NT, lds, a)" in api
    # the two refusals, and which lengths meet them
    unsup = 'return fail(c, DS_ERR_UNSUP, std::string(what) + ": '
    assert "if (2 * L - 1 > kMaxBigFft) " + unsup + xc.refusal(3 << 22) + '");' in api
    assert "if (n > kMaxBigFft) " + unsup + xc.refusal(1 << 25) + '");' in api
    assert "if (!is_pow2(q.n_fft)) return check_blue_len(c, q.n_fft, what.c_str());" in api
    assert "if (q.n_fft > kMaxFft) return check_big_len(c, q.n_fft, what.c_str());" in api
    assert 'const std::string w(q.who), what = w + " n_fft";' in api


def test_the_four_step_cases_cover_every_rows_kernel():
    api = open(os.path.join(CSRC, "api.hip")).read()
    sizes = [int(s) for s in re.findall(r"case (\d+): \{ constexpr int NN = \1; __VA_ARGS__; \} break;", api)]
    assert sizes == [1 << k for k in range(3, 15)]
    plans = {N: xc.four_plan(N) for N in xc.FOUR}
    assert [p["n2"] for p in plans.values()] == [s for s in sizes if s >= 32]
    assert min(xc.FOUR) == 2 * xc.MAX_FFT and max(xc.FOUR) == xc.MAX_BIG
    for N, p in plans.items():
        assert p["cols_ct"] == 8 and p["cols_threads"] == 512 and p["cols_lds"] == 71744 <= xc.LDS_LIMIT
        assert xc.N1 % p["rows_ct"] == 0 and p["n2"] % p["cols_ct"] == 0 and p["rows_threads"] <= 1024, N
        assert p["rows_lds"] <= xc.LDS_LIMIT, (N, p)
    # rows per workgroup: sixteen where the thread count allows, then what 70 KB hold; one row from 2^23 on
    assert [p["rows_ct"] for p in plans.values()] == [16, 16, 16, 16, 8, 4, 4, 2, 1, 1]
    assert plans[1 << 23]["rows_lds"] == 69896 and plans[1 << 24]["rows_lds"] == 139528 <= xc.LDS_LIMIT


def test_every_bluestein_length_runs_on_the_m_it_claims():
    for L, M in xc.BLUE.items():
        assert L & (L - 1) and xc.blue_len(L) == M and xc.refusal(L) is None, L
        assert M == xc.BLUE_MIN or M // 2 < 2 * L - 1 <= M, L
    full = {M: M // 2 - 1 for M in (1 << k for k in range(15, 25))}
    assert all(xc.BLUE[L] == M and 2 * L - 1 == M - 3 for M, L in full.items())
    assert {M for M in xc.BLUE.values()} == set(full)  # every M from 2^15 to 2^24 is launched
    for M in (1 << 16, 1 << 17, 1 << 18, 1 << 24):
        assert xc.BLUE[M // 4 + 1] == M and 2 * (M // 4 + 1) - 1 == M // 2 + 1
    assert max(xc.BLUE) == (1 << 23) - 1 and xc.refusal(max(xc.BLUE) + 2) is not None
    for prime in (1009, 100003):
        assert all(prime % d for d in range(2, int(prime ** 0.5) + 1))
    assert 1001 == 7 * 11 * 13 and (3 << 19) % 2 == 0 and xc.BLUE[3 << 19] == 1 << 22
    assert set(xc.BLUE_DECONV) <= set(xc.BLUE)
    for n in xc.REFUSED:
        assert xc.refusal(n) is not None
    assert [n & (n - 1) == 0 for n in xc.REFUSED] == [False, False, True]
    assert set(xc.EMULATION) == {(f, n) for f in LENGTHS for n in LENGTHS[f]}


def test_the_case_lists_are_what_the_docstring_says():
    for N in xc.FOUR:
        assert xc.channels(N) == ((1, 3) if N <= 1 << 21 else (2,))
        assert {(s[1], s[2]) for s in xc.rfft_specs(N)} == {(n, c) for n in (N, N // 2 + 1) for c in xc.channels(N)}
        specs = xc.deconv_specs(N)
        assert all(outs == (N, N // 2 + 3) for _, outs in specs)
        if N <= 1 << 21:
            assert {s[1:] for s, _ in specs} == {(n, rpc, items, 3) for n in (N, N // 2 + 1) for rpc in (0, 1)
                                                 for items in ((1, 2) if N <= 1 << 17 else (1,))}
        else:
            assert {s[1:] for s, _ in specs} == {(n, 1, 1, 2) for n in (N, N // 2 + 1)}
    for L in xc.BLUE:
        assert xc.channels(L) == ((1, 3) if L < 1 << 20 else (2,))
        assert {(s[1], s[2]) for s in xc.rfft_specs(L)} == {(n, c) for n in (L, (L + 1) // 2) for c in xc.channels(L)}
    for L in xc.BLUE_DECONV:
        assert all(outs == (L, L // 2 + 3) for _, outs in xc.deconv_specs(L))
    keys = [k for fam in LENGTHS for n in LENGTHS[fam] for k, _, _, _ in xc.calls(fam, n)]
    assert len(keys) == len(set(keys))
    # ragged lengths leave a zero tail; seeded; float32; zero mean
    p = xc.problem("rfft", (1001, 501, 3))
    q = xc.rfft_problem(1001, 501, 3)
    assert p["n"] < p["n_fft"] and p["xp"].dtype == np.float32 and p["xp"].shape == (3, 501) and np.array_equal(p["xp"], q["xp"])
    assert abs(float(p["xp"].mean())) < 0.05 and 0.45 < float(p["xp"].std()) < 0.55
    for fam in LENGTHS:
        for n_fft in LENGTHS[fam]:
            assert {s[1] for _, _, (_, s), _ in xc.calls(fam, n_fft)} == {n_fft, xc.short(n_fft)}
            assert 1 <= xc.short(n_fft) < n_fft
    # r as route_cases.deconv_problem draws it
    import route_cases as rcs
    assert np.array_equal(xc.deconv_problem(1024, 1024, 1, 1, 3)["r"], rcs.deconv_problem(1024, False, 1, 1)["r"])


@pytest.mark.parametrize("L", [L for L in xc.BLUE if L % 2])
def test_the_partner_bins_of_an_odd_length_pair_up_exactly_once(L):
    """k_unpack / k_mul_r read bin (L - k) % L beside bin k <= L/2 and k_mul_r writes both: for odd L the partners of
    1 ... L/2 are L/2 + 1 ... L - 1, each once, and km == k only at DC."""
    k = np.arange(L // 2 + 1, dtype=np.int64)
    km = (L - k) % L
    assert km[0] == 0 and np.all(km[1:] != k[1:])
    both = np.concatenate([k[1:], km[1:]])
    assert len(both) == L - 1 and np.array_equal(np.sort(both), np.arange(1, L))


@functools.lru_cache(maxsize=None)
def _fractions(family, n_fft):
    fr = xc.emulation_fractions(family, n_fft)
    return tuple(sorted(fr.items()))


@pytest.mark.parametrize("n_fft", LENGTHS["rfft"])
def test_rfft_emulation_is_the_recorded_figure(n_fft):
    _emulation_is_recorded("rfft", n_fft)


@pytest.mark.parametrize("n_fft", LENGTHS["deconv"])
def test_deconv_emulation_is_the_recorded_figure(n_fft):
    _emulation_is_recorded("deconv", n_fft)


def _emulation_is_recorded(family, n_fft):
    """Every entry of EMULATION measured again: within HOST_MARGIN of the recorded figure, and so within tol / 4."""
    t0 = ros.seconds["oracle"]
    fr = dict(_fractions(family, n_fft))
    worst, rec, tol = max(fr.values()), xc.EMULATION[(family, n_fft)], xc.tolerance((family, n_fft))
    print(f"float32 emulation {family} {n_fft}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()) +
          f"; recorded {rec}; tol {tol:.3g}; oracles took {ros.seconds['oracle'] - t0:.1f} s")
    assert set(fr) == ({"plain", "chirp-z"} if n_fft & (n_fft - 1) else {"plain"})
    assert rec / ros.HOST_MARGIN <= worst <= rec * ros.HOST_MARGIN, (family, n_fft, fr, rec)
    assert worst * ros.BASE_TOL <= tol / 4
    assert ros.BASE_TOL <= tol <= 2e-5  # (the bounds of this sweep: 1e-6 ... 2e-5 of the row's rms)


@pytest.mark.parametrize("family,L", [("rfft", L) for L in xc.BLUE] + [("deconv", L) for L in xc.BLUE_DECONV])
def test_the_float32_chirp_z_keeps_a_quarter_of_its_bound(family, L):
    fr = dict(_fractions(family, L))
    assert fr["chirp-z"] * ros.BASE_TOL <= xc.tolerance((family, L)) / 4, (family, L, fr)


def test_the_restatement_in_float64_is_the_oracle():
    """Restatement(float64), with scipy's transforms and with the four-step split, against route_oracles: 1e-12 of the
    row's rms (the wrong oracles below differ from it in one thing only)."""
    for family, spec in (("rfft", (1 << 15, (1 << 14) + 1, 3)), ("deconv", (1 << 15, 1 << 15, 1, 2, 3)),
                         ("rfft", (1001, 501, 3)), ("deconv", (1001, 1001, 0, 2, 3)), ("deconv", (16384 + 1, 16385, 1, 1, 3)),
                         ("deconv", (3 << 10, 3 << 10, 1, 1, 2))):
        p = xc.problem(family, spec)
        for four in (False, True):
            assert xc.fraction(p, xc.Restatement(np.float64, four=four).run(p)) < 1e-6, (family, spec, four)


WRONG_CASES = {
    "wrap": (("rfft", (16383, 16383, 3)), ("rfft", ((1 << 20) - 1, (1 << 20) - 1, 3))),
    "pair_sign": (("rfft", (1 << 15, 1 << 15, 3)), ("rfft", (1 << 21, 1 << 21, 3))),
    "edge_imag": (("deconv", (1001, 1001, 1, 1, 3)), ("deconv", (1 << 21, 1 << 21, 1, 1, 3))),
    "twiddle": (("rfft", (1 << 15, 1 << 15, 3)), ("rfft", (1 << 21, (1 << 20) + 1, 3))),
}


@pytest.mark.parametrize("wrong", list(xc.WRONG))
def test_a_wrong_oracle_misses_the_bound_ten_times_over(wrong):
    """Each of xform_cases.WRONG, computed in float64 so that nothing but the defect separates it from the oracle, on a
    small and on a large length of the sweep: its worst error is at least ten times the bound of that length."""
    for family, spec in WRONG_CASES[wrong]:
        assert spec in ([s for s, _ in xc.deconv_specs(spec[0])] if family == "deconv" else xc.rfft_specs(spec[0]))
        p = xc.problem(family, spec)
        tol = xc.tolerance((family, spec[0]))
        over = xc.fraction(p, xc.Restatement(np.float64, wrong=wrong).run(p)) * ros.BASE_TOL / tol
        print(f"wrong oracle {wrong} at {family} {spec}: {over:.3g} x the bound")
        assert over >= 10.0, (wrong, family, spec, over)
        with pytest.raises(AssertionError):
            out = xc.Restatement(np.float64, wrong=wrong).run(p).astype(np.complex64 if family == "rfft" else np.float32)
            xc.judge_call(wrong, p, out, p["n_fft"] if family == "deconv" else None)
