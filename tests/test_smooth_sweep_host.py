"""The smoothing sweep without a GPU: the constants restated in tests/smooth_cases.py are the header's; every case sits
on the edge it is there for; the long-double oracle of k_to_log agrees with scipy's PchipInterpolator and the one of
k_unwrap with numpy.unwrap; a float64 numpy emulation of every entry stays within a quarter of the oracle's bound on
every element of every case; and each of the subtly wrong emulations (smooth_cases.FAULTS) exceeds the bound on a named
case, so the device test (tests/test_smooth_sweep_gpu.py), which holds the kernels to the same bounds, would notice
the same fault in a kernel."""

import os
import re

import numpy as np
import pytest
from scipy.interpolate import PchipInterpolator

import smooth_cases as sc
import smooth_oracle as so

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "kernels_smooth.hpp")).read()

    def const(name):
        return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))

    assert (const("NT"), const("R"), const("MAX_TC"), const("LDS_DOUBLES")) == (sc.NT, sc.R, sc.MAX_TC, sc.LDS_DOUBLES)
    assert const("E") == sc.UNWRAP_LANE and "t0 += (int64_t)NT * E" in src and sc.UNWRAP_TILE == sc.NT * const("E") == 2048
    assert "inline int smooth_tile_bins(int tc) { return NT / tc * R; }" in src
    assert "inline int smooth_chunk(int tc) { return LDS_DOUBLES / tc - smooth_tile_bins(tc) + 1; }" in src
    assert [sc.TB(tc) for tc in (1, 2, 4, 8, 16)] == [2048, 1024, 512, 256, 128]
    assert [sc.CH(tc) for tc in (1, 2, 4, 8, 16)] == [2049, 1025, 513, 257, 129]
    api = open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", "api.hip")).read()
    assert "while (tc < MAX_TC && tc < n_ch) tc <<= 1, ++lg;" in api
    for name in ("smooth", "smooth_to_log", "smooth_to_lin", "smooth_clip", "smooth_polar", "smooth_unwrap",
                 "smooth_recombine", "fft64_unwrap"):
        assert f'launch(c, "{name}", ' in api, name


def test_case_lists_sit_on_their_edges():
    names = sc.all_cases()
    assert len(set(names)) == len(names)
    assert [sc.tc_of(c) for c in sc.PARTIAL.values()] == list(sc.PARTIAL) == [1, 2, 4, 8, 16]
    assert [sc.tc_of(c) for c in (4, 8, 16, 17)] == [4, 8, 16, 16]
    assert all(c % tc or tc <= 2 for tc, c in sc.PARTIAL.items())  # partial groups (one and two channels cannot be)
    assert len(sc.bins_cases()) == 5 * 9 * 2 + 4 and len(sc.window_cases()) == 5 * 10 + 1
    # the largest direct sum of the sweep
    work = {n: np.prod([sc._fields(n)[k] for k in "NLC"]) for n in sc.bins_cases() + sc.window_cases()}
    assert max(work, key=work.get) == "window-C1-N2049-L4099"
    f = sc._fields(sc.CLAMPED)
    assert f["L"] > 2 * f["N"] and f["N"] == 33
    # every window tap matters
    for name in ("bins-C5-N9-L8", "window-C9-N129-L259", "pipeline-N2049-C2-F1-plain"):
        assert sc.problem(name)["window"].min() >= 0.1
    assert sc.complex_window(9).min() > 0.07 and list(sc.complex_window(1)) == [1.0]
    assert [len(sc.problem(n)["window"]) for n in ("pipeline-N2049-C2-F1-plain", "pipeline-N4097-C2-F3-plain")] == [187, 115]


def test_interpolation_data_reaches_every_branch():
    for N in (256, 1000):
        # the three branches of the end rule, at the first and at the last interval
        for branch, kind in enumerate(("edgeA", "edgeB", "edgeC")):
            v = sc.interp_data(N, 3, kind, np.random.default_rng(0))
            m = np.diff(v, axis=0)
            assert (so.edge_branch(m[0], m[1]) == branch).all() and (so.edge_branch(m[-1], m[-2]) == branch).all(), (N, kind)
        v = sc.interp_data(N, 1, "flat", np.random.default_rng(0))[:, 0]
        m = np.diff(v)
        zero = np.flatnonzero(m == 0)
        assert len(zero) == 5 and (np.diff(zero) == 1).sum() == 3  # one lone zero slope, four side by side
        p = N // 5
        assert m[p - 1] > 0 > m[p]                                   # a sign change at a single knot
        assert (np.diff(sc.interp_data(N, 1, "ramp", np.random.default_rng(0)), axis=0) > 0).all()
        assert (np.diff(np.sign(sc.interp_data(N, 1, "alternating", np.random.default_rng(0))), axis=0) != 0).all()
        assert not sc.interp_data(N, 3, "zero", np.random.default_rng(0))[:, 0].any()
    for N in sc.INTERP_NS:
        for kind in sc.INTERP_AXES:
            k = sc.interp_axis(N, kind)
            assert len(k) == N and k[0] <= 1.0 and k[-1] >= N and (np.diff(k) > 0).all(), (N, kind)  # what the entry accepts
        assert (sc.interp_axis(N, "identity") == np.arange(1, N + 1)).all()
        k = sc.interp_axis(N, "uniform")
        assert k[0] == 0.5 and k[-1] == N + 0.75
    # the logarithmic guess of k_to_lin against the bracket that is right
    for kind, least in (("standard", 0), ("uniform", 100), ("top", 100)):
        k = sc.interp_axis(1000, kind)
        guess = np.clip((999 / np.log(1000.0) * np.log(np.arange(1, 1001.0))).astype(np.int64), 0, 998)
        off = np.abs(guess - so.lin_bracket(k)).max()
        assert off >= least and (kind != "standard" or off <= 1), (kind, off)


def test_to_log_oracle_is_scipys_pchip():
    worst = 0.0
    for name in sc.interp_cases():
        p = sc.problem(name)
        value, bound = so.to_log(p["v"], p["k_log"])
        ref = PchipInterpolator(np.arange(1, len(p["v"]) + 1, dtype=np.float64), p["v"], axis=0)(p["k_log"])
        r = so.ratio(ref, value, bound)
        worst = max(worst, r)
        assert r <= 1.0, (name, r)
    print(f"to_log against PchipInterpolator, {len(sc.interp_cases())} cases: worst {worst:.3g} of the stage's bound")


def test_unwrap_oracle_is_numpys_unwrap():
    worst = 0.0
    phases = [np.asarray(sc.problem(n)["stages"]["wrapped"], dtype=np.float64) for n in ("complex-steps-L9", "complex-axis-L9")]
    for n in sc.GDELAY_NS:
        for d in sc.gdelay_delays(n):
            k = np.arange(n // 2 + 1)
            exact = -2 * so.PI * ((k * d) % n).astype(so.LD) / n  # in (-2 pi, 0]: wrapped to (-pi, pi]
            exact = np.where(exact <= -so.PI, exact + so.TWO_PI, exact)
            phases.append(np.asarray(exact, dtype=np.float64)[:, None])
    for ph in phases:
        value, bound = so.unwrap(ph)
        r = so.ratio(np.unwrap(ph, axis=0), value, bound)
        worst = max(worst, r)
        assert r <= 0.25, r
    print(f"unwrap against numpy.unwrap, {len(phases)} phase arrays: worst {worst:.3g} of the stage's bound")


def test_steps_keep_their_margin_and_the_axis_case_has_none():
    st = sc.problem("complex-steps-L9")["stages"]
    ph = np.asarray(st["wrapped"], dtype=np.float64)
    margin = so.step_margin(ph)
    print(f"the steps' smallest distance from pi: {margin:.3g}")
    assert sc.MARGIN <= margin <= 3e-6                # the step at bin 2048 is 2e-6 inside pi
    turns, d = so.unwrap_turns(ph)
    assert (turns != 0).sum(axis=0).min() > 400       # the carry grows through every seam
    assert (np.asarray(st["smoothed"], dtype=np.float64)[:, 2:] < 0).all()  # what the clip must leave alone
    assert (np.asarray(sc.problem("complex-steps-L1")["stages"]["smoothed"], dtype=np.float64)[:, 2:] < 0).all()
    ax = np.asarray(sc.problem("complex-axis-L9")["stages"]["wrapped"], dtype=np.float64)[:, 0]
    assert list(ax[:5]) == [0.0, np.pi, 0.0, -np.pi, 0.0] and set(np.abs(np.diff(ax))) == {np.pi}
    assert not so.unwrap_turns(ax[:, None])[0].any()  # numpy's rule: a step of exactly +-pi takes no turn
    assert (np.unwrap(ax) == ax).all()
    # the group delay's steps lie 2 pi / n on either side of pi at n / 2 -+ 1
    for n in sc.GDELAY_NS:
        assert 2 * np.pi / n > 1e9 * sc.fft_phase_tolerance(n)


FAMILIES = {"bins": sc.bins_cases, "window": sc.window_cases, "interp": sc.interp_cases, "pipeline": sc.pipeline_cases,
            "gdelay": sc.gdelay_cases, "complex": lambda: list(sc.COMPLEX_CASES)}


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_emulation_stays_within_a_quarter_of_the_bound(fam):
    worst, at = 0.0, None
    for name in FAMILIES[fam]():
        r = sc.judge(name, sc.emulate(name))
        assert r <= 0.25, (name, r)
        if r > worst:
            worst, at = r, name
    rec = sc.SMOOTH_EMULATION[fam]
    print(f"{fam}: float64 emulation at {worst:.3g} of the bound at worst ({at}); recorded {rec:.3g}")
    assert rec / 2 <= worst <= min(2 * rec, 0.25), (fam, worst, rec)  # (another host's numpy rounds a little differently)


# fault -> the case that has to notice it
NOTICED_BY = {
    "last_tap": "bins-C5-N9-L8", "first_tap": "bins-C5-N9-L8",
    "clamp_front": "bins-C3-N9-L9", "clamp_back": "bins-C3-N9-L9",
    "chunk_seam": f"window-C5-N{sc.TB(8) + 1}-L{sc.CH(8) + 1}",
    "even_padding": "bins-C2-N8-L8",
    "zero_slope": "interp-N256-C1-flat-uniform",
    "edge_branch": "interp-N256-C1-edgeB-standard",
    "bracket_high": "interp-N256-C1-noise-standard",
    "tile_carry": "gdelay-n4098-C1-d4", "lane_carry": "gdelay-n4098-C1-d4",
    "plus_pi": "complex-axis-L9",
    "clip_all": "complex-clip-L9",
}
ALSO_NOTICED_BY = {"tile_carry": "complex-steps-L9", "lane_carry": "complex-steps-L9", "clamp_front": sc.CLAMPED,
                   "clamp_back": sc.CLAMPED, "last_tap": "window-C1-N2049-L4099", "first_tap": "window-C1-N2049-L4099",
                   "zero_slope": "interp-N5-C1-zero-uniform", "bracket_high": "interp-N1000-C3-ramp-identity"}


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_wrong_emulation_misses(fault):
    assert set(NOTICED_BY) == set(sc.FAULTS)
    for name in (NOTICED_BY[fault], ALSO_NOTICED_BY.get(fault)):
        if name is None:
            continue
        assert name in sc.all_cases()
        right, wrong = sc.judge(name, sc.emulate(name)), sc.judge(name, sc.emulate(name, fault))
        print(f"{fault} on {name}: {wrong:.3g} of the bound (the right emulation: {right:.3g})")
        assert right <= 0.25 and wrong > 1.0, (fault, name, right, wrong)


def test_faults_that_stay_hidden_where_the_issue_says_so():
    # a slipped 2 pi vanishes in cos and sin unless the window straddles it: a one-tap window cannot see the carry
    assert sc.judge("complex-steps-L1", sc.emulate("complex-steps-L1", "tile_carry")) <= 1.0
    assert sc.judge("complex-steps-L9", sc.emulate("complex-steps-L9", "tile_carry")) > 1.0
