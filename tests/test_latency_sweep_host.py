"""The latency sweep without a GPU: the constants restated in tests/latency_sweep_cases.py are the headers'; every case
sits on the edge it is named for; the spike oracle of the correlation is scipy.signal.correlate and the long-double
Pearson oracle scipy.stats.pearsonr; every correlation case's runner-up is at least 1 below its peak; both calls of every
phase case unwrap alike; a float64 numpy emulation of every entry stays within a quarter of the oracle's bound (or gives
the very rows, where the oracle is exact); and each of the subtly wrong emulations (latency_sweep_cases.FAULTS) exceeds
the bound, or gives another row, on a named case -- so the device test (tests/test_latency_sweep_gpu.py), which holds the
kernels to the same oracles, would notice the same fault in a kernel."""

import os
import re

import numpy as np
import pytest
from scipy.signal import correlate
from scipy.stats import pearsonr

import fft64_cases as fc
import latency_sweep_cases as sw
import levels_oracle
from dsptoolbox_amd import backend

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "dsptoolbox_amd", "csrc")


def test_constants_are_the_headers():
    lat = open(os.path.join(CSRC, "kernels_latency.hpp")).read()
    dist = open(os.path.join(CSRC, "kernels_dist.hpp")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()
    guards = open(os.path.join(CSRC, "size_guards.hpp")).read()

    def const(src, name):
        return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))

    assert (const(lat, "NT"), const(lat, "PEAK_SPAN")) == (sw.NT, sw.PEAK_SPAN)
    assert (const(dist, "NT"), const(dist, "PER_LANE")) == (sw.NT, sw.PER_LANE)
    assert "constexpr int SPAN = NT * PER_LANE;" in dist and sw.SPAN == sw.NT * sw.PER_LANE
    assert const(guards, "kLatencyMaxPoints") == sw.MAX_POINTS == backend.LATENCY_MAX_POINTS == max(sw.NEAR_P)
    assert "std::max<int64_t>(d_min - 200, 0), m = std::min(d_max + 200, L) - lo" in api
    assert sw.WINDOW_MARGIN == backend.LATENCY_WINDOW_MARGIN == 200
    assert "for (int w = t; w < p.n_wg; w += NT)" in lat and sw.FINAL_ROUND == 1 << 20  # both final kernels' rounds
    assert "RowView{(const double*)r1.x, 2 * r1.pl.ld, 2, n_fft - (n_a - 1), n_fft}" in api
    for n in (1, 2, 255, 256, 257, 4095, 4096, 4097, 8193, 256 * 4096 + 1, (1 << 20) + 4097):
        assert sw.depth(n) == levels_oracle.reduction_depth(n), n


def test_direct_cases_sit_on_their_edges():
    names = sw.all_cases()
    assert len(set(names)) == len(names)
    S = sw.PEAK_SPAN
    assert sw.DIRECT_LENGTHS == (1, 255, 256, 257, S - 1, S + 1, 256 * S + 1, 257 * S + 1) and sw.LONGEST * 8 < 8.5e6
    for name in sw.direct_cases():
        p = sw.problem(name)
        if p["must"] is not None:
            assert list(p["expect"]) == p["must"], name
    lane, wave, wg = (lambda r: r % sw.NT), (lambda r: (r % sw.NT) // 64), (lambda r: r // S)
    a, b = sw.TIES["lane"]
    assert lane(a) == lane(b) and wg(a) == wg(b)
    a, b = sw.TIES["lanes"]
    assert lane(a) != lane(b) and wave(a) == wave(b) and a // sw.NT == b // sw.NT
    a, b = sw.TIES["waves"]
    assert wave(a) != wave(b) and wg(a) == wg(b)
    a, b = sw.TIES["workgroups"]
    assert wg(a) != wg(b) and wg(b) < sw.NT
    x = sw.problem("direct-ties")["x"]
    for c, (a, b) in enumerate(sw.TIES.values()):
        assert x[a, c] == -x[b, c] and abs(x[a, c]) == 2.0 and np.abs(np.delete(x[:, c], [a, b])).max() < 1.0
    assert not x[:, len(sw.TIES)].any()
    a, b = sw.ROUND_TIES["direct-rounds-lane"]   # the same lane of the final kernel, its first and second round
    assert wg(b) == wg(a) + sw.NT and wg(b) * S < sw.LONGEST
    a, b = sw.ROUND_TIES["direct-rounds-lanes"]  # the lower row in the higher lane
    assert wg(a) < sw.NT <= wg(b) and wg(a) % sw.NT > wg(b) % sw.NT
    for name, (a, b) in sw.ROUND_TIES.items():
        x = sw.problem(name)["x"]
        assert x[a, 0] == -x[b, 0] == -2.0 and len(x) == sw.LONGEST
    assert sw.problem("direct-last-row")["must"] == [sw.LONGEST - 1]


def test_correlation_cases_sit_on_their_edges_and_have_no_ties():
    assert sw.CORR_SHAPES == ((1, 7), (7, 1), (2049, 2048), (2049, 2049), (4096, 4097), (1 << 20, 4098))
    n_fft = {s: sw.pow2_at_least(s[0] + s[1] - 1) for s in sw.CORR_SHAPES}
    assert 2049 + 2048 - 1 == n_fft[(2049, 2048)] and 2049 + 2049 - 1 == n_fft[(2049, 2049)] // 2 + 1
    assert n_fft[(1, 7)] - (1 - 1) == n_fft[(1, 7)]  # Na = 1: rot == n_mod
    Na, Nb = sw.LONG_SHAPE
    assert Na + Nb - 1 > sw.FINAL_ROUND and sw.LONG_ROW // sw.PEAK_SPAN == sw.NT and n_fft[sw.LONG_SHAPE] == 1 << 21
    seen = {}
    for name in sw.corr_cases():
        p = sw.problem(name)
        assert list(p["expect"]) == p["must"], name
        for c in range(sw.N_CH):
            row, top, second = sw.peak_of(p["full"][c])
            assert top == 12 and second <= top - 1, (name, c, top, second)
        key = (p["Na"], p["Nb"], p["cb"])
        seen.setdefault(key, set()).update(p["must"])
        assert len(p["sp1"]) == sw.N_CH and len(p["sp2"]) == p["cb"]
        if p["cb"] == 1 and p["Na"] > 1:
            assert len(set(p["must"])) > 1, name  # each channel its own peak row
        if sw.LONG_ROW in p["must"]:  # smaller rivals in the rows the final kernel's first round covers
            c = p["must"].index(sw.LONG_ROW)
            assert any(k < sw.FINAL_ROUND for k in p["full"][c])
    for (Na, Nb, cb), rows in seen.items():
        assert rows >= set(sw.corr_targets(Na, Nb)), (Na, Nb, cb)
    assert set(sw.corr_targets(2049, 2049)) == {0, 2047, 2048, 4095, 4096}
    assert set(sw.corr_targets(*sw.LONG_SHAPE)) == {0, 4095, 4096, Na - 2, Na - 1, sw.LONG_ROW, Na + Nb - 2}


def test_spike_oracle_is_scipys_correlate():
    for name in sw.corr_cases():
        p = sw.problem(name)
        if p["Na"] > 4096:
            continue
        td1, td2 = sw.corr_inputs(p)
        assert td1.shape == (p["Na"], sw.N_CH) and td2.shape == (p["Nb"], p["cb"])
        for c in range(sw.N_CH):
            ref = correlate(td2[:, c if p["cb"] > 1 else 0], td1[:, c], method="direct")
            mine = np.zeros(len(ref))
            for k, v in p["full"][c].items():
                mine[k] = v
            assert np.array_equal(ref, mine), (name, c)
            assert np.argmax(np.abs(ref)) == p["expect"][c]


def test_pearson_oracle_is_scipys_pearsonr():
    worst = 0.0
    for name in sw.pearson_cases(257) + sw.pearson_cases(sw.SPAN + 1) + [sw.PEARSON_ENTRY]:
        p = sw.problem(name)
        for j, (ct, co, lag) in enumerate(p["rows"]):
            x, y = sw.overlap(p["t"], p["o"], ct, co, lag)
            if np.isnan(p["value"][j]):
                assert x.std() == 0 or y.std() == 0
                continue
            e = abs(float(p["value"][j]) - pearsonr(x, y)[0])
            worst = max(worst, e)
            assert e <= 1e-12, (name, j, e)
    print(f"long-double Pearson oracle against scipy.stats.pearsonr: {worst:.3g} at worst")


def test_pearson_cases_sit_on_their_edges():
    S = sw.SPAN
    assert sw.PEARSON_LENGTHS == (0, 1, 2, 3, 255, 256, 257, S - 1, S, S + 1, 2 * S + 1, 256 * S + 1, (1 << 20) + 4097)
    assert -(-(256 * S + 1) // S) == 257 == -(-((1 << 20) + 4097) // S) - 1  # the final kernel's second round
    configs, shorter, longer = set(), 0, 0
    for name in sw.pearson_cases():
        p = sw.problem(name)
        t, o = p["t"], p["o"]
        for ct, co, lag in p["rows"]:
            x, y = sw.overlap(t, o, ct, co, lag)
            assert len(x) == len(y) == p["n"], name
            n_del, n_und = (len(o), len(t)) if lag > 0 else (len(t), len(o))
            shorter += n_del < n_und
            longer += n_del > n_und
        assert len(t) != len(o) or p["n"] == 0
        assert (np.asarray(t, np.float32) == t).all() and (np.asarray(o, np.float32) == o).all()  # float32-valued
        if "special" in name:
            nan = np.isnan(np.asarray(p["value"], dtype=np.float64))
            if p["n"] >= 2 and p["n"] <= sw.FINAL_ROUND:
                assert list(nan) == [False, False, True, True, False] and abs(p["value"][0] - 1) < 1e-18 \
                    and abs(p["value"][1] + 1) < 1e-18
            continue
        if p["n"] <= sw.FINAL_ROUND:
            assert t.shape[1] != o.shape[1] and {t.shape[1], o.shape[1]} <= {1, 2, 5}
            configs.add((t.shape[1], o.shape[1]))
        if p["n"] >= 256:
            rho = sw.RHOS[name.split("-")[3]]
            assert np.abs(np.asarray(p["value"], dtype=np.float64) - rho).max() < 4 / np.sqrt(p["n"]), name
        if name.endswith("-offset") and p["n"] >= 2:
            assert abs(t.mean() - 1000) < 2 and abs(o.mean() - 500) < 2
        if p["n"] < 2:
            assert np.isnan(np.asarray(p["value"], dtype=np.float64)).all()
    assert configs == set(sw.CHANNELS) and shorter > 100 and longer > 100
    lags = {sw.WAYS[w][0] for w in sw.WAYS}
    assert min(lags) < 0 < max(lags) and 0 in lags


def test_window_cases_sit_on_their_edges():
    L, m = sw.DIRECT_L, sw.WINDOW_MARGIN

    def win(k):
        return sw.problem(f"window-direct-{k}")["window"]

    assert win("ends") == (0, L)
    assert win("e198") == (0, L) and win("e199") == (0, L) and win("e200") == (0, L - 1)  # clipped by two, one and no row
    assert sw.WINDOW_LAYOUTS["e199"] == (m - 1, L - m) and sw.WINDOW_LAYOUTS["e200"] == (m, L - 1 - m)
    assert win("pow2") == (500, 4096) and win("pow2p1") == (500, 4097)
    for name in sw.window_cases():
        p = sw.problem(name)
        lo, M = p["window"]
        assert p["must"] == list(sw.emulate(name)[0]), name  # the rows the case names are the peaks
        assert np.isfinite(np.asarray(p["value"], dtype=np.float64)[~p["nan"]]).all() and (p["bound"] > 0).all()
        if "-near-" not in name:
            assert p["nan"].any() == name.endswith("-ends")
            continue
        pp = p["p"]
        rows = p["must"]
        if len(rows) == 4:
            assert rows == [0, pp, p["L"] - 2 - pp, p["L"] - 1] and (lo, M) == (0, p["L"])
            # row 0: the first p values are missing; rows p and L - 2 - p: none, by one row; row L - 1: the last p + 1
            assert [int(v) for v in p["nan"].sum(axis=1)] == [pp, 0, 0, pp + 1]
            assert p["nan"][0, :pp].all() and p["nan"][3, pp + 1:].all()
        elif rows == [0]:
            assert (lo, M) == (0, m) and p["nan"][0, :pp].all() and p["nan"].sum() == pp
        else:
            assert (lo, M) == (p["L"] - 1 - m, m + 1) and p["nan"][0, pp + 1:].all() and p["nan"].sum() == pp + 1
    # window lengths whose Hilbert transform the fft64 table knows
    assert ("hilbert", fc.plan(sw.NEAR_L)[1]) in fc.FFT64_EMULATION and ("hilbert", fc.plan(L)[1]) in fc.FFT64_EMULATION
    assert ("hilbert", fc.plan(4097)[1]) in fc.FFT64_EMULATION
    assert sw.hilbert_tolerance(5000) == fc.tolerance(("hilbert", 16384)) and sw.hilbert_tolerance(200) >= sw.hilbert_tolerance(4095)
    assert sw.pow2_tolerance(8192) == fc.tolerance(("lds", 8192)) == sw.pow2_tolerance(4096)


def test_both_phase_calls_unwrap_alike():
    assert sw.PHASE_NS == (64, 1000, 4097, 32768)
    for name in sw.phase_cases():
        p = sw.problem(name)
        assert (p["margin"] >= 0).all(), (name, p["margin"])  # max |dphi| + 2 pi |tau| / n <= pi - 0.5
    each = sw.problem("phase-n1000-each")["tau"]
    assert len(set(each)) == 3 and each.min() < 0 and (sw.problem("phase-n1000-frac")["tau"] % 1 != 0).all()
    assert (sw.problem("phase-n1000-d")["tau"] == sw.problem("phase-n1000-d")["d"]).all()
    assert sw.PHASE_C >= 4 * sw.PHASE_EMULATION_UNITS


FAMILIES = {"direct": sw.direct_cases, "corr": sw.corr_cases, "pearson": lambda: sw.pearson_cases() + [sw.PEARSON_ENTRY],
            "window": sw.window_cases, "phase": sw.phase_cases}


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_emulation_stays_within_a_quarter_of_the_bound(fam):
    worst, at = 0.0, None
    for name in FAMILIES[fam]():
        r = sw.judge(name, sw.emulate(name))
        assert r <= 0.25, (name, r)
        if r >= worst:
            worst, at = r, name
    if fam in ("direct", "corr"):
        print(f"{fam}: the emulation gives every row exactly, {len(FAMILIES[fam]())} cases")
        return
    rec = sw.LATENCY_EMULATION[fam]
    print(f"{fam}: float64 emulation at {worst:.3g} of the bound at worst ({at}); recorded {rec:.3g}")
    assert rec / 2 <= worst <= min(2 * rec, 0.25), (fam, worst, rec)  # (another host's numpy rounds a little differently)
    if fam == "phase":
        units = max(sw.phase_units(sw.problem(n), sw.emulate(n)) for n in sw.phase_cases())
        print(f"phase: {units:.3g} units of 2^-53 (1 + |tau| + P / pi) / df at worst; recorded {sw.PHASE_EMULATION_UNITS}")


LONG_PEARSON = f"pearson-n{(1 << 20) + 4097}-pos_short-r95-offset"
# fault -> the cases that have to notice it
NOTICED_BY = {
    "raw_moment": ["pearson-n257-pos_short-r50-offset", "pearson-n3-zero_t-r95-offset", LONG_PEARSON],
    "means_uncut": ["pearson-n257-pos_short-r50-plain", "pearson-n4097-neg_long-r05-offset"],
    "lag_sign": ["pearson-n257-pos_short-r95-plain", "pearson-n4096-neg_long-rm70-plain"],
    "stride_swap": ["pearson-n257-pos_short-r95-plain", "pearson-n255-zero_o-r50-offset"],
    "final_drop": [LONG_PEARSON, f"pearson-n{256 * 4096 + 1}-zero_t-r05-plain", "direct-last-row",
                   f"corr-{1 << 20}x4098-b3-s1", f"corr-{1 << 20}x4098-b1-s2"],
    "tie_later": ["direct-ties", "direct-rounds-lane", "direct-rounds-lanes"],
    "rot_off": ["corr-1x7-b3-s0", "corr-2049x2048-b3-s0", "corr-2049x2048-b1-s0", f"corr-{1 << 20}x4098-b1-s0",
                "window-near-corr2049x2048-p3"],
    "window_first_channel": ["window-direct-ends", "window-direct-pow2"],
    "near_clamp": ["window-near-direct-p3", "window-near-first-p1", "window-near-corr2049x2049-p16"],
    "fs_df_swapped": ["phase-n1000-d", "phase-n64-neg"],
    "latency_channel0": ["phase-n1000-each", "phase-n32768-each"],
}


@pytest.mark.parametrize("fault", sw.FAULTS)
def test_wrong_emulation_misses(fault):
    assert set(NOTICED_BY) == set(sw.FAULTS) and len(sw.FAULTS) == 11
    for name in NOTICED_BY[fault]:
        assert name in sw.all_cases(), name
        right, wrong = sw.judge(name, sw.emulate(name)), sw.judge(name, sw.emulate(name, fault))
        print(f"{fault} on {name}: {wrong:.3g} of the bound (the right emulation: {right:.3g})")
        assert right <= 0.25 and wrong > 1.0, (fault, name, right, wrong)


def test_raw_moments_miss_at_every_offset_case():
    """what the looser bound of test_latency_gpu.py (4 n 2^-53 + 1e-15) would let through"""
    least = np.inf
    for n in sw.PEARSON_LENGTHS[4:11]:
        for name in sw.pearson_cases(n):
            if not name.endswith("-offset") or "special" in name:
                continue
            wrong = sw.judge(name, sw.emulate(name, "raw_moment"))
            least = min(least, wrong)
            assert wrong > 1.0, (name, wrong)
    print(f"raw-moment Pearson on the offset cases, n = 255 .. {2 * sw.SPAN + 1}: at least {least:.3g} of the bound")
