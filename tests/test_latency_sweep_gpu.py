"""The latency kernels (csrc/kernels_latency.hpp) and their entries at their lane, workgroup, round, rotation and window
edges (tests/latency_sweep_cases.py): the peak rows and the window bounds exactly, the NaN pattern of the neighbourhood
exactly, Pearson's r, the neighbourhood's values and the latency's phase shift within the bounds of the long-double
oracles there.  Nothing is left out.  The printed figures are the worst error / bound per group of cases;
tests/test_latency_sweep_host.py shows that a float64 emulation stays within a quarter of the same bounds and that eleven
subtly wrong ones exceed them or give another row."""

import numpy as np
import pytest

import latency_sweep_cases as sw
from dsptoolbox_amd import backend

pytestmark = pytest.mark.gpu


def run(name):
    """the case through the entry its family names, in the shape latency_sweep_cases.judge takes"""
    p, fam = sw.problem(name), sw.family(name)
    if fam == "direct":
        return backend.latency_peaks(p["x"], None, 0)[0]
    if fam == "corr":
        td1, td2 = sw.corr_inputs(p)
        return backend.latency_peaks(td1, td2, 0)[0]
    if name == sw.PEARSON_ENTRY:
        peaks, _, _, r = backend.latency_peaks(p["td1"], p["td2"], 0, pearson=True)
        assert r.shape == (3, 1)
        return peaks, np.ascontiguousarray(r[:, 0])
    if fam == "pearson":
        rows = p["rows"]
        return backend.lag_pearson(p["t"], p["o"], rows[:, 2], rows[:, 0], rows[:, 1])
    if fam == "window":
        peaks, window, near, _ = backend.latency_peaks(p["td1"], p["td2"], p["p"])
        return peaks, window, near
    with_latency = backend.group_delay_phase(p["x"], p["df"], p["tau"], p["fs"])
    return with_latency - backend.group_delay_phase(p["x"], p["df"])


def sweep(names, what):
    worst, at = 0.0, None
    for name in names:
        r = sw.judge(name, run(name))
        assert r <= 1.0, f"{name}: {r:.3g} of the bound"
        if r >= worst:
            worst, at = r, name
    print(f"{what}, {len(names)} cases: worst {worst:.3g} of the bound ({at})")
    return worst


@pytest.mark.parametrize("name", sw.direct_cases() + sw.corr_cases())
def test_peak_rows_are_exact(name):
    out = run(name)
    expect = sw.problem(name)["expect"]
    print(f"{name}: rows {[int(v) for v in out]}")
    assert out.dtype == np.int64 and list(out) == list(expect), (name, list(out), list(expect))


@pytest.mark.parametrize("n", sw.PEARSON_LENGTHS + ("entry",))
def test_pearson_at_a_lag(n):
    if n == "entry":
        sweep([sw.PEARSON_ENTRY], "latency_peaks(..., pearson=True)")
        return
    names = sw.pearson_cases(n)
    assert len(names) == len(sw.pearson_ways(n)) * len(sw.pearson_kinds(n))
    sweep(names, f"lag_pearson over {n} samples")


@pytest.mark.parametrize("name", sw.window_cases())
def test_window_bounds_and_neighbourhood(name):
    peaks, window, near = out = run(name)
    p = sw.problem(name)
    assert list(peaks) == p["must"] and window == p["window"], (name, list(peaks), window, p["window"])
    assert np.array_equal(np.isnan(near), p["nan"]), (name, near)
    r = sw.judge(name, out)
    print(f"{name}: window {window}, neighbourhood at {r:.3g} of the bound")
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("n", sw.PHASE_NS)
def test_latency_removed_from_the_phase(n):
    names = [name for name in sw.phase_cases() if name.startswith(f"phase-n{n}-")]
    assert len(names) == len(sw.PHASE_TAUS)
    sweep(names, f"group_delay_phase with and without the latency, n = {n}")


@pytest.mark.parametrize("name", ["direct-ties", "corr-2049x2049-b1-s1", "pearson-n8193-neg_long-rm70-offset",
                                  "window-near-corr2049x2048-p3", "phase-n4097-each"])
def test_two_calls_return_the_same_bits(name):
    assert name in sw.all_cases()
    a, b = run(name), run(name)
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
