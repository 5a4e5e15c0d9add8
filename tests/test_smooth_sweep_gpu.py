"""The smoothing kernels (csrc/kernels_smooth.hpp) at their tile, chunk, lane and branch edges (tests/smooth_cases.py)
against the long-double oracles of tests/smooth_oracle.py: every element of every case within the oracle's own forward
error bound, |device - oracle| <= bound, and bit for bit where the bound is zero.  Nothing is left out.  The printed
figures are the worst error / bound per case group; tests/test_smooth_sweep_host.py shows that a float64 emulation stays
within a quarter of the same bounds and that thirteen subtly wrong ones exceed them."""

import numpy as np
import pytest

import smooth_cases as sc
from dsptoolbox_amd import backend

pytestmark = pytest.mark.gpu


def run(name):
    """the case through the entry its family names"""
    p, fam = sc.problem(name), sc.family(name)
    if fam in ("bins", "window", "interp"):
        ctx = backend.get_context()
        v, w, k_log = p["v"], p["window"], p["k_log"]
        out = np.empty_like(v)
        ctx.check(ctx.lib.ds_octave_smooth(ctx.handle, backend._ptr(v), v.shape[0], v.shape[1],
                                           None if k_log is None else backend._ptr(k_log), backend._ptr(w), len(w),
                                           p["clip"], backend._ptr(out)), "ds_octave_smooth")
        return out
    if fam == "pipeline":
        return backend.fractional_octave_smoothing(p["v"], None, p["fractions"], None, p["window"], clip_values=bool(p["clip"]))
    if fam == "gdelay":
        return backend.group_delay_phase(p["x"], 1.0 / p["n"])
    return backend.smooth_complex_spectrum(p["z"], 1, sc.COMPLEX_SPACING[p["L"]], "hamming", clip_magnitude=p["clip"])


def sweep(names, what):
    worst, at = 0.0, None
    for name in names:
        r = sc.judge(name, run(name))
        assert r <= 1.0, f"{name}: {r:.3g} of the bound"
        if r >= worst:
            worst, at = r, name
    print(f"{what}, {len(names)} cases: worst {worst:.3g} of the bound ({at})")
    return worst


@pytest.mark.parametrize("n_ch", [1, 2, 3, 5, 9, "full"])
def test_bins_sweep(n_ch):
    names = [n for n in sc.bins_cases() if (sc._fields(n)["C"] in (4, 8, 16, 17)) == (n_ch == "full")
             and (n_ch == "full" or sc._fields(n)["C"] == n_ch)]
    assert len(names) == (4 if n_ch == "full" else 18)
    sweep(names, f"k_smooth over n_bins, {n_ch} channels" if n_ch != "full" else "k_smooth, full groups and a second group")


@pytest.mark.parametrize("tc", list(sc.PARTIAL) + ["clamped"])
def test_window_sweep(tc):
    if tc == "clamped":
        sweep([sc.CLAMPED], "k_smooth, every row clamped at both ends")
        return
    names = [n for n in sc.window_cases() if n != sc.CLAMPED and sc.tc_of(sc._fields(n)["C"]) == tc]
    assert len(names) == 10
    sweep(names, f"k_smooth over the window length, tc = {tc} (chunks of {sc.CH(tc)} taps)")


@pytest.mark.parametrize("n", sc.INTERP_NS)
def test_interpolation_stages(n):
    names = [name for name in sc.interp_cases() if sc._fields(name)["N"] == n]
    assert len(names) == 2 * len(sc.INTERP_DATA) * len(sc.INTERP_AXES)
    sweep(names, f"k_to_log and k_to_lin at N = {n}")


@pytest.mark.parametrize("name", sc.pipeline_cases())
def test_pipeline_on_the_standard_axis(name):
    out = run(name)
    if name.endswith("-clip"):
        plain = sc.problem(name[:-len("clip")] + "plain")["value"]
        assert out.min() >= 0.0 and (out == 0.0).any() and (plain < 0).any()  # the clip acts
    sweep([name], "fractional_octave_smoothing")


@pytest.mark.parametrize("n", sc.GDELAY_NS)
def test_unwrap_through_the_group_delay(n):
    names = [name for name in sc.gdelay_cases() if sc._fields(name)["n"] == n]
    assert len(names) == 8
    sweep(names, f"group_delay_phase of unit impulses, n = {n} ({n // 2 + 1} bins)")


@pytest.mark.parametrize("name", sc.COMPLEX_CASES)
def test_unwrap_through_complex_smoothing(name):
    sweep([name], "smooth_complex_spectrum")


@pytest.mark.parametrize("name", ["bins-C5-N513-L8", "interp-N1000-C3-flat-uniform", "pipeline-N2049-C5-F3-clip",
                                  "gdelay-n4098-C3-d3", "complex-steps-L9"])
def test_two_calls_return_the_same_bits(name):
    assert name in sc.all_cases()
    a, b = run(name), run(name)
    assert a.tobytes() == b.tobytes()


def test_launch_names():
    ctx = backend.get_context()

    def names(case):
        ctx.routes()
        run(case)
        return ctx.routes()

    assert names("bins-C5-N513-L8") == {"smooth"}
    assert names("interp-N1000-C3-flat-uniform") == {"smooth_to_log", "smooth", "smooth_to_lin"}
    assert names("pipeline-N2049-C5-F3-clip") == {"smooth_to_log", "smooth", "smooth_to_lin"}  # (k_to_lin clips)
    assert names("complex-steps-L9") == {"smooth_polar", "smooth_unwrap", "smooth", "smooth_recombine"}
    assert names("complex-clip-L9") == {"smooth_polar", "smooth_unwrap", "smooth", "smooth_clip", "smooth_recombine"}
    got = names("gdelay-n4098-C3-d3")
    assert "fft64_unwrap" in got and not any(n.startswith("smooth") or n.startswith("csmooth") for n in got), got
