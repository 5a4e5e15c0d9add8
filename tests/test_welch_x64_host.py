"""The route matrix of the float64 Welch entries (x64_cases.py) without a GPU: the constants it mirrors are the
sources', the float64 emulation stays within the recorded table and a quarter of the 1e-11 cap, the transfer-function
inputs are coherent, the long-double oracle agrees with oracle/dsp_oracle.py, and the judge rejects three subtly wrong
float64 computations."""

import functools
import os
import re

import numpy as np
import pytest

import x64_cases as xc
from dsptoolbox_amd import backend
from dsptoolbox_amd.standard.enums import SpectrumScaling
from oracle import dsp_oracle as orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsptoolbox_amd", "csrc")
# the cases the perturbed emulations run on: everything but the long windows and the 1024-channel matrix
QUICK = [i for i in xc.IDENTS if xc._specs[i]["W"] <= 512 and xc._specs[i]["n_cx"] <= 128]


def test_the_constants_are_the_sources():
    hpp = open(os.path.join(CSRC, "kernels_welch_f64.hpp")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()

    def one(text, pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    assert one(hpp, r"constexpr int LONG_M = (\d+)") == xc.LONG_M
    assert one(hpp, r"CSM_PAIRS_PER_THREAD = (\d+)") == xc.CSM_PAIRS_PER_THREAD
    assert one(hpp, r"CSM_PAIRS_PER_WG = CSM_PAIRS_PER_THREAD \* (\d+)") == 256
    assert one(hpp, r"CSM_MAX_CH = (\d+)") == xc.CSM_MAX_CH
    assert one(hpp, r"CSM_MEDIAN_TILE = (\d+)") == xc.CSM_MEDIAN_TILE
    assert one(hpp, r"CSM_MEDIAN_MAX_FRAMES = (\d+)") == xc.CSM_MEDIAN_MAX_FRAMES
    assert one(api, r"std::min\(n_frames, (\d+) / n_ch\)") == xc.CSM_TILE_VALUES
    assert one(api, r"if \(n_ch >= (\d+) && n_samples <= kMaxX64PlanarSamples\)") == xc.PLANAR_FROM_CH
    assert one(api, r"q\.median\(\) && q\.n_frames > (\d+)") == xc.MEDIAN_MAX_FRAMES
    assert one(api, r"const bool packed = W > (\d+);") == xc.LONG_M
    assert one(api, r"if \(W <= (\d+)\) \{\n        // four channels or more") == xc.PACKED_W
    assert one(api, r"kMaxX64Window = (\d+);") == xc.MAX_W
    assert "const int rc = (W / 2) / w64::LONG_M;" in api  # (the classes of a long window)


def test_every_listed_branch_has_a_case():
    s = xc._specs
    tile = lambda i: min(s[i]["n_frames"], xc.CSM_TILE_VALUES // s[i]["n_cx"])
    pairs = lambda i: s[i]["n_cx"] * (s[i]["n_cx"] + 1) // 2
    wg = 256 * xc.CSM_PAIRS_PER_THREAD
    assert -(-s["csm|16|c68|F60"]["n_frames"] // tile("csm|16|c68|F60")) == 1
    assert -(-s["csm|16|c68|F61"]["n_frames"] // tile("csm|16|c68|F61")) == 2
    assert -(-s["csm|16|c68|F121"]["n_frames"] // tile("csm|16|c68|F121")) == 3
    assert pairs("csm|16|c64|F5") <= wg < pairs("csm|16|c68|F5") and -(-pairs("csm|8|c1024|F5") // wg) == 228
    assert {s[i]["n_frames"] for i in s if i.startswith("median|")} >= {1, 2, 3, 255, 256, 257, 300, xc.MEDIAN_MAX_FRAMES}
    assert s["tf|512|cx1|amp|det0"]["W"] // 2 + 1 > 256  # a second workgroup of bins
    for C in (3, 4, 33):
        assert s[f"frames|256|c{C}|det0"]["n"] % 32 and s[f"frames|8192|c{C}|det0"]["n"] % 32  # (k_planar's sample tiles)
    # strided reads, the planar copy within one channel tile, one channel tile and one channel
    assert {s[i]["n_cx"] for i in s if i.startswith("frames|8192|")} == {2, xc.PLANAR_FROM_CH - 1, xc.PLANAR_FROM_CH, 33}
    assert s["packed|16384|c2|odd|det0"]["n"] % 2 == 1 and s["packed|16384|c2|even|det0"]["n"] % 2 == 0
    assert {s[i]["W"] // 2 // xc.LONG_M for i in s if i.startswith("long|")} == {2, 4, 8, 16}
    assert {s[i]["n_cx"] for i in s if i.startswith("csm_median|")} == {2, 32, 33, 65}
    assert {s[i]["n_frames"] for i in s if i.startswith("csm_median|")} == {1, 2, 63, 64, 65, 127, 128}


@functools.lru_cache(maxsize=None)
def _sweep():
    """Every problem once: {ident: (emulation fractions, lowest judged coherence, perturbed fractions)}."""
    rows = {}
    for ident in xc.IDENTS:
        p = xc.problem(ident)
        ref = xc.oracle(p)
        coh = 1.0
        for entry in p["entries"]:
            for name, r, scale, _, bins in xc.targets(p, entry, ref[entry]):
                assert np.all(np.isfinite(r[bins])), (ident, entry, name)
                assert np.all(np.broadcast_to(scale, r.shape)[bins] > 0), (ident, entry, name)
                if name == "coherence":
                    coh = min(coh, float(r[bins].min()))
        bad = {k: xc.emulation_fractions(p, k) for k in xc.PERTURBATIONS} if ident in QUICK else {}
        rows[ident] = (xc.emulation_fractions(p), coh, bad)
    return rows


def test_float64_emulation_stays_within_the_recorded_table_and_the_cap():
    worst = {}
    for ident, (fracs, _, _) in _sweep().items():
        for tk, frac in fracs.items():
            if frac >= worst.get(tk, (0.0, None))[0]:
                worst[tk] = (frac, ident)
    assert set(worst) == set(xc.X64_EMULATION)
    for tk, (frac, ident) in sorted(worst.items(), key=lambda kv: (kv[0][0], kv[0][2], kv[0][1])):
        print(f"float64 emulation {tk}: worst error / (eps scale) {frac:.3g} at {ident}; bound {xc.tolerance(tk):.3g}")
    for tk, (frac, ident) in worst.items():
        assert frac <= xc.X64_EMULATION[tk] * xc.HOST_MARGIN, (tk, ident, frac)
        assert xc.tolerance(tk) <= xc.CAP and frac * xc.EPS <= xc.CAP / 4, (tk, ident, frac)


def test_transfer_function_inputs_are_coherent():
    n = 0
    for ident, (_, coh, _) in _sweep().items():
        if any(e.startswith("tf") for e in xc._specs[ident]["entries"]):
            assert coh >= 0.5, (ident, coh)
            n += 1
    assert n >= 12


# ---- the two oracles cannot drift apart ---------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:Casting complex values to real")
@pytest.mark.parametrize("ident,scaling", [("tf|512|cx3|amp|det0", "AmplitudeSpectralDensity"),
                                           ("median|16|F257", "PowerSpectralDensity"), ("csm|16|c68|F61", "FFTBackward")])
def test_the_long_double_oracle_agrees_with_the_pinned_oracle(ident, scaling):
    """oracle/dsp_oracle.py (the reference's own steps in float64) on the case's signals, with the scaling mapped by
    backend._finish_params as the API does: 5e-13 by the matrix's error rule."""
    fs = 48000
    p = xc.problem(ident)
    assert p["hop"] == p["W"] // 2 and -(-p["n"] // p["hop"]) == p["n_frames"]  # the reference's own framing
    p["ident"] += "|" + scaling
    p["amp_sqrt"], p["norm_scale"], p["factor"], p["halve_edges"] = backend._finish_params(SpectrumScaling[scaling], p["W"], fs,
                                                                                           p["w"])
    kw = dict(fs_hz=fs, window_spec="hann", window_length_samples=p["W"], overlap_percent=50.0, detrend=bool(p["detrend"]),
              average=p["average"], scaling=scaling)
    for entry in p["entries"]:
        if entry == "psd":
            out = orc.welch(p["x"], None, **kw).astype(np.complex128)
        elif entry == "csd":
            out = orc.welch(p["x"], p["y"], **kw)
        elif entry == "csm":
            out = orc.csm_welch(p["x"], fs, p["W"], "hann", 50.0, bool(p["detrend"]), p["average"], scaling)[1]
        else:
            out = orc.compute_transfer_function(p["y"], p["x"], fs, p["W"], entry[3:], detrend=bool(p["detrend"]),
                                                average=p["average"], scaling=scaling)
        worst = xc.judge_entry(p, entry, out, 5e-13)
        print(ident, entry, {k: f"{v * 5e-13:.2e}" for k, v in worst.items()})


# ---- the judge rejects a subtly wrong float64 computation ----------------------------------------------------------------------
def _as_returned(entry, a):
    if entry == "psd":
        return a.astype(np.complex128)
    return tuple(np.ascontiguousarray(v) for v in a) if isinstance(a, tuple) else a


@pytest.mark.parametrize("perturb", xc.PERTURBATIONS)
def test_the_judge_rejects_a_subtly_wrong_result(perturb):
    """The emulation with the window rounded to float32, with the frame mean summed in float32, and with the frames of
    n_frames - 1 followed by one duplicated frame: the bound catches each in at least one case of every kind, and the
    judge raises on it.  The float32 mean is the exception the error rule itself makes: subtracting another constant from
    a frame moves its DC bin and nothing else, and with detrend the DC bin of a transfer function is not judged -- so for
    tf it is asserted that nothing but that bin moved."""
    best = {}
    for ident, (_, _, bad) in _sweep().items():
        for tk, frac in bad.get(perturb, {}).items():
            ratio = frac * xc.EPS / xc.tolerance(tk)
            if ratio > best.get(tk[0], (0.0, None))[0]:
                best[tk[0]] = (ratio, ident)
    print(perturb, {k: (round(v[0], 1), v[1]) for k, v in best.items()})
    kinds = {"psd", "csd", "tf", "csm"}
    assert set(best) == kinds
    for kind in kinds:
        ratio, ident = best[kind]
        p = xc.problem(ident)
        if perturb == "mean32" and kind == "tf":
            q = xc.problem("tf|512|cx3|raw|det1")
            good, moved = xc.answers(q, np.float64), xc.answers(q, np.float64, perturb)
            X, Xm = xc._spectra(q, q["x"], np.float64, None), xc._spectra(q, q["x"], np.float64, perturb)
            assert np.abs(Xm[0] - X[0]).max() > 1e-9 * np.abs(X[1:]).max()  # the DC bins did move
            for e in q["entries"]:
                assert xc.judge_entry(q, e, _as_returned(e, moved[e]))  # ... and the judged bins pass
                assert np.abs(moved[e][0][1:] - good[e][0][1:]).max() <= 1e-13 * np.abs(good[e][0][1:]).max()
            continue
        assert ratio > 1.0, (perturb, kind, ratio, ident)
        wrong = xc.answers(p, np.float64, perturb)
        raised = 0
        for entry in p["entries"]:
            if entry.split(":")[0] != kind:
                continue
            try:
                xc.judge_entry(p, entry, _as_returned(entry, wrong[entry]))
            except AssertionError:
                raised += 1
        assert raised, (perturb, kind, ident)
    # ... and the unperturbed emulation of the same cases passes
    for kind, (_, ident) in best.items():
        p = xc.problem(ident)
        good = xc.answers(p, np.float64)
        for entry in p["entries"]:
            assert max(xc.judge_entry(p, entry, _as_returned(entry, good[entry])).values()) <= 0.25 * xc.HOST_MARGIN + 1e-9
