"""Golden vectors for the structure filters, made by RUNNING THE REFERENCE (dsptoolbox 0.8: LatticeLadderFilter,
WarpedFIR, WarpedIIR and KautzFilter of dsptoolbox.filterbanks):
    python tools/gen_golden_sfilt.py

Writes tests/golden/sfilt/cases.npz.  `meta` is a JSON string with `fs`, `bound` and the case lists; `x` (N, 2) is the
input of every filtering case, noise rounded to float32 and stored as float32.
- `lattice`: a list of {"name", "filter"}; the Filter is rebuilt from `lat_<name>_sos` or `lat_<name>_b`, `_a`.  Stored:
  `lat_<name>_k`, `_c` (what from_filter made; no `_c` for the FIR lattice), `lat_<name>_y1`, `_s1` (output and state after
  filter_signal over x[:CUT]) and `lat_<name>_y2`, `_s2` (after a second call over x[CUT:], which continues the recursion).
- `warped`: a list of {"name", "lam"} with `wrp_<name>_b` (and `_a`: a WarpedIIR, then `_sigmas` too) and `wrp_<name>_y`.
- `kautz`: `kz_poles`, `kz_c_real`, `kz_c_complex`, `kz_y` (filter_signal over x), `kz_ir` (N_IR, 1) the single-channel impulse
  response that was fitted, `kz_fit_real`, `kz_fit_complex` (fit_coefficients_to_ir), `kz_get_ir` (get_ir(64) with the fitted
  weights), and from_ir(ir, 6, 5): `kz_from_ir_poles_real`, `_poles_complex`, `_c_real`, `_c_complex`.

The script ASSERTS that on every stored output the reference agrees with the long-double recursion of
tests/sfilt_oracle.py within BOUND of each channel's peak (the reference's lattice loops are float64 sums in the oracle's
order, its Kautz filter runs scipy.signal.lfilter per tap); it fails otherwise."""

import json
import os
import sys
import warnings

import numpy as np
from scipy.signal import butter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import sfilt_oracle as so  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sfilt", "cases.npz")
FS = 48000
BOUND = 1e-12
N, CUT, N_IR = 700, 333, 300


def main():
    dsp = import_reference()
    warnings.simplefilter("ignore")
    fb = dsp.filterbanks
    rng = np.random.default_rng(2718)
    z = {"x": rng.standard_normal((N, 2)).astype(np.float32)}
    x = z["x"].astype(np.float64)
    worst = {}

    def judge(what, got, want):
        e = so.stream_error(got, want)
        print(f"{what}: {e:.2e}")
        assert e <= BOUND, (what, e)
        worst[what.split()[0]] = max(worst.get(what.split()[0], 0.0), e)

    def signal(td):
        return dsp.Signal(None, td.copy(), FS, constrain_amplitude=False)

    # ---- lattice ----------------------------------------------------------------------------------------------------
    b4, a4 = butter(4, 0.3)
    lattice = [dict(name="sos", filter="sos", sos=butter(6, 0.2, output="sos")),
               dict(name="ba", filter="ba", b=b4, a=a4),
               dict(name="fir", filter="ba", b=np.array([2.0, 1.0, -0.4, 0.2, 0.3]), a=np.array([1.0]))]
    for case in lattice:
        name = case["name"]
        if case["filter"] == "sos":
            z[f"lat_{name}_sos"] = case["sos"]
            filt = dsp.Filter.from_sos(case["sos"].copy(), FS)
        else:
            z[f"lat_{name}_b"], z[f"lat_{name}_a"] = case["b"], case["a"]
            filt = dsp.Filter.from_ba(case["b"].copy(), case["a"].copy(), FS)
        lat = fb.LatticeLadderFilter.from_filter(filt)
        z[f"lat_{name}_k"] = np.array(lat.k)
        if lat.c is None:
            s = dict(kind="fir_lattice", k=lat.k)
        elif lat.k.ndim == 2:
            s = dict(kind="sos_lattice", k=lat.k, c=lat.c)
        else:
            s = dict(kind="iir_lattice", k=lat.k, c=lat.c)
        if lat.c is not None:
            z[f"lat_{name}_c"] = np.array(lat.c)
        y1 = lat.filter_signal(signal(x[:CUT])).time_data
        s1 = lat.state.copy()
        y2 = lat.filter_signal(signal(x[CUT:])).time_data
        s2 = lat.state.copy()
        want, zf = so.serial(s, x)
        judge(f"lattice {name} output", np.concatenate([y1, y2]), want)
        judge(f"lattice {name} state", s2.reshape(-1, 1), zf.reshape(-1, 1))
        z[f"lat_{name}_y1"], z[f"lat_{name}_s1"], z[f"lat_{name}_y2"], z[f"lat_{name}_s2"] = y1, s1, y2, s2
    # ---- warped -----------------------------------------------------------------------------------------------------
    b8, a8 = butter(8, 0.25)
    warped = [dict(name="fir", lam=0.6, b=rng.standard_normal(9)),
              dict(name="iir_p50", lam=0.5, b=b8, a=a8),
              dict(name="iir_m876", lam=-0.876, b=b8, a=a8),
              dict(name="iir_zero", lam=0.0, b=b8, a=a8),
              dict(name="iir_short_b", lam=0.3, b=np.array([0.5, 0.2]), a=np.array([2.0, -0.8, 0.5, 0.1]))]
    for case in warped:
        name, lam = case["name"], case["lam"]
        z[f"wrp_{name}_b"] = case["b"]
        if "a" in case:
            z[f"wrp_{name}_a"] = case["a"]
            w = fb.WarpedIIR(case["b"].copy(), case["a"].copy(), lam, FS)
            z[f"wrp_{name}_sigmas"] = np.array(w.sigmas)
            b = np.zeros(w.N)
            b[:len(w.b)] = w.b
            s = dict(kind="warped_iir", lam=lam, b=b, sigma=w.sigmas)
        else:
            w = fb.WarpedFIR(case["b"].copy(), lam, FS)
            s = dict(kind="warped_fir", lam=lam, b=case["b"])
        y = w.filter_signal(signal(x)).time_data
        judge(f"warped {name} output", y, so.serial(s, x)[0])
        z[f"wrp_{name}_y"] = y
    # ---- Kautz ------------------------------------------------------------------------------------------------------
    poles = np.array([0.5, -0.3, 0.7 * np.exp(0.4j), 0.9 * np.exp(2.0j), 0.97 * np.exp(0.05j)])
    c_real, c_complex = rng.standard_normal(2), rng.standard_normal(6)
    kz = fb.KautzFilter(poles, FS)
    kz.set_filter_coefficients(c_real, c_complex)
    z["kz_poles"], z["kz_c_real"], z["kz_c_complex"] = poles, c_real, c_complex
    z["kz_y"] = kz.filter_signal(signal(x)).time_data
    judge("kautz output", z["kz_y"], so.serial(so.kautz_structure(poles, c_real, c_complex), x)[0])
    ir = (rng.standard_normal((N_IR, 1)) * np.exp(-np.arange(N_IR) / 40.0)[:, None]).astype(np.float32).astype(np.float64)
    z["kz_ir"] = ir
    kz.fit_coefficients_to_ir(dsp.ImpulseResponse(None, ir.copy(), FS, constrain_amplitude=False))
    z["kz_fit_real"], z["kz_fit_complex"] = np.array(kz.coefficients_real_poles), np.array(kz.coefficients_complex_poles)
    unit = so.kautz_structure(poles)
    taps = so.kautz_taps(so.cast(unit, so.LD), so.serial(unit, ir[::-1])[1])
    judge("kautz fit", np.concatenate([z["kz_fit_real"], z["kz_fit_complex"]])[:, None], taps)
    z["kz_get_ir"] = kz.get_ir(64).time_data
    d = np.zeros((64, 1))
    d[0] = 1.0
    want = so.serial(so.kautz_structure(poles, z["kz_fit_real"], z["kz_fit_complex"]), d)[0]
    # (the impulse is an amplitude-constrained ImpulseResponse, and so is its filtered copy: a peak above one is scaled to one)
    judge("kautz get_ir", z["kz_get_ir"], want / max(1.0, np.max(np.abs(want))))
    found = fb.KautzFilter.from_ir(dsp.ImpulseResponse(None, ir.copy(), FS, constrain_amplitude=False), 6, 5)
    z["kz_from_ir_poles_real"], z["kz_from_ir_poles_complex"] = np.array(found.poles_real), np.array(found.poles_complex)
    z["kz_from_ir_c_real"] = np.array(found.coefficients_real_poles)
    z["kz_from_ir_c_complex"] = np.array(found.coefficients_complex_poles)

    print("worst reference error against long double:", {k: f"{v:.2e}" for k, v in worst.items()})
    strip = lambda cases: [{k: v for k, v in c.items() if not isinstance(v, np.ndarray)} for c in cases]
    z["meta"] = np.array(json.dumps({"fs": FS, "bound": BOUND, "cut": CUT, "lattice": strip(lattice), "warped": strip(warped),
                                     "worst": worst}))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300000


if __name__ == "__main__":
    main()
