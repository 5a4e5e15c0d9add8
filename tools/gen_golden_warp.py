"""Golden vectors for frequency warping, made by RUNNING THE REFERENCE (dsptoolbox 0.8: transforms.warp,
transforms.laguerre and transforms.warp_filter, transforms/transforms.py:955-1196):
    python tools/gen_golden_warp.py

Writes tests/golden/warp/cases.npz.  `meta` is a JSON string:
- `signals`: {name: {"n", "channels", "seed"}}; the samples are stored under the name as float32.
- `warp`: a list of {"sig", "factor", "shift_ir", "total_length"}; case i stores `warp_<i>`, the time data of the Signal
  the reference returned (float64), and `used` holds the float factor it applied (what it returns for a string).
- `laguerre`: a list of {"sig", "factor"}; case i stores `laguerre_<i>`.
- `filters`: a list of {"kind": "zpk" | "ba", "factor"}; entry i stores the filter as `filt_<i>_z`, `_p`, `_k` or
  `filt_<i>_b`, `_a` and the zpk of the reference's warped filter as `filt_<i>_wz`, `_wp`, `_wk`.
- `factors`: what the reference's _get_warping_factor answers for the four strings at `fs`.

Every signal is a little noise (1e-3) before an onset at n / 16 + 3 per channel, then noise under an exponential envelope
that falls by 60 dB over the rest, rounded to float32: an impulse response with something for `shift_ir` to find.

The script ASSERTS that on every stored case the reference agrees with the long-double table of tests/warp_oracle.py
within 1e-13 of each channel's peak; it fails otherwise."""

import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np
from scipy.signal import butter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import warp_oracle as wo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "warp", "cases.npz")
FS = 48000
BOUND = 1e-13

SIGNALS = {
    "n65c1": dict(n=65, channels=1, seed=65),
    "n300c2": dict(n=300, channels=2, seed=300),
    "n1030c3": dict(n=1030, channels=3, seed=1030),   # two tile rows, five tile columns
    "n2500c2": dict(n=2500, channels=2, seed=2500),   # three tile rows, ten tile columns
}
WARP = [
    dict(sig="n65c1", factor=0.5, shift_ir=False, total_length=None),
    dict(sig="n300c2", factor="bark", shift_ir=False, total_length=None),
    dict(sig="n300c2", factor="erb-", shift_ir=True, total_length=None),
    dict(sig="n300c2", factor=0.0, shift_ir=False, total_length=None),
    dict(sig="n1030c3", factor=-0.7, shift_ir=True, total_length=None),
    dict(sig="n1030c3", factor=0.9, shift_ir=False, total_length=700),
    dict(sig="n2500c2", factor="bark", shift_ir=False, total_length=None),
    dict(sig="n2500c2", factor=0.999, shift_ir=True, total_length=2049),
]
LAGUERRE = [
    dict(sig="n65c1", factor=0.5),
    dict(sig="n300c2", factor=-0.876),
    dict(sig="n1030c3", factor=0.9),
    dict(sig="n2500c2", factor=-0.7),
    dict(sig="n2500c2", factor=0.999),
]


def make_signal(n, channels, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, channels))
    for ch in range(channels):
        onset = n // 16 + 3 * ch
        tail = n - onset
        x[:onset, ch] = 1e-3 * rng.standard_normal(onset)
        x[onset:, ch] = rng.standard_normal(tail) * np.exp(-6.9 * np.arange(tail) / tail)
    return (x / np.abs(x).max()).astype(np.float32)


def filters():
    z, p, k = butter(4, 0.2, output="zpk")
    return [
        dict(kind="zpk", factor=-0.5, z=z, p=p, k=k),
        dict(kind="zpk", factor=0.3, z=np.array([0.5]), p=np.array([0.2 + 0.3j, 0.2 - 0.3j, -0.4]), k=2.0),  # poles > zeros
        dict(kind="ba", factor=0.7, b=np.array([0.2, 0.3, 0.1]), a=np.array([1.0, -0.5, 0.25])),
        dict(kind="ba", factor=-0.876, b=np.array([0.1, 0.4, 0.3, -0.2, 0.05]), a=np.array([1.0])),  # FIR: zeros only
    ]


def main():
    dsp = import_reference()
    from dsptoolbox.room_acoustics._room_acoustics import _find_ir_start
    from dsptoolbox.transforms._transforms import _get_warping_factor
    warnings.simplefilter("ignore")
    z = {name: make_signal(**p) for name, p in SIGNALS.items()}
    sig = {name: z[name].astype(np.float64) for name in SIGNALS}

    def signal_of(name):
        return dsp.ImpulseResponse(None, sig[name].copy(), FS, constrain_amplitude=False)

    worst = dict(warp=0.0, laguerre=0.0)
    used = []
    for i, case in enumerate(WARP):
        with contextlib.redirect_stdout(io.StringIO()):  # the reference prints its progress
            got = dsp.transforms.warp(signal_of(case["sig"]), case["factor"], case["shift_ir"], case["total_length"])
        if type(case["factor"]) is str:
            got, factor = got
        else:
            factor = case["factor"]
        used.append(float(factor))
        td = sig[case["sig"]].copy()
        if case["shift_ir"]:
            for ch in range(td.shape[1]):
                td[:, ch] = np.roll(td[:, ch], -_find_ir_start(td[:, ch], -20))
        td = td[:case["total_length"]]
        e = wo.channel_error(got.time_data, wo.warp(td, factor))
        print(f"warp {i} {case}: factor {factor!r}, {e:.2e}")
        assert got.time_data.shape == td.shape and e <= BOUND, (case, e)
        worst["warp"] = max(worst["warp"], e)
        z[f"warp_{i}"] = got.time_data
    for i, case in enumerate(LAGUERRE):
        got = dsp.transforms.laguerre(signal_of(case["sig"]), case["factor"]).time_data
        e = wo.channel_error(got, wo.laguerre(sig[case["sig"]], case["factor"]))
        print(f"laguerre {i} {case}: {e:.2e}")
        assert e <= BOUND, (case, e)
        worst["laguerre"] = max(worst["laguerre"], e)
        z[f"laguerre_{i}"] = got
    meta_filters = []
    for i, f in enumerate(filters()):
        if f["kind"] == "zpk":
            filt = dsp.Filter.from_zpk(f["z"], f["p"], f["k"], FS)
            z[f"filt_{i}_z"], z[f"filt_{i}_p"], z[f"filt_{i}_k"] = np.asarray(f["z"]), np.asarray(f["p"]), np.asarray(f["k"])
        else:
            filt = dsp.Filter.from_ba(f["b"], f["a"], FS)
            z[f"filt_{i}_b"], z[f"filt_{i}_a"] = f["b"], f["a"]
        wz, wp, wk = dsp.transforms.warp_filter(filt, f["factor"]).get_coefficients(dsp.FilterCoefficientsType.Zpk)
        assert len(wz) == len(wp)
        z[f"filt_{i}_wz"], z[f"filt_{i}_wp"], z[f"filt_{i}_wk"] = np.asarray(wz), np.asarray(wp), np.asarray(wk)
        meta_filters.append(dict(kind=f["kind"], factor=f["factor"]))
    factors = {name: float(_get_warping_factor(name, FS)) for name in ("bark", "erb", "bark-", "erb-")}
    print("worst reference error against long double:", {k: f"{v:.2e}" for k, v in worst.items()}, factors)
    z["meta"] = np.array(json.dumps({"signals": SIGNALS, "warp": WARP, "used": used, "laguerre": LAGUERRE,
                                     "filters": meta_filters, "factors": factors, "fs": FS}))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1000000


if __name__ == "__main__":
    main()
