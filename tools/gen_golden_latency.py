"""Golden vectors for latency, delay, find_ir_latency and the latency-free group delays, made by RUNNING THE REFERENCE
(dsptoolbox 0.8: standard.latency / delay, standard/latency_delay.py; transfer_functions.find_ir_latency / group_delay /
excess_group_delay, transfer_functions.py:862-915, 1009-1083, 1380-1406):
    python tools/gen_golden_latency.py

Writes tests/golden/latency/cases.npz.  The signals are those of tests/latency_cases.py (CASES, IRS); arrays up to 1000
samples are stored (float32), the longer ones are rebuilt from their seeds and the fixture holds `<key>_probe`, the
first 16 samples of channel 0 and the sum, to prove the rebuild.  `meta` is a JSON string:
- `signals`, `irs`: the parameters of make_pair / make_ir per name.
- `latency`: {name: {p: {"lo", "m", "peaks", "runner_up", "h_floor"}}} -- the shared window [lo, lo + m), the peak rows of
  the correlation, the largest ratio of a channel's second-largest |xcor| to its peak and the smallest |h| / max|h| over
  the 2 p + 2 neighbourhood values (p > 0).  Arrays: `<name>_p<p>_lags`, `_corr` (the reference's results) and, p > 0,
  `_near` (channels, 2 p + 2) with `_hmax`, the largest |h| of the window.
- `delay`: a list of {"delay_samples", "channels", "keep_length", "out"} on the `in1` of c1.
- `ir`: {name: {"find_min", "find_peak", "gd", "egd", "egd_analytic", "step_gap"}} naming the stored results; the group
  delays' frequency vectors are `<out>_f` as (length, second, last value).

The script ASSERTS on the reference's own numbers and fails otherwise:
(a) in every channel the second-largest |xcor| is at most (1 - 1e-6) of the peak: the integer lag is not decided by rounding;
(b) every neighbourhood value has |h| >= 1e-6 max|h| over the window: no sign the root finder branches on is rounding's;
(c) the reference raised no warning;
(d) no adjacent-bin phase step after the latency removal lies within 1e-3 of +-pi: unwrap is not decided by rounding.
It also asserts what the cases are there for: c1's window is the whole correlation, c5p's has a power-of-two length, the
Hilbert transform of c6's window needs more than 8192 points."""

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import latency_cases as lc  # noqa: E402
import latency_oracle as lo_  # noqa: E402


def steps_gap(phase):
    d = np.diff(phase, axis=0)
    dm = np.mod(d + np.pi, 2 * np.pi) - np.pi
    return float(np.abs(np.abs(dm) - np.pi).min())


def main():
    dsp = import_reference()
    tf = dsp.transfer_functions
    warnings.simplefilter("error")  # (c)
    z, meta = {}, dict(signals=lc.CASES, irs=lc.IRS, fs=lc.FS, latency={}, delay=[], ir={})

    def keep(key, x):
        if len(x) <= lc.STORED_UP_TO:
            z[key] = x.astype(np.float32)
        else:
            z[key + "_probe"] = lc.probe(x)

    def sig_of(x):
        return dsp.Signal(None, x.copy(), lc.FS, constrain_amplitude=False)

    def ir_of(x):
        return dsp.ImpulseResponse(None, x.copy(), lc.FS, constrain_amplitude=False)

    for name, par in lc.CASES.items():
        in1, in2 = lc.make_pair(**par)
        keep(name + "_in1", in1)
        if in2 is not None:
            keep(name + "_in2", in2)
        xc = lo_.xcorr(in1, in2)
        mag = np.sort(np.abs(xc), axis=0)
        runner_up = float((mag[-2] / mag[-1]).max())
        assert runner_up <= 1 - 1e-6, (name, runner_up)  # (a)
        info = {}
        for p in lc.POINTS:
            lags, corr = dsp.latency(sig_of(in1), None if in2 is None else sig_of(in2), polynomial_points=p)
            assert lags.dtype == (np.int_ if p == 0 else np.float64)
            z[f"{name}_p{p}_lags"], z[f"{name}_p{p}_corr"] = lags, corr
            entry = dict(runner_up=runner_up, peaks=[int(v) for v in np.argmax(np.abs(xc), axis=0)])
            if p > 0:
                rows, d, lo, h = lo_.fractional_peak(xc, p, detail=True)
                assert np.array_equal(in1.shape[0] - rows - 1, lags), name
                near = lo_.neighbourhood(h, d - lo, p)
                hmax = float(np.abs(h).max())
                assert not np.isnan(near).any(), name
                floor = float(np.abs(near).min() / hmax)
                assert floor >= 1e-6, (name, p, floor)  # (b)
                z[f"{name}_p{p}_near"], z[f"{name}_p{p}_hmax"] = near, np.array(hmax)
                entry.update(lo=int(lo), m=int(h.shape[0]), h_floor=floor)
            info[str(p)] = entry
        meta["latency"][name] = info
        print(name, "window", info["1"]["lo"], info["1"]["m"], "runner-up %.4f" % runner_up,
              "h floor %.1e" % min(info[str(p)]["h_floor"] for p in (1, 2, 3)))
    m = {name: meta["latency"][name]["1"] for name in lc.CASES}
    assert m["c1"]["lo"] == 0 and m["c1"]["m"] == 199
    assert m["c5p"]["m"] == 512
    assert 2 * m["c6"]["m"] - 1 > 8192 and m["c6"]["m"] & (m["c6"]["m"] - 1)
    assert 2 * m["c2"]["m"] - 1 <= 8192 and 8192 < 2 * 4097 - 1

    # ---- delay, on the in1 of c1
    x = lc.make_pair(**lc.CASES["c1"])[0]
    for k, (d, ch, keep_length) in enumerate(((0, None, False), (7, [1], False), (7, None, True), (5, [2, 0], False))):
        out = dsp.delay(sig_of(x), d, channels=ch, keep_length=keep_length).time_data
        z[f"delay_{k}"] = out
        meta["delay"].append(dict(delay_samples=d, channels=ch, keep_length=keep_length, out=f"delay_{k}"))

    # ---- the impulse responses
    def add_gd(key, f, gd):
        assert f[0] == 0.0 and np.allclose(np.diff(f), f[1], rtol=1e-9, atol=0.0)
        z[key], z[key + "_f"] = gd, np.array([len(f), f[1], f[-1]])
        return key

    for name, par in lc.IRS.items():
        x = lc.make_ir(**par)
        keep(name, x)
        e = {}
        z[name + "_find_min"] = tf.find_ir_latency(ir_of(x), True)
        z[name + "_find_peak"] = tf.find_ir_latency(ir_of(x), False)
        e["find_min"], e["find_peak"] = name + "_find_min", name + "_find_peak"
        for compare in (True, False):  # (b) for the two searches
            src = lo_.xcorr(x, lo_.min_phase_rows(x, 8)[:len(x)]) if compare else x
            _, d, lo, h = lo_.fractional_peak(src, 1, detail=True)
            assert np.abs(lo_.neighbourhood(h, d - lo, 1)).min() >= 1e-6 * np.abs(h).max(), (name, compare)
        gap = steps_gap(lo_.latency_free_phase(x, lc.FS)[1])
        assert gap > 1e-3, (name, gap)  # (d)
        e["step_gap"] = gap
        e["gd"] = add_gd(name + "_gd", *tf.group_delay(ir_of(x), analytic_computation=False, remove_ir_latency=True))
        e["egd"] = add_gd(name + "_egd", *tf.excess_group_delay(ir_of(x), remove_ir_latency=True, analytic_computation=False))
        e["egd_analytic"] = add_gd(name + "_egda", *tf.excess_group_delay(ir_of(x), remove_ir_latency=True,
                                                                           analytic_computation=True))
        meta["ir"][name] = e
        print(name, "step gap %.3e" % gap, z[name + "_find_min"], z[name + "_find_peak"])

    z["meta"] = np.array(json.dumps(meta))
    os.makedirs(os.path.dirname(lc.PATH), exist_ok=True)
    np.savez_compressed(lc.PATH, **z)
    print(lc.PATH, os.path.getsize(lc.PATH), "bytes")
    assert os.path.getsize(lc.PATH) < (1 << 20)


if __name__ == "__main__":
    main()
