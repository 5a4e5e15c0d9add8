"""Device time of standard.latency (csrc/kernels_latency.hpp on the float64 transforms), run by hand on the GPU:
    python tools/time_latency.py [--reps 5] [--out profiles/latency_timing.txt] [--log2n 20] [--channels 16]

Shape: two signals of 16 channels x 2^20 samples, the second the first delayed by a few hundred samples per channel
(the correlation has 2^21 - 1 rows and runs on 2^21 points, four-step).  For polynomial_points 0 and 1: the summed
HIP-event times of the kernels of one call and of each kernel group, median over --reps warm calls; the wall time of
the whole call (upload, kernels, the read-back of the peaks, download), median; and the reference's computation with
scipy on this machine's CPU (scipy.signal.correlate per channel, hilbert of the window, pearsonr per channel:
tests/latency_oracle.py), once.  There is no threshold: nothing earlier computes this on the device."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools.time_direct import kernel_ms  # noqa: E402
from tools.time_phase import wall_ms  # noqa: E402


def run(reps, log2n, n_ch):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd._lib import get_context
    import latency_oracle as orc
    ctx = get_context()
    n = 1 << log2n
    rng = np.random.default_rng(0)
    base = rng.standard_normal((n + 1024, n_ch))
    lags = 100 + 37 * np.arange(n_ch)
    in2 = base[1024:1024 + n]
    in1 = np.stack([base[1024 - l:1024 - l + n, c] for c, l in enumerate(lags)], axis=1) + 0.01 * rng.standard_normal((n, n_ch))
    s1, s2 = dsp.Signal(None, in1, 48000, constrain_amplitude=False), dsp.Signal(None, in2, 48000, constrain_amplitude=False)
    lines = []
    for p in (0, 1):
        call = lambda: dsp.latency(s1, s2, polynomial_points=p)  # noqa: E731
        out = call()
        assert np.array_equal(np.round(out[0]).astype(int), lags), out[0]
        ms, per = kernel_ms(ctx, call, reps)
        t0 = time.perf_counter()
        ref = orc.latency(in1, in2, p)
        cpu = 1e3 * (time.perf_counter() - t0)
        assert np.abs(ref[0] - out[0]).max() < 1e-6 and np.abs(ref[1] - out[1]).max() < 1e-9
        lines.append(f"latency {n_ch} x 2^{log2n}, polynomial_points {p}: {ms:8.3f} ms kernels ("
                     + ", ".join(f"{k} {v:.3f}" for k, v in sorted(per.items())) + f"); {wall_ms(call, reps):8.2f} ms wall; "
                     + f"scipy on the CPU {cpu:8.1f} ms")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--channels", type=int, default=16)
    a = ap.parse_args()
    out = run(a.reps, a.log2n, a.channels)
    print("\n".join(out))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(out) + "\n")
