"""Device time of fractional-octave smoothing at 64 channels x 32 769 and x 524 289 bins, 1/3 and 1/24 octave:
    python tools/time_smoothing.py [--reps 20] [--out profiles/smoothing_timing.txt]
    python tools/time_smoothing.py --cpu      # the same arithmetic with an FFT convolution on the CPU, 3 channels

Per shape: the summed HIP-event times of the kernels one ds_octave_smooth call launches (k_to_log, k_smooth,
k_to_lin), median over --reps calls after one warm-up, and the rate of k_smooth in multiply-adds per second -- the
number the work bound of csrc/size_guards.hpp is set from."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(32769, 3), (32769, 24), (524289, 3), (524289, 24)]
C = 64


def kernel_ms(ctx, call, reps):
    """median over reps of {kernel: ms} and of their sum, from the library's per-launch events."""
    tot, per = [], {}
    for _ in range(reps):
        ctx.lib.ds_profile_report(ctx.handle)
        call()
        rep = ctx.lib.ds_profile_report(ctx.handle).decode()
        rows = {line.split()[0]: float(line.split()[1]) for line in rep.splitlines() if line.strip()}
        tot.append(sum(rows.values()))
        for k, v in rows.items():
            per.setdefault(k, []).append(v)
    return float(np.median(tot)), {k: float(np.median(v)) for k, v in per.items()}


def run_gpu(reps):
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    lines = []
    for n, fr in SHAPES:
        v = np.random.default_rng(n + fr).standard_normal((n, C))
        k_log, beta = backend._smooth_axis(n, None)
        nw = backend._smooth_window_length(fr, beta)
        backend.fractional_octave_smoothing(v, None, fr)  # warm-up: workspace
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        ms, per = kernel_ms(ctx, lambda: backend.fractional_octave_smoothing(v, None, fr), reps)
        wall = (time.perf_counter() - t0) / reps
        ctx.profile_enable(False)
        work = float(n) * nw * C
        lines.append(f"{C} x {n} bins, 1/{fr} octave ({nw} taps): {ms:9.3f} ms kernels ("
                     + ", ".join(f"{k} {x:.3f}" for k, x in sorted(per.items()))
                     + f"); k_smooth {work / (per['smooth'] * 1e-3):.3e} multiply-adds/s; "
                     f"host call with upload and download {1e3 * wall:.1f} ms")
    return lines


def run_cpu():
    from scipy.interpolate import PchipInterpolator
    from scipy.signal import oaconvolve
    from scipy.signal.windows import get_window
    lines = []
    for n, fr in SHAPES:
        v = np.random.default_rng(n + fr).standard_normal((n, 3))
        t0 = time.perf_counter()
        l1 = np.arange(n, dtype=np.float64)
        k_log = n ** (l1 / (n - 1))
        l1 += 1.0
        nw = int(1 / (fr * np.log2(k_log[1])) + 0.5)
        nw += 1 - nw % 2
        w = get_window("hann", nw, fftbins=False)
        w /= w.sum()
        x = PchipInterpolator(l1, v, axis=0)(k_log)
        x = oaconvolve(np.pad(x, ((nw // 2, nw // 2), (0, 0)), mode="edge"), w[:, None], mode="valid", axes=0)
        np.stack([np.interp(l1, k_log, x[:, c]) for c in range(3)], axis=1)
        lines.append(f"CPU (scipy PCHIP, oaconvolve, np.interp), 3 x {n} bins, 1/{fr} octave ({nw} taps): "
                     f"{time.perf_counter() - t0:.3f} s")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = run_cpu() if a.cpu else run_gpu(a.reps)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/time_smoothing.py" + (" --cpu" if a.cpu else f" --reps {a.reps}") + "\n"
                     + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
