"""Device time of frequency warping (csrc/kernels_warp.hpp), run by hand on the GPU:
    python tools/time_warp.py [--reps 5] [--channels 2] [--max-log2 17] [--out profiles/warp_timing.txt]

For N = 4096, 8192, ... 2^max-log2 samples, `--channels` channels of decaying noise, warping factor -0.876 ("bark"), from a
host float64 array (ds_allpass_table) and, at the largest N, from device-resident planar float32 (ds_allpass_table_dev):
- the launches of the call (one per anti-diagonal of tiles) and the sum of their kernel times, median over --reps warm
  calls, from the begin / end events the library puts on every launch;
- the device time of the whole call, median, from ds_timer_start / ds_timer_stop around it on the call's stream: the
  uploads of the samples and the boundary image, the launches with the gaps between them, the download;
- the rate in table cells (N x N x channel groups) per second of whole-call time, the number the work bound of
  csrc/size_guards.hpp is set from;
- this file's restatement of the reference's loop (N first-order all-pass filters by scipy's lfilter, each over N
  samples, and N scaled additions) on this machine's CPU: timed once up to --cpu-max samples (default 4096), beyond that
  extrapolated with the square of N from the largest timed size, and marked so.
Then one many-channel call at N = 2^max-log2 / 4 (--wide-channels, default 64) for the rate with every group busy.
Hardware counters are not collected here."""

import argparse
import os
import sys
import time

import numpy as np
from scipy.signal import lfilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_direct import kernel_ms  # noqa: E402
from tools.time_lpc import call_ms  # noqa: E402

LAMBDA = -0.876


def reference_loop(x, lam):
    """what the reference's _warp_time_series does: the all-pass applied again and again to a unit pulse"""
    n = len(x)
    pulse = np.zeros(n)
    pulse[0] = 1.0
    b, a = np.array([-lam, 1.0]), np.array([1.0, -lam])
    out = pulse[:, None] * x[0]
    for i in range(1, n):
        pulse = lfilter(b, a, pulse)
        out += pulse[:, None] * x[i]
    return out


def noise(n, n_ch, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n_ch)) * np.exp(-6.9 * np.arange(n) / n)[:, None]


def run(reps, n_ch, max_log2, cpu_max, wide):
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import DevicePlanar, get_context
    ctx = get_context()
    lines = [f"warp_time_series, factor {LAMBDA}, {n_ch} channels; tiles of 1024 input rows x 256 output columns"]
    cpu_ms, cpu_n = None, None
    sizes = [1 << k for k in range(12, max_log2 + 1)]
    for n in sizes:
        x = noise(n, n_ch)
        if n <= cpu_max:
            t0 = time.perf_counter()
            want = reference_loop(x, LAMBDA)
            cpu_ms, cpu_n = 1e3 * (time.perf_counter() - t0), n
            cpu = f"{cpu_ms:10.0f} ms (timed)"
        else:
            want = None
            cpu = f"{cpu_ms * (n / cpu_n) ** 2:10.0f} ms (extrapolated from N = {cpu_n} with N^2)" if cpu_ms else "not timed"
        runs = [("host float64", x)]
        if n == sizes[-1]:
            runs.append(("resident float32", DevicePlanar.from_planar(ctx, np.ascontiguousarray(x.T, dtype=np.float32))))
        for what, samples in runs:
            call = lambda: backend.warp_time_series(samples, LAMBDA)  # noqa: E731
            got = call()
            if want is not None and what == "host float64":
                err = float((np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)).max())
                assert err < 1e-12, err
            launches = (n - 2) // 1024 + (n - 2) // 256 + 1
            k_ms, _ = kernel_ms(ctx, call, reps)
            whole = call_ms(ctx, call, reps)
            cells = float(n) * n * -(-n_ch // backend.WARP_GROUP)
            lines.append(f"N {n:7d}, {what:16s}: {launches:4d} launches, kernels {k_ms:9.3f} ms (event pairs on the launches), "
                         f"whole call {whole:9.2f} ms (ds_timer), {cells / (whole * 1e-3):.3e} cells/s; "
                         f"the reference's loop on this CPU: {cpu}")
    n = sizes[-1] // 4
    x = noise(n, wide)
    call = lambda: backend.warp_time_series(x, LAMBDA)  # noqa: E731
    k_ms, _ = kernel_ms(ctx, call, reps)
    whole = call_ms(ctx, call, reps)
    cells = float(n) * n * -(-wide // backend.WARP_GROUP)
    lines.append(f"N {n:7d}, {wide} channels, host float64: kernels {k_ms:9.3f} ms, whole call {whole:9.2f} ms, "
                 f"{cells / (whole * 1e-3):.3e} cells/s")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--max-log2", type=int, default=17)
    ap.add_argument("--cpu-max", type=int, default=4096)
    ap.add_argument("--wide-channels", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = run(args.reps, args.channels, args.max_log2, args.cpu_max, args.wide_channels)
    print("\n".join(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")
