"""Device time of linear prediction (csrc/kernels_lpc.hpp), run by hand on the GPU:
    python tools/time_lpc.py [--reps 7] [--channels 64] [--out profiles/lpc_timing.txt]

Shape: 64 channels x 2^20 samples, window 1024, hop 512, order 32 (2048 frames, 131072 (frame, channel) pairs), both
methods, from a host float64 array (ds_lpc) and from device-resident planar float32 (ds_lpc_dev).  Per run:
- the kernel's own time, median over --reps warm calls, from the begin / end events the library puts on the launch;
- the device time of the whole call, median, from ds_timer_start / ds_timer_stop around it on the call's stream: the
  uploads (the samples for the host entry, the window), the kernel and the download of a and var;
- the rate in lag products (frames x channels x window x (order + 1)) per second of kernel time, the number the work
  bound of csrc/size_guards.hpp is set from;
- this file's numpy restatement of the method on ONE (frame, channel) pair on this machine's CPU, median of 5, times
  the number of pairs (the reference loops over the pairs in Python in the same way);
- the time to read the input once at the bandwidth ds_measure_copy reports (which counts read + written bytes).
Hardware counters are not collected here."""

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
from scipy.signal import get_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_direct import kernel_ms  # noqa: E402

L, HOP, ORDER, N = 1024, 512, 32, 1 << 20


def yw_one(x, order):
    n = len(x)
    r = np.array([np.dot(x[:n - k], x[k:]) for k in range(order + 1)]) / n
    E, a = r[0], np.zeros(order)
    for m in range(order):
        k = -(r[m + 1] + np.dot(a[:m], r[m:0:-1])) / E
        E *= 1.0 - k * k
        a[:m] = a[:m] + k * a[:m][::-1]
        a[m] = k
    return a, E


def burg_one(x, order):
    f, b = x[1:], x[:-1]
    den = np.dot(f, f) + np.dot(b, b)
    a = np.zeros(order + 1)
    a[0] = 1.0
    for i in range(order):
        rc = -2.0 * np.dot(b, f) / (den + np.finfo(np.float64).eps)
        a[1:i + 2] = a[1:i + 2] + rc * a[i::-1][:i + 1]
        f, b = f + rc * b, b + rc * f
        den = (1.0 - rc * rc) * den - b[-1] ** 2 - f[0] ** 2
        f, b = f[1:], b[:-1]
    return a, den


def median_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def call_ms(ctx, call, reps):
    """ds_timer_* around the whole call on its stream, median."""
    t = []
    for _ in range(reps):
        ctx.timer_start()
        call()
        t.append(ctx.timer_stop())
    return float(np.median(t))


def run(reps, n_ch):
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import DevicePlanar, get_context
    ctx = get_context()
    rng = np.random.default_rng(0)
    gbs = C.c_double()
    ctx.check(ctx.lib.ds_measure_copy(ctx.handle, C.c_size_t(1 << 30), 5, C.byref(gbs)), "ds_measure_copy")
    x32 = rng.standard_normal((n_ch, N)).astype(np.float32)
    x64 = np.ascontiguousarray(x32.T.astype(np.float64))
    resident = DevicePlanar.from_planar(ctx, x32)
    window = get_window("hann", L, fftbins=True)
    pairs = (N // HOP) * n_ch
    products = float(pairs) * L * (ORDER + 1)
    frame = x64[:L, 0] * window
    lines = [f"shape: {n_ch} channels x {N} samples, window {L}, hop {HOP}, order {ORDER}: {pairs} pairs, "
             f"{products:.3e} lag products; device copy bandwidth (read + written bytes): {gbs.value:.0f} GB/s"]
    for method, one, kernel in (("yule_walker", yw_one, "lpc_yw"), ("burg", burg_one, "lpc_burg")):
        cpu_ms = median_ms(lambda: one(frame, ORDER), 5) * pairs
        for what, samples, n_bytes in (("host float64", x64, x64.nbytes), ("resident float32", resident, x32.nbytes)):
            call = lambda: backend.lpc(samples, ORDER, window, HOP, method)  # noqa: E731
            k_ms, per = kernel_ms(ctx, call, reps)
            lines.append(f"{method}, {what}: kernel {per[kernel]:8.3f} ms (event pair on the launch), whole call "
                         f"{call_ms(ctx, call, reps):8.2f} ms (ds_timer), {products / (per[kernel] * 1e-3):.3e} products/s; "
                         f"numpy on one pair x {pairs}: {cpu_ms:9.0f} ms; reading the input once at the copy bandwidth: "
                         f"{n_bytes / gbs.value / 1e6:.3f} ms")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = run(args.reps, args.channels)
    print("\n".join(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(out) + "\n")
