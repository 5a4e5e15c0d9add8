"""Device time of the float64 any-length transform and the minimum-phase chain (csrc/kernels_fft64.hpp), run by hand on
the GPU:
    python tools/time_phase.py [--reps 9] [--out profiles/phase_timing.txt] [--only fft|min_phase]

Shapes: fft_c128 of 8 real channels at 2^13 (one workgroup per column in LDS), 2^17 and 2^20 (four-step) and 384000
points (Bluestein on 2^20); min_phase_ir of 8 channels x 48000 samples at padding_factor 8 (384000 points, four
transforms).  Per shape: the summed HIP-event times of the kernels of one call and of each kernel group, median over
--reps warm calls; the wall time of the whole call (upload, kernels, download), median; the same computation in numpy
on this machine's CPU, median of 3; and the bytes the kernels of the call move to and from HBM by their own pass count
(every kernel reads and writes its operands once) over the kernel time, beside the device's measured copy bandwidth."""

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_direct import kernel_ms  # noqa: E402

FS = 48000


def wall_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def pow2_passes(n):
    """(read + write) passes over the planar array of one power-of-two transform: 1 in LDS, 3 transposes + 2 above."""
    return 1 if n <= 8192 else 5


def transform_passes(n):
    if n & (n - 1) == 0:
        return pow2_passes(n), n
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return 2 * pow2_passes(m) + 3, m  # chirp in, spectrum product, chirp out; all on M points (the last on n)


def ref_min_phase_ir(x, padding_factor=8):
    from scipy.fft import fft, ifft, next_fast_len
    n_fft = next_fast_len(x.shape[0] * padding_factor)
    y = np.real(ifft(np.log(np.abs(fft(x, n=n_fft, axis=0))), axis=0))
    y[1:(n_fft + 1) // 2] *= 2.0
    y[n_fft // 2 + 1:] = 0.0
    return np.real(np.fft.ifft(np.exp(fft(y, axis=0)), axis=0))[:len(x)]


def run(reps, only=None):
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(0)
    gbs = C.c_double()
    ctx.check(ctx.lib.ds_measure_copy(ctx.handle, C.c_size_t(1 << 30), 5, C.byref(gbs)), "ds_measure_copy")
    lines = [f"device copy bandwidth (read + written bytes): {gbs.value:.0f} GB/s"]

    def report(what, call, cpu_call, n_bytes):
        ms, per = kernel_ms(ctx, call, reps)
        lines.append(f"{what}: {ms:8.3f} ms kernels (" + ", ".join(f"{k} {v:.3f}" for k, v in sorted(per.items()))
                     + f"); {wall_ms(call, reps):8.2f} ms wall; numpy on the CPU {wall_ms(cpu_call, 3):8.2f} ms; "
                     + f"{n_bytes / 1e9:.3f} GB by pass count = {n_bytes / (ms * 1e-3) / 1e9:.0f} GB/s")

    for n in (() if only == "min_phase" else (1 << 13, 1 << 17, 1 << 20, 384000)):
        x = rng.standard_normal((n, 8))
        passes, ld = transform_passes(n)
        n_bytes = (passes * 2 * 16 * ld + 8 * n + 16 * ld + 16 * n + 16 * n) * 8  # + k_load, k_store
        report(f"fft_c128 8 x {n}", lambda: backend.fft_c128(x), lambda: np.fft.fft(x, axis=0), n_bytes)
    if only == "fft":
        return lines
    x = 0.03 * rng.standard_normal((48000, 8)) * np.exp(-np.arange(48000) / 6000.0)[:, None]
    x[100] += 1.0
    passes, ld = transform_passes(384000)
    n_bytes = (4 * passes * 2 * 16 * ld + 3 * 2 * 16 * 384000 + 8 * 48000 + 16 * ld + 16 * 48000 + 8 * 48000) * 8
    report("min_phase_ir 8 x 48000, padding_factor 8 (384000 points)",
           lambda: backend.min_phase(x, 384000, "ir", n_out=48000), lambda: ref_min_phase_ir(x), n_bytes)
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("fft", "min_phase"), default=None, help="one group of shapes (for a profiler run)")
    a = ap.parse_args()
    out = run(a.reps, a.only)
    print("\n".join(out))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(out) + "\n")
