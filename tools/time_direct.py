"""Device time of the direct sums (csrc/kernels_direct.hpp), run by hand on the GPU:
    python tools/time_direct.py [--reps 9] [--out profiles/direct_timing.txt]
    python tools/time_direct.py --cpu     # the reference's own functions on the CPU, 4097 samples x 2 channels

Shapes: dft of 8 channels x 2^20 samples at 1024 log-spaced frequencies; window_frequency_dependent of 8 x 65536
samples with 5 cycles, and the same call with the skip of negligible window terms disabled; complex_smoothing of
8 x 65537 bins at 1/3 octave (RealImaginary).  Per shape: the summed HIP-event times of the kernels of one call, median
over --reps warm calls, and the rate in summed terms per second -- the numbers the work bounds of csrc/size_guards.hpp
are set from."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 48000


def kernel_ms(ctx, call, reps):
    """median over reps of the summed kernel times of one call and of each kernel, from the library's launch events."""
    call()  # warm-up: workspaces, code objects, clocks
    ctx.profile_enable(True)
    tot, per = [], {}
    for _ in range(reps):
        ctx.lib.ds_profile_report(ctx.handle)
        call()
        rep = ctx.lib.ds_profile_report(ctx.handle).decode()
        rows = {line.split()[0]: float(line.split()[1]) for line in rep.splitlines() if line.strip()}
        tot.append(sum(rows.values()))
        for k, v in rows.items():
            per.setdefault(k, []).append(v)
    ctx.profile_enable(False)
    return float(np.median(tot)), {k: float(np.median(v)) for k, v in per.items()}


def ir_like(rng, n, n_ch):
    x = 0.05 * rng.standard_normal((n, n_ch)) * np.exp(-np.arange(n) / (n / 8))[:, None]
    x[100] += 1.0
    return x


def run_gpu(reps):
    from dsptoolbox_amd import backend, transfer_functions as tf
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    rng = np.random.default_rng(0)
    lines = []

    def report(what, terms, call, main):
        ms, per = kernel_ms(ctx, call, reps)
        lines.append(f"{what}: {ms:9.3f} ms kernels (" + ", ".join(f"{k} {v:.3f}" for k, v in sorted(per.items()))
                     + f"); {terms:.3e} terms, {terms / (per[main] * 1e-3):.3e} terms/s")

    x = rng.standard_normal((1 << 20, 8))
    freqs = np.geomspace(0.5, 23999.0, 1024)
    report("dft 8 x 2^20 samples, 1024 frequencies", 1024.0 * x.size, lambda: backend.dft(x, freqs, FS), "dft")

    ir = ir_like(rng, 65536, 8)
    f, alpha, peak, half = tf._fdw_parameters(ir, FS, 5, -50.0)
    kept = backend._windowed_kept_terms(alpha, peak, half, len(ir))
    report(f"window_frequency_dependent 8 x 65536, 5 cycles ({100 * kept / (len(f) * ir.size):.2f} % of the terms kept)",
           kept, lambda: backend.windowed_dft(ir, f, FS, alpha, peak, half), "dft")
    report("window_frequency_dependent 8 x 65536, 5 cycles, nothing skipped", float(len(f)) * ir.size,
           lambda: backend.windowed_dft(ir, f, FS, alpha, peak, half, -np.inf), "dft")

    n_bins = 65537
    sp = 1.0 + 0.2 * (rng.standard_normal((n_bins, 8)) + 1j * rng.standard_normal((n_bins, 8)))
    fb = np.fft.rfftfreq(2 * (n_bins - 1), 1 / FS)
    wy = np.hanning(3000)
    lo, hi, wlen, passed = backend._csmooth_indices(fb, 3)
    terms = float((hi - lo)[passed == 0].sum()) * 8
    report("complex_smoothing 8 x 65537 bins, 1/3 octave, RealImaginary", terms,
           lambda: backend.complex_smoothing(sp, fb, 3, "RealImaginary", wy), "csmooth")
    return lines


def run_cpu():
    from oracle.gen_golden import import_reference
    dsp = import_reference()
    rng = np.random.default_rng(0)
    x = ir_like(rng, 4097, 2)
    ir = dsp.ImpulseResponse(None, x, FS, constrain_amplitude=False)
    lines = []
    for what, call in (
            ("dft at 1024 frequencies", lambda: dsp.transforms.dft(ir, np.geomspace(0.5, 23999.0, 1024))),
            ("window_frequency_dependent, 5 cycles", lambda: dsp.transfer_functions.window_frequency_dependent(ir, 5)),
            ("complex_smoothing, 1/3 octave", lambda: dsp.transfer_functions.complex_smoothing(
                ir, 3, dsp.transfer_functions.SmoothingDomain.RealImaginary))):
        call()
        t0 = time.perf_counter()
        call()
        lines.append(f"reference on the CPU (sequential backends), 4097 samples x 2, {what}: "
                     f"{1e3 * (time.perf_counter() - t0):.1f} ms")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = run_cpu() if a.cpu else run_gpu(a.reps)
    print("\n".join(out))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(out) + "\n")
