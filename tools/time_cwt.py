"""GPU time of the continuous wavelet transform (transforms.cwt) at 8 channels x 2^20 samples (48 kHz), 64
log-spaced frequencies from 50 Hz to 20 kHz, MorletWavelet(h=3, step=1e-3): a 4.3 GB complex64 scalogram.
    python tools/time_cwt.py [--reps 5] [--out profiles/cwt_timing.txt]
    python tools/time_cwt.py --reference     # the reference's CPU seconds at a small shape, extrapolated
Reported: the event-timed kernel time of each size class (the class's frequencies in one call; the class is the
block length M) and of the whole call, against the time to write the scalogram once at 8 TB/s; the resident class
call (wall); the host route at a smaller shape; the squeeze kernel; and the FIR-bank composition the new path
replaces (ds_fir_ola_dev with the 2F real and imaginary filters padded to the longest wavelet)."""

import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS, C, N, F = 48000, 8, 1 << 20, 64
WRITE_TBS = 8.0


def block_length(L, n):
    """The class of a wavelet of L taps on n samples (csrc/api.hip cwt_run)."""
    h = (L - 1) // 2
    lc = min(L - 1, h + n - 1) - max(0, h - n + 1) + 1
    m = 256
    while m < 2 * lc:
        m *= 2
    return m


def kernel_ms(ctx, call, reps):
    """median over reps of the summed event times of every kernel one call launches."""
    tot = []
    for _ in range(reps):
        ctx.lib.ds_profile_report(ctx.handle)
        out = call()
        ctx.sync()
        rep = ctx.lib.ds_profile_report(ctx.handle).decode()
        tot.append(sum(float(line.split()[1]) for line in rep.splitlines() if line.strip()))
        del out
    return float(np.median(tot)), rep


def run_gpu(reps):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import get_context
    from dsptoolbox_amd.transforms import MorletWavelet, cwt
    from dsptoolbox_amd.transforms._wavelets import _normalised_wavelets
    ctx = get_context()
    x = np.random.default_rng(1).standard_normal((C, N)).astype(np.float32)
    sig = dsp.Signal.from_planar_f32(x, FS)
    freqs = np.geomspace(50, 20000, F)
    w = MorletWavelet(h=3, step=1e-3)
    waves = _normalised_wavelets(w, freqs, FS)
    lens = np.array([len(v) for v in waves])
    roof_ms = F * N * C * 8 / (WRITE_TBS * 1e12) * 1e3
    lines = []
    out = cwt(sig, freqs, w, on_device=True)  # warm-up: workspaces, twiddles
    del out
    ctx.profile_enable(True)
    classes = {}
    for i, L in enumerate(lens):
        classes.setdefault(block_length(int(L), N), []).append(i)
    chs = np.arange(C)
    for m in sorted(classes):
        idx = classes[m]
        sub = [waves[i] for i in idx]
        ms, _ = kernel_ms(ctx, lambda: backend.cwt_device(sig.device_samples, chs, sub), reps)
        share = len(idx) / F * roof_ms
        lines.append(f"class M={m:6d} ({'four-step' if m > 16384 else 'LDS'}): {len(idx):2d} frequencies, "
                     f"L {int(lens[idx].min())}-{int(lens[idx].max())}: {ms:8.3f} ms kernels "
                     f"(its write share {share:.3f} ms = {100 * share / ms:.0f} % of roofline)")
    ms, rep = kernel_ms(ctx, lambda: backend.cwt_device(sig.device_samples, chs, waves), reps)
    lines.append(f"all classes, one call: {ms:8.3f} ms kernels; writing 4.3 GB once at {WRITE_TBS:.0f} TB/s: "
                 f"{roof_ms:.3f} ms = {100 * roof_ms / ms:.1f} % of roofline")
    lines.append("  per kernel (last rep): " + "; ".join(" ".join(l.split()[:2]) for l in rep.splitlines() if l.strip()))
    ctx.profile_enable(False)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = cwt(sig, freqs, w, on_device=True)
        ctx.sync()
        walls.append(time.perf_counter() - t0)
        del out
    lines.append(f"resident class call cwt(on_device=True), 8 x 2^20: {1e3 * float(np.median(walls)):8.1f} ms (median "
                 f"of {reps}, wavelets built on the host included)")
    # squeeze kernel on the resident scalogram
    S = cwt(sig, freqs, w, on_device=True)
    ctx.profile_enable(True)
    sq_ms, _ = kernel_ms(ctx, lambda: backend.cwt_squeeze_device(S, freqs, FS), max(1, reps // 2))
    ctx.profile_enable(False)
    lines.append(f"squeeze kernel 8 x 2^20 x 64 (complex128 out, 8.6 GB): {sq_ms:8.3f} ms")
    del S
    # host route, smaller shape
    n_h = 1 << 18
    xh = x[:2, :n_h].T.astype(np.float64)
    hs = dsp.Signal(None, xh, FS)
    cwt(hs, freqs, w)
    t0 = time.perf_counter()
    out = cwt(hs, freqs, w)
    lines.append(f"host route cwt(), 2 x 2^18 x 64 (complex128 result, {out.nbytes / 1e6:.0f} MB): "
                 f"{1e3 * (time.perf_counter() - t0):8.1f} ms (one run)")
    del out
    # composition: real and imaginary parts as 2F real filters, padded to the longest wavelet (ds_fir_ola_dev)
    lmax = int(lens.max())
    bank = np.zeros((2 * F, lmax), dtype=np.float64)
    for i, v in enumerate(waves):
        bank[2 * i, :len(v)] = v.real
        bank[2 * i + 1, :len(v)] = v.imag
    ctx.profile_enable(True)
    comp_ms, _ = kernel_ms(ctx, lambda: backend.fir_filter_bank_device(sig.device_samples, list(bank),
                                                                       backend.DS_FB_PARALLEL), 2)
    ctx.profile_enable(False)
    lines.append(f"composition: ds_fir_ola_dev, {2 * F} real filters x {lmax} taps, 8 x 2^20 (fp32 out 8.6 GB): "
                 f"{comp_ms:8.3f} ms kernels; the interleave into (F, N, C) complex64 not measured (>= "
                 f"{2 * F * N * C * 4 * 2 / (WRITE_TBS * 1e12) * 1e3:.2f} ms more at {WRITE_TBS:.0f} TB/s)")
    return lines


def run_reference():
    from oracle.gen_golden import import_reference
    ref = import_reference()
    n, c, f = 1 << 14, 2, 16
    freqs = np.geomspace(50, 20000, f)
    x = np.random.default_rng(1).standard_normal((n, c))
    w = ref.transforms.MorletWavelet(h=3, step=1e-3)
    sig = ref.Signal(None, x, FS)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        ref.transforms.cwt(sig, freqs, w)
    dt = time.perf_counter() - t0
    scale = (N / n) * (C / c) * (F / f)
    return [f"reference CPU cwt {c} x {n} x {f} frequencies (50 Hz - 20 kHz): {dt:.3f} s; linear in samples, "
            f"channels and frequencies that is ~{dt * scale:.0f} s at 8 x 2^20 x 64 (extrapolated, not run)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cwt_timing.txt"))
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    lines = run_reference() if a.reference else run_gpu(a.reps)
    print("\n".join(lines))
    if not a.reference:
        with open(a.out, "w") as fh:
            fh.write("# tools/time_cwt.py: cwt, 8 channels x 2^20 samples at 48 kHz, 64 log-spaced frequencies "
                     "50 Hz - 20 kHz, MorletWavelet(h=3, step=1e-3).\n# MI355X: kernel times event-timed "
                     "(ds_profile), median; class call = wall time.\n\n## MI355X\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
