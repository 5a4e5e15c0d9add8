"""GPU time of the complex-coefficient recursion and of fw_snr_seg:

- the 40-band gammatone bank ([20, 20000] Hz, 48 kHz: 4 complex one-pole sections a band) over 8 channels x 2^22 samples
  through ds_iir_sos_c128 (host entry, real part only), per kernel, beside ds_iir_sos_dev on 40 filters of four REAL
  sections of the same shape and scipy.signal.sosfilt on the host;
- distances.fw_snr_seg on 10 s at 48 kHz, two channels, resident signals, per kernel.

    python tools/time_gammatone.py [--reps 3] [--out profiles/gammatone_timing.txt]

The generic complex section spends two thirds of its multiplies on the gammatone's zero coefficients (b1, b2, a2 = 0):
the comparison with the real cascade of the same shape says what the complex arithmetic costs as it is built."""

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, N_CH, N = 48000, 8, 1 << 22


def per_kernel(ctx, call, names, reps):
    ctx.profile_enable(True)
    ctx.profile_report()
    for _ in range(reps):
        call()
    prof = ctx.profile_report()
    ctx.profile_enable(False)
    return [f"  {name:16s} {prof.get(name, (0.0, 0))[0] / reps:9.3f} ms per call  ({prof.get(name, (0.0, 0))[1] // reps} launches)"
            for name in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gammatone_timing.txt"))
    args = ap.parse_args()
    import scipy.signal as sig

    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context

    ctx = get_context()
    rng = np.random.default_rng(3)
    bank = dsp.filterbanks.auditory_filters_gammatone([20, 20000], 1, FS)
    sections = [f.sos for f in bank.filters]
    k = len(sections)
    x = rng.standard_normal((N, N_CH))
    lines = [f"gammatone bank: {k} bands x 4 complex sections, {N_CH} ch x 2^22 samples, real part only (ds_iir_sos_c128, host entry)"]

    out = {}

    def complex_call():
        out["y"] = backend.iir_sos_filter_complex(x, sections, real_only=True)

    complex_call()
    t0 = time.perf_counter()
    complex_call()
    lines.append(f"call, wall clock with the {x.nbytes / 1e9:.2f} GB up and {out['y'].nbytes / 1e9:.2f} GB down: {time.perf_counter() - t0:.2f} s")
    lines += per_kernel(ctx, complex_call, ("ciir_group", "ciir_carry", "ciir_apply"), 1)
    ref = sig.sosfilt(sections[k // 2], x[:1 << 18, 0])
    err = float(np.max(np.abs(out["y"][k // 2, :1 << 18, 0] - ref.real)) / np.max(np.abs(ref)))
    lines.append(f"rel-max error of the timed output vs scipy's complex sosfilt (band {k // 2}, channel 0, 2^18 samples): {err:.2e}")
    t0 = time.perf_counter()
    sig.sosfilt(sections[0], x[:, 0])
    scipy_s = time.perf_counter() - t0
    lines.append(f"scipy.signal.sosfilt, host, one band, one channel: {scipy_s:.2f} s (x {k} bands x {N_CH} channels: {scipy_s * k * N_CH:.0f} s)")
    out.clear()

    # the same shape with REAL sections, resident, fp32 out
    real = backend._sos_stack([sig.butter(8, [0.1 + 0.01 * i, 0.3 + 0.01 * i], btype="band", output="sos")[:4] for i in range(k)])
    xd = DevicePlanar.from_planar(ctx, x.T.astype(np.float32))
    yd = DeviceBuffer(ctx, k * N_CH * N * 4)

    def real_call():
        ctx.check(ctx.lib.ds_iir_sos_dev(ctx.handle, C.c_void_p(xd.ptr), N_CH, N, N, real.ctypes.data_as(C.c_void_p), k, 4, None,
                                         backend.DS_FB_PARALLEL, C.c_void_p(yd.ptr), N, None), "ds_iir_sos_dev")

    real_call()
    ctx.sync()
    lines.append(f"real cascade of the same shape: {k} filters x 4 real sections, resident (ds_iir_sos_dev)")
    lines += per_kernel(ctx, real_call, ("iir_group", "iir_carry", "iir_apply"), args.reps)
    yd.free()

    # fw_snr_seg, 10 s at 48 kHz, two channels, resident
    n = 10 * FS
    a = rng.standard_normal((n, 2)).astype(np.float32).astype(np.float64)
    b = (a + 0.3 * rng.standard_normal((n, 2))).astype(np.float32).astype(np.float64)
    sa = dsp.Signal(None, a, FS, constrain_amplitude=False).to_device()
    sb = dsp.Signal(None, b, FS, constrain_amplitude=False).to_device()
    val = {}

    def fw_call():
        val["v"] = dsp.distances.fw_snr_seg(sa, sb)

    fw_call()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fw_call()
        times.append(time.perf_counter() - t0)
    n_band = len(dsp.filterbanks.auditory_filters_gammatone([20, 10e3], 1, FS))
    lines.append(f"fw_snr_seg: 10 s at 48 kHz, 2 channels, resident, {n_band} bands, window 3600 (Bluestein, M = 8192), "
                 f"{-(-n // 1800)} frames -> {val['v']} dB")
    lines.append(f"call, wall clock (median of {args.reps}): {np.median(times) * 1e3:.1f} ms")
    lines += per_kernel(ctx, fw_call, ("ciir_group", "ciir_carry", "ciir_apply", "fw_frame", "fft64_blue", "fft64_lds",
                                       "fw_reduce"), args.reps)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
