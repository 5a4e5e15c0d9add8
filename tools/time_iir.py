"""GPU time of the IIR filter bank: the 1/1-octave 6th-order Butterworth bank (10 bands, 31.5 Hz - 16 kHz, 48 kHz) over
8 channels x 2^22 samples held in HBM, Parallel mode (ds_iir_sos_dev: fp32 planar in and out, float64 recursion),
next to scipy.signal.sosfilt on the host.

    python tools/time_iir.py [--reps 10] [--out profiles/iir_timing.txt]

Reported: the call's event-timed stream time (median of --reps), each pass's kernel time from the library's per-kernel
profile (a separate run of the same calls), the output bytes over the measured device copy bandwidth, and scipy's
sosfilt seconds for the same bank on one channel (single core; the eight channels are eight times that)."""

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, N_CH, N = 48000, 8, 1 << 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iir_timing.txt"))
    args = ap.parse_args()
    import scipy.signal as sig

    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context

    bank = dsp.filterbanks.fractional_octave_bands([31.5, 16e3], 1, 6, FS)[0]
    sos = backend._sos_stack([f.sos for f in bank.filters])
    k, n_sec = sos.shape[:2]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N_CH, N)).astype(np.float32)
    ctx = get_context()
    xd = DevicePlanar.from_planar(ctx, x)
    yd = DeviceBuffer(ctx, k * N_CH * N * 4)

    def call():
        ctx.check(ctx.lib.ds_iir_sos_dev(ctx.handle, C.c_void_p(xd.ptr), N_CH, N, N, sos.ctypes.data_as(C.c_void_p), k,
                                         n_sec, None, backend.DS_FB_PARALLEL, C.c_void_p(yd.ptr), N, None), "ds_iir_sos_dev")

    for _ in range(2):
        call()
    ctx.sync()
    times = []
    for _ in range(args.reps):
        ctx.timer_start()
        call()
        times.append(ctx.timer_stop())
    ctx.profile_enable(True)
    ctx.profile_report()
    for _ in range(args.reps):
        call()
    prof = ctx.profile_report()
    ctx.profile_enable(False)
    gbs = C.c_double(0.0)
    ctx.check(ctx.lib.ds_measure_copy(ctx.handle, 1 << 30, 10, C.byref(gbs)), "ds_measure_copy")
    # correctness of what was timed, on two bands of channel 0
    y0 = np.empty(N, dtype=np.float32)
    errs = []
    for b in (0, 9):
        ctx.check(ctx.lib.ds_download(ctx.handle, y0.ctypes.data_as(C.c_void_p), C.c_void_p(yd.ptr + 4 * b * N_CH * N),
                                      N * 4), "ds_download")
        ref = sig.sosfilt(bank.filters[b].sos, x[0].astype(np.float64))
        errs.append(float(np.max(np.abs(y0 - ref)) / np.max(np.abs(ref))))
    t0 = time.perf_counter()
    for f in bank.filters:
        sig.sosfilt(f.sos, x[0].astype(np.float64))
    scipy_s = time.perf_counter() - t0
    out_bytes = k * N_CH * N * 4
    ms = float(np.median(times))
    lines = [f"IIR bank: 1/1 octave, 6th-order Butterworth, {k} bands x {n_sec} sections (identity-padded), "
             f"{N_CH} ch x 2^22 samples, Parallel, resident (ds_iir_sos_dev)",
             f"call (event-timed, median of {args.reps}): {ms:.3f} ms",
             "per pass (library profile, ms per call):"]
    for name in ("iir_group", "iir_carry", "iir_apply"):
        tot, cnt = prof.get(name, (0.0, 0))
        lines.append(f"  {name:10s} {tot / max(cnt, 1):8.3f}  ({cnt} launches)")
    lines += [f"output {out_bytes / 1e9:.3f} GB; measured copy bandwidth {gbs.value:.0f} GB/s -> writing it alone "
              f"takes {out_bytes / gbs.value / 1e6:.3f} ms ({out_bytes / gbs.value / 1e6 / ms * 100:.0f} % of the call)",
              f"scipy.signal.sosfilt, host, one channel, {k} bands: {scipy_s:.2f} s "
              f"(x {N_CH} channels: {scipy_s * N_CH:.1f} s)",
              f"rel-max error of the timed output vs sosfilt (bands 0 and 9, channel 0): {max(errs):.2e}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    yd.free()


if __name__ == "__main__":
    main()
