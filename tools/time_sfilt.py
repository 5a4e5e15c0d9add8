"""GPU time of the structure filters: a warped FIR filter of order 32 and an IIR lattice-ladder of order 16, each over
8 channels x 2^20 samples held in HBM (ds_sfilt_dev: fp32 planar in and out, float64 recursion).

    python tools/time_sfilt.py [--reps 10] [--out profiles/sfilt_timing.txt]

Reported per filter: the call's event-timed stream time (median of --reps), each pass's kernel time from the library's
per-kernel profile (a separate run of the same calls), and the error of the timed output against the float64 serial
recursion of tests/sfilt_oracle.py on the first 2^13 samples of channel 0."""

import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CH, N, N_CHECK = 8, 1 << 20, 1 << 13


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfilt_timing.txt"))
    args = ap.parse_args()
    import sfilt_oracle as so
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar, get_context

    rng = np.random.default_rng(3)
    x = rng.standard_normal((N_CH, N)).astype(np.float32)
    k = rng.uniform(-0.9, 0.9, 16)
    filters = [("warped FIR, order 32 (33 states), lambda 0.7", backend.SFILT_WARPED_FIR,
                dict(kind="warped_fir", lam=0.7, b=rng.standard_normal(33))),
               ("IIR lattice-ladder, order 16 (16 states)", backend.SFILT_IIR_LATTICE,
                dict(kind="iir_lattice", k=k, c=rng.standard_normal(17)))]
    ctx = get_context()
    xd = DevicePlanar.from_planar(ctx, x)
    yd = DeviceBuffer(ctx, N_CH * N * 4)
    lines = [f"structure filters: {N_CH} ch x 2^20 samples, resident (ds_sfilt_dev)"]
    for title, kind, s in filters:
        coef = np.ascontiguousarray(np.concatenate([[s["lam"]], s["b"]]) if kind == backend.SFILT_WARPED_FIR
                                    else np.concatenate([s["k"], s["c"]]))
        d = so.n_states(s)

        def call():
            ctx.check(ctx.lib.ds_sfilt_dev(ctx.handle, C.c_void_p(xd.ptr), N_CH, N, N, kind, coef.ctypes.data_as(C.c_void_p),
                                           d, 0, None, C.c_void_p(yd.ptr), N, None), "ds_sfilt_dev")

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
        y0 = np.empty(N_CHECK, dtype=np.float32)
        ctx.check(ctx.lib.ds_download(ctx.handle, y0.ctypes.data_as(C.c_void_p), C.c_void_p(yd.ptr), N_CHECK * 4), "ds_download")
        ref = so.serial(s, x[0, :N_CHECK, None].astype(np.float64), dtype=np.float64)[0][:, 0]
        err = float(np.max(np.abs(y0 - ref)) / np.max(np.abs(ref)))
        lines += [title, f"  call (event-timed, median of {args.reps}): {float(np.median(times)):.3f} ms",
                  "  per pass (library profile, ms per call):"]
        for name in ("sfilt_group", "sfilt_carry", "sfilt_apply"):
            tot, cnt = prof.get(name, (0.0, 0))
            lines.append(f"    {name:12s} {tot / max(cnt, 1):8.3f}  ({cnt} launches)")
        lines.append(f"  rel-max error of the timed fp32 output vs the float64 serial recursion (channel 0, 2^13 samples): {err:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    yd.free()


if __name__ == "__main__":
    main()
