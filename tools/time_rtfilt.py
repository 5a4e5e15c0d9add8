"""GPU time of the realtime filters over 8 channels x 2^20 samples: a state-variable filter, a 32-section parallel filter
with a 64-tap FIR part, an order-16 IIRFilter, a 16-state StateSpaceFilter and a 4096-tap FIRFilter, each through the host
entry (float64 arrays in and out, wall time of the call with its transfers) and over samples held in HBM (fp32 planar in
and out, event-timed stream time).

    python tools/time_rtfilt.py [--reps 5] [--out profiles/rtfilt_timing.txt]

Beside each figure: the reference's sample loop on the CPU -- the classes' process_sample is that loop's arithmetic line
by line -- timed over 4096 samples of one channel and scaled by 8 x 2^20 / 4096 (the loop's cost is linear in samples and
channels); for the parallel filter also scipy.signal.sosfilt once per section plus the FIR convolution over the whole
shape on the CPU, which is what the reference's filter_signal really costs; for the order-16 IIR filter also the same
filter as second-order sections through the existing device route (backend._sosfilt), host arrays.  The error of the
resident fp32 output against the float64 serial recursion of tests/rtfilt_oracle.py is taken on the first 2^13 samples
of channel 0."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CH, N, N_CHECK, N_LOOP = 8, 1 << 20, 1 << 13, 4096
FS = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtfilt_timing.txt"))
    args = ap.parse_args()
    import rtfilt_cases as rc
    import rtfilt_oracle as ro
    from scipy.signal import oaconvolve, sosfilt, tf2sos
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import DevicePlanar, get_context
    from dsptoolbox_amd.filterbanks import FIRFilter, IIRFilter, ParallelFilter, StateSpaceFilter, StateVariableFilter

    rng = np.random.default_rng(3)
    planar = rng.standard_normal((N_CH, N)).astype(np.float32)
    x = np.ascontiguousarray(planar.T.astype(np.float64))
    ctx = get_context()
    xd = DevicePlanar.from_planar(ctx, planar)

    par_s = rc.structure("parallel", 64)
    par_s["fir"] = rng.standard_normal(64) / 8
    par = ParallelFilter(np.array([0.5 + 0.1j]), 64, FS)
    par._sos = np.insert(par_s["sos"], 3, 1.0, axis=1)
    par._fir_coefficients = par_s["fir"]
    par._compute_filter_bank()
    tdf2 = rc.structure("tdf2", 16)
    ss = rc.structure("state_space", 16)
    fir_b = rng.standard_normal(4096) / 64
    svf = StateVariableFilter(1500.0, 0.4, FS)
    cases = [
        ("StateVariableFilter (four bands)", rc.pack(ro.svf_structure(1500.0, 0.4, FS)), ro.svf_structure(1500.0, 0.4, FS), svf),
        ("ParallelFilter, 32 sections + 64-tap FIR part", rc.pack(par_s), par_s, par),
        ("IIRFilter, order 16", rc.pack(tdf2), tdf2, IIRFilter(tdf2["b"].copy(), tdf2["a"].copy())),
        ("StateSpaceFilter, 16 states (dense A)", rc.pack(ss), ss,
         StateSpaceFilter(ss["A"], ss["B"][:, None], ss["C"][None, :], np.array([[ss["Dd"]]]))),
    ]
    lines = [f"realtime filters: {N_CH} ch x 2^20 samples; host = float64 arrays through ds_rtfilt / ds_rtfir (wall time with "
             f"transfers), resident = fp32 planar in HBM through the _dev entries (event-timed)"]

    def wall(fn):
        fn()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t))

    def events(fn):
        fn()
        ctx.sync()
        t = []
        for _ in range(args.reps):
            ctx.timer_start()
            out = fn()
            t.append(ctx.timer_stop())
            del out
        return float(np.median(t))

    def loop_scaled(f):
        f.set_n_channels(1)
        t0 = time.perf_counter()
        for v in x[:N_LOOP, 0]:
            f.process_sample(v, 0)
        return (time.perf_counter() - t0) * N_CH * N / N_LOOP

    def profile(fn, names):
        ctx.profile_enable(True)
        ctx.profile_report()
        fn()
        prof = ctx.profile_report()
        ctx.profile_enable(False)
        return "  kernels (library profile, ms): " + ", ".join(f"{n} {prof.get(n, (0.0, 0))[0]:.3f}" for n in names)

    for title, (kind, coef, d, aux, delay, fir), s, obj in cases:
        host = wall(lambda: backend.rtfilt_filter(x, kind, coef, d, aux, delay, fir))
        dev = events(lambda: backend.rtfilt_filter_device(xd, kind, coef, d, aux, delay, fir))
        y = backend.rtfilt_filter_device(xd, kind, coef, d, aux, delay, fir)
        y0 = (y[0] if isinstance(y, list) else y).to_planar()[0, :N_CHECK]
        ref = ro.serial(s, x[:N_CHECK, :1], dtype=np.float64)[0]
        ref = (ref[0] if ref.ndim == 3 else ref)[:, 0]
        err = float(np.max(np.abs(y0 - ref)) / np.max(np.abs(ref)))
        lines += [title, f"  host {host:9.2f} ms   resident {dev:8.3f} ms   (medians of {args.reps})",
                  profile(lambda: backend.rtfilt_filter_device(xd, kind, coef, d, aux, delay, fir),
                          ("rtfir", "rtfilt_group", "rtfilt_carry", "rtfilt_apply")),
                  f"  the reference's sample loop on this CPU, {N_LOOP} samples x 1 channel scaled to the shape: {loop_scaled(obj):9.1f} s",
                  f"  rel-max error of the resident fp32 output vs the float64 serial recursion (channel 0, 2^13 samples): {err:.2e}"]
        if kind == backend.RTFILT_PARALLEL:
            sos6 = np.insert(s["sos"], 3, 1.0, axis=1)
            t0 = time.perf_counter()
            out = oaconvolve(x, s["fir"][:, None], axes=0)[:N]
            for sec in sos6:
                out += sosfilt(sec[None, :], x, axis=0)
            lines.append(f"  scipy on this CPU over the whole shape (oaconvolve + sosfilt once per section): "
                         f"{1e3 * (time.perf_counter() - t0):9.1f} ms")
        if kind == backend.RTFILT_TDF2:
            sos = tf2sos(s["b"], s["a"])
            sos_host = wall(lambda: backend._sosfilt(sos, x))
            lines.append(f"  the same filter as {len(sos)} second-order sections through the existing device route "
                         f"(backend._sosfilt, host arrays): {sos_host:9.2f} ms"
                         + ("   -- the sos route is faster" if sos_host < host else ""))
    host = wall(lambda: backend.rtfir_filter(x, fir_b))
    dev = events(lambda: backend.rtfir_filter_device(xd, fir_b))
    y0 = backend.rtfir_filter_device(xd, fir_b).to_planar()[0, :N_CHECK]
    ref = ro.fir_direct(fir_b, x[:N_CHECK, :1], dtype=np.float64)[:, 0]
    err = float(np.max(np.abs(y0 - ref)) / np.max(np.abs(ref)))
    gflops = 2.0 * N_CH * N * len(fir_b) / (dev * 1e-3) / 1e9
    lines += ["FIRFilter, 4096 taps (direct float64 sum)",
              f"  host {host:9.2f} ms   resident {dev:8.3f} ms   ({gflops:.0f} float64 GFLOP/s resident)",
              profile(lambda: backend.rtfir_filter_device(xd, fir_b), ("rtfir",)),
              f"  the reference's sample loop on this CPU, 64 samples x 1 channel scaled to the shape: "
              f"{_fir_loop(FIRFilter(fir_b.copy()), x) :9.1f} s",
              f"  rel-max error of the resident fp32 output vs the float64 direct sum (channel 0, 2^13 samples): {err:.2e}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


def _fir_loop(f, x, count=64):
    f.set_n_channels(1)
    t0 = time.perf_counter()
    for v in x[:count, 0]:
        f.process_sample(v, 0)
    return (time.perf_counter() - t0) * N_CH * N / count


if __name__ == "__main__":
    main()
