"""Device time of the level and loudness functions (csrc/kernels_level.hpp), run by hand:
    python tools/time_levels.py --cpu levels_cpu.json            (where the reference is installed: its CPU times)
    python tools/time_levels.py [--reps 5] [--cpu levels_cpu.json] [--out profiles/levels_timing.txt]     (on the GPU)

Signal: 8 channels x 2^22 samples at 48 kHz, noise on a line.  Per function -- normalize (peak), fade, detrend(1), rms,
lufs_integrated (on the first 5 channels: it takes no more), both envelopes -- from a host float64 signal and from a device-resident one:
- the kernels' own time, median over --reps warm calls, from the begin / end events the library puts on each launch,
  and the time of each kernel;
- the bytes the kernels must move, counted from the shapes (each pass reads every sample once in its storage type and the
  apply pass writes it once), over that time, beside the device-to-device copy rate ds_measure_copy reports in the same run;
- the time of the whole call as the caller sees it (wall clock, median): staging, kernels, the result;
- beside each, the reference on a CPU (--cpu file, median of 3 calls at the same shape)."""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS, N, N_CH, WINDOW = 48000, 1 << 22, 8, 4800


def signal_data():
    rng = np.random.default_rng(1)
    x = 0.1 * rng.standard_normal((N, N_CH)) + 0.05 + 0.1 * np.linspace(-1, 1, N)[:, None]
    return x.astype(np.float32).astype(np.float64)


def calls(dsp):
    """name -> (call on a signal, passes over the samples read, passes written)"""
    return {
        "normalize (peak)": (lambda s: dsp.normalize(s, -3.0), 2, 1),
        "fade": (lambda s: dsp.fade(s, dsp.FadeType.Logarithmic, 1.0), 1, 1),
        "detrend(1)": (lambda s: dsp.detrend(s, 1), 2, 1),
        "rms": (lambda s: dsp.rms(s), 2, 0),
        "lufs_integrated": (lambda s: dsp.lufs_integrated(s), None, None),
        "envelope (analytic)": (lambda s: dsp.envelope(s), None, None),
        f"envelope (boxcar {WINDOW})": (lambda s: dsp.envelope(s, False, WINDOW), None, None),
    }


def wall_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def run_cpu(path):
    from oracle.gen_golden import import_reference
    dsp = import_reference()
    import warnings
    warnings.simplefilter("ignore")
    x = signal_data()
    s = dsp.Signal(None, x, FS, constrain_amplitude=False)
    s5 = dsp.Signal(None, x[:, :5].copy(), FS, constrain_amplitude=False)
    out = {name: wall_ms(lambda f=f, name=name: f(s5 if name.startswith("lufs") else s), 3) for name, (f, _, _) in calls(dsp).items()}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


def run_gpu(reps, cpu):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd._lib import get_context
    from tools.time_direct import kernel_ms
    ctx = get_context()
    gbs = C.c_double(0.0)
    ctx.check(ctx.lib.ds_measure_copy(ctx.handle, 1 << 30, 10, C.byref(gbs)), "ds_measure_copy")
    x = signal_data()
    host = dsp.Signal(None, x, FS, constrain_amplitude=False)
    res = dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), FS)
    host5 = dsp.Signal(None, x[:, :5].copy(), FS, constrain_amplitude=False)
    res5 = dsp.Signal.from_planar_f32(np.ascontiguousarray(x[:, :5].T, dtype=np.float32), FS)
    lines = [f"levels and loudness, {N_CH} channels x {N} samples at {FS} Hz, median of {reps} warm calls",
             f"device-to-device copy rate of this GPU (ds_measure_copy, 1 GiB, read + written bytes): {gbs.value:.0f} GB/s", ""]
    for name, (f, reads, writes) in calls(dsp).items():
        five = name.startswith("lufs")
        for where, s, width in (("host", host5 if five else host, 8), ("resident", res5 if five else res, 4)):
            def call():
                r = f(s)
                ctx.sync()
                return r
            k_ms, per = kernel_ms(ctx, call, reps)
            w_ms = wall_ms(call, reps)
            ref = f"   reference on a CPU {cpu[name]:10.1f} ms" if name in cpu else ""
            lines.append(f"{name}, {where}")
            rate = ""
            if reads is not None:
                gb = (reads + writes) * width * N * N_CH / 1e9
                rate = f"   {gb:.3f} GB moved, {gb / (k_ms * 1e-3):7.0f} GB/s ({100 * gb / (k_ms * 1e-3) / gbs.value:.0f} % of the copy rate)"
            lines.append(f"    kernels {k_ms:9.3f} ms   call {w_ms:9.3f} ms{rate}{ref}")
            lines.append("    " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(per.items())))
    # the existing two-section sos filter on the same shape, for the loudness figure
    from dsptoolbox_amd.standard.gain_and_level import _k_weighting_sos
    k = dsp.Filter.from_sos(_k_weighting_sos(FS), FS)
    for where, s in (("host", host5), ("resident", res5)):
        def call():
            r = k.filter_signal(s)
            ctx.sync()
            return r
        k_ms, per = kernel_ms(ctx, call, reps)
        lines.append(f"two-section sos filter (Filter.filter_signal) on 5 channels, {where}: kernels {k_ms:9.3f} ms")
        lines.append("    " + "  ".join(f"{kk} {v:.3f}" for kk, v in sorted(per.items())))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cpu and not (a.out or os.path.exists(a.cpu)):
        run_cpu(a.cpu)
    else:
        cpu = json.load(open(a.cpu)) if a.cpu and os.path.exists(a.cpu) else {}
        text = run_gpu(a.reps, cpu)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(text)
