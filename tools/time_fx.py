"""Device time of the audio effects (csrc/kernels_fx.hpp), run by hand on the GPU:
    python tools/time_fx.py [--reps 5] [--out profiles/fx_timing.txt]

Signal: 2 channels x 480 000 samples (10 s at 48 kHz), a tone burst over low noise.  Per effect -- Compressor on the
signal and on an 8-band x 2-channel MultiBandSignal, DigitalDelay at 300 ms, a three-voice Chorus -- from a host float64
signal and from a device-resident one:
- the kernels' own time, median over --reps warm calls, from the begin / end events the library puts on each launch, and
  the time of each kernel;
- the time of the whole apply() as the caller sees it (wall clock, median): tables, staging, kernels, the result;
- for the follower, nanoseconds per sample per stream (its wave is serial in time: streams run side by side);
- beside each, the time of this file's float64 restatement of the reference's per-sample Python loop on this machine's
  CPU, measured at 4000 samples x 2 channels (median of 3) and SCALED linearly to the length and stream count above --
  the reference's loops are linear in both, and at full length they would run for minutes."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools.time_direct import kernel_ms  # noqa: E402

FS, N, N_CPU = 48000, 480000, 4000


def burst(n, n_ch, seed=1):
    rng = np.random.default_rng(seed)
    x = 0.01 * rng.standard_normal((n, n_ch))
    t = np.arange(n // 3, 2 * n // 3)
    for c in range(n_ch):
        x[t, c] += 0.8 / (1 + 0.5 * c) * np.sin(2 * np.pi * (440 + 130 * c) / FS * t)
    return x.astype(np.float32).astype(np.float64)


def wall_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


# ---- the reference's loops, restated in float64 for the CPU figure ------------------------------------------------------
def cpu_compressor(x, thr=-10.0, ratio=3.0, ca=0.5, cr=0.02):
    def knee(d):  # a hard knee on a 0-d value through boolean masks, as the reference's loop reaches its curve
        y = np.zeros_like(d)
        first, second, third = d - thr < 0, np.abs(d - thr) <= 0, d - thr > 0
        y[first] = d[first]
        y[second] = d[second]
        y[third] = thr + (d[third] - thr) / ratio
        return y

    y = x.copy()
    for ch in range(x.shape[1]):
        rms, g = 0, 1
        for i in np.arange(len(x)):
            samp = x[i, ch] ** 2
            rms = (1.0 if samp > rms else 0.01) * samp + (1 - (1.0 if samp > rms else 0.01)) * rms  # (computed, unused)
            d = 10 * np.log10(max(samp, 1e-30))
            f = 10 ** ((knee(d) - d) / 20)
            c = ca if f > g else cr
            g = c * f + (1 - c) * g
            y[i, ch] *= g
    return y


def cpu_delay(x, d, fb=0.1):
    td = np.append(x, np.zeros((int(d * (1 + fb * 15)), x.shape[1])), axis=0)
    for i in np.arange(d, len(td)):
        td[i, :] = td[i, :] + fb * td[i - d, :]
    return td


def cpu_chorus(x, m):
    pad = int(np.abs(m).max())
    td = np.append(x, np.zeros((pad, x.shape[1])), axis=0)
    new = np.zeros_like(td)
    for i in np.arange(len(x)):
        new[i, :] = td[i, :]
        for v in range(m.shape[1]):
            new[i, :] += td[i + m[i, v], :]
    return new


def run(reps):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import effects
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    x = burst(N, 2)
    host = dsp.Signal(None, x, FS, constrain_amplitude=False)
    dev = dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), FS)
    bands_host = dsp.MultiBandSignal([dsp.Signal(None, burst(N, 2, 10 + b), FS, constrain_amplitude=False) for b in range(8)])
    chorus = effects.Chorus([2, 3, 4], [5, 8, 12], [effects.LFO(f, "harmonic", True) for f in (1.5, 3.0, 0.7)])
    jobs = [("Compressor 2 ch x 480000, host", effects.Compressor(), host, 2),
            ("Compressor 2 ch x 480000, resident", effects.Compressor(), dev, 2),
            ("Compressor 8 bands x 2 ch x 480000, host", effects.Compressor(), bands_host, 16),
            ("DigitalDelay 300 ms, 2 ch x 480000, host", effects.DigitalDelay(300, 0.1), host, 2),
            ("DigitalDelay 300 ms, 2 ch x 480000, resident", effects.DigitalDelay(300, 0.1), dev, 2),
            ("Chorus 3 voices, 2 ch x 480000, host", chorus, host, 2),
            ("Chorus 3 voices, 2 ch x 480000, resident", chorus, dev, 2)]
    xs = burst(N_CPU, 2)
    m = np.round((np.sin(np.arange(N_CPU) * 2e-4)[:, None] * [2, 3, 4] + [5, 8, 12]) * 1e-3 * FS).astype(int)
    cpu = {"Compressor": wall_ms(lambda: cpu_compressor(xs), 3), "DigitalDelay": wall_ms(lambda: cpu_delay(xs, 14400), 3),
           "Chorus": wall_ms(lambda: cpu_chorus(xs, m), 3)}
    lines = [f"audio effects, {N} samples a stream at {FS} Hz, median of {reps} warm calls", ""]
    for name, fx, sig, streams in jobs:
        k_ms, per = kernel_ms(ctx, lambda: fx.apply(sig), reps)
        w_ms = wall_ms(lambda: fx.apply(sig), reps)
        kind = name.split()[0]
        # the delay loop's length is the padded one; the others' the signal's
        length = N + int(14400 * 2.5) if kind == "DigitalDelay" else N
        cpu_len = N_CPU + int(14400 * 2.5) if kind == "DigitalDelay" else N_CPU
        scaled = cpu[kind] * (length / cpu_len) * (streams / 2 if kind == "Compressor" else 1)
        lines.append(f"{name}")
        lines.append(f"    kernels {k_ms:9.3f} ms   apply() {w_ms:9.3f} ms   CPU loop restated, scaled from {N_CPU} samples: {scaled / 1e3:8.1f} s")
        lines.append("    " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(per.items())))
        if "fx_follow" in per:
            lines.append(f"    follower: {per['fx_follow'] * 1e6 / N:.2f} ns per sample per stream ({streams} streams side by side)")
    lines.append("")
    lines.append(f"CPU loops as measured: " + ", ".join(f"{k} {v:.1f} ms at {N_CPU} samples x 2 channels" for k, v in cpu.items()))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = run(a.reps)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
