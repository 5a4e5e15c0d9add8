"""Device time of effects.spectral.SpectralSubtractor (csrc/kernels_specsub.hpp), run by hand on the GPU:
    python tools/time_specsub.py [--reps 10] [--out profiles/specsub_timing.txt]

Signal: noise at -40 dB with a tone burst, float32 values, 480000 samples a stream at 48 kHz; the defaults (block 0.1 s:
windows of 4096 samples, 50 % overlap, Hann, exponent 2).  Shapes: 2 channels from a host array and resident, in adaptive
mode and in static mode with a given spectrum; 8 bands x 2 channels (a MultiBandSignal, one call) in both modes from host
arrays.  Per shape, after a preheat of the same call:
- the kernels' own times from the begin / end events the library puts on every launch, summed and one by one: median of
  --reps warm calls;
- the time of apply() as the caller sees it (wall clock, a resident call ended by a synchronise);
- beside each, the time of this file's float64 restatement of the reference's loop -- one numpy irfft per (frame,
  channel) -- on this machine's CPUs at N_CPU samples x 2 channels, scaled linearly to the shape's samples and streams
  (the loop is linear in both);
- per kernel the algorithmic bytes over its median time."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, N, N_CPU = 48000, 480000, 48000
KERNELS = ("ss_analyze", "ss_track", "ss_synth", "ss_ola", "ss_peak", "fx_scale")


def signal_data(n, n_ch, seed=1):
    rng = np.random.default_rng(seed)
    x = 0.01 * rng.standard_normal((n, n_ch))
    t = np.arange(n // 3, 2 * n // 3)
    for c in range(n_ch):
        x[t, c] += 0.8 / (1 + 0.5 * (c % 2)) * np.sin(2 * np.pi * (440 + 130 * c) / FS * t)
    return x.astype(np.float32).astype(np.float64)


def cpu_adaptive(x, window=4096, step=2048, thr=-40.0, ff=0.9, factor=2.0):
    """The reference's adaptive loop restated in float64: frames, one rfft of all of them, then per channel and frame the
    noise update, the clip and ONE irfft; the overlap-add and the peak."""
    from scipy.signal.windows import get_window
    n, n_ch = x.shape
    w = np.clip(get_window("hann", window), 1e-6, None)
    length = n + 2 * window
    frames = -(-length // step)
    td = np.zeros(((frames - 1) * step + window, n_ch))
    td[window:window + n] = x
    fr = np.stack([td[f * step:f * step + window] for f in range(frames)], axis=1)
    level = 10 * np.log10(np.clip(np.var(fr, axis=0), np.finfo(float).tiny, None))
    spec = np.fft.rfft(fr * w[:, None, None], axis=0)
    phase, mag = np.angle(spec), np.abs(spec)
    power = mag ** 2
    for c in range(n_ch):
        noise = np.zeros(window // 2 + 1)
        for f in range(frames):
            if level[f, c] < thr:
                noise = noise * ff + mag[:, f, c] * (1 - ff)
            rest = np.clip(power[:, f, c] - factor * noise ** 2, 0, None)
            fr[:, f, c] = np.fft.irfft(rest ** 0.5 * np.exp(1j * phase[:, f, c]))
    fr *= w[:, None, None]
    out, env = np.zeros_like(td), np.zeros(td.shape[0])
    for f in range(frames):
        out[f * step:f * step + window] += fr[:, f]
        env[f * step:f * step + window] += w * w
    out /= np.clip(env, 1e-4, None)[:, None]
    y = out[window:window + n]
    return y * (np.max(np.abs(x), axis=0) / np.max(np.abs(y), axis=0))


def median_wall_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def kernel_ms(ctx, call, reps):
    """{launch name: median ms of its launches in one call} over reps warm calls"""
    call()
    ctx.profile_enable(True)
    rows = []
    for _ in range(reps):
        ctx.profile_report()
        call()
        rows.append({k: v[0] for k, v in ctx.profile_report().items()})
    ctx.profile_enable(False)
    return {k: float(np.median([r.get(k, 0.0) for r in rows])) for k in KERNELS}


def run(reps):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend
    from dsptoolbox_amd.effects.spectral import SpectralSubtractor
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    x2 = signal_data(N, 2)
    window, step = 4096, 2048
    frames = backend.specsub_frames(N, window, step)
    given = 1e-4 * 1536.0 * np.ones(window // 2 + 1)  # the noise's squared magnitude under the window: 1e-4 x sum w^2
    small = signal_data(N_CPU, 2)
    cpu_ms = median_wall_ms(lambda: cpu_adaptive(small), 3)
    got = SpectralSubtractor().apply(dsp.Signal(None, small, FS, constrain_amplitude=False)).time_data
    want = cpu_adaptive(small)
    err = float(np.max(np.abs(got - want) / np.max(np.abs(want), axis=0)))

    host2 = dsp.Signal(None, x2, FS, constrain_amplitude=False)
    res2 = dsp.Signal.from_planar_f32(np.ascontiguousarray(x2.T, dtype=np.float32), FS)
    bands = dsp.MultiBandSignal([dsp.Signal(None, signal_data(N, 2, 10 + b), FS, constrain_amplitude=False) for b in range(8)])
    shapes = []
    for mode, fx in (("adaptive", SpectralSubtractor()),
                     ("static, given spectrum", SpectralSubtractor(False, spectrum_to_subtract=given))):
        shapes += [(f"{mode}, 2 ch x {N}, host", fx, host2, 2, False), (f"{mode}, 2 ch x {N}, resident", fx, res2, 2, True),
                   (f"{mode}, 8 bands x 2 ch x {N}, host", fx, bands, 16, False)]
    lines = [f"spectral subtraction, {N} samples a stream at {FS} Hz, windows of {window} samples every {step}: {frames} frames a "
             f"stream; median of {reps} warm calls", ""]
    for what, fx, sig, streams, is_resident in shapes:
        def call():
            r = fx.apply(sig)
            if is_resident:
                ctx.sync()
            return r
        for _ in range(2):
            call()
        k = kernel_ms(ctx, call, reps)
        w_ms = median_wall_ms(call, reps)
        scaled = cpu_ms * (N / N_CPU) * (streams / 2)
        slot_gb = 8.0 * (window + 2) * frames * streams / 1e9
        lines += [what,
                  f"    kernels {sum(k.values()):9.3f} ms   apply() {w_ms:9.3f} ms   CPU loop restated, scaled from {N_CPU} samples: "
                  f"{scaled / 1e3:6.2f} s",
                  "    " + "  ".join(f"{name} {k[name]:.3f}" for name in KERNELS),
                  f"    frame workspace {slot_gb:.3f} GB: analyze writes it ({slot_gb / (k['ss_analyze'] * 1e-3):.0f} GB/s), track reads and "
                  f"writes it ({2 * slot_gb / (k['ss_track'] * 1e-3):.0f} GB/s), synth reads and writes it "
                  f"({2 * slot_gb / (k['ss_synth'] * 1e-3):.0f} GB/s), ola reads it ({slot_gb / (k['ss_ola'] * 1e-3):.0f} GB/s)"]
    lines += ["", f"CPU loop as measured: {cpu_ms:.1f} ms at {N_CPU} samples x 2 channels, {os.cpu_count()} CPUs visible, "
              f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}",
              f"device against the restated loop at that length, of the peak: {err:.2e}"]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = run(a.reps)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
