"""Device time of the rational-ratio resampler (csrc/kernels_resample.hpp), run by hand on the GPU:
    python tools/time_resample.py [--reps 30] [--cpu-reps 3] [--out profiles/resample_timing.txt]

Signal: 64 channels x 441000 samples, noise on an offset in float32 values, taken 44100 -> 48000 (160 / 147) and
48000 -> 44100 (147 / 160).  Per direction, after a preheat of the same calls:
- the kernel's own time from the begin / end events the library puts on the launch, resident (float32 planar in and out)
  and from a host array (float64 interleaved in and out): median, smallest and largest of --reps warm calls;
- the time of the whole call as the caller sees it (wall clock around a call that ends in a synchronise): resident, and
  from a host array (staging both ways included);
- scipy.signal.resample_poly(x, up, down, axis=0) on the same data on this machine's CPUs -- the reference's resample IS
  that call -- median of --cpu-reps calls;
- the resident kernel's algorithmic bytes, 4 B read per input and 4 B written per output sample and channel, over its
  median time, as a fraction of 8 TB/s, and its multiply-adds per second."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, N_CH = 441000, 64
HBM_BYTES_PER_S = 8e12
DIRECTIONS = [(44100, 48000, 160, 147), (48000, 44100, 147, 160)]


def signal_data():
    rng = np.random.default_rng(1)
    x = 0.25 * rng.standard_normal((N, N_CH)) + 0.1
    return x.astype(np.float32).astype(np.float64)


def wall_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def kernel_times_ms(ctx, call, reps):
    """the resample_poly launch's time in each of reps warm calls, from the library's launch events"""
    call()
    ctx.profile_enable(True)
    out = []
    for _ in range(reps):
        ctx.lib.ds_profile_report(ctx.handle)
        call()
        rep = ctx.lib.ds_profile_report(ctx.handle).decode()
        rows = {line.split()[0]: float(line.split()[1]) for line in rep.splitlines() if line.strip()}
        assert set(rows) == {"resample_poly"}, rows
        out.append(rows["resample_poly"])
    ctx.profile_enable(False)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def run(reps, cpu_reps):
    from scipy.signal import resample_poly
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend
    from dsptoolbox_amd._lib import get_context
    ctx = get_context()
    x = signal_data()
    planar = np.ascontiguousarray(x.T, dtype=np.float32)
    lines = [f"resample, {N_CH} channels x {N} samples; {reps} warm calls per figure: median (smallest .. largest)", ""]
    for fs, new_fs, up, down in DIRECTIONS:
        host = dsp.Signal(None, x, fs)
        res = dsp.Signal.from_planar_f32(planar, fs)
        n_out = -(-N * up // down)
        tile, chunks, span, lds = backend._resample_tile(up, down, N_CH)

        def resident():
            r = dsp.resample(res, new_fs)
            ctx.sync()
            return r

        def from_host():
            return dsp.resample(host, new_fs)

        for _ in range(3):  # preheat: code objects, workspaces, clocks
            resident()
            from_host()
        k_res = kernel_times_ms(ctx, resident, reps)
        k_host = kernel_times_ms(ctx, from_host, max(3, reps // 5))
        w_res = wall_ms(resident, reps)
        w_host = wall_ms(from_host, max(3, reps // 5))
        cpu = wall_ms(lambda: resample_poly(x, up, down, axis=0), cpu_reps)
        got = resident().time_data
        want = resample_poly(x, up, down, axis=0)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        gb = 4.0 * (N + n_out) * N_CH / 1e9
        terms = -(-(20 * max(up, down) + 1) // up)
        fma = float(n_out) * N_CH * terms
        lines += [
            f"{fs} -> {new_fs} ({up} / {down}): {n_out} output samples; tile {tile} outputs x 4 channels, {chunks} chunk, "
            f"{lds} bytes of LDS, {terms} terms per output",
            f"    kernel, resident (float32 planar)      {k_res[0]:9.3f} ms ({k_res[1]:.3f} .. {k_res[2]:.3f})",
            f"    kernel, host array (float64)           {k_host[0]:9.3f} ms ({k_host[1]:.3f} .. {k_host[2]:.3f})",
            f"    call, resident                         {w_res[0]:9.3f} ms ({w_res[1]:.3f} .. {w_res[2]:.3f})",
            f"    call, host array (staging included)    {w_host[0]:9.3f} ms ({w_host[1]:.3f} .. {w_host[2]:.3f})",
            f"    scipy.signal.resample_poly on the CPU  {cpu[0]:9.1f} ms ({cpu[1]:.1f} .. {cpu[2]:.1f}), {os.cpu_count()} CPUs visible, "
            f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}",
            f"    resident kernel: {gb:.3f} GB algorithmic, {gb / (k_res[0] * 1e-3):.0f} GB/s = "
            f"{100 * gb * 1e9 / (k_res[0] * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s; {fma / (k_res[0] * 1e-3) / 1e12:.2f} T float64 multiply-adds/s",
            f"    resident result against scipy, of the peak: {err:.2e} (float32 storage)", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = run(a.reps, a.cpu_reps)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
