"""GPU time of the time-domain delay-and-sum beamformer (BeamformerDASTime) at 64 microphones x 2500 grid points x
48000 samples (48 kHz), order-30 fractional delay filters.
    python tools/time_das_time.py [--reps 10] [--out profiles/das_time_timing.txt]
    python tools/time_das_time.py --reference     # the reference's CPU seconds at 16 mics x 16 points x 16000 samples
Reported: the k_delay_sum kernel alone (median of --reps, event-timed on the stream) with its FMA rate against the
78.6 TFLOP/s FP64 vector peak (G M N (order + 1) multiply-adds of 2 flops), the tap kernel, and the wall time of
get_beamformer_output on a host signal (float64 result downloaded) and on a device-resident one (float32 result left
in HBM)."""

import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS, SOUND, ORDER, PEAK_TFLOPS = 48000, 343.0, 30, 78.6


class Points:
    def __init__(self, xyz):
        self.coordinates = xyz
        self.number_of_points = len(xyz)

    def get_distances_to_point(self, pts):
        pts = np.atleast_2d(pts)
        return np.sqrt(((self.coordinates[:, None, :] - pts[None, :, :]) ** 2).sum(-1)).squeeze()


def geometry(n_mics, n_line):
    rng = np.random.default_rng(7)
    mics = np.stack([rng.uniform(-0.5, 0.5, n_mics), rng.uniform(-0.5, 0.5, n_mics), np.zeros(n_mics)], axis=1)
    line = np.linspace(-0.5, 0.5, n_line)
    gx, gy = np.meshgrid(line, line, indexing="ij")
    return Points(mics), Points(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.5)], axis=1))


def run_gpu(reps: int):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd.beamforming import BeamformerDASTime
    from dsptoolbox_amd._lib import get_context
    m, n = 64, 48000
    mics, grid = geometry(m, 50)
    g = grid.number_of_points
    x = np.random.default_rng(1).standard_normal((n, m)).astype(np.float32)
    s_dev = dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T), FS)
    bf = BeamformerDASTime(s_dev, mics, grid)
    out = bf.get_beamformer_output()  # warm-up (and the workspace)
    total = out.length_samples
    del out
    ctx = get_context()
    ctx.profile_enable(True)
    ctx.lib.ds_profile_report(ctx.handle)
    times = {"delay_sum": [], "delay_taps": []}
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = bf.get_beamformer_output()
        ctx.check(ctx.lib.ds_sync(ctx.handle), "ds_sync")  # the launch is asynchronous: time it to completion
        walls.append(time.perf_counter() - t0)
        del out
        rep = ctx.lib.ds_profile_report(ctx.handle).decode()
        for line in rep.splitlines():
            name, ms, _ = line.split()
            if name in times:
                times[name].append(float(ms))
    ctx.profile_enable(False)
    k_ms = float(np.median(times["delay_sum"]))
    taps_ms = float(np.median(times["delay_taps"]))
    fma = g * m * n * (ORDER + 1)
    tflops = 2 * fma / (k_ms * 1e-3) / 1e12
    s_host = dsp.Signal(None, x.astype(np.float64), FS)
    bf_h = BeamformerDASTime(s_host, mics, grid)
    t0 = time.perf_counter()
    out = bf_h.get_beamformer_output()
    host_s = time.perf_counter() - t0
    assert out.time_data.shape == (total, g)
    del out
    shape = f"M={m} G={g} N={n} order={ORDER}"
    return [f"k_delay_sum  {shape}: {k_ms:8.3f} ms (median of {reps}, min {min(times['delay_sum']):.3f})   "
            f"{fma / 1e9:.1f} G FMA = {tflops:.1f} TFLOP/s = {100 * tflops / PEAK_TFLOPS:.0f} % of {PEAK_TFLOPS} FP64",
            f"k_delay_taps {shape}: {taps_ms:8.3f} ms ({g * m} filters)",
            f"class call, resident route (float32 result in HBM): {1e3 * float(np.median(walls)):8.1f} ms (median)",
            f"class call, host route (float64 result, {total * g * 8 / 1e6:.0f} MB downloaded): {1e3 * host_s:8.1f} ms "
            f"(one run)"]


def run_reference():
    from oracle.gen_golden import import_reference
    ref = import_reference()
    m, side, n = 16, 4, 16000
    mics, grid = geometry(m, side)
    rmics = ref.beamforming.MicArray(dict(x=mics.coordinates[:, 0], y=mics.coordinates[:, 1], z=mics.coordinates[:, 2]))
    rgrid = ref.beamforming.Grid(dict(x=grid.coordinates[:, 0], y=grid.coordinates[:, 1], z=grid.coordinates[:, 2]))
    x = np.random.default_rng(1).standard_normal((n, m))
    bf = ref.beamforming.BeamformerDASTime(ref.Signal(None, x, FS), rmics, rgrid)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        bf.get_beamformer_output()
    dt = time.perf_counter() - t0
    pairs = m * grid.number_of_points
    return [f"reference CPU M={m} G={grid.number_of_points} N={n}: {dt:.3f} s ({1e3 * dt / pairs:.2f} ms per pair; "
            f"at M=64 G=2500 N=48000 that is ~{dt / pairs * 64 * 2500 * 3 / 60:.1f} min)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "das_time_timing.txt"))
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    lines = run_reference() if a.reference else run_gpu(a.reps)
    print("\n".join(lines))
    if not a.reference:
        with open(a.out, "w") as fh:
            fh.write("# tools/time_das_time.py: BeamformerDASTime, 64 microphones, 2500 grid points (50 x 50 at 0.5 m), "
                     "48000 samples at 48 kHz,\n# order-30 fractional delay filters.  MI355X: kernel = k_delay_sum alone "
                     "(event-timed, median); class call = get_beamformer_output wall time.\n\n## MI355X\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
