"""GPU time of the CleanSC, Orthogonal, Functional and MVDR beamformers at 48 and 64 microphones x 2500 grid points
x a 1/3-octave band at 4 kHz (48 kHz, 2048-sample window: 40 bins), and how far each map moves when the CSM comes
from the fp32 Welch route (128 frames or more) instead of a float64 one.

    python tools/time_beamformers.py [--reps 20] [--out profiles/beamformers_timing.txt]
    python tools/time_beamformers.py --reference      # the reference's CPU seconds, same shapes (needs its source)

Reported per method and array size: the device time of the map call alone (ds_bf_eig_map_dev / ds_bf_cleansc_dev on
inputs already in HBM, median of --reps, event-timed on the stream) and the wall time of the class's
get_beamformer_map with a cached CSM (steering vectors built in numpy, upload, map, download, integration)."""

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, W, FC, FRAC, SOUND = 48000, 2048, 4000.0, 3, 343.0
METHODS = ("mvdr", "functional", "orthogonal", "cleansc")


def geometry(n_mics: int):
    rng = np.random.default_rng(7)
    mics = np.stack([rng.uniform(-0.5, 0.5, n_mics), rng.uniform(-0.5, 0.5, n_mics), np.zeros(n_mics)], axis=1)
    line = np.linspace(-0.5, 0.5, 50)
    gx, gy = np.meshgrid(line, line, indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.5)], axis=1)  # 2500 points, 0.5 m in front
    return mics, grid, line


def signals(mics, n_samples: int, seed: int = 11):
    """three white-noise monopoles of distinct power (integer-sample delays, 1/r) plus sensor noise"""
    rng = np.random.default_rng(seed)
    td = rng.standard_normal((n_samples, len(mics))) * 0.05
    for amp, pos in ((1.0, (0.2, -0.1, 0.5)), (0.5, (-0.25, 0.2, 0.5)), (0.25, (0.1, 0.3, 0.5))):
        src = rng.standard_normal(n_samples + 400) * amp
        r = np.linalg.norm(mics - np.array(pos), axis=1)
        for c, (d, rc) in enumerate(zip(np.round(r / SOUND * FS).astype(int), r)):
            td[:, c] += src[400 - d: 400 - d + n_samples] / rc
    return td


class Grid:
    def __init__(self, points, n_line):
        self.points, self.number_of_points, self.shape = points, len(points), (n_line, n_line)

    def reconstruct_map_shape(self, m):
        return np.asarray(m).reshape(self.shape)


class Steering:  # the reference's "Classic" formulation: exp(-j k r) / C ... built in numpy, as the reference does
    def __init__(self, mics):
        self.mics = mics

    def get_vector(self, wave_numbers, grid, mic):
        r = np.linalg.norm(self.mics[:, None, :] - grid.points[None, :, :], axis=2)  # (C, G)
        return np.exp(-1j * wave_numbers[:, None, None] * r[None]) / len(self.mics)


def band_ids(f):
    from dsptoolbox_amd.transfer_functions import find_nearest_points_index_in_vector
    ids = find_nearest_points_index_in_vector(np.array([FC * 2 ** (-1 / FRAC / 2), FC * 2 ** (1 / FRAC / 2)]), f)
    return int(ids[0]), int(ids[1])


def run_gpu(reps: int):
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend, beamforming
    from dsptoolbox_amd._lib import DeviceBuffer, get_context
    ctx = get_context()
    lines = []
    classes = dict(mvdr=beamforming.BeamformerMVDR, functional=beamforming.BeamformerFunctional,
                   orthogonal=beamforming.BeamformerOrthogonal, cleansc=beamforming.BeamformerCleanSC)
    for n_mics in (48, 64):
        mics, grid_pts, line = geometry(n_mics)
        s = dsp.Signal(None, signals(mics, 64 * W // 2 + W // 2), FS)  # 64 frames: a short (float64) estimate
        s.set_spectrum_parameters(window_length_samples=W)
        f, csm = s.get_csm()
        id1, id2 = band_ids(f)
        st, grid = Steering(mics), Grid(grid_pts, len(line))
        h = st.get_vector(f[id1:id2] * 2 * np.pi / SOUND, grid, None)
        cs = np.ascontiguousarray(csm[id1:id2])
        nb, G = id2 - id1, grid.number_of_points
        d_c, d_h = DeviceBuffer.from_array(ctx, cs), DeviceBuffer.from_array(ctx, np.ascontiguousarray(h))
        d_m = DeviceBuffer(ctx, G * nb * 8)
        for method in METHODS:
            def call():
                if method == "cleansc":
                    return ctx.lib.ds_bf_cleansc_dev(ctx.handle, C.c_void_p(d_c.ptr), C.c_void_p(d_h.ptr), nb, n_mics,
                                                     G, 2 * n_mics, 0.5, 0, C.c_void_p(d_m.ptr))
                return ctx.lib.ds_bf_eig_map_dev(ctx.handle, C.c_void_p(d_c.ptr), C.c_void_p(d_h.ptr), nb, n_mics, G,
                                                 backend.BF_METHODS[method], 10.0, n_mics // 2, C.c_void_p(d_m.ptr))
            ctx.check(call(), method)
            ctx.sync()
            dev = []
            for _ in range(reps):
                ctx.timer_start()
                ctx.check(call(), method)
                dev.append(ctx.timer_stop())
            bf = classes[method](s, None, grid, st)
            bf.get_beamformer_map(FC, FRAC)
            wall = []
            for _ in range(max(3, reps // 4)):
                t0 = time.perf_counter()
                bf.get_beamformer_map(FC, FRAC)
                wall.append(time.perf_counter() - t0)
            lines.append(f"{method:10s} C={n_mics} G={G} bins={nb}: device {np.median(dev):8.3f} ms "
                         f"(min {np.min(dev):.3f})   class call {1e3 * np.median(wall):8.1f} ms")
            print(lines[-1], flush=True)
        for d in (d_c, d_h, d_m):
            d.free()
    return lines


def run_fp32_route():
    """the same maps from the fp32-route CSM (256 frames) and from a float64 CSM of the same signals (the CPU oracle)"""
    import dsptoolbox_amd as dsp
    from dsptoolbox_amd import backend
    from oracle import dsp_oracle as orc
    n_mics = 48
    mics, grid_pts, line = geometry(n_mics)
    td = signals(mics, 256 * W // 2 + W // 2, seed=12)
    s = dsp.Signal(None, td, FS)
    s.set_spectrum_parameters(window_length_samples=W)
    f, csm32 = s.get_csm()  # 256 frames: the fp32 kernels
    _, csm64 = orc.csm_welch(td, FS, W, "hann", 50, True, "mean", "FFTBackward")
    id1, id2 = band_ids(f)
    h = Steering(mics).get_vector(f[id1:id2] * 2 * np.pi / SOUND, Grid(grid_pts, len(line)), None)
    a, b = csm32[id1:id2], csm64[id1:id2]
    rel = lambda x, y: float(np.max(np.abs(x - y)) / np.max(np.abs(y)))  # noqa: E731
    lines = [f"fp32-route CSM against float64 (C={n_mics}, 256 frames of {W}, FFTBackward, 1/3 octave at 4 kHz): "
             f"CSM {rel(a, b):.2e}"]
    for method in METHODS:
        if method == "cleansc":
            ma, mb = (backend.beamformer_cleansc_map(x, h, 2 * n_mics, 0.5, False) for x in (a, b))
        else:
            ma, mb = (backend.beamformer_eig_map(x, h, method, 10.0, n_mics // 2) for x in (a, b))
        extra = ""
        if method in ("orthogonal", "cleansc"):
            extra = f", same non-zero points: {np.array_equal(np.flatnonzero(ma), np.flatnonzero(mb))}"
        lines.append(f"  {method:10s} map moves {rel(ma, mb):.2e} (relative max over the band's bins){extra}")
        print(lines[-1], flush=True)
    return lines


def run_reference():
    from oracle.gen_golden import import_reference
    dsp = import_reference()
    import contextlib
    import io
    lines = []
    for n_mics in (48, 64):
        mics, grid_pts, line = geometry(n_mics)
        s = dsp.Signal(None, signals(mics, 64 * W // 2 + W // 2), FS)
        s.set_spectrum_parameters(window_length_samples=W)
        ma = dsp.beamforming.MicArray(dict(x=mics[:, 0], y=mics[:, 1], z=mics[:, 2]))
        g = dsp.beamforming.Regular2DGrid(line, line, ["x", "y"], value3=0.5)
        st = dsp.beamforming.SteeringVector()
        s.get_csm()
        for method, cls in (("mvdr", dsp.beamforming.BeamformerMVDR), ("functional", dsp.beamforming.BeamformerFunctional),
                            ("orthogonal", dsp.beamforming.BeamformerOrthogonal), ("cleansc", dsp.beamforming.BeamformerCleanSC)):
            bf = cls(s, ma, g, st)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                bf.get_beamformer_map(FC, FRAC)
            lines.append(f"{method:10s} C={n_mics} G={g.number_of_points}: reference CPU {time.perf_counter() - t0:8.2f} s")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    lines = run_reference() if a.reference else run_gpu(a.reps) + [""] + run_fp32_route()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
