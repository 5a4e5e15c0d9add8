"""Golden vectors for fractional delays and the time-domain delay-and-sum beamformer, made by RUNNING THE REFERENCE
(dsptoolbox 0.8: standard.fractional_delay, standard/latency_delay.py:159-285; beamforming.MonopoleSource,
mix_sources_on_array and BeamformerDASTime, beamforming/beamforming.py:1317-1512):  python tools/gen_golden_delay.py

Writes
- tests/golden/delay/cases.npz: input signals (float32 values, (samples, channels)) and, per case
  `fd_<i>`, the reference's fractional_delay output (float64) with its arguments in `fd_<i>_args`
  (delay_seconds, fs, order, keep_length, input name, channel subset or -1 for all, constrained 0/1);
  `mb_*` a MultiBandSignal of two bands.
- tests/golden/beamformers/das_time.npz: microphone / grid / source distances as the reference computed them
  (the tests hand them back through a stand-in geometry object), the array signals of one source and of two
  sources of unequal length (mix_sources_on_array), and BeamformerDASTime's output on a small 2-D grid, plain and
  for a constrained signal whose grid channels peak above 1."""

import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT_DELAY = os.path.join(ROOT, "tests", "golden", "delay", "cases.npz")
OUT_BF = os.path.join(ROOT, "tests", "golden", "beamformers", "das_time.npz")


def main():
    dsp = import_reference()
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20261015)
    z = {}
    # inputs: three channels of noise; a "hot" one whose half-sample delay overshoots (a tone at fs / 4)
    z["x_noise"] = (0.5 * rng.standard_normal((400, 3))).astype(np.float32)
    hot = np.tile([1.0, 1.0, -1.0, -1.0], 100)[:, None] * np.array([[1.0, 0.6]]) + 0.05 * rng.standard_normal((400, 2))
    z["x_hot"] = (3.0 * hot).astype(np.float32)
    fs = 1024
    delays = [10 / fs, 10.25 / fs, 10.5 / fs, 10.75 / fs, (10 - 1e-12) / fs, 0.0, 3.3 / fs, 0.4 / fs]
    cases = []
    for d in delays:
        for order in (30, 31, 8):
            cases.append((d, fs, order, False, "x_noise", -1, 0))
    cases += [(10.25 / fs, fs, 30, True, "x_noise", -1, 0), (10.75 / fs, fs, 31, True, "x_noise", -1, 0),
              (0.3 / fs, fs, 8, True, "x_noise", -1, 0), (10.5 / fs, fs, 30, False, "x_noise", 1, 0),
              (2.6 / fs, fs, 31, True, "x_noise", 2, 0), (0.0001875, 48000, 30, False, "x_noise", -1, 0),
              (10.5 / fs, fs, 30, False, "x_hot", -1, 1), (7.5 / fs, fs, 8, True, "x_hot", 0, 1)]
    for i, (d, fsi, order, keep, name, ch, constrained) in enumerate(cases):
        s = dsp.Signal(None, z[name].astype(np.float64), fsi, constrain_amplitude=bool(constrained))
        out = dsp.standard.fractional_delay(s, d, channels=None if ch < 0 else ch, keep_length=keep, order=order)
        z[f"fd_{i}"] = out.time_data
        z[f"fd_{i}_args"] = np.array([d, fsi, order, keep, ["x_noise", "x_hot"].index(name), ch, constrained],
                                     dtype=np.float64)
    bands = [dsp.Signal(None, z["x_noise"][:, :2].astype(np.float64), fs),
             dsp.Signal(None, 0.5 * z["x_noise"][:, 1:].astype(np.float64), fs)]
    mb = dsp.MultiBandSignal(bands)
    out = dsp.standard.fractional_delay(mb, 5.6 / fs, order=30)
    z["mb_0"], z["mb_1"] = out.bands[0].time_data, out.bands[1].time_data
    os.makedirs(os.path.dirname(OUT_DELAY), exist_ok=True)
    np.savez_compressed(OUT_DELAY, **z)

    # ---- array signals and the time-domain beamformer ----
    b = {}
    fs = 8000
    mic_xyz = np.stack([rng.uniform(-0.4, 0.4, 8), rng.uniform(-0.4, 0.4, 8), np.zeros(8)])
    mics = dsp.beamforming.MicArray(dict(x=mic_xyz[0], y=mic_xyz[1], z=mic_xyz[2]))
    gx, gy = np.meshgrid(np.linspace(-1, 1, 4), np.linspace(-0.5, 0.5, 3))
    grid = dsp.beamforming.Grid(dict(x=gx.ravel(), y=gy.ravel(), z=np.full(gx.size, 1.5)))
    s1 = (0.8 * rng.standard_normal(700)).astype(np.float32)
    s2 = (0.8 * rng.standard_normal(600)).astype(np.float32)
    p1, p2 = np.array([0.3, -0.2, 1.2]), np.array([-0.5, 0.4, 2.0])
    b["s1"], b["s2"], b["fs"] = s1, s2, np.array(fs)
    b["d_src1"] = mics.get_distances_to_point(p1)
    b["d_src2"] = mics.get_distances_to_point(p2)
    src1 = dsp.beamforming.MonopoleSource(dsp.Signal(None, s1.astype(np.float64), fs), p1)
    b["one_source"] = src1.get_signals_on_array(mics).time_data
    srcs = [dsp.beamforming.MonopoleSource(dsp.Signal(None, s1.astype(np.float64), fs), p1),
            dsp.beamforming.MonopoleSource(dsp.Signal(None, s2.astype(np.float64), fs), p2)]
    b["two_sources"] = dsp.beamforming.mix_sources_on_array(srcs, mics).time_data
    srcs = [dsp.beamforming.MonopoleSource(dsp.Signal(None, s2.astype(np.float64), fs), p2),
            dsp.beamforming.MonopoleSource(dsp.Signal(None, s1.astype(np.float64), fs), p1)]
    b["two_sources_short_first"] = dsp.beamforming.mix_sources_on_array(srcs, mics).time_data
    arr = b["two_sources"].astype(np.float32)
    b["array_signal"] = arr
    b["d_grid"] = mics.get_distances_to_point(grid.coordinates)
    for constrained in (False, True):
        x = arr.astype(np.float64) * (4.0 if constrained else 1.0)
        sig = dsp.Signal(None, x, fs, constrain_amplitude=constrained)
        bf = dsp.beamforming.BeamformerDASTime(sig, mics, grid)
        with contextlib.redirect_stdout(io.StringIO()):
            out = bf.get_beamformer_output()
        b["das_time_constrained" if constrained else "das_time"] = out.time_data
    os.makedirs(os.path.dirname(OUT_BF), exist_ok=True)
    np.savez_compressed(OUT_BF, **b)
    for p in (OUT_DELAY, OUT_BF):
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
