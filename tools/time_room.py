"""Dev tool: wall time of the shoebox room calls on the device (upload, kernels, download), and the device time of
their kernels: the default 5 x 4 x 3 m / T60 0.5 s / 48 kHz response; 10 x 8 x 4 m / T60 2 s / 2 s of output; the same room
with 8 absorption bands; the modal sum at max_mode_order 40 on 24000 frequencies.   python tools/time_room.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsptoolbox_amd import backend  # noqa: E402
from dsptoolbox_amd._lib import get_context  # noqa: E402
from dsptoolbox_amd.room_acoustics import ShoeboxRoom  # noqa: E402

ctx = get_context()


def timed(label, call, work, unit, repeats=3):
    call()  # sizes the workspaces
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(repeats):
        call()
    ctx.sync()
    ms = (time.perf_counter() - t0) / repeats * 1e3
    ctx.profile_enable(True)
    call()
    ctx.sync()
    print(f"{label}: {ms:9.2f} ms per call, {work:.3g} {unit}, {work / ms / 1e6:.3g} G{unit}/s", flush=True)
    print("   kernels (ms, one call):", ctx.profile_report(), flush=True)
    ctx.profile_enable(False)


def ism(dim, t60, sr, seconds, n_band):
    room = ShoeboxRoom(dim, t60_s=t60)
    alphas = np.linspace(0.6, 1.4, n_band)[:, None] * room.absorption_coefficient * np.ones((1, 6))
    limit = backend.ism_limit(room.dimensions_m, room.t60_s, None)
    sources = 8 * (2 * limit + 1) ** 3
    timed(f"image sources {dim} T60 {t60} s, {sr} Hz, {seconds} s, {n_band} band(s), LIMIT {limit}",
          lambda: backend.image_source_rir(room.dimensions_m, alphas, [1.1, 2.3, 1.2], [3.7, 0.9, 1.6], room.t60_s, None, sr,
                                           int(seconds * sr)), sources, "sources")


ism((5, 4, 3), 0.5, 48000, 0.5, 1)
ism((10, 8, 4), 2.0, 48000, 2.0, 1)
ism((10, 8, 4), 2.0, 48000, 2.0, 8)
room = ShoeboxRoom((5, 4, 3), t60_s=0.5)
freqs = np.linspace(1.0, 2000.0, 24000)
timed("modal sum, max_mode_order 40, 24000 frequencies",
      lambda: room.get_analytical_transfer_function([1.1, 2.3, 1.2], [3.7, 0.9, 1.6], freqs, max_mode_order=40,
                                                    generate_plot=False), (41 ** 3 - 1) * 24000, "terms")
