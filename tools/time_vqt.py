"""Dev tool: transforms.vqt at the defaults (48 kHz, octaves 1 to 5, 24 bins: d = 22, 120 rows).
  - 2 channels x 2^20 samples, the result left on the device (4 GB of complex128): ms per call, ms per kernel, and the
    last interpolation stage's store bandwidth beside the copy ceiling measured in the same process (ds_measure_copy
    counts bytes read + written);
  - 2 channels x 2^16 samples through the host-returning path (252 MB downloaded);
  - with --reference, instead of the above: the reference's time for the 2^16 case on the CPU (needs the reference
    package on the path; no device is touched).
    python tools/time_vqt.py [--reference]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 48000


def signal(n):
    return np.random.default_rng(0).standard_normal((n, 2))


if "--reference" in sys.argv:
    from oracle.gen_golden import import_reference
    ref = import_reference()
    x = signal(1 << 16)
    t0 = time.perf_counter()
    ref.transforms.vqt(ref.Signal(None, x, FS, constrain_amplitude=False))
    print(f"reference, 2 x 2^16 on the CPU: {time.perf_counter() - t0:.2f} s")
    sys.exit(0)

import dsptoolbox_amd as dsp  # noqa: E402
from dsptoolbox_amd import transforms  # noqa: E402
from dsptoolbox_amd._lib import get_context  # noqa: E402

ctx = get_context()
gbs = C.c_double()
ctx.check(ctx.lib.ds_measure_copy(ctx.handle, 1 << 30, 10, C.byref(gbs)), "ds_measure_copy")
print(f"copy ceiling: {gbs.value / 1e3:.2f} TB/s read + written")

n = 1 << 20
s = dsp.Signal(None, signal(n), FS).to_device()
for _ in range(2):
    scal = transforms.vqt(s, on_device=True)[1]
    del scal
K = 5
t0 = time.perf_counter()
for _ in range(K):
    scal = transforms.vqt(s, on_device=True)[1]
    del scal
ms = (time.perf_counter() - t0) / K * 1e3
out_bytes = 16 * 120 * n * 2
print(f"2 x 2^20 resident, result on the device ({out_bytes / 1e9:.2f} GB): {ms:.2f} ms per call")
ctx.profile_enable(True)
for _ in range(K):
    scal = transforms.vqt(s, on_device=True)[1]
    del scal
ctx.sync()
rep = ctx.profile_report()
ctx.profile_enable(False)
for name, (total, count) in sorted(rep.items()):
    print(f"   {name:20s} {total / K:8.3f} ms per call ({count // K} launches)")
last = rep["vqt_interp"][0] / K
print(f"   last stage: {out_bytes / last / 1e9:.2f} TB/s stored, {out_bytes / last / 1e9 / (gbs.value / 1e3) * 100:.0f} % of the "
      f"bytes per second the copy kernel moves")

x = signal(1 << 16)
sig = dsp.Signal(None, x, FS)
transforms.vqt(sig)
t0 = time.perf_counter()
for _ in range(3):
    transforms.vqt(sig)
print(f"2 x 2^16 from and to the host ({16 * 120 * 2 * (1 << 16) / 1e6:.0f} MB): {(time.perf_counter() - t0) / 3 * 1e3:.1f} ms per call")
