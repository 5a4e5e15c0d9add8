"""Prints FFT64_EMULATION of tests/fft64_cases.py: the worst error of the float64 emulation of the device's any-length
transform against the long-double oracle, per (route, points of the power-of-two transform), as a multiple of
eps64 * the column rms.  CPU only, no device.  tests/test_fft64_host.py measures the entries up to 2^18 points again on
every run; the larger ones (a Bluestein length on M = 2^22 takes about half a minute per call) are measured here.

    python tools/measure_fft64_emulation.py [--jobs 4] [ident ...]
"""

import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import fft64_cases as fc  # noqa: E402


def one(ident):
    t0 = time.time()
    c = fc.case(ident)
    return ident, c["key"], fc.emulation_fraction(c), time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("idents", nargs="*")
    args = ap.parse_args()
    idents = args.idents or sorted(fc.IDENTS, key=lambda i: -fc.case(i)["key"][1])  # the long ones first
    worst = {}
    with ProcessPoolExecutor(args.jobs) as pool:
        for ident, key, frac, dt in pool.map(one, idents):
            print(f"# {ident}: {frac:.3g} eps of the column rms ({dt:.1f} s)", flush=True)
            worst[key] = max(worst.get(key, 0.0), frac)
    order = {"lds": 0, "four": 1, "blue": 2, "hilbert": 3}
    print("FFT64_EMULATION = {")
    for route in sorted({k[0] for k in worst}, key=order.get):
        print("    " + " ".join(f"({route!r}, {m}): {float(f'{v:.3g}')}," for (r, m), v in sorted(worst.items()) if r == route))
    print("}")
    cap = max(worst.values()) * 4 * fc.HOST_MARGIN * fc.EPS
    print(f"# the largest bound: {cap:.3g} of the column rms (cap {fc.CAP:g})")


if __name__ == "__main__":
    main()
