"""The conditioning sweep behind the carry-gain limit MAX_GAIN_COMPANION (csrc/kernels_rtfilt.hpp):
    python tools/sweep_rtfilt_gain.py [designs per family [family]]
The table of DESIGN section 26 is `... 400`.

Butterworth and elliptic designs of orders 2 .. 16 at random cutoffs, as scipy.signal.tf2ss's controller-canonical
state-space system (StateSpaceFilter.from_filter) and as the transposed direct form II of the same b / a (IIRFilter), run
on the CPU through the float64 emulation of the blocked algorithm (tests/rtfilt_oracle.blocked_f64) and through the
long-double serial recursion, over 4160 samples of noise (two groups and a partial one, so the carry over groups is
crossed twice).  For every design it takes the carry gain -- the largest magnitude in Phi = A^32 and Phi^64 -- and the
emulation's worst error relative to the output's peak, and prints the worst error per decade of gain and the smallest
gain at which a design misses 1e-6 / 4.4 of the peak (the project's 1e-6 contract after the GPU tests' margin of 4 x 1.1),
as tools/sweep_sfilt_gain.py does for the structure filters."""

import os
import sys

import numpy as np
from scipy import signal as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtfilt_oracle as ro  # noqa: E402

N = 4160
TARGET = 1e-6 / 4.4


def _design(rng):
    order = int(rng.integers(2, 17))
    wn = float(10 ** rng.uniform(np.log10(0.002), np.log10(0.9)))
    if rng.integers(2):
        b, a = sg.butter(order, wn)
        what = f"butter order {order} wn {wn:.4f}"
    else:
        b, a = sg.ellip(order, 1.0, 60.0, wn)
        what = f"ellip order {order} wn {wn:.4f}"
    return b / a[0], a / a[0], what


def state_space(rng):
    b, a, what = _design(rng)
    A, B, C, D = sg.tf2ss(b, a)
    return dict(kind="state_space", A=A, B=B[:, 0], C=C[0], Dd=float(D[0, 0])), what


def tdf2(rng):
    b, a, what = _design(rng)
    return dict(kind="tdf2", b=b, a=a), what


FAMILIES = (("state_space", state_space), ("tdf2", tdf2))


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    only = sys.argv[2] if len(sys.argv) > 2 else None
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((N, 1))
    rows = []
    for family, make in FAMILIES:
        if only not in (None, family):
            continue
        done = 0
        while done < count:
            s, what = make(rng)
            if not np.all(np.abs(np.roots(s["a"] if family == "tdf2" else np.poly(s["A"]))) < 1):
                continue
            gain = ro.carry_gain(s)
            if not np.isfinite(gain) or gain > 1e9:
                continue
            done += 1
            with np.errstate(all="ignore"):
                y_ref, _ = ro.serial(s, x)
                y, _ = ro.blocked_f64(s, x)
            err = ro.stream_error(y, y_ref) if np.all(np.isfinite(y)) else np.inf
            rows.append((family, gain, err, what))
            print(f"{family:12s} gain {gain:10.3g} error {err:9.2e}  {what}", flush=True)
    print("\nfamily        gain decade      designs  worst error   within target")
    for family, _ in FAMILIES:
        for lo in range(-1, 9):
            sel = [r for r in rows if r[0] == family and 10.0 ** lo <= r[1] < 10.0 ** (lo + 1)]
            if sel:
                worst = max(r[2] for r in sel)
                print(f"{family:12s}  1e{lo:+d} .. 1e{lo + 1:+d}   {len(sel):5d}   {worst:10.2e}   {worst <= TARGET}")
        sel = [r for r in rows if r[0] == family and r[1] < 0.1]
        if sel:
            print(f"{family:12s}  below 0.1        {len(sel):5d}   {max(r[2] for r in sel):10.2e}   True")
        missed = sorted(r[1] for r in rows if r[0] == family and not r[2] <= TARGET)
        if missed:
            below = [r for r in rows if r[0] == family and r[1] < missed[0]]
            print(f"{family:12s}  smallest gain that misses the target: {missed[0]:.3g}; {len(below)} designs below it, "
                  f"worst error {max(r[2] for r in below) if below else 0.0:.2e}")


if __name__ == "__main__":
    main()
