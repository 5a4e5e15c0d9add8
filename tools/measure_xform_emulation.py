"""Prints EMULATION of tests/xform_cases.py: the worst error of the float32 emulations of the whole-signal transforms
(scipy in single precision; for Bluestein lengths also the float32 chirp-z restatement) against the float64 oracle, per
(family, length), as a multiple of 1e-6 * the row's rms.  CPU only, no device.  tests/test_xform_sweep_host.py measures
every entry again on every run.

    python tools/measure_xform_emulation.py [length ...]
"""

import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import xform_cases as xc  # noqa: E402


def main():
    lengths = [int(a) for a in sys.argv[1:]]
    table = {}
    for family, cases in (("rfft", xc.FOUR + tuple(xc.BLUE)), ("deconv", xc.FOUR + xc.BLUE_DECONV)):
        for n_fft in cases:
            if lengths and n_fft not in lengths:
                continue
            t0 = time.time()
            fr = xc.emulation_fractions(family, n_fft)
            table[(family, n_fft)] = max(fr.values())
            print(f"# {family} {n_fft}: " + ", ".join(f"{k} {v:.3g}" for k, v in fr.items()) + f" ({time.time() - t0:.1f} s)",
                  flush=True)
    print("EMULATION = {")
    for family in ("rfft", "deconv"):
        row = [f"({family!r}, {n}): {float(f'{v:.3g}')}," for (f, n), v in table.items() if f == family]
        for i in range(0, len(row), 4):
            print("    " + " ".join(row[i:i + 4]))
    print("}")


if __name__ == "__main__":
    main()
