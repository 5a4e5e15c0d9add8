"""Golden vectors for the direct sums, made by RUNNING THE REFERENCE (dsptoolbox 0.8: transforms.dft,
transforms/transforms.py:1286-1327; transfer_functions.window_frequency_dependent, transfer_functions.py:1288-1377;
transfer_functions.complex_smoothing, :1788-1876 -- their sequential backends, numba is not installed):
    python tools/gen_golden_direct.py

Writes tests/golden/direct/cases.npz.  `meta` is a JSON string with three lists:
- `dft`: signal `<sig>` (float32 values; "sig65536" is not stored: `long_signal()` below rebuilds it from its seed and
  the fixture holds `sig65536_probe`, its first 16 samples and its sum, to prove the rebuild), frequencies `dft_freqs`,
  output `dft_<i>_out`.
- `fdw`: impulse response `<sig>`, `cycles`, `end_db`, output `fdw_<i>_out` (the spectral data with its zero DC row).
- `smooth`: impulse response `<sig>`, `fraction`, `domain`, `window`, output `smooth_<i>_out`; the float64 spectrum
  and frequency vector that the reference's get_spectrum returned are `<sig>_spectrum` and `<sig>_freqs`.

All signals are rounded to float32.  The smoothing signals are a unit impulse at sample 3 or 5 plus Gaussian noise of
0.02 rms under an exp(-n / 200) envelope; for each this script ASSERTS that every bin-to-bin phase step of its float64
spectrum is below pi - 0.5 and that the smallest bin magnitude is above 0.2 of the largest: an fp32 spectrum then
unwraps as the float64 one does and angle() of a near-zero value decides nothing."""

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "direct", "cases.npz")
FS = 48000
LONG_SEED = 65536


def noise_under_envelope(rng, n, n_ch, decay):
    x = rng.standard_normal((n, n_ch)) * np.exp(-np.arange(n) / decay)[:, None]
    return x.astype(np.float32).astype(np.float64)


def long_signal():
    """The 65536 x 1 signal of the dft cases: seeded, so the fixture need not carry its 512 KB."""
    return noise_under_envelope(np.random.default_rng(LONG_SEED), 65536, 1, 9000.0)


def main():
    dsp = import_reference()
    from dsptoolbox.standard.enums import Window
    from dsptoolbox.transfer_functions import SmoothingDomain
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20261018)
    z, meta = {}, {"dft": [], "fdw": [], "smooth": []}

    # ---- dft
    z["sig1000x2"] = noise_under_envelope(rng, 1000, 2, 300.0)
    z["sig4097x3"] = noise_under_envelope(rng, 4097, 3, 900.0)
    long = long_signal()
    z["sig65536_probe"] = np.concatenate([long[:16, 0], [long.sum()]])
    z["dft_freqs"] = np.concatenate([np.geomspace(0.5, 23999.0, 40), [0.0, FS / 2, 1234.5678, -440.0, 30000.0]])
    for name, x in (("sig1000x2", z["sig1000x2"]), ("sig4097x3", z["sig4097x3"]), ("sig65536", long)):
        i = len(meta["dft"])
        z[f"dft_{i}_out"] = dsp.transforms.dft(dsp.Signal(None, x.copy(), FS, constrain_amplitude=False),
                                               z["dft_freqs"].copy())
        meta["dft"].append({"sig": name})

    # ---- window_frequency_dependent: peaks at sample 0 and near the end, and far apart
    def make_ir(n, peaks):
        idx = np.arange(n)
        cols = [0.05 * rng.standard_normal(n) * np.exp(-np.abs(idx - p) / 150.0) for p in peaks]
        x = np.stack(cols, axis=1)
        x[peaks, np.arange(len(peaks))] = 1.0
        return x.astype(np.float32).astype(np.float64)

    z["ir1000"] = make_ir(1000, (0, 990))
    z["ir4097"] = make_ir(4097, (100, 2500))
    fdw = [("ir1000", c, db) for c in (1, 5, 20) for db in (-50.0, -20.0)] + [("ir4097", 5, -50.0)]
    for name, cycles, db in fdw:
        i = len(meta["fdw"])
        ir = dsp.ImpulseResponse(None, z[name].copy(), FS, constrain_amplitude=False)
        sp = dsp.transfer_functions.window_frequency_dependent(ir, cycles, db)
        assert np.array_equal(sp.frequency_vector_hz, np.fft.rfftfreq(len(z[name]), 1 / FS))
        z[f"fdw_{i}_out"] = sp.spectral_data
        meta["fdw"].append({"sig": name, "cycles": cycles, "end_db": db})

    # ---- complex_smoothing
    def make_signal(n, delays):
        cols = []
        for d in delays:
            x = 0.02 * rng.standard_normal(n) * np.exp(-np.arange(n) / 200.0)
            x[d] += 1.0
            cols.append(x)
        return np.stack(cols, axis=1).astype(np.float32).astype(np.float64)

    for name, n, delays in (("sm1000", 1000, (3, 5)), ("sm4097", 4097, (5, 3))):
        z[name] = make_signal(n, delays)
        f, sp = dsp.ImpulseResponse(None, z[name].copy(), FS, constrain_amplitude=False).get_spectrum()
        step = np.abs(np.diff(np.unwrap(np.angle(sp), axis=0), axis=0)).max()
        ratio = (np.abs(sp).min(axis=0) / np.abs(sp).max(axis=0)).min()
        print(f"{name}: {len(f)} bins, largest phase step {step:.3f} rad, min/max magnitude {ratio:.3f}")
        assert step < np.pi - 0.5, step
        assert ratio > 0.2, ratio
        z[f"{name}_spectrum"], z[f"{name}_freqs"] = sp, f
    fractions = (1, 3, 12, 0.5)
    cases = []
    for d, dom in enumerate(SmoothingDomain):  # every domain with two fractions, Hann and Hamming
        cases.append(("sm1000", fractions[d % 4], dom, "Hann"))
        cases.append(("sm1000", fractions[(d + 2) % 4], dom, "Hamming"))
    cases.append(("sm4097", 0.5, SmoothingDomain.RealImaginary, "Hann"))
    cases.append(("sm4097", 3, SmoothingDomain.MagnitudePhase, "Hamming"))
    for name, fraction, dom, window in cases:
        i = len(meta["smooth"])
        ir = dsp.ImpulseResponse(None, z[name].copy(), FS, constrain_amplitude=False)
        sp = dsp.transfer_functions.complex_smoothing(ir, fraction, dom, Window[window])
        assert np.array_equal(sp.frequency_vector_hz, z[f"{name}_freqs"])
        z[f"smooth_{i}_out"] = sp.spectral_data
        meta["smooth"].append({"sig": name, "fraction": fraction, "domain": dom.name, "window": window})

    for key in [k for k in z if k.startswith(("sig", "ir", "sm")) and z[k].dtype == np.float64 and z[k].ndim == 2]:
        assert np.array_equal(z[key], z[key].astype(np.float32))
        z[key] = z[key].astype(np.float32)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **z)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
