"""Golden vectors for the continuous wavelet transform, made by RUNNING THE REFERENCE (dsptoolbox 0.8:
transforms.cwt, transforms/transforms.py:687-760; MorletWavelet and _squeeze_scalogram, transforms/_transforms.py:
29-301):  python tools/gen_golden_cwt.py

Writes tests/golden/cwt/cases.npz:
- `x`: the input signal (500 samples x 2 channels at 8000 Hz, float32 values held as float64);
- `wv_<i>`: MorletWavelet(...).get_wavelet(f, fs) with its arguments in `wv_<i>_args`
  (b or nan, h or nan, scale, precision_bounds, step, interpolation 0/1, f, fs);
- `cwt_<i>`: the reference's cwt(...) with `cwt_<i>_freqs`, `cwt_<i>_args` (h, step, channel or -1 for all,
  synchrosqueezed 0/1, normalisation 0/1)."""

import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cwt", "cases.npz")
FS = 8000


def main():
    dsp = import_reference()
    from dsptoolbox.transforms import _transforms as rt
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20261016)
    z = {}
    n = np.arange(500)
    x = np.stack([0.6 * np.sin(2 * np.pi * 440 * n / FS) + 0.1 * rng.standard_normal(500),
                  0.5 * rng.standard_normal(500)], axis=1).astype(np.float32).astype(np.float64)
    z["x"] = x
    wv_cases = [(np.nan, 3.0, 1.0, 1e-5, 1e-3, 1, 100.0, 48000), (np.nan, 3.0, 1.0, 1e-5, 5e-3, 0, 1000.0, 8000),
                (1.5, np.nan, 1.0, 1e-5, 5e-3, 1, 333.0, 8000), (1.5, np.nan, 1.0, 1e-4, 2e-3, 0, 50.0, 8000),
                (np.nan, 2.0, 2.0, 1e-5, 5e-3, 1, 700.0, 8000), (0.8, np.nan, 0.5, 1e-6, 1e-2, 0, 2500.0, 16000),
                (np.nan, 4.0, 1.0, 1e-5, 1e-3, 1, 3999.0, 8000)]
    for i, (b, h, scale, pb, step, interp, f, fs) in enumerate(wv_cases):
        w = rt.MorletWavelet(b=None if np.isnan(b) else b, h=None if np.isnan(h) else h, scale=scale,
                             precision_bounds=pb, step=step, interpolation=bool(interp))
        z[f"wv_{i}"] = np.asarray(w.get_wavelet(f, fs))
        z[f"wv_{i}_args"] = np.array([b, h, scale, pb, step, interp, f, fs], dtype=np.float64)
    sig = dsp.Signal(None, x, FS)
    cwt_cases = [
        ([100.0, 250.0, 440.0, 1000.0, 2000.0, 3500.0], 3.0, 5e-3, -1, 0, 0),   # sorted
        ([1000.0, 60.0, 440.0, 3000.0, 150.0], 3.0, 5e-3, -1, 0, 0),             # unsorted, long wavelets (60 Hz: L > N)
        ([440.0, 440.0, 300.0, 1200.0, 300.0], 2.0, 2e-3, 1, 0, 0),              # repeated, channel subset
        ([20.0, 35.0, 3900.0], 3.0, 1e-2, -1, 0, 0),                             # wavelets much longer than the signal
        ([200.0, 300.0, 400.0, 440.0, 480.0, 600.0, 900.0, 1500.0], 3.0, 5e-3, -1, 1, 0),
        ([1500.0, 440.0, 450.0, 430.0, 440.0, 200.0, 3000.0], 3.0, 5e-3, -1, 1, 1),
        ([300.0, 400.0, 440.0, 500.0, 800.0], 6.0, 5e-3, 0, 1, 1),
    ]
    for i, (freqs, h, step, ch, sq, norm) in enumerate(cwt_cases):
        fr = np.array(freqs)
        w = rt.MorletWavelet(h=h, step=step)
        out = dsp.transforms.cwt(sig, fr, w, channel=None if ch < 0 else ch, synchrosqueezed=bool(sq),
                                 apply_synchrosqueezed_normalization=bool(norm))
        z[f"cwt_{i}"] = out
        z[f"cwt_{i}_freqs"] = fr
        z[f"cwt_{i}_args"] = np.array([h, step, ch, sq, norm], dtype=np.float64)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
