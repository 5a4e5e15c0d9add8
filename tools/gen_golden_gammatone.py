"""Golden vectors for the gammatone bank, complex sos filtering and the distance measures, made by RUNNING THE
REFERENCE (dsptoolbox 0.8: filterbanks.auditory_filters_gammatone, filterbanks/filterbanks.py:217-303;
Filter.filter_signal / FilterBank.filter_signal with complex sos, classes/filter_helpers.py:207-285;
distances.*, distances/distances.py):  python tools/gen_golden_gammatone.py

Writes tests/golden/gammatone/cases.npz:
- bank<i>_{args,freq,coef,norm}: frequency range, resolution and sampling rate of bank i and its _frequencies,
  _coefficients, _normalizations, for ([100, 3500], 1, 8000), ([50, 7000], 1, 16000), ([20, 20000], 1, 48000) and
  ([100, 3500], 0.5, 8000);
- x (700, 3) float32 samples at 8 kHz (stored as float32, filtered as float64) and the reference's outputs, complex128:
  par (bands, 700, 2): the bank of [700, 1500] Hz on channels 0, 1, Parallel; zi1 / zi2: two successive activate_zi
  calls of the bank of [900, 1100] Hz on the same channels; single: the bank's first filter alone; sub: that filter on
  channel 1 only (all three channels returned);
- xhat (700, 3) float32 and the reference's value of every distance function: <name>_33 for x against xhat channel
  by channel, <name>_13 for one channel against three (snr: three against one); log_spectral / itakura_saito on
  [100, 3500] Hz with Welch windows of 256 samples, _33 energy-normalised and _raw not (the whole band down to 0 Hz is
  not stored: after the detrend its first bin is rounding noise in the reference too)."""

import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gammatone", "cases.npz")
FS = 8000
N = 700
BANKS = (([100, 3500], 1, 8000), ([50, 7000], 1, 16000), ([20, 20000], 1, 48000), ([100, 3500], 0.5, 8000))
SPECTRUM = dict(window_length_samples=256)


def complex_data(sig):
    return sig.time_data + 1j * sig.time_data_imaginary


def main():
    warnings.simplefilter("ignore")
    dsp = import_reference()
    z = {}
    for i, (f_range, res, fs) in enumerate(BANKS):
        fb = dsp.filterbanks.auditory_filters_gammatone(f_range, res, fs)
        z[f"bank{i}_args"] = np.array([f_range[0], f_range[1], res, fs], dtype=np.float64)
        z[f"bank{i}_freq"], z[f"bank{i}_coef"], z[f"bank{i}_norm"] = fb._frequencies, fb._coefficients, fb._normalizations
    rng = np.random.default_rng(11)
    t = np.arange(N) / FS
    chirp = np.sin(2 * np.pi * (200 * t + 0.5 * 3000 / t[-1] * t ** 2))
    x = np.stack([chirp + 0.1 * rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(N)], axis=1)
    x = x.astype(np.float32).astype(np.float64)
    xhat = (x + 0.3 * rng.standard_normal((N, 3))).astype(np.float32).astype(np.float64)
    z["x"], z["xhat"] = x.astype(np.float32), xhat.astype(np.float32)
    s2 = dsp.Signal(None, x[:, :2], FS, constrain_amplitude=False)
    s3 = dsp.Signal(None, x, FS, constrain_amplitude=False)
    out = dsp.filterbanks.auditory_filters_gammatone([700, 1500], 1, FS).filter_signal(s2, dsp.FilterBankMode.Parallel)
    z["par"] = np.stack([complex_data(b) for b in out.bands])
    fb = dsp.filterbanks.auditory_filters_gammatone([900, 1100], 1, FS)
    for name in ("zi1", "zi2"):
        out = fb.filter_signal(s2, dsp.FilterBankMode.Parallel, activate_zi=True)
        z[name] = np.stack([complex_data(b) for b in out.bands])
    f0 = dsp.filterbanks.auditory_filters_gammatone([900, 1100], 1, FS).filters[0]
    z["single"] = complex_data(f0.filter_signal(s2))
    z["sub"] = complex_data(f0.filter_signal(s3, channels=1))
    h3 = dsp.Signal(None, xhat, FS, constrain_amplitude=False)
    x1 = dsp.Signal(None, x[:, :1], FS, constrain_amplitude=False)
    h1 = dsp.Signal(None, xhat[:, :1], FS, constrain_amplitude=False)
    d = dsp.distances
    z["snr_33"], z["snr_13"] = d.snr(s3, h3), d.snr(s3, h1)
    z["si_sdr_33"], z["si_sdr_13"] = d.si_sdr(s3, h3), d.si_sdr(x1, h3)
    z["fw_snr_seg_33"] = d.fw_snr_seg(s3, h3, f_range_hz=[100, 3500])
    z["fw_snr_seg_13"] = d.fw_snr_seg(x1, h3, f_range_hz=[100, 3500])
    for name, fn in (("log_spectral", d.log_spectral), ("itakura_saito", d.itakura_saito)):
        z[f"{name}_33"] = fn(s3.copy(), h3.copy(), f_range_hz=[100, 3500], spectrum_parameters=SPECTRUM)
        z[f"{name}_raw"] = fn(s3.copy(), h3.copy(), f_range_hz=[100, 3500], energy_normalization=False,
                              spectrum_parameters=SPECTRUM)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes,", len(z), "arrays")
    for k in sorted(z):
        if z[k].size <= 3:
            print(k, z[k])


if __name__ == "__main__":
    main()
