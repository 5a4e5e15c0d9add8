"""Golden vectors for IIR filtering, made by RUNNING THE REFERENCE (dsptoolbox 0.8: Filter.iir_filter / biquad /
filter_signal, classes/filter.py:91-187 and :648-743; FilterBank.filter_signal, classes/filterbank.py:415-477;
filterbanks.fractional_octave_bands, filterbanks/filterbanks.py:336-413):  python tools/gen_golden_iir.py

Writes tests/golden/iir/cases.npz:
- oct_<b>_<fs>_{sos,nsec,center,lower,upper}: the fractional-octave bank's sections (stacked, identity-padded to
  the longest cascade; nsec the real counts) and band frequencies for b = 1, 3 at 44.1 and 48 kHz;
- biquad_<type>: [b, a] of Filter.biquad(type, 1 kHz, 4.5 dB, Q 0.9, 48 kHz) for every BiquadEqType;
- x (N, 2) float32 samples (stored as float32, filtered as float64) and the reference's outputs:
  sos (4th-order Butterworth band pass), ba (the peaking biquad), zi1 / zi2 (two successive sos calls with
  activate_zi), zp_sos / zp_ba (zero phase), sub (the sos filter on channel 1 only);
  bank_{parallel,summed,sequential} of an octave bank's three bands, mixed_{parallel,summed,sequential} of a
  bank of one IIR and one FIR filter."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "iir", "cases.npz")
FS = 48000
N = 700


def main():
    dsp = import_reference()
    z = {}
    for b in (1, 3):
        for fs in (44100, 48000):
            bank, c, (lo, hi) = dsp.filterbanks.fractional_octave_bands([31.5, 16e3], b, 6, fs)
            n_max = max(len(f.sos) for f in bank.filters)  # (a high pass at the top has fewer sections)
            z[f"oct_{b}_{fs}_sos"] = np.stack([np.concatenate([f.sos, np.tile([1.0, 0, 0, 1.0, 0, 0], (n_max - len(f.sos), 1))])
                                               for f in bank.filters])
            z[f"oct_{b}_{fs}_nsec"] = np.array([len(f.sos) for f in bank.filters])
            z[f"oct_{b}_{fs}_center"], z[f"oct_{b}_{fs}_lower"], z[f"oct_{b}_{fs}_upper"] = c, lo, hi
    for t in dsp.BiquadEqType:
        f = dsp.Filter.biquad(t, 1000.0, 4.5, 0.9, FS)
        z[f"biquad_{t.name}"] = np.stack(f.get_coefficients(dsp.FilterCoefficientsType.Ba)) if f.is_iir else \
            np.stack([np.pad(f.ba[0], (0, 3 - len(f.ba[0]))), np.pad(f.ba[1], (0, 3 - len(f.ba[1])))])
    rng = np.random.default_rng(7)
    x = rng.standard_normal((N, 2)).astype(np.float32).astype(np.float64)
    z["x"] = x.astype(np.float32)
    s = dsp.Signal(None, x, FS)
    f_sos = dsp.Filter.iir_filter(4, [300.0, 3000.0], dsp.FilterPassType.Bandpass, FS)
    f_ba = dsp.Filter.biquad(dsp.BiquadEqType.Peaking, 1000.0, 4.5, 0.9, FS)
    z["sos"] = f_sos.filter_signal(s).time_data
    z["ba"] = f_ba.filter_signal(s).time_data
    fz = f_sos.copy()
    z["zi1"] = fz.filter_signal(s, activate_zi=True).time_data
    z["zi2"] = fz.filter_signal(s, activate_zi=True).time_data
    z["zp_sos"] = f_sos.filter_signal(s, zero_phase=True).time_data
    z["zp_ba"] = f_ba.filter_signal(s, zero_phase=True).time_data
    z["sub"] = f_sos.filter_signal(s, channels=1).time_data
    bank = dsp.filterbanks.fractional_octave_bands([250.0, 1000.0], 1, 6, FS)[0]
    mixed = dsp.FilterBank([f_sos, dsp.Filter.fir_filter(40, 2000.0, dsp.FilterPassType.Lowpass, FS)])
    for name, fb in (("bank", bank), ("mixed", mixed)):
        out = fb.filter_signal(s, dsp.FilterBankMode.Parallel)
        z[f"{name}_parallel"] = np.stack([b_.time_data for b_ in out.bands])
        z[f"{name}_summed"] = fb.filter_signal(s, dsp.FilterBankMode.Summed).time_data
        z[f"{name}_sequential"] = fb.filter_signal(s, dsp.FilterBankMode.Sequential).time_data
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
