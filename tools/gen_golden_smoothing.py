"""Golden vectors for fractional-octave smoothing, made by RUNNING THE REFERENCE (dsptoolbox 0.8:
_fractional_octave_smoothing, helpers/smoothing.py:9-129; Signal.get_spectrum, classes/signal.py:861-946;
spectral_deconvolve; Spectrum.apply_octave_smoothing, classes/spectrum.py:805-869):
    python tools/gen_golden_smoothing.py

Writes tests/golden/smoothing/cases.npz.  `meta` is a JSON string with three lists:
- `fos`: calls of _fractional_octave_smoothing.  Case i has its input in `<in>` (shared between cases), its output in
  `fos_<i>_out`, and `spacing` (null: linear bins), `fractions`, `window` (a scipy name, ["gaussian", alpha] or
  null with the vector in `fos_<i>_wvec`), `clip`.
- `spec`: Signal.get_spectrum with the FFT method: time data `<sig>` at 48 kHz, `pad`, `scaling`, `smoothing`,
  output `spec_<i>_out`.
- `deconv`, `spectrum`: spectral_deconvolve with a smoothed input and Spectrum.apply_octave_smoothing.

The signals are a unit impulse at sample 3 or 5 plus Gaussian noise of 0.02 rms under an exp(-n / 200) envelope,
rounded to float32.  For each of them this script ASSERTS that every bin-to-bin phase step of the float64 spectrum is
below pi - 0.5 and that the smallest bin magnitude is above 0.2 of the largest: an fp32 spectrum then unwraps as the
float64 one does, and a comparison of smoothed spectra measures the smoothing."""

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smoothing", "cases.npz")
FS = 48000


def shaped(n, rng):
    """Plateaus, sign changes and exact zeros between knots: every PCHIP derivative branch."""
    v = rng.standard_normal((n, 2))
    v[n // 5:n // 5 + 4] = v[n // 5]            # plateau (zero slopes)
    v[n // 2:n // 2 + 3, 0] = 0.0               # exact zeros
    v[n // 2 + 5:n // 2 + 9:2, 1] = 0.0         # zeros between non-zero knots
    v[:3, 0] = [1.0, 1.0, 2.0]                  # zero first slope at the front edge
    v[-3:, 1] = [0.5, 3.0, 2.9]                 # end rule: slope sign change at the back edge
    v[:3, 1] = [0.0, 1.0, 10.0]                 # end rule: three-point estimate of the wrong sign
    return v


def main():
    dsp = import_reference()
    from dsptoolbox.helpers.smoothing import _fractional_octave_smoothing as fos
    from dsptoolbox.standard.enums import SpectrumMethod, SpectrumScaling as S, Window
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20261017)
    z, meta = {}, {"fos": [], "spec": [], "deconv": [], "spectrum": []}

    def add_fos(key_in, spacing, fractions, window, clip, wvec=None):
        i = len(meta["fos"])
        out = fos(z[key_in].copy(), spacing, fractions, window, None if wvec is None else wvec.copy(), bool(clip))
        z[f"fos_{i}_out"] = out
        if wvec is not None:
            z[f"fos_{i}_wvec"] = wvec
        meta["fos"].append({"in": key_in, "spacing": spacing, "fractions": fractions, "window": window, "clip": clip})

    for n in (2, 3, 5, 17, 257, 2049):
        z[f"v{n}"] = rng.standard_normal((n, 3)) + 0.3
        for fr in (1, 3, 24):
            add_fos(f"v{n}", None, fr, "hann", False)
    for n in (17, 257):                                         # long windows: 17 taps on 17 bins, 129 on 257
        add_fos(f"v{n}", None, 0.25, "hann", False)
    add_fos("v17", None, 0.1, "hann", False)                    # 39 taps on 17 bins: longer than the data
    z["vlog40"] = rng.standard_normal((40, 2))
    add_fos("vlog40", 1 / 48, 1, "hann", False)                 # logarithmic bins: 49 taps on 40 points
    add_fos("v257", None, 3, ["gaussian", 2.5], False)          # alpha -> sigma
    add_fos("vlog40", 1 / 48, 6, None, False, wvec=np.array([1.0, 2.0, 3.0, 4.0, 4.0, 3.0, 2.0, 1.5]))  # 8-tap vector
    z["vshape65"] = shaped(65, rng)
    add_fos("vshape65", None, 3, "hann", False)
    add_fos("vshape65", None, 24, "boxcar", False)              # one tap: the interpolations alone
    add_fos("v257", None, 3, "hann", True)                      # clip on data with negative values
    z["v1d"] = rng.standard_normal(129)
    add_fos("v1d", None, 6, "hamming", True)                    # 1-D input

    # signals for the class-level cases
    def make_signal(n, delays):
        cols = []
        for d in delays:
            x = 0.02 * rng.standard_normal(n) * np.exp(-np.arange(n) / 200.0)
            x[d] += 1.0
            cols.append(x)
        x = np.stack(cols, axis=1).astype(np.float32).astype(np.float64)
        from scipy.fft import next_fast_len, rfft
        for nfft in {n, next_fast_len(n, True)}:
            sp = rfft(x, axis=0, n=nfft)
            step = np.abs(np.diff(np.unwrap(np.angle(sp), axis=0), axis=0)).max()
            ratio = (np.abs(sp).min(axis=0) / np.abs(sp).max(axis=0)).min()
            print(f"signal n={n} nfft={nfft}: largest phase step {step:.3f} rad, min/max magnitude {ratio:.3f}")
            assert step < np.pi - 0.5, step
            assert ratio > 0.2, ratio
        return x

    z["sig1000"] = make_signal(1000, (3, 5))
    z["sig3001"] = make_signal(3001, (5, 3))
    z["sig4096"] = make_signal(4096, (3,))
    sigs = ["sig1000", "sig3001", "sig4096"]
    k = 0
    for sc in (S.FFTBackward, S.FFTForward, S.AmplitudeSpectralDensity, S.PowerSpectrum):
        for sm in (1, 3, 12):
            name, pad = sigs[k % 3], bool((k // 3) % 2)
            s = dsp.Signal(None, z[name].copy(), FS)
            s.set_spectrum_parameters(method=SpectrumMethod.FFT, smoothing=sm, pad_to_fast_length=pad, scaling=sc)
            f, sp = s.get_spectrum()
            z[f"spec_{k}_out"] = sp
            meta["spec"].append({"sig": name, "pad": pad, "scaling": sc.name, "smoothing": sm})
            k += 1

    # spectral_deconvolve: the input (denominator) carries smoothing = 3
    out_sig = dsp.Signal(None, z["sig1000"].copy(), FS)
    in_sig = dsp.Signal(None, z["sig1000"][:, ::-1].copy(), FS)
    in_sig.set_spectrum_parameters(method=SpectrumMethod.FFT, smoothing=3, pad_to_fast_length=True,
                                   scaling=S.FFTBackward)
    ir = dsp.transfer_functions.spectral_deconvolve(out_sig, in_sig, apply_regularization=True,
                                                    start_stop_hz=[100.0, 15000.0])
    z["deconv_0_out"] = ir.time_data
    meta["deconv"].append({"sig": "sig1000", "input_reversed_channels": True, "smoothing": 3,
                           "start_stop_hz": [100.0, 15000.0]})

    # Spectrum.apply_octave_smoothing: complex on a linear vector, magnitude on a logarithmic one
    from scipy.fft import rfft
    sp = rfft(z["sig1000"], axis=0)
    spec = dsp.Spectrum(np.fft.rfftfreq(1000, 1 / FS), sp)
    spec.apply_octave_smoothing(3.0, Window.Hann)
    z["spectrum_0_in"], z["spectrum_0_freqs"], z["spectrum_0_out"] = sp, np.fft.rfftfreq(1000, 1 / FS), spec.spectral_data
    meta["spectrum"].append({"fraction": 3.0, "window": "Hann"})
    fl = 20.0 * 2 ** (np.arange(120) / 12)
    mag = np.abs(rng.standard_normal((120, 2))) + 0.1
    spec = dsp.Spectrum(fl, mag)
    spec.apply_octave_smoothing(2.0, Window.Hamming)
    z["spectrum_1_in"], z["spectrum_1_freqs"], z["spectrum_1_out"] = mag, fl, spec.spectral_data
    meta["spectrum"].append({"fraction": 2.0, "window": "Hamming"})

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **z)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
