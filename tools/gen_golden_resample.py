"""Golden vectors for standard.resample and standard.resample_filter, made by RUNNING THE REFERENCE (dsptoolbox 0.8):
    python tools/gen_golden_resample.py

Writes tests/golden/resample/cases.npz.  The signals are not stored: tests/resample_cases.py rebuilds them from their
seeds.  Per case of resample_cases.GOLDEN: `<name>` holds the reference's time data, `<name>_probe` sixteen input samples
and the input's sum (the test checks that it rebuilt the same signal); `meta` (a JSON string) holds per case the
result's rate, length, type and amplitude scale factor, and what was measured.  Per filter of FILTERS: the zpk form the
reference's filter had (`filt_<i>_z`, `_p`, `_k`) and the one its resample_filter returned (`filt_<i>_rz`, `_rp`, `_rk`).

The script ASSERTS, and fails otherwise:
- the reference agrees with the long-double oracle of tests/resample_oracle.py within twice its forward bound on every
  case (the normalised case: after the scale factor is taken out);
- the overshoot case really is normalised (a scale factor other than 1) and no other case is;
- the resampled filters are stable and have as many zeros as poles."""

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle.gen_golden import import_reference  # noqa: E402
import resample_cases as rc  # noqa: E402
import resample_oracle as ro  # noqa: E402

FILTERS = [("butter4", 48000, 44100), ("butter4", 44100, 96000), ("peaking", 48000, 44100), ("peaking", 44100, 96000)]


def main():
    from fractions import Fraction
    dsp = import_reference()
    warnings.simplefilter("ignore")
    z, cases = {}, {}
    for name, (fs, new_fs, kind, rescaling, constrain) in rc.GOLDEN.items():
        x = rc.golden_signal(name)
        sig = rc.golden_input(dsp, name)
        assert np.array_equal(sig.time_data, x), name  # the input itself is inside the constraint
        out = dsp.resample(sig, new_fs, rescaling)
        up, down = Fraction(new_fs, fs).as_integer_ratio()
        value, a = ro.resample_poly(x, up, down)
        if rescaling:
            value, a = value * (down / up), a * (down / up)
        factor = float(out.amplitude_scale_factor)
        worst = ro.worst_ratio(out.time_data / factor, value, 2 * ro.bound(a, up, down) + 4 * ro.U53 * np.abs(value).astype(float))
        print(f"{name}: {type(out).__name__} {out.time_data.shape} at {out.sampling_rate_hz} Hz, scale factor {factor:.6g}, "
              f"reference against oracle {worst:.3g} of twice the bound")
        assert worst <= 1.0, (name, worst)
        assert (factor != 1.0) == name.startswith("overshoot"), (name, factor)
        assert type(out).__name__ == kind and out.sampling_rate_hz == new_fs
        z[name] = np.asarray(out.time_data, dtype=np.float64)
        z[name + "_probe"] = np.concatenate([x[:16, 0], [x.sum()]])
        cases[name] = dict(rate=int(out.sampling_rate_hz), length=int(out.time_data.shape[0]), type=type(out).__name__,
                           scale_factor=factor, constrain_amplitude=bool(out.constrain_amplitude), worst=worst)
    filters = []
    for i, (kind, fs, new_fs) in enumerate(FILTERS):
        if kind == "butter4":  # low pass of order 4 at 0.02 fs
            filt = dsp.Filter.iir_filter(order=4, frequency_hz=0.02 * fs, type_of_pass=dsp.FilterPassType.Lowpass,
                                         filter_design_method=dsp.IirDesignMethod.Butterworth, sampling_rate_hz=fs)
        else:
            filt = dsp.Filter.biquad(eq_type=dsp.BiquadEqType.Peaking, frequency_hz=0.01 * fs, gain_db=6.0, q=2.0, sampling_rate_hz=fs)
        fz, fp, fk = filt.get_coefficients(dsp.FilterCoefficientsType.Zpk)
        rz, rp, rk = dsp.resample_filter(filt, new_fs).get_coefficients(dsp.FilterCoefficientsType.Zpk)
        assert len(rz) == len(rp) and np.abs(rp).max() < 1.0, (kind, fs, new_fs)
        for key, v in (("z", fz), ("p", fp), ("k", fk), ("rz", rz), ("rp", rp), ("rk", rk)):
            z[f"filt_{i}_{key}"] = np.asarray(v, dtype=np.complex128 if key[-1] != "k" else np.float64)
        filters.append(dict(kind=kind, fs=fs, new_fs=new_fs))
        print(f"filter {i}: {kind} {fs} -> {new_fs}: {len(rp)} poles, largest |p| {np.abs(rp).max():.6f}")
    import scipy
    meta = dict(cases=cases, filters=filters, numpy=np.__version__, scipy=scipy.__version__,
                reference="dsptoolbox 0.8: standard.resample, standard.resample_filter")
    os.makedirs(os.path.dirname(rc.PATH), exist_ok=True)
    np.savez_compressed(rc.PATH, meta=np.array(json.dumps(meta)), **z)
    print(f"{rc.PATH}: {os.path.getsize(rc.PATH) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
