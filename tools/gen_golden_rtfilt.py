"""Golden vectors for the realtime filters, made by RUNNING THE REFERENCE (dsptoolbox 0.8: StateVariableFilter,
ParallelFilter, IIRFilter, FIRFilter, StateSpaceFilter, FilterChain and ExponentialAverageFilter of dsptoolbox.filterbanks):
    python tools/gen_golden_rtfilt.py

Writes tests/golden/rtfilt/cases.npz.  `meta` is a JSON string with `fs`, `bound`, the parameters and `worst`, the
reference's own distance to the long-double oracle per family; `x` (N, 2) is the input of every filtering case, noise
rounded to float32 and stored as float32.
- `svf_y` (4, N, 2), `svf_state`: filter_signal over x from rest; `svf_ps` (5, 4): process_sample of x[:5, 0] after it.
- `iir_b`, `iir_a`; `iir_y` (N, 2), `iir_state`: the process_sample loop over x, channel after channel.
- `fir_b`; `fir_y`, `fir_state`, `fir_ind`: the same for FIRFilter (state: the circular buffer and current_state_ind).
- `ss_A`, `ss_B`, `ss_C`, `ss_D` (from_filter of iir_b / iir_a), `ss_y`, `ss_x`; `sosl_sos` and `sosl_A` (K, 2, 2), `sosl_B`,
  `sosl_C`, `sosl_D` (from_filter_as_sos_list).
- `chain_y`: FilterChain([IIRFilter, FIRFilter, StateSpaceFilter]).process_sample over x.
- `par_poles`, `par_ir` (the fitted impulse response), `par_freqs`, `par_spectrum` (ir.get_spectrum()), `par_sos`,
  `par_fir` (fit_to_ir with n_fir = 3 and delay_iir_samples = 2), `par_y` (filter_signal over x), `par_get_ir` (64 samples),
  `par_ps` (40,): process_sample of x[:40, 0] from rest; `par2_sos`, `par2_fir`: a fit with n_fir = 1 and no delay.
- `ema_y` (N,): ExponentialAverageFilter(0.01, 0.05).process_sample over |x[:, 0]|; `ema_coef` its two coefficients.

The script ASSERTS that on every stored output the reference agrees with the long-double recursion of
tests/rtfilt_oracle.py within BOUND of each channel's peak; it fails otherwise."""

import json
import os
import sys
import warnings

import numpy as np
from scipy.signal import butter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import rtfilt_oracle as ro  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rtfilt", "cases.npz")
FS = 48000
BOUND = 1e-11
N, N_IR = 500, 256
SVF = (1200.0, 0.7)
PAR = dict(n_fir=3, delay=2)


def main():
    dsp = import_reference()
    warnings.simplefilter("ignore")
    fb = dsp.filterbanks
    rng = np.random.default_rng(31415)
    z = {"x": rng.standard_normal((N, 2)).astype(np.float32)}
    x = z["x"].astype(np.float64)
    worst = {}

    def judge(what, got, want):
        e = ro.stream_error(got, want)
        print(f"{what}: {e:.2e}")
        assert e <= BOUND, (what, e)
        worst[what.split()[0]] = max(worst.get(what.split()[0], 0.0), e)

    def signal(td):
        return dsp.Signal(None, td.copy(), FS, constrain_amplitude=False)

    def loop(f, n_ch=2):
        f.set_n_channels(n_ch)
        y = np.zeros((N, n_ch))
        for c in range(n_ch):
            for i in range(N):
                y[i, c] = f.process_sample(x[i, c], c)
        return y

    # ---- state-variable filter --------------------------------------------------------------------------------------
    svf = fb.StateVariableFilter(SVF[0], SVF[1], FS)
    mb = svf.filter_signal(signal(x))
    z["svf_y"] = np.stack([b.time_data for b in mb.bands])
    z["svf_state"] = svf.state.copy()
    s = ro.svf_structure(SVF[0], SVF[1], FS)
    want, zf = ro.serial(s, x)
    judge("svf output", z["svf_y"], want)
    judge("svf state", z["svf_state"].reshape(-1, 1), zf.reshape(-1, 1))
    z["svf_ps"] = np.array([svf.process_sample(x[i, 0], 0) for i in range(5)])
    # ---- IIRFilter, FIRFilter, StateSpaceFilter, FilterChain --------------------------------------------------------
    b4, a4 = butter(4, 0.3)
    z["iir_b"], z["iir_a"] = b4, a4
    iir = fb.IIRFilter(b4.copy(), a4.copy())
    z["iir_y"] = loop(iir)
    z["iir_state"] = iir.state.copy()
    want, zf = ro.serial(dict(kind="tdf2", b=b4 / a4[0], a=a4 / a4[0]), x)
    judge("iir output", z["iir_y"], want)
    judge("iir state", z["iir_state"].reshape(-1, 1), zf.reshape(-1, 1))
    z["fir_b"] = rng.standard_normal(9)
    fir = fb.FIRFilter(z["fir_b"].copy())
    z["fir_y"] = loop(fir)
    z["fir_state"], z["fir_ind"] = fir.state.copy(), fir.current_state_ind.copy()
    judge("fir output", z["fir_y"], ro.fir_direct(z["fir_b"], x))
    ss = fb.StateSpaceFilter.from_filter(dsp.Filter.from_ba(b4.copy(), a4.copy(), FS))
    z["ss_A"], z["ss_B"], z["ss_C"], z["ss_D"] = (np.array(m) for m in (ss.A, ss.B, ss.C, ss.D))
    z["ss_y"] = loop(ss)
    z["ss_x"] = ss.x.copy()
    want, zf = ro.serial(dict(kind="state_space", A=ss.A, B=ss.B, C=ss.C, Dd=float(ss.D)), x)
    judge("ss output", z["ss_y"], want)
    judge("ss state", z["ss_x"].reshape(-1, 1), zf.reshape(-1, 1))
    z["sosl_sos"] = butter(6, 0.2, output="sos")
    lst = fb.StateSpaceFilter.from_filter_as_sos_list(dsp.Filter.from_sos(z["sosl_sos"].copy(), FS))
    for key in "ABCD":
        z[f"sosl_{key}"] = np.stack([np.array(getattr(f, key)) for f in lst])
    chain = fb.FilterChain([fb.IIRFilter(b4.copy(), a4.copy()), fb.FIRFilter(z["fir_b"].copy()),
                            fb.StateSpaceFilter.from_filter(dsp.Filter.from_ba(b4.copy(), a4.copy(), FS))])
    z["chain_y"] = loop(chain)
    want = ro.serial(dict(kind="state_space", A=ss.A, B=ss.B, C=ss.C, Dd=float(ss.D)),
                     ro.fir_direct(z["fir_b"], ro.serial(dict(kind="tdf2", b=b4 / a4[0], a=a4 / a4[0]), x)[0]))[0]
    judge("chain output", z["chain_y"], want)
    # ---- ParallelFilter ---------------------------------------------------------------------------------------------
    poles = np.array([0.6, -0.4, 0.8 * np.exp(0.3j), 0.9 * np.exp(1.1j), 0.95 * np.exp(2.2j)])
    ir = (rng.standard_normal((N_IR, 1)) * np.exp(-np.arange(N_IR) / 30.0)[:, None]).astype(np.float32).astype(np.float64)
    z["par_poles"], z["par_ir"] = poles, ir
    ref_ir = dsp.ImpulseResponse(None, ir.copy(), FS, constrain_amplitude=False)
    z["par_freqs"], z["par_spectrum"] = ref_ir.get_spectrum()
    par = fb.ParallelFilter(poles.copy(), PAR["n_fir"], FS)
    par.set_parameters(delay_iir_samples=PAR["delay"])
    par.fit_to_ir(ref_ir)
    z["par_sos"] = np.array(par._ParallelFilter__sos)
    z["par_fir"] = np.array(par._ParallelFilter__fir_coefficients)
    z["par_y"] = par.filter_signal(signal(x)).time_data
    s = dict(kind="parallel", sos=z["par_sos"][:, [0, 1, 2, 4, 5]], delay=PAR["delay"], fir=z["par_fir"])
    judge("parallel output", z["par_y"], ro.serial(s, x)[0])
    z["par_get_ir"] = par.get_ir(64).time_data
    par.set_n_channels(1)
    par.reset_state()
    z["par_ps"] = np.array([par.process_sample(x[i, 0], 0) for i in range(40)])
    judge("parallel process_sample", z["par_ps"][:, None], ro.serial(s, x[:40, :1])[0])
    par2 = fb.ParallelFilter(poles.copy(), 1, FS)
    par2.fit_to_ir(ref_ir)
    z["par2_sos"] = np.array(par2._ParallelFilter__sos)
    z["par2_fir"] = np.array(par2._ParallelFilter__fir_coefficients)
    # ---- ExponentialAverageFilter -----------------------------------------------------------------------------------
    ema = fb.ExponentialAverageFilter(0.01, 0.05, FS)
    z["ema_coef"] = np.array([ema.increase_coefficient, ema.decrease_coefficient])
    z["ema_y"] = np.array([float(ema.process_sample(abs(x[i, 0]), 0)) for i in range(N)])

    print("worst reference error against long double:", {k: f"{v:.2e}" for k, v in worst.items()})
    z["meta"] = np.array(json.dumps({"fs": FS, "bound": BOUND, "svf": SVF, "par": PAR, "worst": worst}))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300000


if __name__ == "__main__":
    main()
