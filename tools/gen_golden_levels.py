"""Golden vectors for the levels and loudness family, made by RUNNING THE REFERENCE (dsptoolbox 0.8: normalize, rms,
crest_factor, fade, apply_gain, detrend, envelope, lufs_integrated, merge_filters, tools.to_db / from_db):
    python tools/gen_golden_levels.py

Writes tests/golden/levels/cases.npz.  The inputs are not stored: tests/levels_cases.py rebuilds them from their seeds.
Per case of levels_cases.py: `normalize_<name>`, `gain_<name>`, `fade_<name>`, `detrend_<order>`, `env_analytic_<name>`,
`env_boxcar_<name>` hold the reference's output; `rms_<name>`, `rms_db_<name>`, `crest_<name>`, `crest_db_<name>` its
measures of the NORMALIZE inputs; `lufs_<name>` its loudness, `lufs_<name>_z` the block mean squares it formed and
`lufs_<name>_gated` the blocks that pass both gates; `fadetable_<type>` the reference's curve of 300 samples;
`merge_sos`, `merge_fir`, `to_db_*`, `from_db_*` the host helpers.  `meta` is a JSON string with everything measured.

The script ASSERTS, and fails otherwise:
- the reference agrees with the long-double oracle of tests/levels_oracle.py on every stored output (its own error is
  recorded per detrend order, per boxcar case on the mean square, per analytic case: the GPU test's bounds are 4 x these);
- no block of a loudness case lies within 0.01 LU of either gate; over the set at least one block is below -70, one
  between the gates and one above; the lengths Tg - 1 and Tg give NaN, the three lengths above them finite values;
- each deliberately wrong oracle of levels_cases.WRONG_ORACLES misses its bound by orders of magnitude."""

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle.gen_golden import import_reference  # noqa: E402
import fft64_cases as f64c  # noqa: E402
import levels_cases as lc  # noqa: E402
import levels_oracle as lo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "levels", "cases.npz")
SANITY = 1e-9          # the reference against the oracle, of the peak: a wrong restatement misses it by far
GATE_MARGIN_LU = 0.01
LUFS_TOL = 1e-7        # the GPU test's bound on the loudness
WRONG_FACTOR = 1e3     # a wrong oracle misses its bound by at least this factor


def main():
    dsp = import_reference()
    warnings.simplefilter("ignore")
    from dsptoolbox.standard._framed_signal_representation import _get_framed_signal
    z, meas = {}, {}

    def signal(x, fs=lc.FS):
        return dsp.Signal(None, x.copy(), fs, constrain_amplitude=False)

    def judge(key, got, want, bound=SANITY):
        e = lo.relative_to_peak(got, want)
        print(f"{key}: reference against oracle {e:.2e}")
        assert e <= bound, (key, e)
        z[key] = np.asarray(got, dtype=np.float64)
        return e

    # ---- normalize, rms, crest_factor ----
    for name, (seed, n, n_ch, dbfs, pk, each) in lc.NORMALIZE.items():
        x = lc.noise(seed, n, n_ch)
        judge(f"normalize_{name}", dsp.normalize(signal(x), dbfs, pk, each).time_data, lo.normalize(x, dbfs, pk, each))
        r = dsp.rms(signal(x), in_dbfs=False)
        e = float(np.max(np.abs(r - lo.rms(x)) / lo.rms(x)))
        assert e <= 4 * lo.reduction_depth(n) * lc.U, (name, e)
        meas[f"rms_{name}"] = e
        z[f"rms_{name}"], z[f"rms_db_{name}"] = r, dsp.rms(signal(x), in_dbfs=True)
        z[f"crest_{name}"], z[f"crest_db_{name}"] = dsp.crest_factor(signal(x), in_db=False), dsp.crest_factor(signal(x))
        assert np.max(np.abs(z[f"crest_{name}"] - lo.peak(x) / lo.rms(x))) <= 1e-12
    seed, n, n_ch = lc.NORMALIZE["rms_each"][:3]
    x = lc.noise(seed, n, n_ch)
    wrong = float(np.max(np.abs(lo.rms(x, centred=False) - lo.rms(x)) / lo.rms(x)))
    meas["wrong_rms"] = wrong
    assert wrong >= WRONG_FACTOR * 4 * lo.reduction_depth(n) * lc.U, wrong

    # ---- apply_gain, fade ----
    for name, (seed, n, n_ch, g) in lc.GAIN.items():
        x = lc.noise(seed, n, n_ch)
        judge(f"gain_{name}", dsp.apply_gain(signal(x), np.asarray(g) if isinstance(g, list) else g).time_data, lo.gain(x, g))
    for name, (seed, n, n_ch, kind, l_s, a, b) in lc.FADE.items():
        x = lc.noise(seed, n, n_ch)
        got = dsp.fade(signal(x), getattr(dsp.FadeType, kind), lc.fade_seconds(l_s), a, b).time_data
        l_eff = int(n / lc.FS * 0.025 * lc.FS) if l_s is None else l_s
        want = lo.fade(x, kind, l_eff, a, b)
        if kind == "Logarithmic" and l_eff == 1:
            assert np.isnan(got[0]).all()
            z[f"fade_{name}"] = got
        else:
            judge(f"fade_{name}", got, want, 1e-14)
    seed, n, n_ch, kind, l_s, a, b = lc.FADE["exp_start"]
    x = lc.noise(seed, n, n_ch)
    wrong = lo.relative_to_peak(lo.fade(x, kind, l_s, a, b, swapped=True), z["fade_exp_start"].astype(lo.LD))
    meas["wrong_fade"] = wrong
    assert wrong >= WRONG_FACTOR * 1e-14, wrong
    for kind in ("Linear", "Exponential", "Logarithmic"):
        ones = np.ones((400, 1))
        z[f"fadetable_{kind}"] = dsp.fade(signal(ones), getattr(dsp.FadeType, kind), lc.fade_seconds(300), True, False).time_data[:300, 0]
        assert np.max(np.abs(z[f"fadetable_{kind}"] - lo.fade_table(kind, 300))) <= 1e-14, kind

    # ---- detrend ----
    x = lc.detrend_input()
    meas["detrend"] = {}
    for order in lc.DETREND_ORDERS:
        meas["detrend"][str(order)] = judge(f"detrend_{order}", dsp.detrend(signal(x), order).time_data, lo.detrend(x, order))

    # ---- envelope ----
    meas["env_analytic"], meas["env_boxcar"] = {}, {}
    for name, (seed, n, n_ch) in lc.ENVELOPE_ANALYTIC.items():
        x = lc.noise(seed, n, n_ch)
        meas["env_analytic"][name] = judge(f"env_analytic_{name}", dsp.envelope(signal(x), True), lo.envelope_analytic(x))
    for name, (seed, n, n_ch, w, stop) in lc.ENVELOPE_BOXCAR.items():
        x = lc.boxcar_input(name)
        got = dsp.envelope(signal(x), False, w)
        z[f"env_boxcar_{name}"] = got
        want = lo.moving_mean_square(x, w)
        with np.errstate(invalid="ignore"):
            ms = np.where(np.isnan(got), 0.0, got) ** 2  # (a NaN of the reference: a mean square its FFT left below zero)
        e = float(np.max(np.max(np.abs(ms - want), axis=0) / np.max(want, axis=0)))
        print(f"env_boxcar_{name}: reference against oracle {e:.2e} of the peak mean square, {int(np.isnan(got).sum())} NaN")
        assert e <= SANITY, (name, e)
        meas["env_boxcar"][name] = e
        meas.setdefault("env_boxcar_nan", {})[name] = int(np.isnan(got).sum())
    name = "n4095"
    seed, n, n_ch = lc.ENVELOPE_ANALYTIC[name]
    x = lc.noise(seed, n, n_ch)
    wrong = lo.relative_to_peak(lo.envelope_analytic(x, with_detrend=False), z[f"env_analytic_{name}"].astype(lo.LD))
    meas["wrong_envelope"] = wrong
    assert wrong >= WRONG_FACTOR * max(4 * meas["env_analytic"][name], f64c.tolerance(("hilbert", 8192))), wrong

    # ---- loudness ----
    meas["lufs"] = {}
    seen = dict(below=0, between=0, above=0)
    for name in lc.LUFS:
        x, fs = lc.lufs_input(name)
        s = signal(x, fs)
        value = float(dsp.lufs_integrated(s))
        tg, step = lc.lufs_blocks(fs)
        # the block mean squares as the reference forms them: its K-weighting filter, its framing
        k_filter = dsp.merge_filters([
            dsp.Filter.biquad(eq_type=dsp.BiquadEqType.Highshelf, frequency_hz=1500, gain_db=4.0, q=2**0.5 / 2.0, sampling_rate_hz=fs),
            dsp.Filter.biquad(eq_type=dsp.BiquadEqType.Highpass, frequency_hz=38.1, gain_db=0.0, q=0.5, sampling_rate_hz=fs)])
        nb = lo.block_count(len(x), tg, step)
        zr = (np.mean(_get_framed_signal(k_filter.filter_signal(s).time_data ** 2.0, tg, step, False), axis=0)
              if nb else np.zeros((0, x.shape[1])))
        assert zr.shape == (nb, x.shape[1]), (name, zr.shape, nb)
        z[f"lufs_{name}"], z[f"lufs_{name}_z"] = np.float64(value), zr
        zo, pk = lo.lufs_blocks(x, fs)
        v_ref, lj, above, both, gate = lo.lufs_gating(zr)
        v_orc, _, above_o, both_o, _ = lo.lufs_gating(zo)
        z[f"lufs_{name}_gated"] = both
        if nb == 0:
            assert np.isnan(value), name
            continue
        assert np.isfinite(value) and abs(value - v_ref) <= 1e-12 and abs(value - float(v_orc)) <= 1e-9, (name, value, v_ref, v_orc)
        assert np.array_equal(above, above_o) and np.array_equal(both, both_o), name
        e_z = float(np.max(np.abs(zr - zo) / zo))
        margin_a, margin_r = float(np.min(np.abs(lj + 70))), float(np.min(np.abs(lj[above] - gate)))
        assert min(margin_a, margin_r) > GATE_MARGIN_LU, (name, margin_a, margin_r)
        seen["below"] += int((~above).sum())
        seen["between"] += int((above & ~both).sum())
        seen["above"] += int(both.sum())
        meas["lufs"][name] = dict(value=value, blocks=int(nb), below=int((~above).sum()), between=int((above & ~both).sum()),
                                  above=int(both.sum()), margin_absolute=margin_a, margin_relative=margin_r, z_error=e_z,
                                  peak2_over_z=float(np.max((pk * pk / zo)[both])))
        print(f"lufs_{name}: {value:.4f} LUFS, {meas['lufs'][name]}")
    assert min(seen.values()) >= 1, seen
    for n_ch in (2, 5):
        vals = [float(z[f"lufs_edge_{n}_{n_ch}ch"]) for n in lc.LUFS_EDGE_LENGTHS]
        assert np.isnan(vals[0]) and np.isnan(vals[1]) and np.isfinite(vals[2:]).all(), vals
    x, fs = lc.lufs_input("programme_11025")
    tg, step = lc.lufs_blocks(fs)
    assert (tg, step) == (4410, 1103)
    wrong = abs(float(lo.lufs_gating(lo.lufs_blocks(x, fs, tg=4 * step, step=step)[0])[0]) - float(z["lufs_programme_11025"]))
    meas["wrong_lufs"] = wrong
    assert wrong >= WRONG_FACTOR * LUFS_TOL, wrong

    # ---- host helpers ----
    iir = [dsp.Filter.biquad(eq_type=dsp.BiquadEqType.Highshelf, frequency_hz=1500, gain_db=4.0, q=2**0.5 / 2.0, sampling_rate_hz=48000),
           dsp.Filter.biquad(eq_type=dsp.BiquadEqType.Highpass, frequency_hz=38.1, gain_db=0.0, q=0.5, sampling_rate_hz=48000)]
    z["merge_sos"] = dsp.merge_filters(iir).get_coefficients(dsp.FilterCoefficientsType.Sos)
    fir = [dsp.Filter.from_ba(np.array([1.0, 0.5, 0.25]), [1.0], 48000), dsp.Filter.from_ba(np.array([0.5, -0.25]), [1.0], 48000)]
    z["merge_fir"] = dsp.merge_filters(fir).ba[0]
    v = np.array([1.0, 0.5, 1e-3, 0.0, -2.0])
    z["db_in"] = v
    z["to_db_amp"], z["to_db_pow"] = dsp.tools.to_db(v, True), dsp.tools.to_db(v, False)
    z["to_db_range"] = dsp.tools.to_db(v, True, dynamic_range_db=40.0)
    z["to_db_noclip"] = dsp.tools.to_db(v[:3], False, None, None)
    z["from_db_amp"], z["from_db_pow"] = dsp.tools.from_db(np.array([-6.0, 0.0, 3.0]), True), dsp.tools.from_db(np.array([-6.0, 0.0, 3.0]), False)

    meta = dict(fs=lc.FS, measured=meas, gate_margin_lu=GATE_MARGIN_LU, lufs_tol=LUFS_TOL, seen=seen,
                wrong_oracles=dict(lc.WRONG_ORACLES), reference="dsptoolbox 0.8", generator="tools/gen_golden_levels.py")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **z)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    print(json.dumps(meas, indent=1))


if __name__ == "__main__":
    main()
