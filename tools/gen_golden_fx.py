"""Golden vectors for the audio effects, made by RUNNING THE REFERENCE (dsptoolbox 0.8: effects.Compressor, Distortion,
Tremolo, Chorus, DigitalDelay, LFO, the musical-rhythm helpers and activity_detector):
    python tools/gen_golden_fx.py

Writes tests/golden/fx/cases.npz.  `meta` is a JSON string with `fs`, `bound` and what was measured.  The inputs are not
stored: tests/fx_cases.py rebuilds them from their seeds.  Per case of fx_cases.py: `compressor_<name>`, `delay_<name>`,
`chorus_<name>` (and `chorus_<name>_table`, the integer delays), `distortion_<name>`, `tremolo_<name>` (and `_mod`, the
modulator |w depth + 1|) hold the reference's output; `detector_<name>` the boolean signal indices, `_signal` and `_noise`
the two returned signals; `lfo_<i>` the waveforms of fx_cases.LFOS and `rhythm` the frequencies of fx_cases.RHYTHMS.
np.random.seed(k) precedes every call that draws a phase.

The script ASSERTS, and fails otherwise:
- on every stored output the reference agrees with the long-double recursion of tests/fx_oracle.py within BOUND = 1e-12
  of each channel's peak (measured: see `measured` in meta; the reference sits at 7e-17 .. 1.4e-15);
- every follower coefficient of the compressor cases is at least C_MIN = 0.007, which the bound's derivation uses;
- no compressor case with a hard knee has a sample level within 1e-9 dB of its threshold, no detector case a smoothed
  level within 1e-9 dB of its threshold (so the device's mask must equal the reference's exactly), no chorus delay lies
  within 1e-6 of a half-integer;
- each deliberately wrong oracle misses the bound by a wide margin on the case fx_cases.WRONG_ORACLES names.  Observed:
  attack and release swapped 3.9e-01 of the peak, the unreachable knee branch 1.0e-01, the final gain taken from
  post_gain_db 8.8e-01: factors of 1e11 and more above BOUND."""

import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import fx_cases as fc  # noqa: E402
from tests import fx_oracle as fo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fx", "cases.npz")


def main():
    dsp = import_reference()
    warnings.simplefilter("ignore")
    fx = dsp.effects
    z, measured = {}, {}

    def signal(seed, n, n_ch):
        return dsp.Signal(None, fc.burst(seed, n, n_ch), fc.FS, constrain_amplitude=False)

    def judge(family, name, got, want):
        e = fo.stream_error(got, want)
        print(f"{family}_{name}: {e:.2e}")
        assert e <= fo.BOUND, (family, name, e)
        measured[family] = max(measured.get(family, 0.0), e)
        z[f"{family}_{name}"] = np.asarray(got, dtype=np.float64)

    for name, (seed, n, n_ch, p) in fc.COMPRESSOR.items():
        s = signal(seed, n, n_ch)
        got = fc.compressor(fx, p).apply(s).time_data
        want, nearest = fo.compress(s.time_data, fc.FS, **p)
        for ms in (p.get("attack_time_ms", 0.5), p.get("release_time_ms", 20)):
            assert fo.coefficient(int(ms * 1e-3 * fc.FS)) >= fo.C_MIN, (name, ms)
        assert p.get("knee_db", 0) > 0 or nearest > 1e-9, (name, nearest)
        judge("compressor", name, got, want)
    for wrong, name in fc.WRONG_ORACLES.items():
        seed, n, n_ch, p = fc.COMPRESSOR[name]
        e = fo.stream_error(fo.compress(fc.burst(seed, n, n_ch), fc.FS, wrong=wrong, **p)[0], z[f"compressor_{name}"])
        print(f"wrong oracle '{wrong}' on {name}: {e:.2e}")
        assert e > 1e6 * fo.BOUND, (wrong, e)
        measured[f"wrong_{wrong}"] = e

    for name, (seed, n, n_ch, p) in fc.DETECTOR.items():
        s = signal(seed, n, n_ch)
        det, others = dsp.activity_detector(s, p["threshold_dbfs"], 0, p["relative"], None, 1, p["release_time_ms"])
        mask, nearest = fo.detect(s.time_data[:, 0], fc.FS, **p)
        print(f"detector_{name}: {int(mask.sum())} of {n} active, nearest level {nearest:.3g} dB from the threshold")
        assert nearest > 1e-9, (name, nearest)
        assert np.array_equal(mask, others["signal_indices"]), name
        assert (name == "empty") == (not mask.any())
        z[f"detector_{name}"] = others["signal_indices"]
        z[f"detector_{name}_signal"], z[f"detector_{name}_noise"] = det.time_data, others["noise"].time_data

    for name, (seed, n, n_ch, p) in fc.DELAY.items():
        s = signal(seed, n, n_ch)
        judge("delay", name, fc.delay(fx, p).apply(s).time_data, fo.delay(s.time_data, fc.FS, **p))

    for name, (seed, n, n_ch, p) in fc.CHORUS.items():
        s = signal(seed, n, n_ch)
        e = fc.chorus(fx, p)
        np.random.seed(p["seed"])
        table, half = fc.chorus_table(e, n)
        assert half > 1e-6, (name, half)
        assert (name == "negative") == bool((table < 0).any()), name
        np.random.seed(p["seed"])
        judge("chorus", name, e.apply(s).time_data, fo.chorus(s.time_data, table, p["mix_percent"] / 100))
        z[f"chorus_{name}_table"] = table.astype(np.int64)

    for name, (seed, n, n_ch, p) in fc.DISTORTION.items():
        s = signal(seed, n, n_ch)
        kinds, levels, mix, offsets = fc.distortion_lists(p)
        judge("distortion", name, fc.distortion(fx, p).apply(s).time_data,
              fo.distort(s.time_data, kinds, levels, mix, offsets, p["post"]))

    for name, (seed, n, n_ch, p) in fc.TREMOLO.items():
        s = signal(seed, n, n_ch)
        e = fc.tremolo(fx, p)
        np.random.seed(p["seed"])
        mod = np.abs(e.modulator.get_waveform(fc.FS, n) * e.depth + 1)
        np.random.seed(p["seed"])
        judge("tremolo", name, e.apply(s).time_data, fo.tremolo(s.time_data, mod))
        z[f"tremolo_{name}_mod"] = mod

    for i, (freq, waveform, random_phase, smooth, length, seed) in enumerate(fc.LFOS):
        np.random.seed(seed)
        z[f"lfo_{i}"] = fx.LFO(freq, waveform, random_phase, smooth).get_waveform(fc.FS, length)
    z["rhythm"] = np.array([fx.get_frequency_from_musical_rhythm(note, bpm) for note, bpm in fc.RHYTHMS])

    meta = dict(fs=fc.FS, bound=fo.BOUND, measured=measured, generator="tools/gen_golden_fx.py",
                reference="dsptoolbox 0.8 source", numpy=np.__version__)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **z)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB; measured {measured}")


if __name__ == "__main__":
    main()
