"""Golden vectors for spectral subtraction, made by RUNNING THE REFERENCE (dsptoolbox 0.8: effects.SpectralSubtractor):
    python tools/gen_golden_specsub.py

Writes tests/golden/specsub/cases.npz.  Per case of specsub_cases.GOLDEN `out_<name>` holds the reference's output and
`probe_<name>` the first eight samples of the input (the inputs themselves are rebuilt from their seeds by
tests/specsub_cases.py; the probes show that both sides built the same ones); the MultiBandSignal case has `out_bands_0`
and `out_bands_1`.  `meta` is a JSON string: per case `error`, the reference's own error against the long-double oracle of
tests/specsub_oracle.py in units of the channel's peak, and the smallest gate, clip and detector margins.

The script ASSERTS, and fails otherwise:
- no frame level of any case lies within 1e-6 dB of the threshold and no bin within 1e-6 of its clip (the oracle's
  margins), no detector level within 1e-9 dB of its threshold: a case that fails gets another seed in specsub_cases.py;
- the reference agrees with the oracle within SANITY = 1e-9 of the peak (its measured errors are far below; the
  figure only guards against an oracle that restates something else);
- the case meant to end in NaN does, in the channel meant, and nowhere else."""

import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import specsub_cases as sc  # noqa: E402
import specsub_oracle as so  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "specsub", "cases.npz")
SANITY = 1e-9


def main():
    dsp = import_reference()
    warnings.simplefilter("ignore")
    z, meta = {}, {}

    def run(name, x, ctor, adv):
        s = dsp.Signal(None, x, sc.FS, constrain_amplitude=False)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):  # (the reference prints per channel)
            got = sc.effect(dsp.effects, dsp, ctor, adv).apply(s).time_data
            want, gates, clips, nearest = sc.oracle(x, ctor, adv)
        gate, clip, nearest = sc.conditions(gates, clips, nearest, ctor.get("adaptive_mode", True))
        e = so.stream_error(got, want)
        print(f"{name}: reference error {e:.2e} of the peak, floor {so.floor(sc.W):.2e}; margins: gate {gate:.2e} dB, "
              f"clip {clip:.2e}, detector {nearest:.2e} dB")
        assert e <= SANITY, (name, e)
        meta[name] = dict(error=e, gate=gate, clip=clip, detector=None if np.isinf(nearest) else nearest)
        z[f"out_{name}"], z[f"probe_{name}"] = np.asarray(got, dtype=np.float64), x[:8].copy()
        return got

    for name, (seed, n, n_ch, ctor, adv) in sc.GOLDEN.items():
        got = run(name, sc.samples(name), ctor, adv)
        assert got.shape == (n, n_ch)
        if name == "silence":
            assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, 0]).all()
        else:
            assert np.isfinite(got).all(), name
    for name, (seeds, n, n_ch, ctor, adv) in sc.MULTIBAND.items():
        bands = [sc.burst(seed, n, n_ch) for seed in seeds]
        mbs = dsp.MultiBandSignal([dsp.Signal(None, b, sc.FS, constrain_amplitude=False) for b in bands])
        with contextlib.redirect_stdout(io.StringIO()):
            out = sc.effect(dsp.effects, dsp, ctor, adv).apply(mbs)
        for i, b in enumerate(bands):
            run(f"{name}_{i}", b, ctor, adv)  # (the band alone: the reference loops over the bands)
            assert np.array_equal(out.bands[i].time_data, z[f"out_{name}_{i}"])

    info = dict(fs=sc.FS, window=sc.W, floor=so.floor(sc.W), cases=meta, generator="tools/gen_golden_specsub.py",
                reference="dsptoolbox 0.8 source", numpy=np.__version__)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, meta=np.array(json.dumps(info)), **z)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
