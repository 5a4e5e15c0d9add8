"""Golden vectors for the variable-Q transform, made by RUNNING THE REFERENCE (dsptoolbox 0.8: transforms.vqt,
transforms/transforms.py:812-923):
    python tools/gen_golden_vqt.py

Writes tests/golden/vqt/cases.npz for the CASES of tests/vqt_cases.py (signals rebuilt from their seeds; `<name>_probe`
holds the first 16 samples of channel 0 and the sum, to prove the rebuild): `<name>_f`, the frequency vector, and
`<name>_vqt`, the complex128 result -- whole where it has at most vqt_cases.STORE_WHOLE_UP_TO bytes, otherwise the rows
and samples of vqt_cases.subset(name): the top, middle and bottom row of every octave at the first and the last 64
samples and 64 samples spread between them.  `<name>_max` is the largest magnitude of the whole result, the scale of
the tolerances.  The script asserts the shapes the cases are there for (d, the octave lengths, the kernel lengths)."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden import import_reference  # noqa: E402
import vqt_cases as vc  # noqa: E402
import vqt_oracle  # noqa: E402


def main():
    dsp = import_reference()
    z = {}
    for name, p in vc.CASES.items():
        x = vc.signal(name)
        z[name + "_probe"] = np.concatenate([x[:16, 0], [x.sum()]])
        f, out = dsp.transforms.vqt(dsp.Signal(None, x.copy(), p["fs"], constrain_amplitude=False), **p["kw"])
        assert out.shape == (vc.n_rows(name), p["n"], p["c"]) and out.dtype == np.complex128
        z[name + "_f"], z[name + "_max"] = f, np.array(np.abs(out).max())
        if vc.stored_whole(name):
            z[name + "_vqt"] = out
        else:
            rows, samples = vc.subset(name)
            z[name + "_vqt"] = out[np.ix_(rows, samples)]
        octaves = p["kw"].get("octaves", [1, 5])
        hi, d, mid_fs = vqt_oracle.setup(p["fs"], octaves, 440)
        lens = [len(k) for k in vqt_oracle.kernels(p["kw"].get("q", 1), hi, p["kw"].get("bins_per_octave", 24), mid_fs,
                                                   p["kw"].get("window", "hann"), p["kw"].get("gamma", 50) / p["fs"] * mid_fs)]
        print(name, "d", d, "L", min(lens), max(lens), "rows", out.shape[0], "stored", z[name + "_vqt"].shape)
        if name == "default":
            assert d == 22 and (min(lens), max(lens)) == (70, 127)
        if name == "cqt":
            assert d == 14
        if name == "kaiser":
            assert (min(lens), max(lens)) == (10, 16)
        if name == "d1":
            assert d == 1
    os.makedirs(os.path.dirname(vc.PATH), exist_ok=True)
    np.savez_compressed(vc.PATH, **z)
    print(vc.PATH, os.path.getsize(vc.PATH), "bytes")
    assert os.path.getsize(vc.PATH) < (1 << 20)


if __name__ == "__main__":
    main()
