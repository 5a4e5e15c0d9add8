"""Golden vectors for the CleanSC, Orthogonal, Functional and MVDR beamformers, made by RUNNING THE REFERENCE
(dsptoolbox 0.8, beamforming/beamforming.py:883-1314):  python tools/gen_golden_beamformers.py

Writes tests/golden/beamformers/cases.npz: for every case i the reference's final map `map_i` and, once per bin range
`band` (the case's meta entry), the selected bins `f_<band>`, the steering vectors `h_<band>` the reference built
and its CSM slice `csm_<scaling>_<band>`; plus the microphone signals as float32
(`time_data`, fewer than 128 Welch frames: a short estimate) for the end-to-end class test.

Cases that are not well posed are refused: MVDR and Orthogonal recomputed through numpy's eigh must match the
reference's map to 1e-9, and every argmax CleanSC and Orthogonal take must be clear of a near-tie."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beamformers", "cases.npz")  # (a folder of its own: the top-level fixtures are oracle/gen_golden.py's)
FS = 8000
WINDOW = 128
N_MICS = 16
TIE = 1e-6  # smallest relative gap between the best and the second-best grid point of an argmax


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def integrate(m, f):
    from scipy.integrate import simpson
    return simpson(m, dx=f[1] - f[0], axis=1) if len(f) > 1 else m.squeeze()


def gap(v):
    """relative distance between the largest and the second-largest entry of v"""
    top = np.sort(v)[-2:]
    return (top[1] - top[0]) / max(abs(top[1]), 1e-300)


def check_orthogonal(f, csm, h, n_eig, ref):
    m = np.zeros((h.shape[2], len(f)))
    for b in range(len(f)):
        w, v = np.linalg.eigh(csm[b])
        for e in range(n_eig):
            P = np.abs(h[b].conj().T @ v[:, -e - 1]) ** 2
            assert gap(P) > TIE, ("orthogonal near-tie", b, e, gap(P))
            m[np.argmax(P), b] = P[np.argmax(P)] * w[-e - 1]
    assert relmax(integrate(m, f), ref.ravel()) < 1e-9


def check_mvdr(f, csm, h, ref):
    m = np.zeros((h.shape[2], len(f)))
    for b in range(len(f)):
        w, v = np.linalg.eigh(csm[b])
        P = np.abs(h[b].conj().T @ v) ** 2
        m[:, b] = 1 / (P / w).sum(axis=1)
    assert relmax(integrate(m, f), ref.ravel()) < 1e-9


def check_cleansc(f, csm, h, max_it, safety, rm):
    """the argmax of every iteration is clear of a near-tie, and the stopping rule is clear of equality"""
    for b in range(len(f)):
        D = csm[b].copy()
        if rm:
            np.fill_diagonal(D, 0)
        hb = h[b]
        r = np.real(np.einsum("ig,ij,jg->g", hb.conj(), D, hb))
        n_prev, n_cur = 2 * np.linalg.norm(D, 1), np.linalg.norm(D, 1)
        for _ in range(max_it):
            assert gap(r) > TIE, ("cleansc near-tie", b, gap(r))
            i = np.argmax(r)
            p = r[i]
            assert abs(n_cur - n_prev) > 1e-9 * n_prev, "cleansc stopping rule near equality"
            if n_cur >= n_prev:
                break
            w = hb[:, i]
            h_, w2, Dw = w.copy(), np.abs(w) ** 2, D @ w / p
            for _ in range(20):
                H = np.abs(h_) ** 2
                h_ = (Dw + H * w) / np.sqrt(1 + H @ w2)
            G = np.outer(h_, h_.conj()) * p
            if rm:
                np.fill_diagonal(G, 0)
            r -= np.real(np.einsum("ig,ij,jg->g", hb.conj(), G, hb)) * safety
            D = D - safety * G
            n_prev, n_cur = n_cur, np.linalg.norm(D, 1)


def main():
    dsp = import_reference()
    from dsptoolbox.helpers.other import (_get_fractional_octave_bandwidth,
                                          find_nearest_points_index_in_vector)
    from dsptoolbox.standard.enums import SpectrumScaling

    rng = np.random.default_rng(47)
    pts = dict(x=rng.uniform(-0.3, 0.3, N_MICS), y=rng.uniform(-0.3, 0.3, N_MICS), z=np.zeros(N_MICS))
    ma = dsp.beamforming.MicArray(pts)
    n = 1_600  # 24 Welch frames of 128 samples at 50 % overlap: a short estimate, and a full-rank CSM (16 channels)
    sources = [dsp.beamforming.MonopoleSource(dsp.Signal(None, rng.standard_normal(n) * amp, FS), pos)
               for amp, pos in ((1.0, [0.1, -0.12, 0.5]), (0.5, [-0.16, 0.12, 0.5]), (0.25, [0.2, 0.2, 0.5]))]
    s0 = dsp.beamforming.mix_sources_on_array(sources, ma)
    td = s0.time_data + rng.standard_normal(s0.time_data.shape) * 0.05  # sensor noise
    td = td.astype(np.float32)
    g = dsp.beamforming.Regular2DGrid(np.arange(-0.3, 0.3, 0.1), np.arange(-0.3, 0.3, 0.1), ["x", "y"], value3=0.5)
    st = dsp.beamforming.SteeringVector(formulation=dsp.beamforming.SteeringVectorType.TrueLocation)
    classes = dict(mvdr=dsp.beamforming.BeamformerMVDR, functional=dsp.beamforming.BeamformerFunctional,
                   orthogonal=dsp.beamforming.BeamformerOrthogonal, cleansc=dsp.beamforming.BeamformerCleanSC)
    # (method, scaling, centre Hz, octave fraction, keyword arguments)
    combos = []
    for sc in ("PowerSpectralDensity", "FFTBackward"):
        combos += [
            ("mvdr", sc, 2000.0, 3, {}),
            ("mvdr", sc, 1500.0, 0, dict(gamma=3)),
            ("functional", sc, 2000.0, 3, dict(gamma=2.5) if sc == "PowerSpectralDensity" else dict(gamma=4)),
            ("functional", sc, 1500.0, 0, {}),
            ("orthogonal", sc, 2000.0, 3, {}),
            ("orthogonal", sc, 1500.0, 0, dict(number_eigenvalues=3)),
            ("cleansc", sc, 2000.0, 3, {}),
            ("cleansc", sc, 1500.0, 0, dict(maximum_iterations=10, safety_factor=0.8, remove_csm_diagonal=True)),
        ]
    cases, arrs = [], {"time_data": td}
    for i, (method, sc, fc, frac, kw) in enumerate(combos):
        s = dsp.Signal(None, td.astype(np.float64), FS)
        s.set_spectrum_parameters(window_length_samples=WINDOW, scaling=SpectrumScaling[sc])
        f_all, csm_all = s.get_csm()
        bf = classes[method](s, ma, g, st)
        m = bf.get_beamformer_map(fc, frac, **kw)
        ids = find_nearest_points_index_in_vector(_get_fractional_octave_bandwidth(fc, frac), f_all)
        id1, id2 = int(ids[0]), int(ids[1])
        if id1 == id2:
            id2 += 1
        f, csm = f_all[id1:id2], csm_all[id1:id2]
        h = st.get_vector(f * np.pi * 2 / bf.c, grid=g, mic=ma)
        assert np.all(np.isfinite(m)), (method, sc, kw)
        if method == "mvdr":
            check_mvdr(f, csm, h, m)
        elif method == "orthogonal":
            check_orthogonal(f, csm, h, kw.get("number_eigenvalues", N_MICS // 2), m)
        elif method == "cleansc":
            check_cleansc(f, csm, h, kw.get("maximum_iterations", 2 * N_MICS), kw.get("safety_factor", 0.5),
                          kw.get("remove_csm_diagonal", False))
        w = np.linalg.eigvalsh(csm)
        band = f"{id1}_{id2}"  # the steering vectors and CSM slices are stored once per bin range (and scaling)
        arrs[f"f_{band}"], arrs[f"h_{band}"], arrs[f"csm_{sc}_{band}"], arrs[f"map_{i}"] = f, h, csm, m
        cases.append(dict(method=method, scaling=sc, center_hz=fc, octave_fraction=frac, kwargs=kw, band=band,
                          bins=[id1, id2], grid_shape=list(m.shape), n_points=int(g.number_of_points),
                          indefinite=bool((w < 0).any())))
        print(f"{i:2d} {method:10s} {sc:20s} bins {id1}:{id2} {kw} indefinite={cases[-1]['indefinite']}")
    import scipy
    meta = dict(cases=cases, fs=FS, window=WINDOW, n_mics=N_MICS, generator="tools/gen_golden_beamformers.py",
                reference="dsptoolbox 0.8 source", numpy=np.__version__, scipy=scipy.__version__)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrs)
    print(f"beamformers: {os.path.getsize(OUT) / 1024:.1f} KiB, {len(cases)} cases")


if __name__ == "__main__":
    main()
