"""The cases of the structure filters (ds_sfilt: FIR lattice, IIR lattice-ladder, sos lattice-ladder, warped FIR, warped
IIR, Kautz), their oracle results and their bounds.  test_sfilt_host.py checks all of this on the CPU, test_sfilt_gpu.py
holds the kernels to it.

The bound of a case: SFILT_EMULATION holds the worst error of the float64 emulation of the blocked algorithm
(sfilt_oracle.blocked_f64) against the long-double oracle, as a multiple of eps64 times the largest magnitude of the
judged stream (the output of one channel; the final states); the bound is 4 x that x HOST_MARGIN x eps64 -- four for
another equally valid rounding order (the kernels fuse their multiply-adds, numpy does not), a tenth for another host's
numpy.  No bound may exceed 1e-6 (the host test asserts it): a case that cannot meet that is not a valid case.

The sizes sit on the kernels' edges: the block (L = 32 samples a lane), the group (G = L B = 2048 samples a wave) and
4097 samples (three groups, so the carry over groups is crossed twice); D = 1, 2, an odd D, 63 and 64 states (64: one
per lane of the scans; odd: the carry kernel of its own); 1 and 32 sections of the sos lattice; 1 and 3 channels."""

import functools

import numpy as np

import sfilt_oracle as so
from dsptoolbox_amd import backend

# ---- the constants the case list depends on (csrc/carry_tables.hpp, kernels_sfilt.hpp) ------------------------------
L = 32
B = 64
MAX_D = 64
MAX_GAIN = 1.0e6
MAX_GAIN_WARPED_IIR = 30.0

EPS = float(np.finfo(np.float64).eps)
HOST_MARGIN = 1.1
G = L * B
LENGTHS = (1, L - 1, L, L + 1, G - 1, G, G + 1, 2 * G + 1)
KIND_ID = {"fir_lattice": backend.SFILT_FIR_LATTICE, "iir_lattice": backend.SFILT_IIR_LATTICE,
           "sos_lattice": backend.SFILT_SOS_LATTICE, "warped_fir": backend.SFILT_WARPED_FIR,
           "warped_iir": backend.SFILT_WARPED_IIR, "kautz": backend.SFILT_KAUTZ}


# ---- structures by kind and state count ------------------------------------------------------------------------------
def _stable_denominator(order, rng, radius=0.6):
    """A real polynomial 1 + a_1 w + ... of `order` whose roots (in 1 / w) lie within `radius`."""
    n_pairs, single = divmod(order, 2)
    roots = rng.uniform(0.2, radius, n_pairs) * np.exp(1j * rng.uniform(0.1, np.pi - 0.1, n_pairs))
    roots = np.concatenate([roots, np.conj(roots), rng.uniform(-radius, radius, single)])
    return np.real(np.poly(roots)) if order else np.ones(1)


def structure(kind, d, seed=0):
    """A stable structure of `kind` with d states from a fixed seed."""
    rng = np.random.default_rng(1000 * d + seed + sum(map(ord, kind)))
    if kind == "fir_lattice":
        return dict(kind=kind, k=rng.uniform(-0.95, 0.95, d))
    if kind == "iir_lattice":
        k = rng.uniform(-0.9, 0.9, d)
        k[rng.integers(d)] = 0.999
        return dict(kind=kind, k=k, c=rng.standard_normal(d + 1))
    if kind == "sos_lattice":
        assert d % 2 == 0
        k = rng.uniform(-0.9, 0.9, (d // 2, 2))
        c = rng.standard_normal((d // 2, 3)) * 0.5
        c[:, 0] += 1.0
        return dict(kind=kind, k=k, c=c)
    if kind == "warped_fir":
        return dict(kind=kind, lam=0.99 if d == MAX_D else 0.7, b=rng.standard_normal(d))
    if kind == "warped_iir":
        # (the all-pass chain of a long warped IIR filter is far from normal: lambda and the root radius shrink with D so
        # that the carry gain stays under the kernels' limit)
        lam = -0.6 if d < 16 else 0.2
        a = _stable_denominator(d - 1, rng, 0.6 if d < 16 else 0.35)
        b = rng.standard_normal(d) * (1.0 if d < 16 else 0.5 ** np.arange(d))
        return dict(kind=kind, lam=lam, b=b, sigma=so.warped_sigmas(a, lam))
    assert kind == "kautz"
    n_real = d % 2 if d != 2 and d != MAX_D else (0 if d == 2 else 2)
    n_pairs = (d - n_real) // 2
    poles = np.concatenate([rng.uniform(-0.9, 0.9, n_real),
                            rng.uniform(0.5, 0.98, n_pairs) * np.exp(1j * rng.uniform(0.05, np.pi - 0.05, n_pairs))])
    return so.kautz_structure(poles, rng.standard_normal(n_real), rng.standard_normal(2 * n_pairs))


def pack(s):
    """(kind id, packed float64 coefficients, d, aux) of a structure, as include/dsptoolbox_amd.h lays them out."""
    kind, d = s["kind"], so.n_states(s)
    if kind == "fir_lattice":
        coef, aux = s["k"], 0
    elif kind == "iir_lattice":
        coef, aux = np.concatenate([s["k"], s["c"]]), 0
    elif kind == "sos_lattice":
        coef, aux = np.concatenate([s["k"], s["c"]], axis=1).ravel(), 0
    elif kind == "warped_fir":
        coef, aux = np.concatenate([[s["lam"]], s["b"]]), 0
    elif kind == "warped_iir":
        coef, aux = np.concatenate([[s["lam"]], s["b"], s["sigma"]]), len(s["sigma"]) - 1
    else:
        real = np.stack([s["p"], s["g"], s["c"]], axis=1)
        pairs = np.concatenate([s["q"][:, None], s["r"][:, None], s["g2"], s["c2"]], axis=1)
        coef, aux = np.concatenate([real.ravel(), pairs.ravel()]), len(s["p"])
    return KIND_ID[kind], np.ascontiguousarray(coef, dtype=np.float64), d, aux


SMALL_D = {"fir_lattice": 5, "iir_lattice": 5, "sos_lattice": 2, "warped_fir": 5, "warped_iir": 5, "kautz": 5}
EDGE_D = {"fir_lattice": (1, 2, 63, 64), "iir_lattice": (1, 2, 63, 64), "sos_lattice": (64,), "warped_fir": (1, 2, 63, 64),
          "warped_iir": (1, 2, 63, 64), "kautz": (1, 2, 63, 64)}


def _specs():
    s = {}
    for kind in so.KINDS:
        for n in LENGTHS:  # every length at a small D (odd but for the sos lattice, whose K = 1), one channel, from rest
            s[f"{kind}_d{SMALL_D[kind]}_n{n}"] = dict(kind=kind, d=SMALL_D[kind], n=n, n_ch=1, zi=False)
        for d in EDGE_D[kind]:  # the edges of D with a non-zero entry state, three channels, two or three groups
            n = 2 * G + 1 if d in (2, MAX_D) else G + 1
            s[f"{kind}_d{d}_n{n}_zi"] = dict(kind=kind, d=d, n=n, n_ch=3 if d < MAX_D else 1, zi=True)
    return s


CASES = _specs()

# worst error of the float64 emulation / eps64, relative to the stream's peak, per case, as measured on the CPU
SFILT_EMULATION = {
    "fir_lattice_d5_n1": 0.0687, "fir_lattice_d5_n31": 0.679, "fir_lattice_d5_n32": 0.709,
    "fir_lattice_d5_n33": 0.648, "fir_lattice_d5_n2047": 0.918, "fir_lattice_d5_n2048": 0.926,
    "fir_lattice_d5_n2049": 1.04, "fir_lattice_d5_n4097": 0.825, "fir_lattice_d1_n2049_zi": 0.431,
    "fir_lattice_d2_n4097_zi": 0.728, "fir_lattice_d63_n2049_zi": 2.34, "fir_lattice_d64_n4097_zi": 27.2,
    "iir_lattice_d5_n1": 0.614, "iir_lattice_d5_n31": 1.21, "iir_lattice_d5_n32": 2.39, "iir_lattice_d5_n33": 1.73,
    "iir_lattice_d5_n2047": 144, "iir_lattice_d5_n2048": 198, "iir_lattice_d5_n2049": 176,
    "iir_lattice_d5_n4097": 166, "iir_lattice_d1_n2049_zi": 21.1, "iir_lattice_d2_n4097_zi": 74.2,
    "iir_lattice_d63_n2049_zi": 48, "iir_lattice_d64_n4097_zi": 2.13e+03, "sos_lattice_d2_n1": 0.0672,
    "sos_lattice_d2_n31": 0.569, "sos_lattice_d2_n32": 0.647, "sos_lattice_d2_n33": 0.757,
    "sos_lattice_d2_n2047": 0.867, "sos_lattice_d2_n2048": 1.31, "sos_lattice_d2_n2049": 1.65,
    "sos_lattice_d2_n4097": 1.94, "sos_lattice_d64_n4097_zi": 51.1, "warped_fir_d5_n1": 0.247,
    "warped_fir_d5_n31": 1.13, "warped_fir_d5_n32": 1.22, "warped_fir_d5_n33": 1.61, "warped_fir_d5_n2047": 1.54,
    "warped_fir_d5_n2048": 1.3, "warped_fir_d5_n2049": 1.83, "warped_fir_d5_n4097": 1.71,
    "warped_fir_d1_n2049_zi": 0.371, "warped_fir_d2_n4097_zi": 1.12, "warped_fir_d63_n2049_zi": 14.8,
    "warped_fir_d64_n4097_zi": 143, "warped_iir_d5_n1": 1.31, "warped_iir_d5_n31": 2.16, "warped_iir_d5_n32": 1.1,
    "warped_iir_d5_n33": 1.56, "warped_iir_d5_n2047": 3.83, "warped_iir_d5_n2048": 3.54, "warped_iir_d5_n2049": 3.1,
    "warped_iir_d5_n4097": 3.95, "warped_iir_d1_n2049_zi": 0.875, "warped_iir_d2_n4097_zi": 1.2,
    "warped_iir_d63_n2049_zi": 14.5, "warped_iir_d64_n4097_zi": 320, "kautz_d5_n1": 0.956, "kautz_d5_n31": 0.795,
    "kautz_d5_n32": 1.5, "kautz_d5_n33": 0.589, "kautz_d5_n2047": 1.26, "kautz_d5_n2048": 1.14,
    "kautz_d5_n2049": 1.01, "kautz_d5_n4097": 1.07, "kautz_d1_n2049_zi": 0.766, "kautz_d2_n4097_zi": 1.59,
    "kautz_d63_n2049_zi": 5.8, "kautz_d64_n4097_zi": 30.2,
}


def tolerance(name):
    return 4.0 * SFILT_EMULATION[name] * HOST_MARGIN * EPS


@functools.lru_cache(maxsize=None)
def problem(name):
    """(structure, x (N, C), zi (D, C) or None, oracle y (N, C), oracle zf (D, C)) of a case; computed once."""
    spec = CASES[name]
    s = structure(spec["kind"], spec["d"])
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((spec["n"], spec["n_ch"]))
    zi = rng.standard_normal((spec["d"], spec["n_ch"])) if spec["zi"] else None
    y, zf = so.serial(s, x, zi)
    for a in (x, y, zf):
        a.setflags(write=False)
    return s, x, zi, y, zf


def error(name, y, zf):
    """Worst error of a result against the oracle in units of the stream's peak: outputs per channel, the final states
    as one stream."""
    _, _, _, y_ref, zf_ref = problem(name)
    e = so.stream_error(y, y_ref)
    if zf is not None:
        e = max(e, so.stream_error(np.reshape(zf, (-1, 1)), zf_ref.reshape(-1, 1)))
    return e


def emulate(name, **broken):
    s, x, zi, _, _ = problem(name)
    return so.blocked_f64(s, x, zi, L=L, B=B, **broken)


if __name__ == "__main__":  # print the table as it is measured here
    print("SFILT_EMULATION = {")
    for name in CASES:
        s = problem(name)[0]
        print(f'    "{name}": {error(name, *emulate(name)) / EPS:.3g},  # gain {so.carry_gain(s):.3g}', flush=True)
    print("}")
