"""The cases of the realtime filters (ds_rtfilt: state-variable, transposed direct form II, parallel sections, state space;
ds_rtfir: the direct FIR sum), their oracle results and their bounds.  test_rtfilt_host.py checks all of this on the CPU,
test_rtfilt_gpu.py holds the kernels to it.

The bound of a recursion case, by the rule of sfilt_cases.py: RTFILT_EMULATION holds the worst error of the float64
emulation of the blocked algorithm (rtfilt_oracle.blocked_f64) against the long-double oracle, as a multiple of eps64 times
the largest magnitude of the judged stream (the output of one channel in one band; the final states); the bound is 4 x that
x HOST_MARGIN x eps64 -- four for another equally valid rounding order (the kernels fuse their multiply-adds, numpy does
not), a tenth for another host's numpy.  No bound may exceed 1e-6 (the host test asserts it).

The bound of an FIR case is the forward error bound of its float64 dot product, per element:
(order + 1) eps64 sum_i |b_i| |x[n - i]|.

The sizes sit on the kernels' edges: the block (L = 32 samples a lane), the group (G = L B = 2048 samples a wave) and 4097
samples (three groups, so the carry over groups is crossed twice); D = 1, 2, an odd D, 63 and 64 states; 1 and 32 parallel
sections with the delays 0, 1, 33 (past a block) and 2049 (past a group), with and without the FIR part; 1 and 3 channels;
FIR orders 0, 1, 31, 32, 63 and 4095 around the FIR tile of 1024 samples, with and without an entry history."""

import functools

import numpy as np
from scipy.signal import tf2ss

import rtfilt_oracle as ro
from dsptoolbox_amd import backend

# ---- the constants the case list depends on (csrc/carry_tables.hpp, kernels_rtfilt.hpp) -----------------------------
L = 32
B = 64
MAX_D = 64
MAX_GAIN = 1.0e6
MAX_GAIN_COMPANION = 30.0
FIR_TILE = 1024
FIR_MAX_TAPS = 4096

EPS = float(np.finfo(np.float64).eps)
HOST_MARGIN = 1.1
G = L * B
LENGTHS = (1, L - 1, L, L + 1, G - 1, G, G + 1, 2 * G + 1)
KIND_ID = {"svf": backend.RTFILT_SVF, "tdf2": backend.RTFILT_TDF2, "parallel": backend.RTFILT_PARALLEL,
           "state_space": backend.RTFILT_STATE_SPACE}


# ---- filters by kind and state count ---------------------------------------------------------------------------------
def _ba(d, rng):
    """b, a of order d, a[0] = 1, stable; the root radius shrinks until the carry gain of the companion recursion is
    under half the limit (the transposed direct form and tf2ss's form of a long filter are far from normal)."""
    n_pairs, single = divmod(d, 2)
    frac = rng.uniform(0.3, 1.0, n_pairs) * np.exp(1j * rng.uniform(0.1, np.pi - 0.1, n_pairs))
    frac1 = rng.uniform(-1.0, 1.0, single)
    b = rng.standard_normal(d + 1) * (1.0 if d < 16 else 0.5 ** np.arange(d + 1))
    for radius in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2):
        roots = radius * np.concatenate([frac, np.conj(frac), frac1])
        a = np.real(np.poly(roots))
        if ro.carry_gain(dict(kind="tdf2", b=b, a=a)) <= MAX_GAIN_COMPANION / 2:
            return b, a
    raise AssertionError("no stable denominator under the gain limit")


def structure(kind, d, seed=0, delay=0, fir=False):
    """A stable filter of `kind` with d states from a fixed seed."""
    rng = np.random.default_rng(1000 * d + seed + sum(map(ord, kind)))
    if kind == "svf":
        return ro.svf_structure(1500.0, 0.4, 48000)
    if kind == "tdf2":
        b, a = _ba(d, rng)
        return dict(kind=kind, b=b, a=a)
    if kind == "parallel":
        n_sec = d // 2
        p = rng.uniform(0.5, 0.98, n_sec) * np.exp(1j * rng.uniform(0.05, np.pi - 0.05, n_sec))
        sos = np.stack([rng.standard_normal(n_sec), rng.standard_normal(n_sec), 0.5 * rng.standard_normal(n_sec),
                        -2.0 * p.real, np.abs(p) ** 2], axis=1)
        return dict(kind=kind, sos=sos, delay=int(delay), fir=rng.standard_normal(7) if fir else None)
    assert kind == "state_space"
    if d < 16:  # tf2ss's controller-canonical form, as StateSpaceFilter.from_filter builds it
        A, Bm, C, D = tf2ss(*_ba(d, rng))
        return dict(kind=kind, A=A, B=Bm[:, 0], C=C[0], Dd=float(D[0, 0]))
    # a dense normal A: an orthogonal similarity of rotation-scaling blocks of radius below 1
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    blocks = np.zeros((d, d))
    for i in range(0, d - 1, 2):
        r, th = rng.uniform(0.5, 0.95), rng.uniform(0.05, np.pi - 0.05)
        blocks[i:i + 2, i:i + 2] = r * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    if d % 2:
        blocks[-1, -1] = rng.uniform(-0.9, 0.9)
    return dict(kind=kind, A=q @ blocks @ q.T, B=rng.standard_normal(d), C=rng.standard_normal(d),
                Dd=float(rng.standard_normal()))


def pack(s):
    """(kind id, packed float64 coefficients, d, aux, delay, fir) of a filter, as include/dsptoolbox_amd.h lays them out."""
    kind, d = s["kind"], ro.n_states(s)
    aux, delay, fir = 0, 0, None
    if kind == "svf":
        coef = np.array([s["g"], s["r"], s["h"]])
    elif kind == "tdf2":
        coef = np.concatenate([s["b"], s["a"]])
    elif kind == "parallel":
        coef, aux, delay, fir = np.ravel(s["sos"]), len(s["sos"]), int(s["delay"]), s["fir"]
    else:
        coef = np.concatenate([np.ravel(s["A"]), s["B"], s["C"], [s["Dd"]]])
    return KIND_ID[kind], np.ascontiguousarray(coef, dtype=np.float64), d, aux, delay, fir


def unpack(kind_id, coef, d, aux, delay=0, fir=None):
    """The filter dict of packed coefficients (the inverse of pack)."""
    coef = np.asarray(coef, dtype=np.float64)
    if kind_id == backend.RTFILT_SVF:
        return dict(kind="svf", g=coef[0], r=coef[1], h=coef[2])
    if kind_id == backend.RTFILT_TDF2:
        return dict(kind="tdf2", b=coef[:d + 1], a=coef[d + 1:])
    if kind_id == backend.RTFILT_PARALLEL:
        return dict(kind="parallel", sos=coef.reshape(aux, 5), delay=int(delay), fir=fir)
    return dict(kind="state_space", A=coef[:d * d].reshape(d, d), B=coef[d * d:d * d + d], C=coef[d * d + d:d * d + 2 * d],
                Dd=coef[-1])


SMALL_D = {"svf": 2, "tdf2": 5, "parallel": 2, "state_space": 5}
EDGE_D = {"svf": (), "tdf2": (1, 2, 63, 64), "parallel": (), "state_space": (1, 2, 63, 64)}
DELAYS = (0, 1, L + 1, G + 1)


def _specs():
    s = {}
    for kind in ro.KINDS:
        for n in LENGTHS:  # every length at a small D (odd where the kind has one), one channel, from rest
            s[f"{kind}_d{SMALL_D[kind]}_n{n}"] = dict(kind=kind, d=SMALL_D[kind], n=n, n_ch=1, zi=False)
        for d in EDGE_D[kind]:  # the edges of D with a non-zero entry state, three channels, two or three groups
            n = 2 * G + 1 if d in (2, MAX_D) else G + 1
            s[f"{kind}_d{d}_n{n}_zi"] = dict(kind=kind, d=d, n=n, n_ch=3 if d < MAX_D else 1, zi=True)
    for n in (G + 1, 2 * G + 1):  # the four bands from an entry state, three channels
        s[f"svf_d2_n{n}_zi"] = dict(kind="svf", d=2, n=n, n_ch=3, zi=True)
    for n_sec in (1, 32):  # 1 and 32 sections, every delay, with and without the FIR part; an entry state where the
        for delay in DELAYS:  # delay line is empty (the delayed input is no state)
            for fir in (False, True):
                name = f"parallel_d{2 * n_sec}_n{2 * G + 1}_delay{delay}" + ("_fir" if fir else "") + ("_zi" if not delay else "")
                s[name] = dict(kind="parallel", d=2 * n_sec, n=2 * G + 1, n_ch=3 if n_sec == 1 else 1, zi=not delay,
                               delay=delay, fir=fir)
    return s


CASES = _specs()

# worst error of the float64 emulation / eps64, relative to the stream's peak, per case, as measured on the CPU
RTFILT_EMULATION = {
    "svf_d2_n1": 0.282, "svf_d2_n31": 1.6, "svf_d2_n32": 1.86, "svf_d2_n33": 2.8, "svf_d2_n2047": 3.3,
    "svf_d2_n2048": 2.03, "svf_d2_n2049": 2.37, "svf_d2_n4097": 3.91, "svf_d2_n2049_zi": 4.41, "svf_d2_n4097_zi": 2.23,
    "tdf2_d5_n1": 0.589, "tdf2_d5_n31": 11, "tdf2_d5_n32": 4.43, "tdf2_d5_n33": 10.9, "tdf2_d5_n2047": 14.3,
    "tdf2_d5_n2048": 16.3, "tdf2_d5_n2049": 10.7, "tdf2_d5_n4097": 13.8, "tdf2_d1_n2049_zi": 0.885,
    "tdf2_d2_n4097_zi": 2.47, "tdf2_d63_n2049_zi": 165, "tdf2_d64_n4097_zi": 191,
    "parallel_d2_n1": 0.0405, "parallel_d2_n31": 0.532, "parallel_d2_n32": 0.763, "parallel_d2_n33": 0.696,
    "parallel_d2_n2047": 0.923, "parallel_d2_n2048": 0.664, "parallel_d2_n2049": 1.14, "parallel_d2_n4097": 1.04,
    "state_space_d5_n1": 0.0523, "state_space_d5_n31": 2.19, "state_space_d5_n32": 8.4, "state_space_d5_n33": 2.36,
    "state_space_d5_n2047": 4.13, "state_space_d5_n2048": 4.18, "state_space_d5_n2049": 8.69, "state_space_d5_n4097": 4.97,
    "state_space_d1_n2049_zi": 0.69, "state_space_d2_n4097_zi": 0.863, "state_space_d63_n2049_zi": 4.08,
    "state_space_d64_n4097_zi": 2.65,
    "parallel_d2_n4097_delay0_zi": 1.17, "parallel_d2_n4097_delay0_fir_zi": 0.924, "parallel_d2_n4097_delay1": 1.14,
    "parallel_d2_n4097_delay1_fir": 1.1, "parallel_d2_n4097_delay33": 0.928, "parallel_d2_n4097_delay33_fir": 0.966,
    "parallel_d2_n4097_delay2049": 1.26, "parallel_d2_n4097_delay2049_fir": 0.921,
    "parallel_d64_n4097_delay0_zi": 19, "parallel_d64_n4097_delay0_fir_zi": 13.8, "parallel_d64_n4097_delay1": 54.8,
    "parallel_d64_n4097_delay1_fir": 30.6, "parallel_d64_n4097_delay33": 12.9, "parallel_d64_n4097_delay33_fir": 13,
    "parallel_d64_n4097_delay2049": 13.6, "parallel_d64_n4097_delay2049_fir": 11.6,
}


def tolerance(name):
    return 4.0 * RTFILT_EMULATION[name] * HOST_MARGIN * EPS


@functools.lru_cache(maxsize=None)
def problem(name):
    """(filter, x (N, C), zi (D, C) or None, oracle y (N, C) or (4, N, C), oracle zf (D, C)) of a case; computed once."""
    spec = CASES[name]
    s = structure(spec["kind"], spec["d"], delay=spec.get("delay", 0), fir=spec.get("fir", False))
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((spec["n"], spec["n_ch"]))
    zi = rng.standard_normal((spec["d"], spec["n_ch"])) if spec["zi"] else None
    y, zf = ro.serial(s, x, zi)
    for a in (x, y, zf):
        a.setflags(write=False)
    return s, x, zi, y, zf


def error(name, y, zf):
    """Worst error of a result against the oracle in units of the stream's peak: outputs per channel and band, the final
    states as one stream."""
    _, _, _, y_ref, zf_ref = problem(name)
    e = ro.stream_error(y, y_ref)
    if zf is not None:
        e = max(e, ro.stream_error(np.reshape(zf, (-1, 1)), zf_ref.reshape(-1, 1)))
    return e


def emulate(name, **broken):
    s, x, zi, _, _ = problem(name)
    return ro.blocked_f64(s, x, zi, L=L, B=B, **broken)


# ---- the direct FIR sum ----------------------------------------------------------------------------------------------
def _fir_specs():
    s = {}
    for order, n in ((0, 1), (0, FIR_TILE + 1), (1, FIR_TILE), (31, FIR_TILE - 1), (32, 2 * FIR_TILE + 1), (63, 33),
                     (FIR_MAX_TAPS - 1, 1), (FIR_MAX_TAPS - 1, FIR_TILE + 1)):
        for hist in (False, True):
            if order or not hist:
                s[f"fir_o{order}_n{n}" + ("_hist" if hist else "")] = dict(order=order, n=n, n_ch=3 if order < 64 else 1,
                                                                           hist=hist)
    return s


FIR_CASES = _fir_specs()


@functools.lru_cache(maxsize=None)
def fir_problem(name):
    """(b, x (N, C), hist (C, order) or None, oracle y (N, C), the bound per element (N, C)) of an FIR case."""
    spec = FIR_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    b = rng.standard_normal(spec["order"] + 1)
    x = rng.standard_normal((spec["n"], spec["n_ch"]))
    hist = rng.standard_normal((spec["n_ch"], spec["order"])) if spec["hist"] else None
    y = ro.fir_direct(b, x, hist)
    bound = (spec["order"] + 1) * EPS * ro.fir_direct(np.abs(b), np.abs(x), None if hist is None else np.abs(hist))
    for a in (b, x, y, bound):
        a.setflags(write=False)
    return b, x, hist, y, bound.astype(np.float64)


if __name__ == "__main__":  # print the table as it is measured here
    print("RTFILT_EMULATION = {")
    for name in CASES:
        s = problem(name)[0]
        print(f'    "{name}": {error(name, *emulate(name)) / EPS:.3g},  # gain {ro.carry_gain(s):.3g}', flush=True)
    print("}")
