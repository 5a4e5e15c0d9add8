"""The cases of the complex-coefficient recursion (ds_iir_sos_c128) and of the distance kernels (ds_pair_moments,
ds_fw_snr_seg), their oracle results and their bounds.  test_ciir_host.py / test_distances_host.py check all of this on
the CPU, test_ciir_gpu.py / test_distances_gpu.py hold the kernels to it.

The bound of a recursion case: CIIR_EMULATION holds the worst error of the float64 emulation of the blocked
algorithm (ciir_oracle.blocked_f64) against the clongdouble oracle, as a multiple of eps64 times the largest
magnitude of the judged stream (the output of one filter on one channel; the final states of one filter); the bound
is 4 x that x HOST_MARGIN x eps64 -- four for another equally valid rounding order (the kernels fuse their
multiply-adds, numpy does not), a tenth for another host's numpy.  The same rule gives the bounds of snr and si_sdr
from the emulation of the reduction's summation order (PAIR_EMULATION, in dB).

The bound of a segmental-SNR case: the device's transform is the any-length float64 transform whose GPU tests assert
1e-9 of a column's largest magnitude for every length (tests/test_phase_gpu.py: TOL).  FW_PERTURBED holds the change
of the oracle's result in dB when every frame spectrum is moved by that much; the bound is 4 x that x HOST_MARGIN.

The sizes sit on the kernels' edges, which depend on the constants mirrored below (the host test reads them out of
the sources and fails when they differ)."""

import functools

import numpy as np

import ciir_oracle as co
import dsptoolbox_amd as dsp

# ---- the constants the case list depends on (csrc/carry_tables.hpp, kernels_ciir.hpp, kernels_dist.hpp) --------------
L = 32
B = 64
CIIR_MAX_SEC = 16
PAIR_NT = 256          # workgroup width of the reductions
PAIR_SPAN = 4096       # samples per workgroup of k_pair_partial
FFT_TOL = 1e-9         # tests/test_phase_gpu.py: TOL

EPS = float(np.finfo(np.float64).eps)
HOST_MARGIN = 1.1
G = L * B
LENGTHS = (1, L - 1, L, L + 1, G - 1, G, G + 1, 2 * G + 1)


# ---- the recursion ----------------------------------------------------------------------------------------------------------
def one_pole(radius, angle, gain=1.0):
    return np.array([[gain, 0, 0, 1, -radius * np.exp(1j * angle), 0]], dtype=np.complex128)


def general_sections(n_sec, seed):
    """n_sec complex biquads with two distinct poles each, radii in [0.5, 0.95], and complex numerators."""
    rng = np.random.default_rng(seed)
    sos = np.zeros((n_sec, 6), dtype=np.complex128)
    for k in range(n_sec):
        p = rng.uniform(0.5, 0.95, 2) * np.exp(1j * rng.uniform(-np.pi, np.pi, 2))
        sos[k, :3] = (rng.standard_normal(3) + 1j * rng.standard_normal(3)) * 0.3
        sos[k, 3:] = (1.7 - 0.4j) * np.array([1.0, -(p[0] + p[1]), p[0] * p[1]])  # (a0 != 1: the rows are divided by it)
    return sos


def gammatone_sos(f_range, fs):
    return np.stack([f.sos for f in dsp.filterbanks.auditory_filters_gammatone(f_range, 1, fs).filters])


def _recursion_specs():
    s = {}
    near0, quarter, near_pi = 0.01, np.pi / 2 + 0.003, np.pi - 0.01
    for n in LENGTHS:
        s[f"one_pole_near0_n{n}"] = dict(sos=one_pole(0.9999, near0)[None], n=n, n_ch=1, zi=False)
    for n in (L + 1, 2 * G + 1):
        s[f"two_poles_n{n}_zi"] = dict(sos=np.stack([one_pole(0.9999, quarter), one_pole(0.9999, near_pi, 0.5j)]), n=n, n_ch=3,
                                       zi=True)
    s["gammatone23_n2049"] = dict(sos=gammatone_sos([100, 3500], 8000), n=G + 1, n_ch=3, zi=False)
    s["gammatone23_n4097_zi"] = dict(sos=gammatone_sos([100, 3500], 8000), n=2 * G + 1, n_ch=1, zi=True)
    for n, zi in ((L - 1, True), (G, False), (2 * G + 1, True)):
        s[f"max_sections_n{n}{'_zi' if zi else ''}"] = dict(sos=general_sections(CIIR_MAX_SEC, 5)[None], n=n, n_ch=1, zi=zi)
    return s


RECURSION = _recursion_specs()

# worst error of the float64 emulation / eps64, relative to the stream's peak, per case, as measured on the CPU
CIIR_EMULATION = {
    "one_pole_near0_n1": 0.325, "one_pole_near0_n31": 0.705, "one_pole_near0_n32": 0.679, "one_pole_near0_n33": 0.371,
    "one_pole_near0_n2047": 141, "one_pole_near0_n2048": 115, "one_pole_near0_n2049": 142, "one_pole_near0_n4097": 192,
    "two_poles_n33_zi": 2.88, "two_poles_n4097_zi": 348, "gammatone23_n2049": 14.4, "gammatone23_n4097_zi": 8.87,
    "max_sections_n31_zi": 1.4, "max_sections_n2048": 13.7, "max_sections_n4097_zi": 6.28,
}


def recursion_tolerance(name):
    return 4.0 * CIIR_EMULATION[name] * HOST_MARGIN * EPS


@functools.lru_cache(maxsize=None)
def recursion_problem(name):
    """(x (N, C), zi (F, K, 2, C) or None, oracle y (F, N, C), oracle zf (F, K, 2, C)) of a case; computed once."""
    spec = RECURSION[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((spec["n"], spec["n_ch"]))
    sos = spec["sos"]
    zi = None
    if spec["zi"]:
        shape = (sos.shape[0], sos.shape[1], 2, spec["n_ch"])
        zi = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    y, zf = co.bank_ld(sos, x, zi)
    for a in (x, y, zf):
        a.setflags(write=False)
    return x, zi, y, zf


def recursion_error(name, y, zf):
    """Worst error of a result against the oracle in units of the stream's peak: outputs per (filter, channel), final
    states per filter."""
    _, _, y_ref, zf_ref = recursion_problem(name)
    e = max(co.stream_error(y[f], y_ref[f]) for f in range(len(y_ref)))
    if zf is not None:
        e = max(e, max(co.stream_error(zf[f].reshape(-1, 1), zf_ref[f].reshape(-1, 1)) for f in range(len(zf_ref))))
    return e


def emulate_recursion(name, **broken):
    x, zi, _, _ = recursion_problem(name)
    sos = RECURSION[name]["sos"]
    out = [co.blocked_f64(sos[f], x, None if zi is None else zi[f], L=L, B=B, **broken) for f in range(len(sos))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- snr and si_sdr -----------------------------------------------------------------------------------------------------------
PAIR_LENGTHS = (1, 63, 64, 65, PAIR_SPAN + 1)


@functools.lru_cache(maxsize=None)
def pair_problem(name):
    """name: 'n<length>' (three channels against three), 'broadcast' (one against three), 'cancel' (shat = 0.999 s +
    1e-9 noise).  -> (s, shat)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "cancel":
        s = rng.standard_normal((1000, 2)) + 0.5
        out = s, 0.999 * s + 1e-9 * rng.standard_normal(s.shape)
    elif name == "broadcast":
        s = rng.standard_normal((700, 1))
        out = s, s + 0.3 * rng.standard_normal((700, 3))
    else:
        n = int(name[1:])
        s = rng.standard_normal((n, 3)) + 0.25
        out = s, 0.8 * s + 0.3 * rng.standard_normal((n, 3))
    for a in out:
        a.setflags(write=False)
    return out


PAIR_CASES = tuple(f"n{n}" for n in PAIR_LENGTHS) + ("broadcast", "cancel")
# the cases whose dB values are judged: at one sample the standard deviations are zero and si_sdr's residual is rounding
# noise, in the reference too -- there the sums themselves are judged (each is ONE rounded product: 2 eps64)
PAIR_JUDGED = PAIR_CASES[1:]
# worst error of the emulated summation order against the long double oracle, in dB, per case and function
PAIR_EMULATION = {
    ("n63", "si_sdr"): 1.67e-15, ("n63", "snr"): 9.44e-16, ("n64", "si_sdr"): 2.21e-15, ("n64", "snr"): 1.53e-15,
    ("n65", "si_sdr"): 1.54e-15, ("n65", "snr"): 1.47e-15, ("n4097", "si_sdr"): 1.26e-15, ("n4097", "snr"): 1.89e-15,
    ("broadcast", "si_sdr"): 9.51e-16, ("broadcast", "snr"): 5.94e-16, ("cancel", "si_sdr"): 5.65e-09,
    ("cancel", "snr"): 7.49e-16,
}


def pair_tolerance(name, fn):
    return 4.0 * PAIR_EMULATION[(name, fn)] * HOST_MARGIN


def emulate_si_sdr(s, shat):
    out = np.empty(shat.shape[1])
    for c in range(shat.shape[1]):
        a = s[:, 0 if s.shape[1] == 1 else c]
        m = co.pair_sums_f64(a, shat[:, c], (0.0, 0.0, 0.0), PAIR_NT, PAIR_SPAN // PAIR_NT)
        alpha = m[2] / m[0]
        r = co.pair_sums_f64(a, shat[:, c], (alpha, 0.0, 0.0), PAIR_NT, PAIR_SPAN // PAIR_NT)
        out[c] = 10 * np.log10(alpha ** 2 * m[0] / r[5])
    return out


def emulate_snr(s, noise):
    out = np.empty(s.shape[1])
    n = len(s)
    for c in range(s.shape[1]):
        b = noise[:, 0 if noise.shape[1] == 1 else c]
        m = co.pair_sums_f64(s[:, c], b, (0.0, 0.0, 0.0), PAIR_NT, PAIR_SPAN // PAIR_NT)
        m = co.pair_sums_f64(s[:, c], b, (0.0, m[3] / n, m[4] / n), PAIR_NT, PAIR_SPAN // PAIR_NT)
        out[c] = 20 * np.log10(np.sqrt(m[0] / n) / np.sqrt(m[1] / n))
    return out


# ---- the segmental SNR ------------------------------------------------------------------------------------------------------
def window_length(fs):
    lw = int(75e-3 * fs)
    return lw + lw % 2


def _fw_specs():
    s = {}
    w8 = window_length(8000)
    # rate -> window -> transform: 6827 -> 512 (LDS radix-2), 8000 -> 600 (Bluestein, M = 2048), 48000 -> 3600 (Bluestein,
    # M = 8192), 8014 -> 601 rounded up to 602
    s["fs6827"] = dict(fs=6827, n=512 + 1, f_range=[100, 3000], ch=(1, 1))
    for n in (w8, w8 + 1, 2 * w8, 2 * w8 + 1):
        s[f"fs8000_n{n}"] = dict(fs=8000, n=n, f_range=[100, 3500], ch=(1, 1))
    s["fs8000_long"] = dict(fs=8000, n=5000, f_range=[100, 3500], ch=(2, 2))
    s["fs48000"] = dict(fs=48000, n=2 * 3600 + 1, f_range=[20, 20000], ch=(1, 1))
    s["fs8014"] = dict(fs=8014, n=602 + 1, f_range=[100, 3500], ch=(1, 1))
    s["one_band"] = dict(fs=8000, n=w8 + 1, f_range=[950, 1050], ch=(1, 1))
    s["one_against_three"] = dict(fs=8000, n=w8 + 1, f_range=[100, 3500], ch=(1, 3))
    for g in (0.1, 2):
        s[f"gamma{g}"] = dict(fs=8000, n=w8 + 1, f_range=[100, 3500], ch=(1, 1), gamma=g)
    # the input of fs8000_long under a range that its frames leave on both sides
    s["both_clips"] = dict(fs=8000, n=5000, f_range=[100, 3500], ch=(2, 2), snr_range=[12, 18], judged_inside=False,
                           input_of="fs8000_long")
    return s


FW = _fw_specs()
# change of the oracle's result, in dB, when every frame spectrum moves by FFT_TOL of its largest magnitude
FW_PERTURBED = {
    "fs6827": 1.62e-06, "fs8000_n600": 2.01e-05, "fs8000_n601": 7.31e-05, "fs8000_n1200": 0.00128,
    "fs8000_n1201": 0.000158, "fs8000_long": 0.000147, "fs48000": 6.14e-05, "fs8014": 9.13e-06, "one_band": 2.57e-05,
    "one_against_three": 2.28e-05, "gamma0.1": 3.34e-06, "gamma2": 7.35e-08, "both_clips": 9.2e-05,
}


def fw_tolerance(name):
    return 4.0 * FW_PERTURBED[name] * HOST_MARGIN


@functools.lru_cache(maxsize=None)
def fw_problem(name):
    """-> (x (N, Cx), xhat (N, C), per channel the oracle's unclipped frame values, the oracle's result (C,), the
    perturbed oracle's result (C,)).  Broadband inputs: a chirp plus noise on channel 0, noise on the others;
    xhat = x + 0.3 noise."""
    from scipy.signal import windows
    spec = FW[name]
    fs, n = spec["fs"], spec["n"]
    rng = np.random.default_rng(sum(map(ord, spec.get("input_of", name))))
    t = np.arange(n) / fs
    n_cx, n_c = spec["ch"]
    x = rng.standard_normal((n, n_cx))
    x[:, 0] = np.sin(2 * np.pi * (0.03 * fs * t + 0.5 * 0.4 * fs / max(t[-1], 1 / fs) * t ** 2)) + 0.1 * x[:, 0]
    xhat = x[:, [0] * n_c if n_cx == 1 else slice(None)] + 0.3 * rng.standard_normal((n, n_c))
    sos = gammatone_sos(np.sort(spec["f_range"]), fs)
    xb = co.bank_ld(sos, x)[0].real    # (bands, N, Cx)
    xhb = co.bank_ld(sos, xhat)[0].real
    window = windows.hamming(window_length(fs), sym=False)
    rng_db, gamma = spec.get("snr_range", [-10, 35]), spec.get("gamma", 0.2)
    frames, value, moved = [], np.empty(n_c), np.empty(n_c)
    for c in range(n_c):
        a, b = xb[:, :, 0 if n_cx == 1 else c].T, xhb[:, :, c].T
        f, v = co.fw_frames_ld(a, b, window, rng_db, gamma)
        frames.append(np.asarray(f, dtype=np.float64))
        value[c] = v
        moved[c] = co.fw_frames_ld(a, b, window, rng_db, gamma, perturb=FFT_TOL, seed=c)[1]
    for a_ in (x, xhat, value, moved):
        a_.setflags(write=False)
    return x, xhat, frames, value, moved


def fw_call(name, x, xhat):
    """distances.fw_snr_seg with the case's parameters."""
    spec = FW[name]
    fs = spec["fs"]
    mk = lambda a: dsp.Signal(None, np.array(a), fs, constrain_amplitude=False)
    return dsp.distances.fw_snr_seg(mk(x), mk(xhat), f_range_hz=spec["f_range"], snr_range_db=spec.get("snr_range", [-10, 35]),
                                    gamma=spec.get("gamma", 0.2))


if __name__ == "__main__":  # print the tables as they are measured here
    print("CIIR_EMULATION = {")
    for name in RECURSION:
        print(f'    "{name}": {recursion_error(name, *emulate_recursion(name)) / EPS:.3g},')
    print("}\nPAIR_EMULATION = {")
    for name in PAIR_JUDGED:
        s, h = pair_problem(name)
        print(f'    ("{name}", "si_sdr"): {np.max(np.abs(emulate_si_sdr(s, h) - co.si_sdr_ld(s, h))):.3g},')
        print(f'    ("{name}", "snr"): {np.max(np.abs(emulate_snr(h, s) - co.snr_ld(h, s))):.3g},')
    print("}\nFW_PERTURBED = {")
    for name in FW:
        _, _, frames, value, moved = fw_problem(name)
        print(f'    "{name}": {np.max(np.abs(moved - value)):.3g},  # frames {[np.round(f, 1).tolist() for f in frames]}')
    print("}")
