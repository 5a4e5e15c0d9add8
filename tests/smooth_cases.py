"""The cases of the smoothing sweep (tests/test_smooth_sweep_host.py, tests/test_smooth_sweep_gpu.py): the tile constants
of csrc/kernels_smooth.hpp restated, the data, axes and windows the tests draw, the case lists, each case's long-double
oracle with its bound (tests/smooth_oracle.py) and a float64 numpy emulation of every entry that can be made subtly wrong
in thirteen ways (FAULTS: the clamp can be wrong at either end).  Pure numpy / scipy, no device.

Families, by the name's head:
  bins      k_smooth alone (ds_octave_smooth, k_log None): every channel-group width tc as a partial group at n_bins on
            both sides of one lane's R bins, of one tile TB(tc) and of two tiles; windows of 9 and 8 taps; full groups
            and a second group once each at TB + 1
  window    k_smooth alone at TB + 1 bins: window lengths on both sides of R, of one chunk CH(tc) and of two chunks, and
            one window longer than twice the data
  interp    k_to_log and k_to_lin alone (a one-tap window makes k_smooth the identity, bit for bit): data that reaches
            every branch of the PCHIP rules, on four axes
  pipeline  backend.fractional_octave_smoothing on the standard axis, with and without the clip
  gdelay    k_unwrap through backend.group_delay_phase: a unit impulse at sample d has the phase -2 pi k d / n, whose
            steps the unwrap leaves alone (d < n / 2) or corrects one and all (d > n / 2)
  complex   k_polar, k_unwrap, k_smooth, k_clip, k_recombine through backend.smooth_complex_spectrum

Every window is rng.random(L) + 0.1, end taps included, except in the complex family, whose entry builds its window
from a name: "hamming" there (end taps 0.08; "hann" has none).

SMOOTH_EMULATION records the emulation's worst error / bound per family as measured on the CPU; the host test holds every
case to a quarter of its bound, which leaves the device room for another summation order and FMA."""

import functools
import zlib

import numpy as np
from scipy.interpolate import PchipInterpolator

import fft64_cases as fc
import smooth_oracle as so
from dsptoolbox_amd import backend

LD = so.LD

# ---- csrc/kernels_smooth.hpp ---------------------------------------------------------------------------------------------
NT, R, MAX_TC, LDS_DOUBLES = 256, 8, 16, 4096
UNWRAP_LANE = 8                 # consecutive bins per lane of k_unwrap (its E)
UNWRAP_TILE = NT * UNWRAP_LANE  # bins per pass of its one workgroup: 2048


def TB(tc: int) -> int:
    """output bins of one k_smooth workgroup"""
    return NT // tc * R


def CH(tc: int) -> int:
    """window taps per staged chunk"""
    return LDS_DOUBLES // tc - TB(tc) + 1


def tc_of(n_ch: int) -> int:
    """smooth_run's channel-group width"""
    tc = 1
    while tc < MAX_TC and tc < n_ch:
        tc *= 2
    return tc


PARTIAL = {1: 1, 2: 2, 4: 3, 8: 5, 16: 9}  # tc -> a channel count that leaves its group partial (tc = 1, 2: full)

SMOOTH_EMULATION = {"bins": 0.0858, "window": 0.128, "interp": 0.193, "pipeline": 0.0195, "gdelay": 0.0216, "complex": 0.0575}


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def window_taps(rng, L: int) -> np.ndarray:
    return rng.random(L) + 0.1


# ---- case lists -----------------------------------------------------------------------------------------------------------
def bins_cases():
    out = []
    for n_ch in PARTIAL.values():
        tb = TB(tc_of(n_ch))
        for n_bins in (1, 2, 7, 8, 9, tb - 1, tb, tb + 1, 2 * tb + 1):
            for L in (9, 8):
                out.append(f"bins-C{n_ch}-N{n_bins}-L{L}")
    for n_ch in (4, 8, 16, 17):
        out.append(f"bins-C{n_ch}-N{TB(tc_of(n_ch)) + 1}-L9")
    return out


CLAMPED = "window-C3-N33-L71"  # every row clamped at both ends


def window_cases():
    out = []
    for tc, n_ch in PARTIAL.items():
        ch = CH(tc)
        for L in (1, 2, 7, 8, 9, ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1):
            out.append(f"window-C{n_ch}-N{TB(tc) + 1}-L{L}")
    return out + [CLAMPED]


INTERP_NS = (2, 3, 4, 5, 255, 256, 257, 1000)
INTERP_CHANNELS = (1, 3)
INTERP_DATA = ("noise", "flat", "ramp", "alternating", "zero", "edgeA", "edgeB", "edgeC")
INTERP_AXES = ("standard", "identity", "uniform", "top")


def interp_cases():
    return [f"interp-N{n}-C{c}-{d}-{a}" for n in INTERP_NS for c in INTERP_CHANNELS for d in INTERP_DATA
            for a in INTERP_AXES]


def pipeline_cases():
    return [f"pipeline-N{n}-C{c}-F{f}-{clip}" for n in (2049, 4097) for c in (2, 5) for f in (1, 3)
            for clip in ("plain", "clip")]


GDELAY_NS = (4094, 4096, 4098, 8194)


def gdelay_delays(n: int) -> tuple:
    return (1, n // 4, n // 2 - 1, n // 2 + 1, 3 * n // 4, n - 1)


def gdelay_cases():
    out = []
    for n in GDELAY_NS:
        out += [f"gdelay-n{n}-C1-d{i}" for i in range(6)]
        out += [f"gdelay-n{n}-C3-d{i}" for i in (0, 3)]  # three channels: the delays i, i + 1, i + 2 of gdelay_delays
    return out


COMPLEX_BINS = 4100
STEP_BINS = (7, 8, 9, 2047, 2048, 2049, 4096)
COMPLEX_CASES = ("complex-steps-L1", "complex-steps-L9", "complex-axis-L1", "complex-axis-L9", "complex-clip-L9")
COMPLEX_SPACING = {1: 1.0, 9: 1.0 / 9.0}  # bin spacing in octaves at num_fractions = 1 -> window taps
MARGIN = 1e-6                             # every step of the "steps" spectra keeps this distance from +-pi


def all_cases():
    return bins_cases() + window_cases() + interp_cases() + pipeline_cases() + gdelay_cases() + list(COMPLEX_CASES)


def family(name: str) -> str:
    return name.split("-")[0]


def _fields(name: str) -> dict:
    out = {}
    for part in name.split("-")[1:]:
        head = part.rstrip("0123456789")
        if head in ("C", "N", "L", "F", "n", "d") and part[len(head):]:
            out[head] = int(part[len(head):])
    return out


# ---- data -----------------------------------------------------------------------------------------------------------------
EDGE_SLOPES = {"edgeA": 5.0, "edgeB": -5.0, "edgeC": 1.5}  # the second slope beside a first slope of 1 (mirrored at the end)


def interp_data(N: int, n_ch: int, kind: str, rng) -> np.ndarray:
    v = rng.standard_normal((N, n_ch))
    b = np.arange(N, dtype=np.float64)[:, None]
    if kind == "flat":  # a strict peak (a run of one knot), two equal knots, five equal knots
        p = N // 5
        if 0 < p < N - 1:
            v[p] = np.maximum(v[p - 1], v[p + 1]) + 1.0
        for run, start in ((2, N // 2), (5, 3 * N // 4)):
            v[start:start + run] = v[min(start, N - 1)]
    elif kind == "ramp":  # monotone, one kink
        v = np.where(b < N // 2, 0.5 * b, 0.5 * (N // 2) + 3.0 * (b - N // 2)) * (1.0 + np.arange(n_ch))
    elif kind == "alternating":
        v = (1.0 - 2.0 * (b % 2)) * (1.0 + 0.1 * rng.random((N, n_ch)))
    elif kind == "zero":
        v[:, 0] = 0.0
    elif kind in EDGE_SLOPES and N >= 3:
        m1 = EDGE_SLOPES[kind]
        v[0], v[1], v[2] = 0.0, 1.0, 1.0 + m1                # first interval: slopes 1, m1
        if N >= 6:
            v[N - 1], v[N - 2], v[N - 3] = 0.0, 1.0, 1.0 + m1  # last interval: slopes -1, -m1
    return np.ascontiguousarray(v, dtype=np.float64)


def interp_axis(N: int, kind: str) -> np.ndarray:
    t = np.arange(N, dtype=np.float64) / (N - 1)
    if kind == "standard":
        return backend._smooth_axis(N, None)[0]
    if kind == "identity":  # every query is a knot
        return np.arange(1, N + 1, dtype=np.float64)
    if kind == "uniform":   # extrapolates at both ends; k_to_lin's logarithmic guess is far off
        return 0.5 + (N + 0.25) * t
    if kind == "top":       # clustered at the top: the last spacing is 1 / (N - 1)
        return 1.0 + (N - 1) * (1.0 - (1.0 - t) ** 2)
    raise KeyError(kind)


def pipeline_data(N: int, n_ch: int, rng) -> np.ndarray:
    """three slow periods plus noise: smoothed values of both signs"""
    b = np.arange(N)[:, None] / N
    return np.sin(2 * np.pi * (3 * b + 0.13 * np.arange(n_ch))) + 0.2 * rng.standard_normal((N, n_ch))


def complex_spectrum(kind: str, rng) -> np.ndarray:
    N = COMPLEX_BINS
    b = np.arange(N, dtype=np.float64)[:, None]
    if kind == "axis":  # (else: "steps", which "clip" shares) 1, -1 + 0i, 1, -1 - 0i, ...: steps of exactly +-fl(pi)
        z = np.empty((N, 1), dtype=np.complex128)
        z.real[:, 0] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        z.imag[:, 0] = np.where(np.arange(N) % 4 == 3, -0.0, 0.0)
        return z
    slopes = np.array([[-2.0, -0.7]])
    phi = slopes * (b + 1.0)  # negative from the first bin on
    jumps = (2.5, -1.0, 3.0, -0.9, 2.0 - (np.pi - 2e-6), 1.1, -1.3)  # 2048: a step 2e-6 inside pi
    for at, j in zip(STEP_BINS, jumps):
        phi[at:, 0] += j
        phi[at:, 1] -= 0.5 * j
    # (the unwrap starts from the first bin's wrapped phase, -2 and -0.7, and the jumps add up to less than the delay
    # takes off before them: the unwrapped phase is negative throughout, smoothed or not)
    m = 1.0 + 0.5 * np.sin(0.01 * b + np.array([[0.0, 1.0]])) + 0.05 * rng.random((N, 2))
    return np.ascontiguousarray(m * np.exp(1j * phi))


def complex_window(L: int) -> np.ndarray:
    n_window = backend._smooth_window_length(1, COMPLEX_SPACING[L])
    assert n_window == L
    return backend._smooth_window(n_window, "hamming", None)


# ---- the group delay's oracle ----------------------------------------------------------------------------------------------
def fft_phase_tolerance(n: int) -> float:
    """fft64_cases.tolerance for an n-point transform, as an error of every bin relative to the column's rms (1 for a
    unit impulse).  Where the table has no entry for this route at this many points, the nearest larger one of the
    route stands in (the error grows with the number of butterfly stages)."""
    route, M, _ = fc.plan(n)
    sizes = sorted(m for r, m in fc.FFT64_EMULATION if r == route and m >= M)
    return fc.tolerance((route, sizes[0]))


def gdelay_oracle(n: int, delays) -> tuple:
    """(expected, bound), both (nb, C).  The spectrum of a unit impulse at d is exp(-2 pi i k d / n): steps of
    -2 pi d / n, which the unwrap keeps for d < n / 2 and turns into -2 pi (d - n) / n beyond -- the group delay is d,
    or d - n, in every bin, exactly.

    Bound.  A wrapped phase errs by e_w = 1.01 tol (the transform's error against a unit magnitude) + 4 u pi (atan2).
    Where the exact phase is +-pi the sign is the error's, so the corrections are not known bin by bin: K_b <= b,
    S_b <= 2 pi b in smooth_oracle.unwrap's bound, E_b = e_w + 4 (b + 2) u 2 pi b.  The central difference divides
    E_(k+1) + E_(k-1) by 4 pi / n (the ends: E_1 + E_0 and E_(nb-1) + E_(nb-2) by 2 pi / n); 1 / n as a float64, the
    subtraction, the two divisions and the rounded pi add 6 u |d|."""
    nb = n // 2 + 1
    d = np.array([dd if dd < n / 2 else dd - n for dd in delays], dtype=np.float64)
    u = float(so.U)
    b = np.arange(nb, dtype=np.float64)
    E = 1.01 * fft_phase_tolerance(n) + 4 * u * np.pi + 4 * (b + 2) * u * 2 * np.pi * b
    g = np.empty(nb)
    g[1:-1] = (E[2:] + E[:-2]) * n / (4 * np.pi)
    g[0] = (E[1] + E[0]) * n / (2 * np.pi)
    g[-1] = (E[-1] + E[-2]) * n / (2 * np.pi)
    return np.broadcast_to(d, (nb, len(d))).astype(LD), (g[:, None] + 6 * u * np.abs(d)[None, :]).astype(LD)


# ---- a case's inputs, oracle and bound ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(name: str) -> dict:
    """the inputs of a case and its oracle: `value`, `bound` (long double, the output's shape; complex outputs as
    (re, im) with one bound for both), computed once"""
    fam, f, rng = family(name), _fields(name), _rng(name)
    if fam in ("bins", "window"):
        v = np.ascontiguousarray(rng.standard_normal((f["N"], f["C"])) + 0.2)
        w = window_taps(rng, f["L"])
        value, bound = so.smooth(v, w)
        return dict(v=v, k_log=None, window=w, clip=0, value=value, bound=bound)
    if fam == "interp":
        _, _, _, kind, axis = name.split("-")
        v, k_log = interp_data(f["N"], f["C"], kind, rng), interp_axis(f["N"], axis)
        w = np.array([1.0])
        value, bound = so.pipeline(v, k_log, w)
        return dict(v=v, k_log=k_log, window=w, clip=0, value=value, bound=bound)
    if fam == "pipeline":
        v = np.ascontiguousarray(pipeline_data(f["N"], f["C"], rng))
        k_log, beta = backend._smooth_axis(f["N"], None)
        w = window_taps(rng, backend._smooth_window_length(f["F"], beta))
        clip = name.endswith("-clip")
        value, bound = so.pipeline(v, k_log, w, f["C"] if clip else 0)
        return dict(v=v, k_log=k_log, window=w, clip=int(clip), fractions=f["F"], value=value, bound=bound)
    if fam == "gdelay":
        n = f["n"]
        delays = gdelay_delays(n)[f["d"]:f["d"] + f["C"]]
        x = np.zeros((n, f["C"]))
        x[list(delays), np.arange(f["C"])] = 1.0
        value, bound = gdelay_oracle(n, delays)
        return dict(x=x, n=n, delays=delays, value=value, bound=bound)
    if fam == "complex":
        _, kind, Ls = name.split("-")
        L = int(Ls[1:])
        z = complex_spectrum(kind, _rng("complex"))
        w = complex_window(L)
        clip = kind == "clip"
        re, im, bound, stages = so.complex_pipeline(z, None, w, clip)
        return dict(z=z, window=w, L=L, clip=clip, value=(re, im), bound=bound, stages=stages)
    raise KeyError(name)


def judge(name: str, out) -> float:
    """worst |out - oracle| / bound over every element of the case's output"""
    p = problem(name)
    if family(name) == "complex":
        assert out.shape == p["z"].shape and out.dtype == np.complex128, name
        return max(so.ratio(out.real, p["value"][0], p["bound"]), so.ratio(out.imag, p["value"][1], p["bound"]))
    assert out.shape == p["value"].shape and out.dtype == np.float64, (name, out.shape)
    return so.ratio(out, p["value"], p["bound"])


# ---- float64 emulations, right and subtly wrong --------------------------------------------------------------------------------
SMOOTH_FAULTS = ("last_tap", "first_tap", "clamp_front", "clamp_back", "chunk_seam", "even_padding")
LOG_FAULTS, LIN_FAULTS = ("zero_slope", "edge_branch"), ("bracket_high",)
UNWRAP_FAULTS = ("tile_carry", "lane_carry", "plus_pi")
FAULTS = SMOOTH_FAULTS + LOG_FAULTS + LIN_FAULTS + UNWRAP_FAULTS + ("clip_all",)


def _only(fault, stage):
    return fault if fault in stage else None


def emu_smooth(v, w, fault=None):
    """np.convolve on the edge-padded data.  Faults, in the kernel's terms (tap m of the reversed window): the last or
    the first tap dropped; the clamp one row short of either end; tap CH(tc) skipped; an even window's padding swapped"""
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, L = v.shape[0], len(w)
    wr = (w / w.sum())[::-1].copy()
    if fault == "last_tap":
        wr[L - 1] = 0.0
    if fault == "first_tap":
        wr[0] = 0.0
    if fault == "chunk_seam":
        wr[CH(tc_of(v.shape[1]))] = 0.0
    front = L // 2
    if fault == "even_padding":
        front = L - 1 - L // 2
    lo, hi = (1 if fault == "clamp_front" else 0), (N - 2 if fault == "clamp_back" else N - 1)
    padded = v[np.clip(np.arange(-front, N + L - 1 - front), lo, hi)]
    return np.stack([np.convolve(padded[:, c], wr[::-1], mode="valid") for c in range(v.shape[1])], axis=1)


def emu_to_log(v, k_log, fault=None):
    """scipy's PchipInterpolator on the knots 1 .. N.  Faults: the harmonic mean without the zero-slope rule; the end
    rule without its second branch (both in float64 with the device's formulas otherwise)"""
    if fault is None:
        return PchipInterpolator(np.arange(1, len(v) + 1, dtype=np.float64), v, axis=0)(k_log)
    terms = so.pchip_terms(v, k_log, np.float64, zero_rule=fault != "zero_slope", second_branch=fault != "edge_branch")
    return so.pchip_eval(*terms[:5])


def emu_to_lin(y, k_log, fault=None):
    """np.interp back to the bins 1 .. N.  Fault: the bracket one interval too high when the bin is a knot
    (searchsorted "right"); a row past the end reads the last one"""
    N = len(k_log)
    l = np.arange(1, N + 1, dtype=np.float64)
    if fault is None:
        return np.stack([np.interp(l, k_log, y[:, c]) for c in range(y.shape[1])], axis=1)
    lo = np.clip(np.searchsorted(k_log, l, side="right") - 1, 0, N - 1)
    hi = np.minimum(lo + 1, N - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (y[hi] - y[lo]) / (k_log[hi] - k_log[lo])[:, None]
        return slope * (l - k_log[lo])[:, None] + y[lo]


def emu_unwrap(ph, fault=None):
    """np.unwrap along the bins.  Faults: the carry into the second tile dropped; the prefix of the lanes before
    lane 1 dropped; a rising step that lands on -pi not put back to +pi"""
    if fault is None:
        return np.unwrap(ph, axis=0)
    dd = np.diff(ph, axis=0)
    ddmod = np.mod(dd + np.pi, 2 * np.pi) - np.pi
    if fault != "plus_pi":
        ddmod[(ddmod == -np.pi) & (dd > 0)] = np.pi
    corr = np.where(np.abs(dd) < np.pi, 0.0, ddmod - dd)
    cum = np.concatenate([np.zeros((1,) + ph.shape[1:]), np.cumsum(corr, axis=0)], axis=0)
    if fault == "tile_carry" and len(ph) > UNWRAP_TILE:
        cum[UNWRAP_TILE:] -= cum[UNWRAP_TILE - 1]
    if fault == "lane_carry" and len(ph) > UNWRAP_LANE:
        cum[UNWRAP_LANE:2 * UNWRAP_LANE] -= cum[UNWRAP_LANE - 1]
    return ph + cum


def emu_gdelay(x, n, fault=None):
    ph = emu_unwrap(np.angle(np.fft.rfft(x, axis=0)), fault)
    return -np.gradient(ph, 1.0 / n, axis=0) / np.pi / 2.0


def emulate(name: str, fault=None) -> np.ndarray:
    """the case's entry in float64 numpy; `fault` reaches the stage it belongs to"""
    p, fam = problem(name), family(name)
    if fam == "gdelay":
        return emu_gdelay(p["x"], p["n"], _only(fault, UNWRAP_FAULTS))
    if fam == "complex":
        z = p["z"]
        C = z.shape[1]
        both = np.concatenate([np.abs(z), emu_unwrap(np.angle(z), _only(fault, UNWRAP_FAULTS))], axis=1)
        sm = emu_smooth(both, p["window"], _only(fault, SMOOTH_FAULTS))
        if p["clip"]:
            cols = 2 * C if fault == "clip_all" else C
            sm[:, :cols] = np.clip(sm[:, :cols], 0, None)
        return sm[:, :C] * np.exp(1j * sm[:, C:])
    v = p["v"]
    if p["k_log"] is not None:
        v = emu_to_log(v, p["k_log"], _only(fault, LOG_FAULTS))
    v = emu_smooth(v, p["window"], _only(fault, SMOOTH_FAULTS))
    if p["k_log"] is not None:
        v = emu_to_lin(v, p["k_log"], _only(fault, LIN_FAULTS))
    return np.clip(v, 0, None) if p["clip"] else v


if __name__ == "__main__":  # prints the table above
    worst = {}
    for name in all_cases():
        worst[family(name)] = max(worst.get(family(name), 0.0), judge(name, emulate(name)))
    print("SMOOTH_EMULATION = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in worst.items()) + "}")
