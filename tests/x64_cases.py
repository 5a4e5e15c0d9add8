"""The route matrix of the float64 Welch entries (ds_welch_spec_x64, ds_welch_tf_x64, ds_csm_x64; kernels in
csrc/kernels_welch_f64.hpp): the problems, their oracle, the bound and the judge.  test_welch_x64_host.py checks all
of this on the CPU, test_welch_x64_gpu.py holds the kernels to it.

The oracle.  route_oracles.py's restatement (frame_spectra, average_frames, finish and the expressions of its welch()
and csm()) run in numpy.longdouble (scipy.fft keeps it: complex256, eps 1.1e-19 on x86-64) on the float64 samples and
window the entries are handed.  One problem holds one pair of signals and one framing; its frame spectra are computed
once and every entry of the problem (auto spectra of x, cross spectra, H1 / H2 / H3 with coherence, the matrix of x)
is contracted from them.  answers(p, numpy.float64) is the same code in the kernels' own precision: the emulation.

The error rule is route_oracles.py's: |out - oracle| <= tol * scale elementwise, scale = the rms of the oracle over the
bins of a channel (tf: of |H| over the judged bins; a matrix element: of sqrt(ref_ii ref_jj)), coherence absolute,
with detrend the DC bin of a transfer function is not judged, nothing else is excluded, and a row whose oracle is
identically zero must be exactly zero.

The bound.  X64_EMULATION holds the emulation's worst error over the cases of one (kind, window, average) as a multiple
of eps64 * scale, measured on the CPU (the host test measures it again); the bound is 4 x that x HOST_MARGIN x eps64:
four for another equally valid summation order and twiddle rounding, a tenth for another host's numpy -- route_oracles.
tolerance()'s reasoning.  No bound may exceed CAP = 1e-11, the tightest bound the suite already asserts for this
route, and the emulation alone has to stay within a quarter of that; the signals are made so that it does (responses
without spectral nulls: decaying positive taps, 1e-2 of noise, coherence >= 0.5 at every judged bin).

The cases sit on the kernels' edges, which depend on the constants mirrored below (the host test reads them out of the
sources and fails when they differ).  A "ragged" n is (F - 1) hop + 3: the last frame is nearly all zero padding.
"""

import zlib
from collections import OrderedDict

import numpy as np
from scipy.signal import get_window

import route_oracles as ros

# ---- the constants the case list depends on (csrc/kernels_welch_f64.hpp, csrc/api.hip) ---------------------------------------
LONG_M = 8192                 # points of the LDS transform: W <= 8192 k_frames<false>, 16384 k_frames<true>, more k_frames_cls
CSM_PAIRS_PER_THREAD = 9      # x 256 = 2304 channel pairs per workgroup of k_csm
CSM_MAX_CH = 1024
CSM_MEDIAN_TILE = 32
CSM_MEDIAN_MAX_FRAMES = 128
CSM_TILE_VALUES = 4096        # frame tile of k_csm: min(F, 4096 / n_ch) frames
PLANAR_FROM_CH = 4            # x64_launch_frames: k_planar from four channels on
MEDIAN_MAX_FRAMES = 4096      # x64_check
PACKED_W = 2 * LONG_M
MAX_W = 262144

EPS = float(np.finfo(np.float64).eps)
CAP = 1e-11
HOST_MARGIN = ros.HOST_MARGIN
LD = np.longdouble

# worst error of the float64 emulation / (eps64 * scale) per (kind, window, average), as measured on the CPU
X64_EMULATION = {
    ("csd", 8, "mean"): 0.874, ("csd", 16, "mean"): 0.95, ("csd", 256, "mean"): 7.99, ("csd", 512, "mean"): 5.07,
    ("csd", 8192, "mean"): 13.1, ("csd", 16384, "mean"): 13.9, ("csd", 32768, "mean"): 17.5,
    ("csd", 65536, "mean"): 18.1, ("csd", 131072, "mean"): 21.9, ("csd", 262144, "mean"): 19.8,
    ("csd", 8, "median"): 0.661, ("csd", 16, "median"): 3.09, ("csm", 8, "mean"): 4.4, ("csm", 16, "mean"): 4.93,
    ("csm", 16, "median"): 46.9, ("psd", 8, "mean"): 1.4, ("psd", 16, "mean"): 2.46, ("psd", 256, "mean"): 8.34,
    ("psd", 512, "mean"): 5.43, ("psd", 8192, "mean"): 15.6, ("psd", 16384, "mean"): 17.3,
    ("psd", 32768, "mean"): 18.5, ("psd", 65536, "mean"): 16.8, ("psd", 131072, "mean"): 17,
    ("psd", 262144, "mean"): 26.6, ("psd", 8, "median"): 0.763, ("psd", 16, "median"): 3.36,
    ("tf", 512, "mean"): 5.86, ("tf", 8, "median"): 1.92, ("tf", 16, "median"): 7.78,
}


def tolerance(tk):
    return 4.0 * X64_EMULATION[tk] * HOST_MARGIN * EPS


# ---- the problems ---------------------------------------------------------------------------------------------------------------
FIN = {"raw": lambda W: (0, 1.0, 1.0, 0), "power": lambda W: (0, 1.0 / W, 2.0, 1), "amp": lambda W: (1, 1.0 / W, 2.0, 1)}
_specs = OrderedDict()


def _add(ident, entries, W, hop, F, n_cx, n_cy=None, det=0, avg="mean", fin="power", n=None, signal="noise"):
    assert ident not in _specs, ident
    n_cy = n_cx if n_cy is None else n_cy
    _specs[ident] = dict(ident=ident, entries=tuple(entries), W=W, hop=hop, n_frames=F, n_cx=n_cx, n_cy=n_cy, detrend=det,
                         average=avg, fin=fin, n=(F - 1) * hop + 3 if n is None else n, signal=signal)


SPEC = ("psd", "csd")
TFS = ("tf:H1", "tf:H2", "tf:H3")


def _build():
    for det, fin in ((0, "power"), (1, "amp")):
        d = f"det{det}"
        # k_frames<false>: strided reads (fewer than 4 channels) and the planar copy (32 x 32 tiles on both axes)
        for W in (8, 256, 512, LONG_M):
            _add(f"frames|{W}|c2|{d}", SPEC, W, W // 2, 3, 2, det=det, fin=fin)
        for W in (256, LONG_M):
            for C in (PLANAR_FROM_CH - 1, PLANAR_FROM_CH, CSM_MEDIAN_TILE + 1):
                _add(f"frames|{W}|c{C}|{d}", SPEC, W, W // 2, 3, C, det=det, fin=fin)
        _add(f"frames|256|hopW|{d}", SPEC, 256, 256, 3, 2, det=det, fin=fin)
        _add(f"frames|256|hopW/4|{d}", SPEC, 256, 64, 7, 2, det=det, fin=fin)
        _add(f"frames|16|hop5|{d}", SPEC, 16, 5, 9, 2, det=det, fin=fin)
        # k_frames<true>: the last sample the first (n odd) and the second (n even) of a packed pair
        for C in (2, 5):
            _add(f"packed|{PACKED_W}|c{C}|odd|{d}", SPEC, PACKED_W, LONG_M, 3, C, det=det, fin=fin, n=2 * LONG_M + 3)
            _add(f"packed|{PACKED_W}|c{C}|even|{d}", SPEC, PACKED_W, LONG_M, 3, C, det=det, fin=fin, n=2 * LONG_M + 4)
        # k_frames_cls (2, 4, 8, 16 classes) + k_split
        for W in (4 * LONG_M, 8 * LONG_M, 16 * LONG_M, 32 * LONG_M):
            _add(f"long|{W}|f3c2|ragged|{d}", SPEC, W, W // 2, 3, 2, det=det, fin=fin)
            _add(f"long|{W}|f3c2|full|{d}", SPEC, W, W // 2, 3, 2, det=det, fin=fin, n=2 * W)
            _add(f"long|{W}|f1c1|ragged|{d}", SPEC, W, W // 2, 1, 1, det=det, fin=fin)
            _add(f"long|{W}|f1c1|n=W|{d}", SPEC, W, W // 2, 1, 1, det=det, fin=fin, n=W)
    # k_tf: 257 bins (two workgroups of bins), one or three inputs, a channel of negative gain (detrend off: Gxy real and
    # negative at the DC and Nyquist bins -- H2's `sxy.y == 0` branch, the branch cut of the square root)
    for n_cx in (1, 3):
        for fin in ("power", "amp"):
            _add(f"tf|512|cx{n_cx}|{fin}|det0", TFS, 512, 256, 5, n_cx, 3, det=0, fin=fin, signal="negative")
    _add("tf|512|cx3|raw|det1", TFS, 512, 256, 5, 3, 3, det=1, fin="raw", signal="negative")
    # k_tf_median, k_spec_median: the rank loop's strides of 256 frames, the LDS limit of 4096 frames, all ranks tied
    # (two and three frames: whole frames -- the median of three frames of which two are mostly padding has no coherence)
    for F in (1, 2, 3, 255, 256, 257):
        _add(f"median|16|F{F}", SPEC + ("tf:H1",), 16, 8, F, 2, det=F % 2, avg="median", fin=("power", "amp", "raw")[F % 3],
             n=(F - 1) * 8 + 16 if F in (2, 3) else None)
    _add(f"median|8|F{MEDIAN_MAX_FRAMES}", SPEC + ("tf:H2",), 8, 4, MEDIAN_MAX_FRAMES, 2, det=1, avg="median", fin="amp")
    _add("median|16|F300|ties", SPEC + ("tf:H1",), 16, 8, 300, 2, det=0, avg="median", fin="amp", signal="periodic")
    _add("median|16|F2|ties", SPEC + ("tf:H3",), 16, 8, 2, 2, det=1, avg="median", fin="power", n=8 + 16, signal="periodic")
    # k_spec
    for F in (1, 100):
        _add(f"spec|512|F{F}", SPEC, 512, 256, F, 2, det=1, fin="raw")
    # k_csm: pair groups of 2304 pairs (64 channels: 2080, 68: 2346), frame tiles of 4096 / n_ch frames
    for C in (1, 2, 64, 68, 70):
        _add(f"csm|16|c{C}|F5", ("csm",), 16, 8, 5, C, 0, det=C % 2, fin=("power", "raw")[C % 2])
    for F in (60, 61, 121):
        _add(f"csm|16|c68|F{F}", ("csm",), 16, 8, F, 68, 0, det=1, fin="power")
    _add(f"csm|8|c{CSM_MAX_CH}|F5", ("csm",), 8, 4, 5, CSM_MAX_CH, 0, det=1, fin="power")
    _add("csm|16|c6|coherent|amp", ("csm",), 16, 8, 5, 6, 0, det=0, fin="amp", signal="coherent")
    # k_csm_median: one, two and three channel tiles; one and two frames a lane; all ranks tied
    for C in (2, CSM_MEDIAN_TILE, CSM_MEDIAN_TILE + 1, 2 * CSM_MEDIAN_TILE + 1):
        for F in (1, 2, 63, 64, 65, CSM_MEDIAN_MAX_FRAMES - 1, CSM_MEDIAN_MAX_FRAMES):
            _add(f"csm_median|16|c{C}|F{F}", ("csm",), 16, 8, F, C, 0, det=(C + F) % 2, avg="median",
                 fin=("power", "amp", "raw")[(C + F) % 3])
    for F in (65, CSM_MEDIAN_MAX_FRAMES):
        _add(f"csm_median|16|c33|F{F}|ties", ("csm",), 16, 8, F, 33, 0, det=0, avg="median", fin="amp", signal="periodic")


_build()
IDENTS = list(_specs)


def _response(rng, n_ch):
    """decaying positive taps: |H| between 0.5 and 2.3 everywhere, no null"""
    return np.exp(-np.arange(5) / 1.5)[:, None] * (1.0 + 0.2 * rng.random((5, n_ch)))


def problem(ident):
    """The arrays of one case: x (n, n_cx), y (n, n_cy) or None, the Hann window, all float64 and C-contiguous."""
    p = dict(_specs[ident])
    rng = np.random.default_rng(zlib.crc32(ident.encode()))
    n, W, hop, n_cx, n_cy = p["n"], p["W"], p["hop"], p["n_cx"], p["n_cy"]
    periodic = p["signal"] == "periodic"
    m = hop if periodic else n  # one period
    x = 0.3 * rng.standard_normal((m, n_cx))
    if p["signal"] == "coherent":  # one source through gains of either sign, a little noise
        gains = np.array([1.0, -0.7, 0.4, -1.3, 0.9, -0.2])[:n_cx]
        x = 0.3 * rng.standard_normal((m, 1)) * gains + 3e-3 * rng.standard_normal((m, n_cx))
    y = None
    if n_cy:
        h = _response(rng, n_cy)
        if p["signal"] == "negative":
            h[:, 1] *= -1.0
        src = x if n_cx == n_cy else np.repeat(x[:, :1], n_cy, axis=1)
        if periodic:  # circular: y has the period of x
            y = np.stack([np.real(np.fft.ifft(np.fft.fft(src[:, c]) * np.fft.fft(h[:, c], m))) for c in range(n_cy)], axis=1)
        else:
            y = np.stack([np.convolve(src[:, c], h[:, c])[:m] for c in range(n_cy)], axis=1)
        y = y + 1e-2 * rng.standard_normal((m, n_cy))
    if periodic:
        reps = -(-n // m)
        x = np.tile(x, (reps, 1))[:n]
        y = None if y is None else np.tile(y, (reps, 1))[:n]
    p["x"] = np.ascontiguousarray(x, np.float64)
    p["y"] = None if y is None else np.ascontiguousarray(y, np.float64)
    p["w"] = np.ascontiguousarray(get_window("hann", W, fftbins=True), dtype=np.float64)
    p["amp_sqrt"], p["norm_scale"], p["factor"], p["halve_edges"] = FIN[p["fin"]](W)
    return p


def tol_key(p, entry):
    kind = entry.split(":")[0]
    return (kind, p["W"], p["average"])


def routes(p, entry):
    """the launch names ctx.routes() has to report after one call of the entry"""
    frames = {"welch_f64_frames"} if p["W"] <= PACKED_W else {"welch_f64_frames@long", "welch_f64_split"}
    med = "_median" if p["average"] == "median" else ""
    kind = entry.split(":")[0]
    return frames | {{"psd": "welch_f64_spec", "csd": "welch_f64_spec", "tf": "welch_f64_tf", "csm": "csm_f64"}[kind] + med}


# ---- the restatement: dt = longdouble is the oracle, float64 the emulation ----------------------------------------------------
PERTURBATIONS = ("window32", "mean32", "dupframe")


def _spectra(p, sig, dt, perturb):
    """(B, F, C) frame spectra of sig (n, C) -- route_oracles.frame_spectra, or a subtly wrong version of it"""
    W, hop, F, det = p["W"], p["hop"], p["n_frames"], p["detrend"]
    w = p["w"].astype(np.float32) if perturb == "window32" else p["w"]
    if perturb == "mean32" and det:
        f = np.ascontiguousarray(ros.frames(np.asarray(sig, dt), W, hop, F) * np.asarray(w, dt))
        f -= f.astype(np.float32).mean(axis=-1, keepdims=True).astype(dt)
        X = ros.sfft.rfft(f, axis=-1).transpose(2, 1, 0)
    else:
        X = ros.frame_spectra(sig, w, W, hop, F, det, dt=dt)
    if perturb == "dupframe" and F > 1:  # the frames of n_frames - 1, the last one twice
        X = X.copy()
        X[:, -1] = X[:, -2]
    return X


def answers(p, dt=LD, perturb=None):
    """{entry: array or (tf, coherence)} of every entry of the problem, in precision dt"""
    fin = lambda P: ros.finish(ros.average_frames(P, p["average"]), dt(p["norm_scale"]), dt(p["factor"]), p["halve_edges"],
                               p["amp_sqrt"])
    X = _spectra(p, p["x"], dt, perturb)
    Y = None if p["y"] is None else _spectra(p, p["y"], dt, perturb)
    out = {}
    for entry in p["entries"]:
        if entry == "psd":
            out[entry] = fin(np.abs(X) ** 2)
        elif entry == "csd":
            out[entry] = fin(X.conj() * Y)
        elif entry == "csm":
            out[entry] = _csm(p, X, dt)
        else:
            out[entry] = _tf(entry[3:], X, Y, fin)
    return out


def _tf(mode, X, Y, fin):
    if X.shape[2] == 1:
        X = np.broadcast_to(X, Y.shape)
    Gxx, Gyy, Gxy = fin(np.abs(X) ** 2), fin(np.abs(Y) ** 2), fin(X.conj() * Y)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "H1":
            tf = Gxy / Gxx
        elif mode == "H2":
            tf = Gyy / fin(Y.conj() * X)
        else:
            tf = Gxy / np.abs(Gxy) * (Gyy / Gxx) ** 0.5
        return tf, np.abs(Gxy) ** 2 / Gxx / Gyy


def _csm(p, X, dt):
    """route_oracles.csm from given frame spectra (the same expressions; its median runs chunked on threads there)"""
    B, F, C = X.shape
    fp = (dt(p["norm_scale"]), dt(p["factor"]), p["halve_edges"])
    if p["average"] == "mean" and not p["amp_sqrt"]:
        return ros.finish(np.matmul(X.transpose(0, 2, 1), X.conj()) / dt(F), *fp, 0)
    ii, jj = np.tril_indices(C)
    Xt = X.transpose(0, 2, 1)
    S = np.zeros((B, C, C), X.dtype)
    S[:, ii, jj] = ros._pair_averages(np.ascontiguousarray(Xt.real), np.ascontiguousarray(Xt.imag), ii, jj, p["average"])
    S = ros.finish(S, *fp, p["amp_sqrt"])
    S[:, jj, ii] = np.where((ii != jj)[None], S[:, ii, jj].conj(), S[:, ii, jj])
    return S


_cache: OrderedDict = OrderedDict()


def oracle(p):
    """one long-double oracle per problem, for all its entries (the last few problems are kept)"""
    ref = _cache.get(p["ident"])
    if ref is None:
        ref = _cache[p["ident"]] = answers(p, LD)
        while len(_cache) > 2:
            _cache.popitem(last=False)
    return ref


# ---- the judge ------------------------------------------------------------------------------------------------------------------
def targets(p, entry, ref):
    """[(name, oracle, scale, dtype of the output, judged bins)] of the arrays one call of the entry returns"""
    every = slice(None)
    kind = entry.split(":")[0]
    if kind == "tf":
        bins = slice(1, None) if p["detrend"] else every
        return [("tf", ref[0], ros._rms(ref[0][bins], 0), np.complex128, bins),
                ("coherence", ref[1], np.ones((1, 1), LD), np.float64, bins)]
    if kind == "csm":
        d = np.einsum("bii->bi", ref).real
        return [("csm", ref, ros._rms(np.sqrt(d[:, :, None] * d[:, None, :]), 0), np.complex128, every)]
    return [(kind, ref, ros._rms(ref, 0), np.complex128, every)]


def judge_entry(p, entry, out, tol=None):
    """The arrays one call returned against the oracle -> {name: worst error / bound}.  (Auto spectra come back as
    complex128 with an imaginary part of exactly 0.)"""
    tol = tolerance(tol_key(p, entry)) if tol is None else tol
    outs = out if isinstance(out, tuple) else (out,)
    tg = targets(p, entry, oracle(p)[entry])
    assert len(outs) == len(tg), (p["ident"], entry, len(outs))
    worst = {}
    for o, (name, ref, scale, dtype, bins) in zip(outs, tg):
        key = f"{p['ident']} {entry} {name}"
        if name == "psd":
            assert o.dtype == dtype and not o.imag.any(), (key, "auto spectra with an imaginary part")
            ref = ref.astype(np.clongdouble)
        worst[name] = ros.judge(key, o, ref, scale, tol, dtype, bins)
        if name == "csm":  # exactly Hermitian, an exactly real diagonal: every element and its mirror were written
            assert np.array_equal(o, o.conj().transpose(0, 2, 1)), (key, "not Hermitian")
            assert not np.einsum("bii->bi", o).imag.any(), (key, "diagonal not real")
    return worst


def emulation_fractions(p, perturb=None):
    """{(kind, W, average): the float64 emulation's worst error / (eps64 * scale)} over the problem's entries"""
    ref, emu = oracle(p), answers(p, np.float64, perturb)
    worst = {}
    for entry in p["entries"]:
        e = emu[entry] if isinstance(emu[entry], tuple) else (emu[entry],)
        for o, (name, r, scale, _, bins) in zip(e, targets(p, entry, ref[entry])):
            o, r = o[bins], r[bins]
            s = np.broadcast_to(scale, r.shape)
            frac = float(np.max(np.abs(o.astype(r.dtype) - r)[s > 0] / (EPS * s[s > 0]), initial=0.0))
            tk = tol_key(p, entry)
            worst[tk] = max(worst.get(tk, 0.0), frac)
    return worst
