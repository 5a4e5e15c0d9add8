"""What every output of the route matrices (tests/route_cases.py) has to be: one plain restatement per kernel family,
in float64, and the judge that holds an output against it.

The restatements take the arguments of the C-ABI entries as include/dsptoolbox_amd.h states them (window array, hop,
n_frames, detrend, norm_scale, factor, halve_edges, scale, edge_scale, frame_offset, ...), not the reference's
scaling names: test_route_oracles_host.py calls them through backend.py's own parameter mapping on the reference's
golden data (tests/golden/*.npz) and finds them within 1e-12 of it.

    welch   frame k = samples [k hop, k hop + W), zero padded, times the window, minus its mean if detrend; rFFT;
            mean over frames, or median of the real and of the imaginary parts times n (n = F or F - 1, odd: the
            reference's `csd /= sum((-1)**(n+1)/n)`); then S *= norm_scale; if halve_edges: S *= factor, bins 0 and
            W/2 halved; if amp_sqrt: principal square root.  tf: H1 = Gxy / Gxx, H2 = Gyy / Gyx, H3 = Gxy / |Gxy|
            sqrt(Gyy / Gxx), coherence |Gxy|^2 / (Gxx Gyy).
    stft    frame k = samples [k hop - pad_front, ... + W); window; detrend; rFFT of length nfft (crop / zero pad);
            bins 0 and nfft/2 times edge_scale; times scale (power: |.|^2 times scale).
    istft   unnormalised inverse rFFT of length nfft of every frame (the imaginary parts of the DC and Nyquist bins
            do not enter: a real signal has none) times scale, cropped to W, windowed, overlap-added at
            (f + frame_offset) step, divided by the sum of window^2 over n_frames_total positions clipped at 1e-4.
    fir     y_k = (x * taps_k)[0:n]; parallel: every k; summed: their sum; sequential: the cascade, every stage cut
            to n samples.
    rfft    rfft(x zero padded to n_fft) * scale.
    deconv  irfft(rfft(y, n_fft) * r, n_fft)[0:n_out], r one inverse spectrum for all channels or one per channel.
    csm     csm[b][i][j] = finish(average over frames of X_i conj(X_j)) for i >= j, the upper triangle its conjugate.

Every `_f64` entry narrows its float64 arrays to float32 while it uploads them (csrc/api.hip: upload_signal and
upload_narrow_f64 in stft_host, istft_host, rfft_host, deconv_host, fir_ola_host, welch_host, csm_host) and runs the
kernels of the float32 entry; the device entries take float32.  So there is ONE oracle per problem for all its
entries, on the float32-rounded samples, taps, window and spectra, computed in float64.  No entry of these matrices
computes in float64 (the float64 Welch entries have a matrix of their own, judged in long double: tests/x64_cases.py).

The error rule.  |out - oracle| <= tol * scale elementwise, scale = the root mean square of the oracle over the
transform axis of that row (rfft: bins of a channel; deconv, istft, fir: samples of a row; stft: bins of a frame of
a channel; welch psd, csd, tf: bins of a channel, tf on |H|; csm: bins of sqrt(ref_ii ref_jj) of an element, over
the requested bin range).  This is how a float32 FFT pipeline errs (about eps log N ||x||_2 per bin) and, unlike the
array maximum, leaves no room under a large DC bin.  Coherence lies in [0, 1]: the same tol, absolute.  With detrend
the DC bin of a transfer function is 0/0 rounding noise in the reference itself: it is not judged and does not enter
the scale.  Nothing else is excluded.  A row with scale 0 (an oracle that is identically zero) must be exactly zero.

The tolerance.  The project's 1e-6 was stated against the array maximum, so it is measured anew against a
single-precision emulation, not against the library: the same restatement run in float32 (scipy.fft keeps single
precision, float32 oaconvolve, float32 sums; frame means summed pairwise).  EMULATION below holds its worst error as
a fraction of 1e-6 * scale over all cases of one (family, transform length) of the matrices, as measured on the CPU
(test_route_oracles_host.py measures it again in every run).  Where that stays at or below 0.25 the bound is 1e-6;
otherwise it is 4 x the emulation's worst error, the factor of four for the kernels' different but equally valid
summation order and twiddle rounding, times HOST_MARGIN: a tenth for another host's FFT and summation rounding
(numpy and scipy choose their vector code by the processor), applied in tolerance() and nowhere else.
test_route_oracles_host.py asserts that the emulation keeps tol / 4 in every case.  The figures are recorded per length, not per family, because one length
would otherwise set the bound of all: a float32 number cannot be closer to the oracle than 6e-8 of ITSELF, and
    - the DC bin of a 2^20-point spectrum of a signal on an offset of 0.25 is 400 times the rms of its bins
      (emulation 29 at rfft 2^20, 0.07 ... 3.5 up to 32768 points);
    - a detrended frame's DC bin is what the float32 mean of the frame leaves behind, 7e-9 at best, against an rms of
      3e-4 at 2^20 points (emulation 71 at stft 2^20, 0.3 ... 3.4 up to 32768 points);
    - the median of the 5 or 9 frames of a 2^20-sample Welch window, two of them mostly padding, moves by a whole
      frame's rounding (emulation 645 at tf 2^20, 16 and 11 at psd and csd; 0.6 ... 8.5 up to 32768 samples);
    - the inverse STFT divides by the window envelope, down to 1e-4 at both ends of the signal (emulation 2 ... 7).
So hardly any bound is 1e-6 itself: a peak of three times the rms already rounds by 0.18e-6 of the rms in float32.
The bounds lie between 1e-6 and 4e-5 up to 32768 points.  At 2^20 samples the median transfer function's bound is
2.8e-3 of rms |H|: there the rule yields a check that guards against gross errors only (a wrong frame, bin, channel
or scaling), no more; the mean estimates of the same window are held to 1e-5.

The cross-spectral matrices' median (130 channels x 192 frames x 513 bins: 1.7e9 numbers to select from) is taken
over the lower triangle only, in chunks of bins on a few threads: 12 s for the largest problem, once for its three
entries.

On an MI355X (worst error / bound over all lengths and entries, the same under every switch of a family unless
noted): welch tf 0.26 (tf_dev, 16384, median), psd 0.27, csd 0.32; stft 0.44 (8 points; default and STFT_GENERIC);
rfft 0.45 (1000 points, Bluestein); deconv 0.55 (3 points; all five switch settings); fir 0.34 ... 0.44 (one tap;
FIR_4K=1 0.44, default 0.35, the other five settings 0.34); istft 0.38 (1000 points; all four settings).  One case
exceeded its bound when the values were first judged, 14 times over: istft 2048|full|2|2 on istft@wave and
istft@fused, a last frame pair without a second frame (test_istft_last_frame_dropped_vs_oracle); 0.27 since the fix.
csm 0.24 (4096, median, 65 channels; 0.09 ... 0.11 at 1024 and 32, 0.17 and 0.22 at 16384 and 32768; the same under
default, CSM_GENERIC, CSM_F32 and CSM_CHUNKS=3; every call at 1000 points is refused and held to its zeros).
What judging adds to a parametrized test: welch tf at 2^20 samples 8 ... 9 s (csd 4 s, psd 2 s there), csm at 1024
points 15 s (10 s of it the oracles) and at 4096 points 6 s, under a second everywhere else.
"""

import os
import time
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.fft as sfft
from scipy.signal import oaconvolve

BASE_TOL = 1e-6
HOST_MARGIN = 1.1
# worst error of the float32 emulation / (1e-6 * scale) per (family or Welch kind, transform length), as measured
EMULATION = {
    ("tf", 32): 1.93, ("tf", 64): 1.84, ("tf", 128): 1.39, ("tf", 256): 1.12, ("tf", 1024): 1.11, ("tf", 2048): 1.72,
    ("tf", 4096): 2.48, ("tf", 8192): 4.68, ("tf", 16384): 4.95, ("tf", 32768): 8.39, ("tf", 1048576): 643,
    ("psd", 32): 0.753, ("psd", 64): 0.665, ("psd", 128): 0.816, ("psd", 256): 0.664, ("psd", 1024): 0.816,
    ("psd", 2048): 1.36, ("psd", 4096): 1.25, ("psd", 8192): 1.55, ("psd", 16384): 1.92, ("psd", 32768): 2.43,
    ("psd", 1048576): 15.7, ("csd", 32): 0.884, ("csd", 64): 0.667, ("csd", 128): 0.653, ("csd", 256): 0.648,
    ("csd", 1024): 0.6, ("csd", 2048): 0.805, ("csd", 4096): 0.983, ("csd", 8192): 1.63, ("csd", 16384): 1.61,
    ("csd", 32768): 1.76, ("csd", 1048576): 11.5,
    ("stft", 8): 0.288, ("stft", 16): 0.359, ("stft", 32): 0.418, ("stft", 64): 0.466, ("stft", 128): 0.479,
    ("stft", 256): 0.579, ("stft", 512): 0.733, ("stft", 1000): 1.01, ("stft", 1024): 1.02, ("stft", 2048): 1.19,
    ("stft", 4096): 1.52, ("stft", 8192): 2.58, ("stft", 16384): 2.86, ("stft", 32768): 3.44, ("stft", 262144): 18.9,
    ("stft", 524288): 33.3, ("stft", 1048576): 70.6,
    ("istft", 16): 2.53, ("istft_short", 16): 2.06, ("istft", 256): 4.18, ("istft_short", 256): 5.94,
    ("istft", 1000): 5.53, ("istft_short", 1000): 5.59, ("istft", 1024): 4.34, ("istft_short", 1024): 6.97,
    ("istft", 2048): 3.67, ("istft_short", 2048): 4.02, ("istft", 4096): 3.41, ("istft_short", 4096): 4.19,
    ("istft", 8192): 3.68, ("istft_short", 8192): 4.51, ("istft", 16384): 4.07, ("istft_short", 16384): 5.18,
    ("istft", 32768): 4.5, ("istft_short", 32768): 4.9, ("istft", 524288): 5.67, ("istft_short", 524288): 7.14,
    ("fir", 1): 0.56, ("fir", 2): 1.27, ("fir", 64): 2.39, ("fir", 1024): 3.02, ("fir", 1025): 2.48,
    ("fir", 2049): 4.46, ("fir", 4097): 3.72, ("fir", 8193): 4.06, ("fir", 32769): 4.18,
    ("rfft", 2): 0.073, ("rfft", 3): 0.0942, ("rfft", 4): 0.0661, ("rfft", 8): 0.0928, ("rfft", 1000): 0.71,
    ("rfft", 1024): 1.7, ("rfft", 8192): 1.87, ("rfft", 16384): 3.5, ("rfft", 32768): 3.19, ("rfft", 100000): 11.8,
    ("rfft", 1048576): 29.5,
    ("deconv", 2): 0.0968, ("deconv", 3): 0.15, ("deconv", 4): 0.147, ("deconv", 8): 0.203, ("deconv", 1000): 1.08,
    ("deconv", 1024): 0.732, ("deconv", 8192): 0.927, ("deconv", 16384): 1.11, ("deconv", 32768): 1.02,
    ("deconv", 100000): 1.48, ("deconv", 1048576): 1.43,
    ("csm", 32): 1.69, ("csm", 1000): 16.8, ("csm", 1024): 16.7, ("csm", 4096): 14.7, ("csm", 16384): 21,
    ("csm", 32768): 24.2,
}


def tolerance(tk):
    """the bound of one (family or Welch kind, length): 1e-6 where the emulation keeps a quarter of it, else four times the
    emulation's worst error (and the margin for another host's rounding)"""
    e = EMULATION[tk] * HOST_MARGIN
    return BASE_TOL if e <= 0.25 else 4.0 * e * BASE_TOL


# ---- the restatements: dt = numpy.float64 is the oracle, numpy.float32 the single-precision emulation ----------------
def _cdt(dt):
    # (long double: the oracle of the float64 Welch entries, tests/x64_cases.py)
    return np.complex64 if dt == np.float32 else np.clongdouble if dt == np.longdouble else np.complex128


def frames(x, W, hop, n_frames, pad_front=0):
    """x (n, C) -> (C, F, W): frame k = samples [k hop - pad_front, k hop - pad_front + W), 0 outside the signal"""
    n = x.shape[0]
    buf = np.zeros((x.shape[1], max(pad_front + n, (n_frames - 1) * hop + W)), x.dtype)
    buf[:, pad_front:pad_front + n] = x.T
    return buf[:, hop * np.arange(n_frames)[:, None] + np.arange(W)[None, :]]


def frame_spectra(x, w, W, hop, n_frames, detrend, nfft=None, pad_front=0, dt=np.float64):
    """x (n, C), w (W,) -> (nfft/2 + 1, F, C) spectra of the windowed (and detrended) frames.  (The samples of a frame
    lie along the last, contiguous axis: numpy then sums the mean pairwise, as a reduction tree on a device does; a
    running float32 sum over 2^20 samples would be an emulation of nothing.)"""
    f = np.ascontiguousarray(frames(np.asarray(x, dt), W, hop, n_frames, pad_front) * np.asarray(w, dt))
    if detrend:
        f -= f.mean(axis=-1, keepdims=True)
    return sfft.rfft(f, n=nfft, axis=-1).transpose(2, 1, 0)


def average_frames(P, average):
    """P (B, F, ...) -> (B, ...): the mean, or the reference's median with its bias n"""
    if average == "mean":
        return P.mean(axis=1)
    F = P.shape[1]
    m = np.median(P.real, axis=1)
    if np.iscomplexobj(P):
        m = m + 1j * np.median(P.imag, axis=1)
    return m * max(1, F if F % 2 else F - 1)


def finish(S, norm_scale, factor, halve_edges, amp_sqrt):
    S = S * norm_scale
    if halve_edges:
        S = S * factor
        S[0] /= 2
        S[-1] /= 2
    return np.sqrt(S) if amp_sqrt else S


def welch(kind, x, y, w, W, hop, n_frames, detrend, average, mode, amp_sqrt, norm_scale, factor, halve_edges,
          dt=np.float64):
    """x (n, n_cx), y (n, n_cy) or None -> psd (B, n_cx) real; csd (B, n_ch) complex; tf: (H (B, n_cy), coherence)"""
    fin = lambda P: finish(average_frames(P, average), norm_scale, factor, halve_edges, amp_sqrt)
    X = frame_spectra(x, w, W, hop, n_frames, detrend, dt=dt)
    if kind == "psd":
        return fin(np.abs(X) ** 2)
    Y = frame_spectra(y, w, W, hop, n_frames, detrend, dt=dt)
    if kind == "csd":
        return fin(X.conj() * Y)
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
        coh = np.abs(Gxy) ** 2 / Gxx / Gyy
    return tf, coh


def stft(x, w, W, hop, nfft, pad_front, n_frames, detrend, scale, edge_scale, power, dt=np.float64):
    """x (n, C) -> (nfft/2 + 1, F, C)"""
    S = frame_spectra(x, w, W, hop, n_frames, detrend, nfft, pad_front, dt)
    S[0] *= dt(edge_scale)
    if nfft % 2 == 0:
        S[-1] *= dt(edge_scale)
    return np.abs(S) ** 2 * dt(scale) if power else S * dt(scale)


def istft(spec, w, nfft, W, step, frame_offset, n_frames_total, scale, total, dt=np.float64):
    """spec (B, F, C) -> (total, C)"""
    s = np.array(spec, _cdt(dt))
    s[0].imag = 0
    if nfft % 2 == 0 and s.shape[0] > nfft // 2:
        s[nfft // 2].imag = 0
    w = np.asarray(w, dt)
    fr = sfft.irfft(s, n=nfft, axis=0, norm="forward")[:W] * dt(scale) * w[:, None, None]
    td, env = np.zeros((total, s.shape[2]), dt), np.zeros(total, dt)
    for f in range(s.shape[1]):
        a = (f + frame_offset) * step
        m = max(0, min(W, total - a))
        td[a:a + m] += fr[:m, f]
    for f in range(n_frames_total):
        a = f * step
        m = max(0, min(W, total - a))
        env[a:a + m] += w[:m] ** 2
    return td / np.clip(env, dt(1e-4), None)[:, None]


def fir(x, taps, mode, dt=np.float64):
    """x (n, C), taps (K, T) -> (K or 1, C, n)"""
    x, taps, n = np.asarray(x, dt), np.asarray(taps, dt), x.shape[0]
    one = lambda sig, b: oaconvolve(sig, b[:, None], mode="full", axes=0)[:n]
    if mode == "sequential":
        y = x
        for b in taps:
            y = one(y, b)
        return y.T[None]
    bands = np.stack([one(x, b).T for b in taps])
    return bands.sum(axis=0)[None] if mode == "summed" else bands


def rfft(x, n_fft, scale, dt=np.float64):
    """x (C, n) -> (n_fft/2 + 1, C)"""
    return (sfft.rfft(np.asarray(x, dt), n=n_fft, axis=1) * dt(scale)).T


def deconv(y, r, n_items, n_ch, n_fft, n_out, dt=np.float64):
    """y (items x C, n), r (1 or C, B) -> (items, C, n_out)"""
    P = sfft.rfft(np.asarray(y, dt), n=n_fft, axis=1).reshape(n_items, n_ch, -1) * np.asarray(r, _cdt(dt))[None]
    P[..., 0].imag = 0
    if n_fft % 2 == 0:
        P[..., -1].imag = 0
    return sfft.irfft(P, n=n_fft, axis=2)[..., :n_out]


def _threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", 0)) or min(8, os.cpu_count() or 1)))


def _pair_averages(Xr, Xi, ii, jj, average):
    """Xr, Xi (b, C, F) real and imaginary parts of the spectra -> (b, pairs): the average over frames of
    X_i conj(X_j) for the pairs (ii, jj).  The frames lie along the last, contiguous axis, parts apart: the median is
    then a selection within rows of F numbers."""
    a, b, c, d = Xr[:, ii], Xi[:, ii], Xr[:, jj], Xi[:, jj]
    P = np.empty(a.shape, _cdt(Xr.dtype.type))
    P.real = a * c + b * d
    P.imag = b * c - a * d
    return average_frames(P.transpose(0, 2, 1), average)


def csm(x, w, W, hop, n_frames, detrend, average, amp_sqrt, norm_scale, factor, halve_edges, dt=np.float64):
    """x (n, C) -> (W/2 + 1, C, C)"""
    X = frame_spectra(x, w, W, hop, n_frames, detrend, dt=dt)
    B, F, C = X.shape
    if average == "mean" and not amp_sqrt:
        S = np.matmul(X.transpose(0, 2, 1), X.conj()) / dt(F)
        return finish(S, norm_scale, factor, halve_edges, 0)
    # the lower triangle only, in chunks of bins of about 64 MB of pair products, on a few threads (numpy's median
    # releases the interpreter): 130 channels x 192 frames x 513 bins are 1.7e9 numbers to select from
    ii, jj = np.tril_indices(C)
    Xt = X.transpose(0, 2, 1)
    Xr, Xi = np.ascontiguousarray(Xt.real), np.ascontiguousarray(Xt.imag)
    S = np.zeros((B, C, C), X.dtype)
    step = max(1, (1 << 22) // (F * len(ii)))
    chunks = [(b, min(B, b + step)) for b in range(0, B, step)]
    work = lambda c: _pair_averages(Xr[c[0]:c[1]], Xi[c[0]:c[1]], ii, jj, average)
    if len(chunks) > 1 and _threads() > 1:
        with ThreadPoolExecutor(_threads()) as pool:
            parts = list(pool.map(work, chunks))
    else:
        parts = [work(c) for c in chunks]
    for (b0, b1), part in zip(chunks, parts):
        S[b0:b1, ii, jj] = part
    S = finish(S, norm_scale, factor, halve_edges, amp_sqrt)  # (of the lower triangle, as the reference)
    S[:, jj, ii] = np.where((ii != jj)[None], S[:, ii, jj].conj(), S[:, ii, jj])
    return S


def compute(p, dt=np.float64):
    """The answer to one problem of route_cases, on the float32 arrays the entries are handed, in precision dt."""
    fam = p["family"]
    if fam == "welch":
        return welch(p["kind"], p["xp"].T, None if p["kind"] == "psd" else p["yp"].T, p["w"], p["W"], p["hop"],
                     p["n_frames"], p["detrend"], p["average"], p["mode"], p["amp_sqrt"], p["norm_scale"], p["factor"],
                     p["halve_edges"], dt)
    if fam == "stft":
        return stft(p["xp"].T, p["w"], p["W"], p["hop"], p["nfft"], p["pad_front"], p["n_frames"], p["detrend"],
                    p["scale"], p["edge_scale"], p["power"], dt)
    if fam == "istft":
        return istft(p["spec32"], p["w"], p["nfft"], p["W"], p["step"], p["frame_offset"], p["n_frames_total"],
                     p["scale"], p["total"], dt)
    if fam == "fir":
        return fir(p["xp"].T[:p["n"]], p["taps"], p["mode"], dt)
    if fam == "rfft":
        return rfft(p["xp"], p["n_fft"], p["scale"], dt)
    if fam == "deconv":
        return deconv(p["yp"], p["r"], p["n_items"], p["n_ch"], p["n_fft"], p["n_out"], dt)
    if fam == "csm":
        return csm(p["xp"].T, p["w"], p["W"], p["hop"], p["n_frames"], p["detrend"], p["average"], p["amp_sqrt"],
                   p["norm_scale"], p["factor"], p["halve_edges"], dt)
    raise KeyError(fam)


# ---- one oracle per problem, shared by its three or five entries ----------------------------------------------------------
CACHE_BYTES = 400 << 20  # (a 130-channel matrix at 513 bins alone is 138 MB)
_cache: OrderedDict = OrderedDict()
seconds = {"oracle": 0.0}  # CPU time spent computing oracles (the tests print what a case added)


def _nbytes(v):
    return sum(a.nbytes for a in v) if isinstance(v, tuple) else v.nbytes


def oracle(p):
    ref = _cache.get(p["ident"])
    if ref is None:
        t0 = time.perf_counter()
        ref = compute(p)
        seconds["oracle"] += time.perf_counter() - t0
        _cache[p["ident"]] = ref
        while len(_cache) > 1 and sum(_nbytes(v) for v in _cache.values()) > CACHE_BYTES:
            _cache.popitem(last=False)
    else:
        _cache.move_to_end(p["ident"])
    return ref


# ---- an oracle in the layout of one entry, with the scale of every element ------------------------------------------------
def _rms(a, axis):
    return np.sqrt(np.mean(np.abs(a) ** 2, axis=axis, keepdims=True))


def targets(p, entry, ref):
    """[(name, oracle in the entry's layout, scale (broadcasts to it), dtype of the output, judged bins)] of the arrays
    a call of `entry` on p returns"""
    fam, f64 = p["family"], entry.endswith("_f64")
    every = slice(None)
    if fam == "welch":
        bins = slice(1, None) if (p["kind"] == "tf" and p["detrend"]) else every
        if p["kind"] == "tf":
            return [("tf", ref[0], _rms(ref[0][bins], 0), np.complex64, bins),
                    ("coherence", ref[1], np.ones((1, 1)), np.float32, bins)]
        return [(p["kind"], ref, _rms(ref, 0), np.float32 if p["kind"] == "psd" else np.complex64, every)]
    if fam == "stft":
        return [("stft", ref, _rms(ref, 0), np.complex128 if f64 else np.complex64, every)]
    if fam == "istft":  # host float64: the reference's (samples, channels); otherwise planar rows
        return [("istft", ref, _rms(ref, 0), np.float64, every)] if f64 else \
               [("istft", ref.T, _rms(ref, 0).T, np.float32, every)]
    if fam == "fir":  # host float64: (bands, samples, channels)
        s = _rms(ref, 2)
        return [("fir", ref.transpose(0, 2, 1), s.transpose(0, 2, 1), np.float64, every)] if f64 else \
               [("fir", ref, s, np.float32, every)]
    if fam == "rfft":
        return [("rfft", ref, _rms(ref, 0), np.complex128 if f64 else np.complex64, every)]
    if fam == "deconv":  # host float64: one item, (samples, channels)
        s = _rms(ref, 2)
        return [("deconv", ref[0].T, s[0].T, np.float64, every)] if f64 else [("deconv", ref, s, np.float32, every)]
    if fam == "csm":
        part = ref[p["b0"]:p["b0"] + p["bc"]]
        d = np.einsum("bii->bi", part).real
        return [("csm", part, _rms(np.sqrt(d[:, :, None] * d[:, None, :]), 0), np.complex64, every)]
    raise KeyError(fam)


def judge(name, out, ref, scale, tol, dtype=None, bins=slice(None)):
    """Shape and dtype, finiteness, then |out - ref| <= tol * scale elementwise; an element whose scale is 0 must be 0.
    -> the worst error as a fraction of its bound."""
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert dtype is None or out.dtype == dtype, (name, out.dtype, dtype)
    out, ref = out[bins], ref[bins]
    assert np.all(np.isfinite(out)), (name, "not finite at", np.argwhere(~np.isfinite(out))[:8].tolist())
    scale = np.broadcast_to(scale, ref.shape)
    zero = scale == 0
    if zero.any():
        assert not out[zero].any(), (name, "must be zero, is not at", np.argwhere(zero & (out != 0))[:8].tolist())
    err = np.abs(out.astype(ref.dtype) - ref)
    ratio = np.divide(err, tol * scale, out=np.zeros_like(err), where=~zero)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    worst = float(ratio[at]) if ratio.size else 0.0
    assert worst <= 1.0, (name, "index", tuple(int(i) for i in at), "error / scale", float(err[at] / scale[at]), "tol", tol,
                          "out", out[at], "oracle", ref[at])
    return worst


def judge_case(key, entry, p, out, tol=None):
    """Every array one call returned against the problem's oracle -> the worst fraction of the bound."""
    tol = tolerance(tol_key(p)) if tol is None else tol
    outs = out if isinstance(out, tuple) else (out,)
    tg = targets(p, entry, oracle(p))
    assert len(outs) == len(tg), (key, len(outs))
    worst = 0.0
    for o, (name, ref, scale, dtype, bins) in zip(outs, tg):
        if o.ndim == 1 and ref.ndim > 1:  # the device Welch entries hand their rows back flat
            o = o.reshape(ref.shape)
        worst = max(worst, judge(f"{key} {name}", o, ref, scale, tol, dtype, bins))
        if p["family"] == "csm":  # as Hermitian as the oracle (which is exactly): |out_ij - conj(out_ji)| within the bound
            skew = o.astype(np.complex128) - o.conj().transpose(0, 2, 1)
            worst = max(worst, judge(f"{key} out - out^H", skew, np.zeros_like(skew), scale, tol))
    return worst


def judge_rejected(key, entry, out):
    """A refused call has written nothing: the helper's host arrays are still the zeros it made them.  (A device entry's
    output buffer was never initialised, so there is nothing to hold it to.)"""
    if entry.endswith("_dev"):
        return
    for o in (out if isinstance(out, tuple) else (out,)):
        assert not o.any(), (key, "a rejected call wrote its output at", np.argwhere(o != 0)[:8].tolist())


def tol_key(p):
    """(family or Welch kind, transform length): what a tolerance is recorded per.  The inverse STFT divides by the
    window envelope, down to 1e-4 at the ends of the signal, which multiplies every rounding there: how much depends on
    whether the window fills the frame, so its two window kinds are recorded apart."""
    fam = p["family"]
    if fam == "welch":
        return (p["kind"], p["W"])
    if fam == "istft":
        return ("istft_short" if p["short"] else "istft", p["nfft"])
    return (fam, p.get("nfft", p.get("n_fft", p.get("n_taps", p.get("W")))))


def emulation_fraction(p):
    """The float32 emulation's worst error / (1e-6 * scale) over the problem's outputs."""
    ref, emu = oracle(p), compute(p, np.float32)
    entry = {"welch": p.get("kind"), "csm": "csm"}.get(p["family"], p["family"])
    emus = emu if isinstance(emu, tuple) else (emu,)
    worst = 0.0
    for e, (name, r, scale, _, bins) in zip(emus, targets(p, entry, ref)):
        if p["family"] == "istft":
            e = e.T
        if p["family"] == "csm":
            e = e[p["b0"]:p["b0"] + p["bc"]]
        e, r = e[bins], r[bins]
        s = np.broadcast_to(scale, r.shape)
        worst = max(worst, float(np.max(np.abs(e.astype(r.dtype) - r)[s > 0] / (BASE_TOL * s[s > 0]), initial=0.0)))
    return worst
