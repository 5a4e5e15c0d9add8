"""The problems of the route matrices of tests/test_gpu_parity.py, rebuilt without a device.

Every builder is pure numpy: matrix key -> a dict of inputs (float64 as drawn, the float32 arrays the entries are
handed), shapes and entry parameters.  test_gpu_parity.py calls the library on these problems, route_oracles.py states
what the answer is, test_route_oracles_host.py checks both on a machine without a GPU.  Seeds, shapes and keys are the
ones the route tables (tests/golden/*_routes.json) were recorded with; routes do not depend on sample values.

A problem does not depend on which entry of its family (host float32, host float64 layout, device-resident) runs it:
`ident` names it, and is what an oracle is cached under."""

import numpy as np

# backend.DS_AVG / DS_TF / DS_FB_* (include/dsptoolbox_amd.h); test_route_oracles_host.py checks them against backend
DS_AVG = {"mean": 0, "median": 1}
DS_TF = {"H1": 1, "H2": 2, "H3": 3}
DS_FB = {"parallel": 1, "sequential": 2, "summed": 3}

WELCH_ROUTE_WINDOWS = [32, 64, 128, 256, 1024, 2048, 4096, 8192, 16384, 32768, 2**20]
# the transfer function, auto and cross spectra: host float32, host float64 and (tf, psd) device-resident entries
WELCH_ROUTE_ENTRIES = {"tf": ("tf", "tf_f64", "tf_dev"), "psd": ("psd", "psd_f64", "psd_dev"), "csd": ("csd", "csd_f64")}
STFT_ROUTE_NFFTS = [8, 16, 32, 64, 128, 256, 512, 1000, 1024, 2048, 4096, 8192, 16384, 32768, 262144, 2**19, 2**20]
ISTFT_ROUTE_NFFTS = [16, 256, 1000, 1024, 2048, 4096, 8192, 16384, 32768, 2**19]
STFT_ROUTE_ENTRIES = {"stft": ("stft", "stft_f64", "stft_dev"), "istft": ("istft", "istft_f64", "istft_dev")}
FIR_ROUTE_TAPS = [1, 2, 64, 1024, 1025, 2049, 4097, 8193, 2**15 + 1]
FIR_ROUTE_MODES = ("parallel", "summed", "sequential")
# (entry, output row stride): "odd" = a device output stride that is not a multiple of 4 (no plain 16k blocks)
FIR_ROUTE_ENTRIES = (("fir_ola", "n"), ("fir_ola_f64", "n"), ("fir_ola_dev", "n"), ("fir_ola_dev", "odd"))
XFORM_ROUTE_NFFTS = [1, 2, 3, 4, 8, 1000, 1024, 8192, 16384, 32768, 100000, 2**20]
CSM_ROUTE_WINDOWS = [32, 1000, 1024, 4096, 16384, 32768]
TF_TAPS = 24  # length of the seeded FIR between input and output of a transfer-function problem


def hann32(W):
    """the periodic Hann window the helpers hand to every entry, float32"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(W) / W)).astype(np.float32)


def planar32(a):
    """(samples, channels) float64 -> the (channels, samples) float32 rows a host float32 or device entry takes"""
    return np.ascontiguousarray(np.asarray(a).T, dtype=np.float32)


def tf_responses(rng, n_ch):
    """One short FIR per output channel, as _resident_pair's (decaying Gaussian taps), with the first tap raised
    above the sum of the others: |H_c(f)| >= 0.5 at every frequency, so no bin of Y = H X is left to the noise."""
    h = rng.standard_normal((n_ch, TF_TAPS)) * np.exp(-np.arange(TF_TAPS) / 6.0)
    h[:, 0] = np.abs(h[:, 1:]).sum(axis=1) + 0.5
    return h


def welch_problem(kind, W, hop_div, average, one_in, n_ch=3):
    """One small Welch estimate.  `one_in`: one input channel (transfer function) / one channel (spectra)."""
    hop, n = W // hop_div, 2 * W + 3000
    rng = np.random.default_rng(W + hop_div)
    if kind == "tf":
        # the input first, the outputs from it: y_c = h_c * x + noise is coherent with x at every bin (with
        # x = y_0 / 2 + noise the other outputs were incoherent with it, and H2 = Gyy / Gyx over the 5 frames of a
        # 2^20-sample window was ill-conditioned in float64 itself)
        n_cx = 1 if one_in else n_ch
        x = rng.standard_normal((n, n_cx)) * 0.5
        h = tf_responses(rng, n_ch)
        y = np.stack([np.convolve(x[:, 0 if one_in else c], h[c])[:n] for c in range(n_ch)], axis=1)
        y = y + 0.05 * rng.standard_normal((n, n_ch))
    else:
        y = rng.standard_normal((n, n_ch))
        x = (y[:, :1] if one_in else y) * 0.5 + 0.1 * rng.standard_normal((n, 1 if one_in else n_ch))
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    n_out = n_ch if kind == "tf" else x.shape[1]
    if kind == "csd":  # channel pairs (x_c, y_c)
        y = np.ascontiguousarray(y[:, :n_out])
    return dict(family="welch", ident=("welch", kind, W, hop_div, average, bool(one_in), n_ch), kind=kind, x=x, y=y,
                xp=planar32(x), yp=planar32(y), w=hann32(W), W=W, hop=hop, n=n, n_frames=-(-n // hop), B=W // 2 + 1,
                n_cx=x.shape[1], n_cy=y.shape[1], n_out=n_out, average=average, detrend=1, mode="H2", amp_sqrt=0,
                norm_scale=1.0 / W, factor=2.0, halve_edges=1)


def stft_problem(nfft, short, detrend, n_ch, power=0):
    """One short spectrogram: "short" = a window of 3 nfft / 4 samples, zero padded to nfft."""
    W = 3 * nfft // 4 if short else nfft
    hop, n = W // 2, 2 * nfft + 3000
    rng = np.random.default_rng(nfft + n_ch)
    x = rng.standard_normal((n, n_ch)) * 0.5 + 0.25
    return dict(family="stft", ident=("stft", nfft, bool(short), int(detrend), n_ch, power), x=np.ascontiguousarray(x),
                xp=planar32(x), w=hann32(W), W=W, hop=hop, n=n, nfft=nfft, n_ch=n_ch, pad_front=0,
                n_frames=1 + (n - W) // hop, B=nfft // 2 + 1, detrend=int(detrend), scale=np.float32(1.0 / W),
                edge_scale=np.float32(0.5), power=power)


def istft_problem(nfft, short, step_div, n_ch, drop_last=False):
    """One short inverse transform.  Three channels give an odd output length: the one-sample overlap-add kernel as
    well as the four-sample one.  drop_last: without the last frame, the output as long as with it (the matrices'
    frame counts at 50 % overlap are even up to 1024 points; the fused kernels transform frames in pairs)."""
    W = 3 * nfft // 4 if short else nfft
    step, total = nfft // step_div, 2 * nfft + 3000 + (n_ch == 3)
    n_frames, B = 1 + (total - W) // step - bool(drop_last), nfft // 2 + 1
    rng = np.random.default_rng(nfft + 10 * step_div + n_ch)
    spec = rng.standard_normal((B, n_frames, n_ch)) + 1j * rng.standard_normal((B, n_frames, n_ch))
    return dict(family="istft", ident=("istft", nfft, bool(short), step_div, n_ch, bool(drop_last)), spec=spec,
                spec32=spec.astype(np.complex64), w=hann32(W), W=W, short=bool(short), step=step, total=total, nfft=nfft,
                n_ch=n_ch, n_frames=n_frames, B=B, frame_offset=0, n_frames_total=n_frames, scale=np.float32(1.0 / nfft))


def fir_problem(n_taps, n, n_filt, mode, n_ch=3):
    """One filter bank.  n may be 0 (the call is rejected): the arrays then hold one sample."""
    rng = np.random.default_rng(n_taps + n + n_filt)
    x = rng.standard_normal((max(n, 1), n_ch)) * 0.5 + 0.25
    taps = (rng.standard_normal((n_filt, n_taps)) / np.sqrt(n_taps)).astype(np.float32)
    return dict(family="fir", ident=("fir", n_taps, n, n_filt, mode, n_ch), x=np.ascontiguousarray(x), xp=planar32(x),
                taps=taps, n_taps=n_taps, n=n, ns=max(n, 1), n_filt=n_filt, n_ch=n_ch, mode=mode,
                n_out=n_filt if mode == "parallel" else 1)


def xform_signal(n_fft, short, n_rows, seed):
    """(n_samples, rows x n_samples float64): "full" = n_fft samples, "short" = half of them (rounded up)."""
    n = (n_fft + 1) // 2 if short else n_fft
    return n, np.random.default_rng(seed).standard_normal((n_rows, n)) * 0.5 + 0.25


def rfft_problem(n_fft, short, n_ch):
    """One whole-signal spectrum; x is (channels, samples)."""
    n, x = xform_signal(n_fft, short, n_ch, n_fft + n_ch)
    return dict(family="rfft", ident=("rfft", n_fft, bool(short), n_ch), x=x, xp=np.ascontiguousarray(x, dtype=np.float32),
                n=n, n_fft=n_fft, n_ch=n_ch, B=n_fft // 2 + 1, scale=np.float32(1.0 / n_fft))


def deconv_problem(n_fft, short, r_per_channel, n_items, n_ch=3):
    """One batch of deconvolutions; y is (items x channels, samples), r the inverse spectrum per channel or one for all."""
    n, y = xform_signal(n_fft, short, n_items * n_ch, n_fft + 10 * n_items + r_per_channel)
    B, n_r = n_fft // 2 + 1, (n_ch if r_per_channel else 1)
    rng = np.random.default_rng(n_fft)
    r = (rng.standard_normal((n_r, B)) + 1j * rng.standard_normal((n_r, B))).astype(np.complex64)
    return dict(family="deconv", ident=("deconv", n_fft, bool(short), r_per_channel, n_items, n_ch), y=y,
                yp=np.ascontiguousarray(y, dtype=np.float32), r=r, n=n, n_fft=n_fft, n_ch=n_ch, n_items=n_items,
                r_per_channel=r_per_channel, B=B, n_out=n_fft)


def csm_problem(W, average, n_ch, n_frames, bins):
    """One cross-spectral matrix.  bins: "all", or "part" (ds_csm_bins_dev: a quarter of the bins from the first
    quarter on).  The bin range is not part of `ident`: the oracle is the full matrix, cut by the caller."""
    hop = W // 2
    n, nb = (n_frames - 1) * hop + W, W // 2 + 1
    x = np.random.default_rng(W + n_ch + n_frames).standard_normal((n, n_ch)) * 0.5 + 0.25
    b0, bc = (nb // 4, max(1, nb // 4)) if bins == "part" else (0, nb)
    return dict(family="csm", ident=("csm", W, average, n_ch, n_frames), x=np.ascontiguousarray(x), xp=planar32(x),
                w=hann32(W), W=W, hop=hop, n=n, n_ch=n_ch, n_frames=n_frames, nb=nb, b0=b0, bc=bc, average=average,
                detrend=1, amp_sqrt=0, norm_scale=1.0 / W, factor=2.0, halve_edges=1)


# ---- the matrices: (key, entry, builder arguments) in the order test_gpu_parity.py runs them ---------------------------
def welch_keys(kinds=("tf", "psd", "csd"), windows=WELCH_ROUTE_WINDOWS):
    for kind in kinds:
        for W in windows:
            for hop_div in (2, 4):
                for average in ("mean", "median"):
                    for one_in in (True, False):
                        for entry in WELCH_ROUTE_ENTRIES[kind]:
                            yield f"{entry}|{W}|{hop_div}|{average}|{1 if one_in else 3}", entry, (kind, W, hop_div, average, one_in)


def stft_keys(kind, nffts):
    for nfft in nffts:
        for short in (False, True):
            for a in ((False, True) if kind == "stft" else (2, 4)):  # detrend / step divisor
                for n_ch in ((1, 3) if kind == "stft" else (1, 2, 3)):
                    for entry in STFT_ROUTE_ENTRIES[kind]:
                        yield f"{entry}|{nfft}|{'short' if short else 'full'}|{int(a)}|{n_ch}", entry, (nfft, short, a, n_ch)


def fir_keys(taps_list, modes):
    for n_taps in taps_list:
        for n in (n_taps - 1, 5000, 50000):  # shorter than the filter, a few blocks, several 16k blocks
            for n_filt in (1, 3):
                for mode in modes:
                    for entry, ld in FIR_ROUTE_ENTRIES:
                        yield f"{entry}|{n_taps}|{n}|{n_filt}|{mode}|{ld}", (entry, ld), (n_taps, n, n_filt, mode)


def rfft_keys(nffts):
    for n_fft in nffts:
        for short in (False, True):
            for n_ch in (1, 3):
                for entry in ("rfft", "rfft_f64", "rfft_dev"):
                    yield f"{entry}|{n_fft}|{'short' if short else 'full'}|{n_ch}", entry, (n_fft, short, n_ch)


def deconv_keys(nffts):
    for n_fft in nffts:
        for short in (False, True):
            for rpc in (0, 1):
                for n_items in (1, 2):
                    for entry in ("deconv", "deconv_f64", "deconv_dev") if n_items == 1 else ("deconv", "deconv_dev"):
                        yield f"{entry}|{n_fft}|{'short' if short else 'full'}|{rpc}|{n_items}", entry, (n_fft, short, rpc, n_items)


def csm_keys(windows):
    """Up to 1024-sample windows: 1 ... 130 channels and also 192 frames (three chunks of >= 64 frames under
    CSM_CHUNKS=3); at 4096 samples up to 65 channels; longer windows 1 and 3 channels (a 32768-sample matrix of 130
    channels alone is 2.2 GB)."""
    for W in windows:
        chans = (1, 3, 64, 65, 130) if W <= 1024 else ((1, 3, 64, 65) if W <= 4096 else (1, 3))
        for average in ("mean", "median"):
            for n_ch in chans:
                for n_frames in (4, 8, 192) if W <= 1024 else (4, 8):
                    cases = [("csm", "all"), ("csm_f64", "all"), ("csm_dev", "all")]
                    if average == "mean":
                        cases += [("csm_bins_dev", "all"), ("csm_bins_dev", "part")]
                    for entry, bins in cases:
                        yield f"{entry}|{W}|{average}|{n_ch}|{n_frames}|{bins}", entry, (W, average, n_ch, n_frames, bins)


BUILDERS = {"welch": welch_problem, "stft": stft_problem, "istft": istft_problem, "fir": fir_problem,
            "rfft": rfft_problem, "deconv": deconv_problem, "csm": csm_problem}


def degenerate(p):
    """A problem with nothing to compute, which every entry refuses: a one-point transform, a signal of no samples.
    (The library refuses more, e.g. lengths a route does not take; the route tables record those as "ERR<code>" and
    the judge goes by the recorded call, not by this.)"""
    if p["family"] in ("rfft", "deconv"):
        return p["n_fft"] < 2
    return p["family"] == "fir" and p["n"] == 0
