"""The calls tests/test_feature_entries_gpu.py makes through the C ABI of the feature families (beamformer maps, IIR,
delay-and-sum, CWT, smoothing, direct DFT, the float64 FFT family, LPC, ds_fir_freqz), and how one of them is run.

A call is (entry, [(argument name, value)], [names of its outputs]).  A value is a number, None (a null pointer), a numpy
array (a host pointer) or Dev(array) (uploaded first, a device pointer).  ROUTES are accepted calls at the smallest shapes
where the host shim has a decision to make; REJECTED are the same calls with one argument spoilt, so that the argument
checks refuse them and nothing is launched.  tools/record_feature_contract.py writes what a library answers to
tests/golden/feature_routes.json and feature_rejected.json.  Inputs come from fixed seeds.
"""

import ctypes as C

import numpy as np

PAR, SEQ, SUM = 1, 2, 3  # DS_FB_*


class Dev:
    """An array that is on the device for the call."""

    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr)


def _rng(seed):
    return np.random.default_rng(seed)


def _c128(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _loc(dev):
    return Dev if dev else np.ascontiguousarray


# ---- builders: keyword arguments select the variant -----------------------------------------------------------------
def fir_freqz():
    rng = _rng(1)
    taps = _c128(rng, 2, 3)
    freqs = np.linspace(0.0, 24000.0, 257)
    return "ds_fir_freqz", [("taps", taps), ("n_filt", 2), ("n_taps", 3), ("freqs_hz", freqs), ("n_freq", 257),
                            ("fs_hz", 48000.0), ("out", np.zeros((2, 257), np.complex128))], ["out"]


def _csm_h(rng, n_bins, n_ch, n_grid, dtype):
    a = _c128(rng, n_bins, n_ch, n_ch)
    csm = a @ np.conj(np.swapaxes(a, 1, 2))
    return csm.astype(dtype), _c128(rng, n_bins, n_ch, n_grid).astype(dtype)


def das_map(dev=False, n_bins=2):
    csm, h = _csm_h(_rng(2), n_bins, 3, 5, np.complex64)
    w = _loc(dev)
    return "ds_das_map" + "_dev" * dev, [("csm", w(csm)), ("h", w(h)), ("n_bins", n_bins), ("n_ch", 3), ("n_grid", 5),
                                         ("map", w(np.zeros(5 * n_bins, np.float32)))], ["map"]


def bf_eigh(dev=False):
    csm, _ = _csm_h(_rng(3), 2, 3, 5, np.complex128)
    w = _loc(dev)
    return "ds_bf_eigh" + "_dev" * dev, [("a", w(csm)), ("n_bins", 2), ("n_ch", 3), ("w", w(np.zeros((2, 3)))),
                                         ("v", w(np.zeros((2, 3, 3), np.complex128)))], ["w", "v"]


def bf_eig_map(dev=False, method=0):
    csm, h = _csm_h(_rng(4), 2, 3, 5, np.complex128)
    w = _loc(dev)
    return "ds_bf_eig_map" + "_dev" * dev, [("csm", w(csm)), ("h", w(h)), ("n_bins", 2), ("n_ch", 3), ("n_grid", 5),
                                            ("method", method), ("gamma", 4.0), ("n_eig", 2),
                                            ("map", w(np.zeros(10)))], ["map"]


def bf_cleansc(dev=False):
    csm, h = _csm_h(_rng(5), 2, 3, 5, np.complex128)
    w = _loc(dev)
    return "ds_bf_cleansc" + "_dev" * dev, [("csm", w(csm)), ("h", w(h)), ("n_bins", 2), ("n_ch", 3), ("n_grid", 5),
                                            ("max_iter", 4), ("safety", 0.5), ("remove_diagonal", 1),
                                            ("map", w(np.zeros(10)))], ["map"]


def _sos(n_filt, n_sec):
    sos = np.empty((n_filt, n_sec, 6))
    for f in range(n_filt):
        for k in range(n_sec):
            sos[f, k] = (0.2 + 0.01 * f, 0.4, 0.2 - 0.01 * k, 1.0, -0.3 - 0.05 * k, 0.2 + 0.03 * f)
    return sos


def iir_sos_dev(n=2048, mode=PAR, n_sec=2):
    x = _rng(6).standard_normal((2, n)).astype(np.float32)
    n_out = 2 if mode == PAR else 1
    return "ds_iir_sos_dev", [("x", Dev(x)), ("n_ch", 2), ("ldx", n), ("n_samples", n), ("sos", _sos(2, n_sec)),
                              ("n_filt", 2), ("n_sec", n_sec), ("zi", None), ("mode", mode),
                              ("y", Dev(np.zeros((n_out, 2, n), np.float32))), ("ld_y", n), ("zf", None)], ["y"]


def iir_sos(n=2048, mode=PAR, state=False, n_sec=2):
    rng = _rng(7)
    x = rng.standard_normal((n, 2))
    n_out = 2 if mode == PAR else 1
    zi = 0.1 * rng.standard_normal((2, n_sec, 2, 2)) if state else None
    zf = np.zeros((2, n_sec, 2, 2)) if state else None
    return "ds_iir_sos", [("x", x), ("n_ch", 2), ("n_samples", n), ("sos", _sos(2, n_sec)), ("n_filt", 2),
                          ("n_sec", n_sec), ("zi", zi), ("mode", mode), ("y", np.zeros((n_out, n, 2))),
                          ("zf", zf)], ["y"] + ["zf"] * state


def delay_sum(dev=False, y=True, peak=True):
    rng = _rng(8)
    n_x, n_src, n_rows, n_terms, out_len = 600, 2, 3, 2, 513
    x = rng.standard_normal((n_x, n_src))
    tables = [("src_len", np.array([600, 590], np.int64)), ("n_rows", n_rows), ("n_terms", n_terms),
              ("src", np.array([0, 1, 1, 0, 0, 0], np.int32)), ("shift", np.array([0, 3, -2, 7, 11, 1], np.int64)),
              ("frac", np.array([0.0, 0.25, 0.5, 0.75, 0.1, 0.9])), ("weight", rng.standard_normal(6)), ("order", 3),
              ("beta", 6.0), ("out_len", out_len)]
    pk = ("peak", np.zeros(n_rows) if peak else None)
    outs = ["y"] * y + ["peak"] * peak
    if dev:
        yv = Dev(np.zeros((n_rows, out_len), np.float32)) if y else None
        return "ds_delay_sum_dev", [("x", Dev(x.T.astype(np.float32))), ("n_src", n_src), ("ldx", n_x)] + tables + [
            ("y", yv), ("ld_y", out_len), pk], outs
    yv = np.zeros((out_len, n_rows)) if y else None
    return "ds_delay_sum", [("x", x), ("n_src", n_src), ("n_x", n_x)] + tables + [("y", yv), pk], outs


def _wavelets(rng, lens):
    tap_len = np.array(lens, np.int64)
    return tap_len, _c128(rng, int(tap_len.sum())).astype(np.complex64)


def cwt(dev=False, big=False, f64=False, lens=None):
    rng = _rng(9)
    n, n_ch = (9000, 1) if big else (300, 2)
    tap_len, taps = _wavelets(rng, lens or ([17001] if big else [5, 200]))
    nf = len(tap_len)
    x = rng.standard_normal((n, n_ch))
    if dev:
        return "ds_cwt_dev", [("x", Dev(x.T.astype(np.float32))), ("n_ch", n_ch), ("ldx", n), ("n_samples", n),
                              ("channels", np.arange(n_ch, dtype=np.int32)), ("n_out_ch", n_ch), ("n_freq", nf),
                              ("tap_len", tap_len), ("taps", taps),
                              ("out", Dev(np.zeros((nf, n, n_ch), np.complex64)))], ["out"]
    out = np.zeros((nf, n, n_ch), np.complex128 if f64 else np.complex64)
    return "ds_cwt", [("x", x), ("n_ch", n_ch), ("n_samples", n), ("n_freq", nf), ("tap_len", tap_len), ("taps", taps),
                      ("out_f64", int(f64)), ("out", out)], ["out"]


def cwt_squeeze(norm=True):
    rng = _rng(10)
    s = _c128(rng, 3, 300, 2).astype(np.complex64)
    freqs = np.array([100.0, 200.0, 400.0])
    return "ds_cwt_squeeze_dev", [("s", Dev(s)), ("n_freq", 3), ("n_samples", 300), ("n_ch", 2), ("freqs", freqs),
                                  ("delta_f", 0.1 * freqs), ("norm", (freqs / 1000.0) ** 1.5 if norm else None),
                                  ("fs", 1000.0), ("out", Dev(np.zeros((3, 300, 2), np.complex128)))], ["out"]


def _k_log(n_bins):
    k = np.logspace(0.0, np.log10(n_bins), n_bins)
    k[0], k[-1] = 1.0, float(n_bins)
    return k


def octave_smooth(cplx=False, k_log=False, clip=False):
    rng = _rng(11)
    v = _c128(rng, 9, 2) if cplx else np.abs(rng.standard_normal((9, 2)))
    name = "ds_octave_smooth_complex" if cplx else "ds_octave_smooth"
    return name, [("z" if cplx else "v", v), ("n_bins", 9), ("n_ch", 2), ("k_log", _k_log(9) if k_log else None),
                  ("window", np.array([0.25, 0.5, 0.25])), ("n_window", 3), ("clip", int(clip)),
                  ("out", np.zeros_like(v))], ["out"]


def complex_smooth(domain=0, n_bins=9, n_ch=2, span=False):
    """span: every band is the whole spectrum"""
    z = np.zeros((n_bins, n_ch), np.complex128) if span else _c128(_rng(12), n_bins, n_ch)
    i = np.arange(n_bins)
    lo, hi = np.maximum(i - 1, 0).astype(np.int32), np.minimum(i + 2, n_bins).astype(np.int32)
    if span:
        lo, hi = np.zeros(n_bins, np.int32), np.full(n_bins, n_bins, np.int32)
    wx = np.linspace(-1.0, 1.0, 5)
    return "ds_complex_smooth", [("z", z), ("n_bins", n_bins), ("n_ch", n_ch), ("ind_low", lo), ("ind_high", hi),
                                 ("window_length", np.full(n_bins, n_bins if span else 3, np.int32)),
                                 ("pass", ((i == 0) & (not span)).astype(np.int32)), ("window_x", wx),
                                 ("window_y", 0.5 + 0.5 * np.cos(np.pi * wx)), ("n_window", 5), ("domain", domain),
                                 ("out", np.zeros_like(z))], ["out"]


def dft(dev=False, windowed=False, n_freq=17):
    rng = _rng(13)
    n, n_ch = 1025, 2
    x = rng.standard_normal((n, n_ch))
    tail = [("freqs_hz", np.linspace(10.0, 20000.0, n_freq)), ("n_freq", n_freq), ("fs_hz", 48000.0),
            ("alpha", np.linspace(1.0, 4.0, n_freq) if windowed else None),
            ("peak", np.array([100, 500], np.int64) if windowed else None), ("half", 200.0),
            ("min_weight_log2", -70.0), ("out", np.zeros((n_freq, n_ch), np.complex128))]
    if dev:
        return "ds_dft_dev", [("x", Dev(x.T.astype(np.float32))), ("n_ch", n_ch), ("ldx", n), ("n_samples", n)] + tail, ["out"]
    return "ds_dft", [("x", x), ("n_samples", n), ("n_ch", n_ch)] + tail, ["out"]


def fft_c128(n=8):
    x = _c128(_rng(14), n, 2)
    return "ds_fft_c128", [("in", x), ("in_complex", 1), ("n_in", n), ("n_ch", 2), ("n_fft", n), ("inverse", 0),
                           ("out", np.zeros((n, 2), np.complex128))], ["out"]


def phase(entry="ds_hilbert", flag=0):
    """ds_hilbert, ds_cepstrum (flag: complex cepstrum), ds_from_cepstrum, ds_group_delay_phase at n = 12 x 2 channels"""
    rng = _rng(15)
    n, n_ch = 12, 2
    x = _c128(rng, n, n_ch) if entry == "ds_from_cepstrum" else rng.standard_normal((n, n_ch)) + 3.0 * (np.arange(n) == 0)[:, None]
    head = [("cepstrum" if entry == "ds_from_cepstrum" else "x", x), ("n", n), ("n_ch", n_ch)]
    if entry == "ds_cepstrum":
        return entry, head + [("complex_cepstrum", flag), ("out", np.zeros((n, n_ch), np.complex128))], ["out"]
    if entry == "ds_group_delay_phase":
        return entry, head + [("delta_f", 10.0), ("out", np.zeros((n // 2 + 1, n_ch)))], ["out"]
    out = np.zeros((n, n_ch), np.float64 if entry == "ds_from_cepstrum" else np.complex128)
    return entry, head + [("out", out)], ["out"]


def min_phase(output=0):
    n, n_ch = 12, 2
    x = np.abs(_rng(16).standard_normal((n, n_ch))) + 0.5
    out = np.zeros((n, n_ch), np.complex128) if output == 0 else np.zeros(((n if output == 2 else n // 2 + 1), n_ch))
    return "ds_min_phase", [("x", x), ("n", n), ("n_ch", n_ch), ("n_fft", n), ("output", output), ("n_out", n),
                            ("delta_f", 10.0), ("out", out)], ["out"]


LPC = dict(L=16, order=2, hop=8, n=40, n_ch=2, n_frames=5)


def lpc(dev=False, method=0):
    q = LPC
    x = _rng(17).standard_normal((q["n"], q["n_ch"]))
    tail = [("window", np.hanning(q["L"] + 2)[1:-1].copy()), ("window_length", q["L"]), ("hop", q["hop"]),
            ("order", q["order"]), ("method", method), ("a", np.zeros((q["order"] + 1, q["n_frames"], q["n_ch"]))),
            ("var", np.zeros((q["n_frames"], q["n_ch"]))), ("singular", np.zeros(1, np.int32))]
    if dev:
        return "ds_lpc_dev", [("x", Dev(x.T.astype(np.float32))), ("n_ch", q["n_ch"]), ("ldx", q["n"]),
                              ("n_samples", q["n"])] + tail, ["a", "var", "singular"]
    return "ds_lpc", [("x", x), ("n_samples", q["n"]), ("n_ch", q["n_ch"])] + tail, ["a", "var", "singular"]


def levinson(order=2):
    r = _rng(18).standard_normal((order + 1, 3)) * 0.1
    r[0] = 1.0
    return "ds_levinson", [("r", r), ("order", order), ("n_cols", 3), ("a", np.zeros((order + 1, 3))),
                           ("var", np.zeros(3)), ("singular", np.zeros(1, np.int32))], ["a", "var", "singular"]


def lpc_synth():
    q = LPC
    rng = _rng(19)
    a = 0.1 * rng.standard_normal((q["order"] + 1, q["n_frames"], q["n_ch"]))
    a[0] = 1.0
    return "ds_lpc_synth", [("a", a), ("sources", rng.standard_normal((q["L"], q["n_frames"], q["n_ch"]))),
                            ("window", np.hanning(q["L"] + 2)[1:-1].copy()), ("window_length", q["L"]),
                            ("n_frames", q["n_frames"]), ("n_ch", q["n_ch"]), ("hop", q["hop"]), ("order", q["order"]),
                            ("n_out", q["n"]), ("y", np.zeros((q["n"], q["n_ch"])))], ["y"]


# ---- the accepted calls: key -> (builder, keyword arguments, times called) -------------------------------------------
def _routes():
    r = {"ds_fir_freqz|2x3x257": (fir_freqz, {}, 1)}
    for dev in (False, True):
        d = "_dev" * dev
        r[f"ds_das_map{d}|2x3x5"] = (das_map, dict(dev=dev), 1)
        r[f"ds_bf_eigh{d}|2x3"] = (bf_eigh, dict(dev=dev), 1)
        for m, name in enumerate(("mvdr", "functional", "orthogonal")):
            r[f"ds_bf_eig_map{d}|{name}"] = (bf_eig_map, dict(dev=dev, method=m), 1)
        r[f"ds_bf_cleansc{d}|2x3x5"] = (bf_cleansc, dict(dev=dev), 1)
        for y, peak in ((True, True), (True, False), (False, True)):
            r[f"ds_delay_sum{d}|{'y' * y}{'+' * (y and peak)}{'peak' * peak}"] = (delay_sum, dict(dev=dev, y=y, peak=peak), 1)
        for windowed in (False, True):
            r[f"ds_dft{d}|{'windowed' if windowed else 'plain'}"] = (dft, dict(dev=dev, windowed=windowed), 1)
        r[f"ds_dft{d}|no_frequencies"] = (dft, dict(dev=dev, n_freq=0), 1)
        for m, name in enumerate(("yule_walker", "burg")):
            r[f"ds_lpc{d}|{name}"] = (lpc, dict(dev=dev, method=m), 1)
        r[f"ds_cwt{d}|big"] = (cwt, dict(dev=dev, big=True), 1)
    for n in (2048, 2049):
        for mode, name in ((PAR, "parallel"), (SEQ, "sequential"), (SUM, "summed")):
            r[f"ds_iir_sos_dev|{n}|{name}"] = (iir_sos_dev, dict(n=n, mode=mode), 1)
            for state in (False, True):
                r[f"ds_iir_sos|{n}|{name}|{'state' if state else 'rest'}"] = (iir_sos, dict(n=n, mode=mode, state=state), 1)
    r["ds_cwt_dev|5+200"] = (cwt, dict(dev=True), 1)
    r["ds_cwt|5+200|c64"] = (cwt, dict(), 1)
    r["ds_cwt|5+200|c128"] = (cwt, dict(f64=True), 1)
    for norm in (True, False):
        r[f"ds_cwt_squeeze_dev|{'norm' if norm else 'plain'}"] = (cwt_squeeze, dict(norm=norm), 1)
    for cplx in (False, True):
        for k_log in (False, True):
            for clip in (False, True):
                key = f"ds_octave_smooth{'_complex' * cplx}|{'log' if k_log else 'lin'}|{'clip' if clip else 'noclip'}"
                r[key] = (octave_smooth, dict(cplx=cplx, k_log=k_log, clip=clip), 1)
    for domain in range(6):
        r[f"ds_complex_smooth|domain{domain}"] = (complex_smooth, dict(domain=domain), 1)
    r["ds_fft_c128|8"] = (fft_c128, dict(n=8), 1)
    r["ds_fft_c128|16384"] = (fft_c128, dict(n=16384), 1)
    r["ds_fft_c128|12"] = (fft_c128, dict(n=12), 2)  # Bluestein: the second call finds the chirp tables
    r["ds_hilbert|12"] = (phase, dict(entry="ds_hilbert"), 1)
    r["ds_cepstrum|real"] = (phase, dict(entry="ds_cepstrum", flag=0), 1)
    r["ds_cepstrum|complex"] = (phase, dict(entry="ds_cepstrum", flag=1), 1)
    r["ds_from_cepstrum|12"] = (phase, dict(entry="ds_from_cepstrum"), 1)
    for o, name in enumerate(("spectrum", "phase", "ir", "group_delay")):
        r[f"ds_min_phase|{name}"] = (min_phase, dict(output=o), 1)
    r["ds_group_delay_phase|12"] = (phase, dict(entry="ds_group_delay_phase"), 1)
    r["ds_levinson|2x3"] = (levinson, {}, 1)
    r["ds_lpc_synth|frames"] = (lpc_synth, {}, 1)
    return r


ROUTES = _routes()


# ---- the refused calls: key -> (builder, keyword arguments, {argument: spoilt value}) --------------------------------
FS = 48000.0  # the work-bound cases of test_direct_gpu.py::test_size_guards_raise, null pointers and all
RAW = {
    "ds_dft|work_bound": ("ds_dft", (None, 1 << 24, 1, None, 1 << 40, FS, None, None, 1.0, -70.0, None)),
    "ds_dft_dev|work_bound": ("ds_dft_dev", (None, 1, 1 << 24, 1 << 24, None, 1 << 40, FS, None, None, 1.0, -70.0, None)),
}


def _rejected():
    r = {}

    def add(entry, builder, kw, nulls=(), zeros=(), shorts=(), **more):
        for a in nulls:
            r[f"{entry}|null:{a}"] = (builder, kw, {a: None})
        for a in zeros:
            r[f"{entry}|zero:{a}"] = (builder, kw, {a: 0})
        for a, v in shorts:
            r[f"{entry}|short:{a}"] = (builder, kw, {a: v})
        for label, (kw2, spoil) in more.items():
            r[f"{entry}|{label}"] = (builder, dict(kw, **kw2), spoil)

    add("ds_fir_freqz", fir_freqz, {}, ("taps", "freqs_hz", "out"), ("n_filt", "n_taps", "n_freq", "fs_hz"))
    for dev in (False, True):
        d, kw = "_dev" * dev, dict(dev=dev)
        add("ds_das_map" + d, das_map, kw, ("csm", "h", "map"), ("n_bins", "n_ch", "n_grid"),
            bins65536=(dict(n_bins=65536), {}))
        add("ds_bf_eigh" + d, bf_eigh, kw, ("a", "w", "v"), ("n_bins", "n_ch"), mics65=({}, dict(n_ch=65)),
            bins65536=({}, dict(n_bins=65536)))
        add("ds_bf_eig_map" + d, bf_eig_map, kw, ("csm", "h", "map"), ("n_bins", "n_ch", "n_grid"),
            mics65=({}, dict(n_ch=65)), bins65536=({}, dict(n_bins=65536)), method3=({}, dict(method=3)),
            n_eig0=(dict(method=2), dict(n_eig=0)), n_eig4=(dict(method=2), dict(n_eig=4)))
        add("ds_bf_cleansc" + d, bf_cleansc, kw, ("csm", "h", "map"), ("n_bins", "n_ch", "n_grid", "max_iter", "safety"),
            mics65=({}, dict(n_ch=65)), bins65536=({}, dict(n_bins=65536)), safety2=({}, dict(safety=2.0)))
        add("ds_delay_sum" + d, delay_sum, kw, ("x", "src_len", "src", "shift", "frac", "weight"),
            ("n_src", "n_rows", "n_terms", "out_len", "order"), (("ldx", 599), ("ld_y", 512)) if dev else (("n_x", 599),),
            no_output=(dict(y=False, peak=False), {}), order256=({}, dict(order=256)), beta_negative=({}, dict(beta=-1.0)))
        add("ds_dft" + d, dft, kw, ("x", "freqs_hz", "out"), ("n_samples", "fs_hz"), (("ldx", 1024),) if dev else (),
            windowed_no_peak=(dict(windowed=True), dict(peak=None)), windowed_half0=(dict(windowed=True), dict(half=0.0)),
            negative_frequencies=({}, dict(n_freq=-1)))
        add("ds_lpc" + d, lpc, kw, ("x", "window", "a", "var", "singular"), ("n_samples", "n_ch", "hop", "order"),
            (("ldx", 39),) if dev else (), method2=({}, dict(method=2)), window8193=({}, dict(window_length=8193)),
            order256=({}, dict(window_length=512, order=256)), order_is_window=({}, dict(order=16)))
    for entry, builder, kw in (("ds_iir_sos", iir_sos, dict(state=True)), ("ds_iir_sos_dev", iir_sos_dev, {})):
        add(entry, builder, kw, ("x", "sos", "y"), ("n_ch", "n_samples", "n_filt", "n_sec"),
            (("ldx", 2047), ("ld_y", 2047)) if entry.endswith("_dev") else (), mode9=({}, dict(mode=9)),
            sections33=(dict(n_sec=33), {}), sequential34=(dict(n_sec=17, mode=SEQ), {}))
    add("ds_cwt", cwt, {}, ("x", "tap_len", "taps", "out"), ("n_ch", "n_samples", "n_freq"),
        taps262145=(dict(lens=[5, (1 << 18) + 1]), {}), taps0=(dict(lens=[5, 0]), {}))
    add("ds_cwt_dev", cwt, dict(dev=True), ("x", "channels", "tap_len", "taps", "out"),
        ("n_ch", "n_samples", "n_out_ch", "n_freq"), (("ldx", 299),), taps262145=(dict(lens=[5, (1 << 18) + 1]), {}),
        taps0=(dict(lens=[5, 0]), {}), channel2=({}, dict(channels=np.array([0, 2], np.int32))))
    add("ds_cwt_squeeze_dev", cwt_squeeze, {}, ("s", "freqs", "delta_f", "out"), ("n_freq", "n_ch"), (("n_samples", 1),))
    for cplx in (False, True):
        entry = "ds_octave_smooth" + "_complex" * cplx
        descending = _k_log(9)[::-1].copy()
        add(entry, octave_smooth, dict(cplx=cplx, k_log=True), ("z" if cplx else "v", "window", "out"),
            ("n_bins", "n_ch", "n_window"), k_log_descending=({}, dict(k_log=descending)),
            k_log_short=({}, dict(k_log=np.linspace(1.0, 8.5, 9))), window_sum0=({}, dict(window=np.array([1.0, 0.0, -1.0]))))
    add("ds_complex_smooth", complex_smooth, {},
        ("z", "ind_low", "ind_high", "window_length", "pass", "window_x", "window_y", "out"), (), (("n_window", 1),),
        domain6=({}, dict(domain=6)), domain_negative=({}, dict(domain=-1)),
        band_outside=({}, dict(ind_high=np.full(9, 10, np.int32))), window_x_flat=({}, dict(window_x=np.zeros(5))))
    # 2^20 bins whose bands all span the spectrum: 1.1e12 band terms
    r["ds_complex_smooth|work_bound"] = (complex_smooth, dict(n_bins=1 << 20, n_ch=1, span=True), {})
    long_fft = dict(fft4194305=({}, dict(n=(1 << 22) + 1)), fft8388608=({}, dict(n=1 << 23)))
    add("ds_fft_c128", fft_c128, {}, ("in", "out"), ("n_in", "n_ch", "n_fft"),
        fft4194305=({}, dict(n_fft=(1 << 22) + 1)), fft8388608=({}, dict(n_fft=1 << 23)), channels65536=({}, dict(n_ch=65536)))
    for entry in ("ds_hilbert", "ds_cepstrum", "ds_from_cepstrum", "ds_group_delay_phase"):
        add(entry, phase, dict(entry=entry), ("cepstrum" if entry == "ds_from_cepstrum" else "x", "out"), ("n", "n_ch"),
            **long_fft)
    add("ds_group_delay_phase", phase, dict(entry="ds_group_delay_phase"), (), ("delta_f",), (("n", 1),))
    add("ds_min_phase", min_phase, {}, ("x", "out"), ("n", "n_ch", "n_fft"), output4=({}, dict(output=4)),
        fft4194305=({}, dict(n_fft=(1 << 22) + 1)), fft8388608=({}, dict(n_fft=1 << 23)),
        ir_n_out13=(dict(output=2), dict(n_out=13)), group_delay_delta_f0=(dict(output=3), dict(delta_f=0.0)))
    add("ds_levinson", levinson, {}, ("r", "a", "var", "singular"), ("order", "n_cols"), order256=({}, dict(order=256)))
    add("ds_lpc_synth", lpc_synth, {}, ("a", "sources", "window", "y"), ("n_frames", "n_ch", "hop", "order", "n_out"),
        window8193=({}, dict(window_length=8193)), order256=({}, dict(window_length=512, order=256)),
        order_is_window=({}, dict(order=16)))
    return r


REJECTED = _rejected()


# ---- running one -----------------------------------------------------------------------------------------------------
def call(ctx, entry, args, outs=(), spoil=None):
    """One call through the C ABI -> (return code, error text, sorted launch names, {output name: array})."""
    from dsptoolbox_amd._lib import DeviceBuffer
    held, argv = {}, []
    for name, v in args:
        if spoil and name in spoil:
            v = spoil[name]
        if isinstance(v, Dev):
            held[name] = DeviceBuffer.from_array(ctx, v.arr)
            v = C.c_void_p(held[name].ptr)
        elif isinstance(v, np.ndarray):
            v = v.ctypes.data_as(C.c_void_p)
        argv.append(v)
    assert not spoil or all(k in dict(args) for k in spoil), (entry, spoil)
    ctx.routes()
    try:
        rc = getattr(ctx.lib, entry)(ctx.handle, *argv)
        err = ctx.last_error() if rc else ""
        routes = sorted(ctx.routes())
        got = {}
        if rc == 0:
            for name, v in args:
                if name in outs and v is not None:
                    got[name] = held[name].to_array(v.arr.shape, v.arr.dtype) if isinstance(v, Dev) else v.copy()
    finally:
        for b in held.values():
            b.free()
    return rc, err, routes, got


def run_route(key):
    """The accepted call `key` in a context of its own (what a call launches depends on the tables the context has cached)
    -> ({key: launch names} with key + "|again" for a second call, {key: its outputs})."""
    from dsptoolbox_amd._lib import Context
    builder, kw, times = ROUTES[key]
    entry, args, outs = builder(**kw)
    ctx = Context()
    try:
        routes, got = {}, {}
        for i in range(times):
            k = key + "|again" * i
            rc, err, routes[k], got[k] = call(ctx, entry, args, outs)
            assert rc == 0, (k, rc, err)
    finally:
        ctx.close()
    return routes, got


def run_rejected(ctx, key):
    """The refused call `key` -> "<code>|<message>"; it must launch nothing."""
    if key in RAW:
        entry, argv = RAW[key]
        ctx.routes()
        rc = getattr(ctx.lib, entry)(ctx.handle, *argv)
        err, routes = ctx.last_error(), sorted(ctx.routes())
    else:
        builder, kw, spoil = REJECTED[key]
        entry, args, _ = builder(**kw)
        rc, err, routes, _ = call(ctx, entry, args, (), spoil)
    assert rc != 0 and not routes, (key, rc, routes)
    return f"{rc}|{err}"


REJECTED_KEYS = sorted(list(REJECTED) + list(RAW))
