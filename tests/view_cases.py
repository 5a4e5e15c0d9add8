"""Resident entries on views: the layouts and the cases of tests/test_resident_views_host.py and
tests/test_resident_views_gpu.py.

DESIGN section 3b: a DevicePlanar is an owner buffer plus n_ch, n_samples, a row pitch ld >= n_samples and a byte offset
that is a multiple of four.  The library builds such views itself (a trimmed inverse STFT, a warped response cut to
total_length, the bands of a filter bank) and every resident entry may be handed one.  `layout` builds the worst such view
of given samples: rows at any 4-byte alignment, every element that is no valid sample POISON -- large values of alternating
sign, or NaN -- with margins in front of the first and behind the last row, so that a kernel that reads past a row lands in
poison inside the allocation.  An entry that forms a row base from n_samples, sizes a range from ld, or lets one sample
from outside [0, n_samples) of a row into a result gives another answer on the view than on a dense upload of the same
samples; the GPU test asserts bit equality.

ENTRIES: C-ABI entry name -> list of Case.  Case.build() -> (planes, run) or (planes, run, judge): `planes` the float32
(channels, samples) inputs, `run(ctx, devs)` calls the entry on DevicePlanar objects of those planes (dense or views) and
returns the results as a tuple of host arrays, `judge(out)` holds the dense result to the family's oracle under the
family's bound where the family's own test does not run the shape.  Importing this module needs numpy alone; the library,
scipy and the families' case and oracle modules (some oracles live in the families' test modules) are imported inside the
build, run and judge functions.  The shapes are the edge shapes the families' own case modules list, not workload sizes."""

import ctypes as C
import json
import os
from collections import OrderedDict, namedtuple

import numpy as np

import route_cases as rcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4096  # poison elements in front of the first and behind the last row, at least (or ld, if that is more)
BIG = np.float32(2.0 ** 20)
FILLS = ("big", "nan")
VIEW_NAMES = ("pitched16", "shifted", "rotating")

Case = namedtuple("Case", "entry name build")


# ---- the view builder -------------------------------------------------------------------------------------------------
def poison(size, fill):
    if fill == "nan":
        return np.full(size, np.nan, dtype=np.float32)
    assert fill == "big"
    out = np.full(size, BIG, dtype=np.float32)
    out[1::2] = -BIG
    return out


def margin(ld):
    return max(MARGIN, int(ld))


def VIEWS(n):
    """The three (front, gap) of VIEWS for rows of n samples; front includes the front margin.
    pitched16: the base 16-byte aligned, ld = n + 4 (every row aligned where n % 4 == 0).
    shifted: every row one float past a 16-byte boundary (ld % 4 == 0).
    rotating: front % 4 == 3 and ld % 4 == 3, so that consecutive rows lie at the residues 3, 2, 1, 0."""
    base = -(-margin(n + 8) // 4) * 4
    g2 = (-n) % 4 or 4
    g3 = (3 - n) % 4 or 4
    return ((base, 4), (base + 1, g2), (base + 3, g3))


def layout(x32, front, gap, fill):
    """(owner, ld, offset_bytes) of a (n_ch, n) float32 array: channel c's samples at owner[front + c ld + [0, n)],
    ld = n + gap, offset_bytes = 4 front; every other element is poison, at least margin(ld) of it at either end."""
    x32 = np.asarray(x32)
    assert x32.dtype == np.float32 and x32.ndim == 2
    n_ch, n = x32.shape
    ld = n + int(gap)
    assert front >= margin(ld) and gap >= 0
    owner = poison(front + n_ch * ld + margin(ld), fill)
    for c in range(n_ch):
        owner[front + c * ld:front + c * ld + n] = x32[c]
    return owner, ld, 4 * front


def valid_mask(size, n_ch, n, ld, front):
    m = np.zeros(size, dtype=bool)
    for c in range(n_ch):
        m[front + c * ld:front + c * ld + n] = True
    return m


# ---- helpers of the run functions -------------------------------------------------------------------------------------
def _vp(v):
    return C.c_void_p(v)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    """(samples, channels) float -> (channels, samples) float32"""
    return np.ascontiguousarray(np.asarray(a).T, dtype=np.float32)


def _planars(y):
    """A DevicePlanar or a list of them -> tuple of host arrays"""
    return tuple(p.to_planar() for p in (y if isinstance(y, (list, tuple)) else [y]))


def _freeing(ctx, *arrays):
    from dsptoolbox_amd._lib import DeviceBuffer
    return [DeviceBuffer.from_array(ctx, a) if isinstance(a, np.ndarray) else DeviceBuffer(ctx, int(a)) for a in arrays]


def route_table(name):
    with open(os.path.join(ROOT, "tests", "golden", f"{name}_routes.json")) as fh:
        return json.load(fh)


def distinct(table, keys):
    """The keys (value, table key) whose recorded launch names differ from those of every earlier key: the first -- for
    ascending sizes the smallest -- of each set of launch names; rejected calls (ERR) left out."""
    seen, out = set(), []
    for value, key in keys:
        names = table[key]
        if names.startswith("ERR") or names in seen:
            continue
        seen.add(names)
        out.append(value)
    return out


# ---- the hot path: Welch, STFT, CSM, rFFT, deconvolution, FIR ---------------------------------------------------------
def _welch_case(kind, W, one_in, n_ch=3):
    def build():
        q = rcs.welch_problem(kind, W, 2, "mean", one_in, n_ch)
        planes = [q["xp"], q["yp"]] if kind == "tf" else [q["xp"]]

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            B, n_out = q["B"], q["n_out"]
            tail = (q["detrend"], backend.DS_AVG[q["average"]]) + ((backend.DS_TF[q["mode"]],) if kind == "tf" else ()) + \
                (q["amp_sqrt"], q["norm_scale"], q["factor"], q["halve_edges"])
            dw, do = _freeing(ctx, q["w"], B * n_out * 12)
            dx = devs[0]
            try:
                if kind == "tf":
                    dy = devs[1]
                    ctx.check(ctx.lib.ds_welch_tf_dev(ctx.handle, _vp(dx.ptr), dx.n_ch, dx.ld, _vp(dy.ptr), dy.n_ch, dy.ld, q["n"],
                                                      W, q["hop"], q["n_frames"], _vp(dw.ptr), *tail, _vp(do.ptr),
                                                      _vp(do.ptr + B * n_out * 8)), "ds_welch_tf_dev")
                    raw = do.to_array((B * n_out * 12,), np.uint8)
                    return raw[:B * n_out * 8].view(np.complex64).copy(), raw[B * n_out * 8:].view(np.float32).copy()
                ctx.check(ctx.lib.ds_welch_psd_dev(ctx.handle, _vp(dx.ptr), dx.n_ch, dx.ld, q["n"], W, q["hop"], q["n_frames"],
                                                   _vp(dw.ptr), *tail, _vp(do.ptr)), "ds_welch_psd_dev")
                return (do.to_array((B, n_out), np.float32),)
            finally:
                dw.free(), do.free()

        def judge(out):  # the route matrix judges three channels; held to its oracle and bound here at any count
            import route_oracles as ros
            return ros.judge_case(f"{kind}|{W}", f"{kind}_dev", q, out)
        return planes, run, judge
    return Case(f"ds_welch_{kind}_dev", f"W{W}_{'one' if one_in else 'each'}_{n_ch}ch", build)


def welch_windows(kind):
    t = route_table("welch")
    return distinct(t, [(W, f"default|{kind}|{W}|2|mean|3") for W in rcs.WELCH_ROUTE_WINDOWS])


def _welch_cases(kind):
    out = []
    for W in welch_windows(kind):
        if W <= 32768:
            out += [_welch_case(kind, W, True), _welch_case(kind, W, False)]
        elif kind == "tf":
            # the whole-frame transform (its launch names differ from the 32768 window's).  2 W + 3000 samples a row: two
            # outputs and their one input are 25 MB; a second input row per output would pass the 32 MB a case may take
            out.append(_welch_case(kind, W, True, n_ch=2))
        else:
            out.append(_welch_case(kind, W, False))  # three rows, 25 MB
    return out


def _stft_case(nfft, short):
    def build():
        q = rcs.stft_problem(nfft, short, 1, 3)

        def run(ctx, devs):
            dx = devs[0]
            B, n_frames, n_ch = q["B"], q["n_frames"], q["n_ch"]
            dw, do = _freeing(ctx, q["w"], B * n_frames * n_ch * 8)
            try:
                ctx.check(ctx.lib.ds_stft_r2c_dev(ctx.handle, _vp(dx.ptr), q["n"], n_ch, dx.ld, q["W"], q["hop"], nfft,
                                                  q["pad_front"], n_frames, _vp(dw.ptr), q["detrend"], C.c_float(q["scale"]),
                                                  C.c_float(q["edge_scale"]), q["power"], _vp(do.ptr)), "ds_stft_r2c_dev")
                return (do.to_array((B, n_frames, n_ch), np.complex64),)
            finally:
                dw.free(), do.free()
        return [q["xp"]], run
    return Case("ds_stft_r2c_dev", f"nfft{nfft}_{'short' if short else 'full'}", build)


def stft_nffts():
    """One nfft per distinct PAIR of launch-name sets (full window, short window)."""
    t = route_table("stft")
    seen, out = set(), []
    for nfft in sorted(rcs.STFT_ROUTE_NFFTS):
        pair = (t[f"default|stft|{nfft}|full|1|3"], t[f"default|stft|{nfft}|short|1|3"])
        if pair not in seen:
            seen.add(pair)
            out.append(nfft)
    return out


def _csm_case(entry, W, n_ch):
    def build():
        q = rcs.csm_problem(W, "mean", n_ch, 8, "part" if entry == "ds_csm_bins_dev" else "all")

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            dx = devs[0]
            bc = q["bc"]
            fin = (q["amp_sqrt"], C.c_double(q["norm_scale"]), C.c_double(q["factor"]), q["halve_edges"])
            dw, do = _freeing(ctx, q["w"], bc * n_ch * n_ch * 8)
            try:
                head = (ctx.handle, _vp(dx.ptr), n_ch, dx.ld, q["n"], W, q["hop"], q["n_frames"], _vp(dw.ptr), q["detrend"])
                if entry == "ds_csm_bins_dev":
                    ctx.check(ctx.lib.ds_csm_bins_dev(*head, *fin, q["b0"], bc, _vp(do.ptr)), entry)
                else:
                    ctx.check(ctx.lib.ds_csm_dev(*head, backend.DS_AVG["mean"], *fin, _vp(do.ptr)), entry)
                return (do.to_array((bc, n_ch, n_ch), np.complex64),)
            finally:
                dw.free(), do.free()
        return [q["xp"]], run
    return Case(entry, f"W{W}_{n_ch}ch", build)


def csm_windows(bins):
    t = route_table("csm")
    return distinct(t, [(W, f"default|csm|{W}|mean|3|8|{bins}") for W in rcs.CSM_ROUTE_WINDOWS])


def _rfft_case(n_fft, short):
    def build():
        q = rcs.rfft_problem(n_fft, short, 3)

        def run(ctx, devs):
            dx = devs[0]
            (do,) = _freeing(ctx, q["B"] * 3 * 8)
            try:
                ctx.check(ctx.lib.ds_rfft_dev(ctx.handle, _vp(dx.ptr), 3, dx.ld, q["n"], n_fft, C.c_float(q["scale"]),
                                              _vp(do.ptr)), "ds_rfft_dev")
                return (do.to_array((q["B"], 3), np.complex64),)
            finally:
                do.free()
        return [q["xp"]], run
    return Case("ds_rfft_dev", f"nfft{n_fft}_{'short' if short else 'full'}", build)


def _deconv_case(n_fft, short, rpc):
    def build():
        q = rcs.deconv_problem(n_fft, short, rpc, 2)

        def run(ctx, devs):
            dy = devs[0]  # rows item * n_ch + c
            n_out = q["n_out"]
            dr, do = _freeing(ctx, q["r"], 6 * n_out * 4)
            try:
                ctx.check(ctx.lib.ds_deconv_dev(ctx.handle, _vp(dy.ptr), 2, 3, dy.ld, q["n"], n_fft, _vp(dr.ptr), rpc, n_out,
                                                n_out, _vp(do.ptr)), "ds_deconv_dev")
                return (do.to_array((2, 3, n_out), np.float32),)
            finally:
                dr.free(), do.free()
        return [q["yp"]], run
    return Case("ds_deconv_dev", f"nfft{n_fft}_{'short' if short else 'full'}_r{rpc}", build)


def xform_nffts(kind, rpc=None):
    t = route_table("xform")
    key = (lambda n: f"default|rfft|{n}|full|3") if kind == "rfft" else (lambda n: f"default|deconv|{n}|full|{rpc}|2")
    return distinct(t, [(n, key(n)) for n in rcs.XFORM_ROUTE_NFFTS])


def _fir_case(n_taps):
    def build():
        q = rcs.fir_problem(n_taps, 5000, 3, "parallel")

        def run(ctx, devs):
            dx = devs[0]
            n, n_ch = q["n"], q["n_ch"]
            dt, dy = _freeing(ctx, q["taps"], 3 * n_ch * n * 4)
            try:
                ctx.check(ctx.lib.ds_fir_ola_dev(ctx.handle, _vp(dx.ptr), n_ch, dx.ld, n, _vp(dt.ptr), 3, n_taps,
                                                 rcs.DS_FB["parallel"], _vp(dy.ptr), n), "ds_fir_ola_dev")
                return (dy.to_array((3, n_ch, n), np.float32),)
            finally:
                dt.free(), dy.free()
        return [q["xp"]], run
    return Case("ds_fir_ola_dev", f"taps{n_taps}", build)


def fir_taps():
    t = route_table("fir")
    return distinct(t, [(k, f"default|fir|{k}|5000|3|parallel|n") for k in rcs.FIR_ROUTE_TAPS])


# ---- judging a dense result where the family's own test does not run the shape -------------------------------------------
F32 = 2.0 ** -24 * 1.001  # a resident result is rounded to float32 once: of the stream's peak (test_sfilt_gpu, test_rtfilt_gpu)


def _x64(plane):
    """(channels, samples) float32 -> the (samples, channels) float64 array a host entry or an oracle takes"""
    return np.ascontiguousarray(plane.T, dtype=np.float64)


def _rows(out):
    """planar float32 results (one array per band) -> (bands, samples, channels) float64, one band squeezed"""
    y = np.stack([np.asarray(o, dtype=np.float64).T for o in out])
    return y[0] if len(y) == 1 else y


# ---- recursive filters --------------------------------------------------------------------------------------------------
def _noise(seed, n, n_ch, scale=1.0, offset=0.0):
    x = scale * np.random.default_rng(seed).standard_normal((n, n_ch)) + offset
    return _f32(x)


N_RECURSIVE = 4097  # 2 G + 1: three groups, the carry over groups crossed twice


def _iir_case(mode):
    def build():
        from scipy.signal import butter
        sos = [butter(4, 0.2, output="sos"), butter(2, [0.3, 0.5], btype="band", output="sos"), butter(3, 0.6, "high", output="sos")]

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.iir_sos_filter_device(devs[0], sos, getattr(backend, f"DS_FB_{mode}")))
        x = _noise(301, N_RECURSIVE, 3)

        def judge(out):  # test_iir_gpu's bound against scipy's sosfilt: 1e-6 of the output's largest magnitude
            from scipy.signal import sosfilt
            bands = [sosfilt(q, _x64(x), axis=0) for q in sos]
            if mode == "SUMMED":
                bands = [sum(bands)]
            elif mode == "SEQUENTIAL":
                bands = [sosfilt(np.concatenate(sos), _x64(x), axis=0)]
            want = np.stack(bands)
            got = np.stack([np.asarray(o, dtype=np.float64).T for o in out])
            e = float(np.max(np.abs(got - want)) / np.max(np.abs(want))) / 1e-6
            assert e < 1.0, (mode, e)
            return e
        return [x], run, judge
    return Case("ds_iir_sos_dev", mode.lower(), build)


def _sfilt_case(kind):
    def build():
        import sfilt_cases as sc
        kid, coef, d, aux = sc.pack(sc.structure(kind, sc.SMALL_D[kind]))

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            y, zf = backend.sfilt_filter_device(devs[0], kid, coef, d, aux, want_zf=True)
            return y.to_planar(), zf
        x = _noise(310 + kid, N_RECURSIVE, 3)

        def judge(out):  # the family's bound of this structure at this length (its case has one channel), per channel
            import sfilt_oracle as so
            tol = sc.tolerance(f"{kind}_d{d}_n{N_RECURSIVE}")
            y, zf = so.serial(sc.structure(kind, sc.SMALL_D[kind]), _x64(x), None)
            e = max(so.stream_error(_rows(out[:1]), y) / (tol + F32), so.stream_error(out[1].reshape(-1, 1), zf.reshape(-1, 1)) / tol)
            assert e <= 1.0, (kind, e)
            return e
        return [x], run, judge
    return Case("ds_sfilt_dev", kind, build)


SFILT_KINDS = ("fir_lattice", "iir_lattice", "sos_lattice", "warped_fir", "warped_iir", "kautz")
RTFILT_KINDS = ("svf", "tdf2", "parallel", "state_space")


def _rtfilt_case(kind, delay=0, fir=False):
    def build():
        import rtfilt_cases as rc
        kid, coef, d, aux, dl, taps = rc.pack(rc.structure(kind, rc.SMALL_D[kind], delay=delay, fir=fir))

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            y, zf = backend.rtfilt_filter_device(devs[0], kid, coef, d, aux, dl, taps, want_zf=True)
            return _planars(y) + (zf,)
        x = _noise(320 + kid + delay, N_RECURSIVE, 3)

        def judge(out):  # the family's bound of this filter at this length, per channel and band
            import rtfilt_oracle as ro
            name = f"{kind}_d{d}_n{N_RECURSIVE}" + (f"_delay{delay}" if delay else "") + ("_fir" if fir else "")
            tol = rc.tolerance(name)
            y, zf = ro.serial(rc.structure(kind, rc.SMALL_D[kind], delay=delay, fir=fir), _x64(x), None)
            e = max(ro.stream_error(_rows(out[:-1]), y) / (tol + F32), ro.stream_error(out[-1].reshape(-1, 1), zf.reshape(-1, 1)) / tol)
            assert e <= 1.0, (name, e)
            return e
        return [x], run, judge
    return Case("ds_rtfilt_dev", kind + (f"_delay{delay}" if delay else "") + ("_fir" if fir else ""), build)


def _rtfir_case(order):
    def build():
        import rtfilt_cases as rc
        n = rc.FIR_TILE + 1
        b = np.random.default_rng(330 + order).standard_normal(order + 1)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.rtfir_filter_device(devs[0], b))
        x = _noise(331 + order, n, 3)

        def judge(out):  # the forward error bound of the float64 dot product per element, and one rounding to float32
            import rtfilt_oracle as ro
            y = ro.fir_direct(b, _x64(x), None)
            bound = (order + 1) * rc.EPS * ro.fir_direct(np.abs(b), np.abs(_x64(x)), None) + F32 * np.abs(y)
            e = float(np.max(np.abs(_rows(out) - y) / np.asarray(bound, dtype=np.float64)))
            assert e <= 1.0, (order, e)
            return e
        return [x], run, judge
    return Case("ds_rtfir_dev", f"order{order}", build)


# ---- two operands, staged --------------------------------------------------------------------------------------------
def _pair_moments_case():
    def build():
        n = 4097  # PAIR_SPAN + 1
        a, b = _noise(340, n, 1, 0.5, 0.1), _noise(341, n, 3, 0.5, -0.2)
        par = np.random.default_rng(342).standard_normal((3, 3)) * 0.1

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.pair_moments_device(devs[0], devs[1], par),)

        def judge(out):
            """Against the sums in long double.  Each of the n terms carries at most four roundings (the products and
            differences that form it) and the sum, in any order, at most n - 1 more: |error| <= (n + 3) eps64 sum |term|."""
            LD = np.longdouble
            A, B = _x64(a).astype(LD), _x64(b).astype(LD)
            worst = 0.0
            for c in range(3):
                u, v = A[:, 0], B[:, c]
                al, mu_a, mu_b = (LD(t) for t in par[c])
                terms = [(u - mu_a) ** 2, (v - mu_b) ** 2, u * v, u, v, (al * u - v) ** 2]
                for k, t in enumerate(terms):
                    bound = (n + 3) * np.finfo(np.float64).eps * float(np.sum(np.abs(t)))
                    worst = max(worst, abs(float(LD(out[0][c, k]) - np.sum(t))) / bound)
            assert worst <= 1.0, worst
            return worst
        return [a, b], run, judge
    return Case("ds_pair_moments_dev", "one_against_three_n4097", build)


def _fw_snr_case():
    """ciir_cases' own "one_against_three" (601 samples at 8000 Hz: one sample past the 600-sample window), its samples
    rounded to float32, through the public function; judged against the family's oracle of the rounded samples under the
    family's tolerance of that case."""
    name = "one_against_three"

    def build():
        import ciir_cases as cc
        spec = cc.FW[name]
        x, xhat = (_f32(v) for v in cc.fw_problem(name)[:2])

        def run(ctx, devs):
            import dsptoolbox_amd as dsp
            sx, sh = (dsp.Signal.from_planar_f32(d, spec["fs"]) for d in devs)
            return (dsp.distances.fw_snr_seg(sx, sh, f_range_hz=spec["f_range"]),)

        def judge(out):
            import ciir_oracle as co
            from scipy.signal import windows
            sos = cc.gammatone_sos(np.sort(spec["f_range"]), spec["fs"])
            xb, xhb = co.bank_ld(sos, _x64(x))[0].real, co.bank_ld(sos, _x64(xhat))[0].real
            window = windows.hamming(cc.window_length(spec["fs"]), sym=False)
            want = np.array([co.fw_frames_ld(xb[:, :, 0].T, xhb[:, :, c].T, window, [-10, 35], 0.2)[1] for c in range(3)])
            e = float(np.max(np.abs(out[0] - want))) / cc.fw_tolerance(name)
            assert e <= 1.0, (out[0], want)
            return e
        return [x, xhat], run, judge
    return Case("ds_fw_snr_seg_dev", "one_against_three_n601", build)


def _delay_sum_case():
    def build():
        n, out_len = 700, 900
        x = _noise(360, n, 3, 0.5)
        src_len = np.array([n, n - 1, 333])  # some below n: what lies behind them reads as zero
        src = np.array([[0, 1], [2, 0], [1, 2], [2, 2]])
        shift = np.array([[0, 5], [-3, 100], [250, -1], [7, 400]])
        frac = np.array([[0.25, -1.0], [0.5, 0.0], [0.75, 0.125], [-1.0, 0.9]])
        weight = np.array([[1.0, 0.5], [-0.5, 0.25], [0.3, 0.7], [1.0, -1.0]])

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.delay_sum_device(devs[0], src_len, src, shift, frac, weight, 11, 60.0, out_len))

        def judge(out):  # test_delay_sum_oracle's oracle, row scale and bound of the device entry
            import test_delay_sum_oracle as tdo
            ref, scale = tdo.oracle(_x64(x), src_len, src, shift, frac, weight, 11, out_len)
            return tdo.judge(dict(name="src_len_below_n"), _rows(out), ref, scale, tdo.TOL_DEV)
        return [x], run, judge
    return Case("ds_delay_sum_dev", "src_len_below_n", build)


def _stack_case():
    def build():
        lens = (500, 301, 444)
        planes = [_noise(370 + i, n, 1) for i, n in enumerate(lens)]

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.stack_device(list(devs), lens))

        def judge(out):  # a pass-through: every row its samples exactly, zeros behind them
            want = np.zeros((len(lens), max(lens)), dtype=np.float32)
            for j, p in enumerate(planes):
                want[j, :lens[j]] = p[0]
            assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
            return 0.0
        return planes, run, judge
    return Case("backend.stack_device", "three_rows", build)


# ---- one edge case of each family -----------------------------------------------------------------------------------------
def _cwt_case():
    def build():
        import cwt_cases as cw
        case = next(c for c in cw.block_cases() if c.name == "block-M256-2V+1")
        rng = np.random.default_rng(380)
        waves = []
        for L in case.lengths:
            w = rng.standard_normal(L) + 1j * rng.standard_normal(L)
            waves.append(w / np.abs(w).sum())
        x = _f32(cw.signal(case.n, 3))

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.cwt_device(devs[0], [2, 0, 1], waves).to_host(),)

        def judge(out):  # the family's bound: every row within cwt_cases.TOL of its channel's peak
            td = _x64(x)[:, [2, 0, 1]]
            e = float(cw.row_ratios(out[0], cw.direct_scalogram(td, waves), td).max())
            assert e <= 1.0, e
            return e
        return [x], run, judge
    return Case("ds_cwt_dev", "block-M256-2V+1_3ch", build)


def _dft_cases():
    def plain():
        freqs = np.random.default_rng(390).uniform(-1000.0, 30000.0, 17)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.dft(devs[0], freqs, 48000),)
        x = _noise(391, 1025, 3)

        def judge(out):  # test_direct_gpu's bound of the float64 sums: 1e-9 of the channel's largest bin
            import test_direct_host as dh
            e = dh.channel_error(out[0], dh.ref_dft(_x64(x), freqs, 48000)) / 1e-9
            assert e <= 1.0, e
            return e
        return [x], run, judge

    def windowed():
        n = 3000
        freqs = np.linspace(100.0, 20000.0, 16)
        alpha = np.linspace(1.0, 40.0, 16)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.windowed_dft(devs[0], freqs, 48000, alpha, np.array([1500, 10, 2990]), 400.0),)
        x = _noise(392, n, 3)

        def judge(out):
            import test_direct_host as dh
            ref = dh.ref_windowed_sum(_x64(x), freqs, 48000, alpha, np.array([1500, 10, 2990]), 400.0)
            e = dh.channel_error(out[0], ref) / 1e-9
            assert e <= 1.0, e
            return e
        return [x], run, judge
    return [Case("ds_dft_dev", "n1025_f17", plain), Case("ds_dft_dev", "windowed_n3000", windowed)]


def _lpc_cases():
    out = []
    for method in ("yule_walker", "burg"):
        def build(method=method):
            import lpc_cases as lc
            case = lc.estimator_case("lags_o16")  # 82 frames, the last holds 3 of its 100 samples: zeros past the end
            x = np.ascontiguousarray(lc.case_signal(case, "coloured").T)

            def run(ctx, devs):
                from dsptoolbox_amd import backend
                return backend.lpc(devs[0], case["order"], lc.hann(case["L"]), case["hop"], method)
            return [x], run
        out.append(Case("ds_lpc_dev", f"lags_o16_{method}", build))
    return out


def _allpass_case():
    def build():
        n_in, n_out, lam = 257, 300, 0.6  # one past a tile of 256 input samples, five channels: a second channel group
        row0 = np.zeros(n_out)
        row0[0] = 1.0
        col0 = (-lam) ** np.arange(n_in)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.allpass_table(devs[0], -lam, lam, row0, col0),)
        x = _noise(400, n_in, 5)

        def judge(out):  # test_warp_gpu's bound: 1e-12 of each output channel's peak of the long-double table
            import warp_oracle as wo
            e = wo.channel_error(out[0], wo.allpass_table(_x64(x), -lam, lam, row0, col0)) / 1e-12
            assert e <= 1.0, e
            return e
        return [x], run, judge
    return Case("ds_allpass_table_dev", "n257_5ch", build)


def _vqt_case(name, n_ch):
    def build():
        import vqt_cases as vqc
        p = vqc.ALL[name]
        x = vqc.signal(name)
        if n_ch != p["c"]:  # further channels: the same rows again, delayed by 1, 2, ... samples
            x = np.stack([np.roll(x[:, c % p["c"]], c // p["c"]) for c in range(n_ch)], axis=1)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.vqt(devs[0], p["fs"], on_device=True, **p["kw"]).to_host(),)
        x32 = _f32(x)

        def judge(out):  # test_vqt_gpu's bound of a resident transform: 2 c 2^-53 A per element, none skipped
            import vqt_oracle
            _, value, a, c = vqt_oracle.vqt(_x64(x32), p["fs"], **p["kw"])
            err, lim = np.abs(out[0] - value).astype(np.float64), vqt_oracle.bound(a, c)
            assert err.shape == lim.shape and not err[lim == 0].any()
            e = float((err / np.where(lim > 0, lim, 1.0)).max())
            assert e <= 1.0, e
            return e
        return [x32], run, judge
    return Case("ds_vqt", f"{name}_{n_ch}ch", build)


def _resample_cases():
    import resample_cases as rsc
    out = []
    for up, down in rsc.RESIDENT_RATIOS:
        for n_ch in (3, 5):
            n = rsc.edge_lengths(up, down, n_ch)[-1]  # the shortest input whose output goes past one tile

            def build(up=up, down=down, n_ch=n_ch, n=n):
                x = _f32(rsc.signal(n, n_ch))

                def run(ctx, devs):
                    from dsptoolbox_amd import backend
                    return _planars(backend.resample_poly_device(devs[0], up, down))
                return [x], run
            out.append(Case("ds_resample_poly_dev", f"{up}_{down}_n{n}_{n_ch}ch", build))
    return out


# ---- effects --------------------------------------------------------------------------------------------------------------
FOLLOW_TILE = 512  # backend.FX_FOLLOW_TILE (the host test compares them)


def _burst32(seed, n, n_ch):
    import fx_cases as fc
    return _f32(fc.burst(seed, n, n_ch))


def _fx_judge(what, out, want):
    """test_fx_gpu's bounds: the float64 result within BOUND of the channel's peak of the long-double oracle, a resident
    result one rounding to float32 from it"""
    import fx_oracle as fo
    e = fo.stream_error(_rows(out), want) / (fo.BOUND + F32)
    assert e <= 1.0, (what, e)
    return e


def _fx_compress_case():
    def build():
        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.fx_compress(devs[0], -14.0, 4.0, 6.0, 8, 240))
        x = _burst32(410, FOLLOW_TILE + 1, 3)

        def judge(out):  # 1 ms and 30 ms at 8000 Hz are the 8 and 240 samples of the call
            import fx_oracle as fo
            want = fo.compress(_x64(x), 8000, -14.0, 1.0, 30.0, 4.0, True, 6.0)[0]
            return _fx_judge("compressor", out, want)
        return [x], run, judge
    return Case("ds_fx_compress", "n513", build)


def _fx_detect_case():
    def build():
        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.fx_detect(devs[0], -20.0, backend.fx_follower_coefficient(200)),)
        x = _burst32(411, FOLLOW_TILE + 1, 3)

        def judge(out):  # the mask exactly, as test_fx_gpu holds it; 25 ms at 8000 Hz are the 200 samples of the call
            import fx_oracle as fo
            for c in range(3):
                mask, nearest = fo.detect(_x64(x)[:, c], 8000, -20.0, True, 25.0)
                assert nearest > 1e-9, ("a level within 1e-9 dB of the threshold", nearest)
                assert np.array_equal(out[0][:, c], mask), (c, np.flatnonzero(out[0][:, c] != mask)[:8])
            return 0.0
        return [x], run, judge
    return Case("ds_fx_detect", "n513", build)


def _fx_delay_case(d):
    def build():
        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.fx_delay(devs[0], d, 2 * d + 3, 0.4, "arctan" if d == 255 else "digital"))
        x = _burst32(412 + d, 700, 2)

        def judge(out):
            import fx_oracle as fo
            return _fx_judge(f"delay {d}", out, fo.delay_samples(_x64(x), d, 2 * d + 3, 0.4, "arctan" if d == 255 else "digital"))
        return [x], run, judge
    return Case("ds_fx_delay", f"d{d}", build)


def _fx_chorus_case():
    def build():
        n, voices = 500, 3
        rng = np.random.default_rng(420)
        # delays of both signs up to 40 samples: at the first samples i + m < 0 wraps "from the end" of the samples
        # followed by max_delay zeros, at the last ones i + m >= n runs into those zeros
        m = rng.integers(-40, 41, (n, voices))
        m[0], m[-1] = (-40, -1, 40), (40, 39, -40)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.fx_chorus(devs[0], m, 0.6))
        x = _burst32(421, n, 2)

        def judge(out):
            import fx_oracle as fo
            return _fx_judge("chorus", out, fo.chorus(_x64(x), m, 0.6))
        return [x], run, judge
    return Case("ds_fx_chorus", "negative_delays_wrap", build)


def _fx_distort_case():
    def build():
        import fx_cases as fc
        p = fc.DISTORTION["combined"][3]
        kinds, levels, mix, offsets = fc.distortion_lists(p)

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            lin = lambda db: [10 ** (v / 20) if np.isfinite(v) else 0.0 for v in db]
            return _planars(backend.fx_distort(devs[0], [backend.FX_CURVES[k] for k in kinds], lin(levels), lin(offsets), mix,
                                               10 ** (p["post"] / 20)))
        x = _burst32(430, 257, 3)

        def judge(out):
            import fx_oracle as fo
            return _fx_judge("distortion", out, fo.distort(_x64(x), kinds, levels, mix, offsets, p["post"]))
        return [x], run, judge
    return Case("ds_fx_distort", "combined_n257", build)


def _fx_tremolo_case():
    def build():
        n = 257
        mod = 1.0 - 0.4 * (0.5 + 0.5 * np.sin(2 * np.pi * 30.0 / 8000 * np.arange(n)))

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.fx_tremolo(devs[0], mod))
        x = _burst32(431, n, 3)

        def judge(out):
            import fx_oracle as fo
            return _fx_judge("tremolo", out, fo.tremolo(_x64(x), mod))
        return [x], run, judge
    return Case("ds_fx_tremolo", "n257", build)


def _fx_specsub_case():
    def build():
        import specsub_cases as ssc
        n = ssc.edge_lengths(ssc.W)[1]  # n % step == 1
        x = ssc.generated(ssc.W, n)[0]

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.fx_specsub(devs[0], "hann", ssc.W, ssc.W // 2, "adaptive", env_floor=1e-4))

        def judge(out):  # test_specsub_gpu's bound of a generated shape, and one rounding to float32
            import specsub_oracle as sso
            want, gates, clips = sso.subtract(x, ssc.generated(ssc.W, n)[1], ssc.W // 2, "adaptive", env_floor=1e-4)
            ssc.conditions(gates, clips)
            e = sso.stream_error(_rows(out), want) / (sso.bound(ssc.W) + F32)
            assert e <= 1.0, e
            return e
        return [_f32(x)], run, judge
    return Case("ds_fx_specsub", "W64_step_plus_1", build)


def _fx_band_stack_case():
    """3 bands x 2 channels as pitched band views in ONE owner, through the public Compressor on a MultiBandSignal:
    effects._consecutive stacks them by ld and offset_bytes, the result is split by y.ld."""
    def build():
        n = 300
        x = _burst32(440, n, 6)  # rows band * 2 + channel

        def run(ctx, devs):
            import dsptoolbox_amd as dsp
            from dsptoolbox_amd._lib import DevicePlanar
            d = devs[0]
            bands = [dsp.Signal.from_planar_f32(DevicePlanar(d.owner, 2, n, d.ld, d.offset_bytes + 4 * b * 2 * d.ld), 8000)
                     for b in range(3)]
            out = dsp.effects.Compressor(-14, 1.0, 30, 4).apply(dsp.MultiBandSignal(bands))
            return tuple(b.device_samples.to_planar() for b in out.bands)

        def judge(out):  # every band and channel a stream of its own: 1 ms and 30 ms at 8000 Hz, no knee
            import fx_oracle as fo
            want = fo.compress(_x64(x), 8000, -14, 1.0, 30, 4)[0]
            return _fx_judge("compressor on stacked bands", (np.concatenate(out),), want)
        return [x], run, judge
    return Case("effects._stack", "three_bands_two_channels", build)


# ---- levels -----------------------------------------------------------------------------------------------------------------
SPAN, TILE = 4096, 1024  # levels_cases.SPAN, levels_cases.TILE (the host test compares them)


def _level32(seed, n, n_ch, **kw):
    import levels_cases as lc
    return _f32(lc.noise(seed, n, n_ch, **kw))


def _level_x(plane):
    """the (samples, channels) float64 array of a plane's float32 values"""
    return _x64(plane)


def _depth_bound(n):
    """test_levels_gpu.sum_bound: four units in the last place per addition along the longest chain of a reduction"""
    import levels_cases as lc
    import levels_oracle as lo
    return 4 * lo.reduction_depth(n) * lc.U


def _level_project_case():
    def build():
        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.level_project(devs[0], 3),)
        plane = _level32(450, SPAN + 1, 3, curve=0.6)

        def judge(out):  # test_levels_gpu.test_reduction_lengths: (4 depth + 64) u of sum |x P_k|, the peak exactly
            import levels_cases as lc
            import levels_oracle as lo
            x, got = _level_x(plane), out[0]
            P = lo.gram_basis(len(x), 3)
            want, weight = P @ x.astype(lo.LD), np.abs(P) @ np.abs(x).astype(lo.LD)
            e = float(np.max(np.abs(got[:, :4].T - want) / weight)) / ((4 * lo.reduction_depth(len(x)) + 64) * lc.U)
            assert got.shape == (3, 10) and e <= 1.0, e
            assert np.array_equal(got[:, 9], np.max(np.abs(x), axis=0)) and not got[:, 4:9].any()
            return e
        return [plane], run, judge
    return Case("ds_level_project", "n4097_order3", build)


def _level_stats_cases():
    def make(common):
        def build():
            def run(ctx, devs):
                from dsptoolbox_amd import backend
                return (backend.level_stats(devs[0], 0, common),)
            plane = _level32(451, SPAN + 1, 3, curve=0.6)

            def judge(out):  # the bounds of test_levels_gpu.test_reduction_lengths, of the mean's residual
                import levels_oracle as lo
                x, st = _level_x(plane), out[0]
                n, b = len(x), _depth_bound(len(x))
                assert st.shape == (3, 3) and np.array_equal(st[:, 2], np.max(np.abs(x), axis=0))
                if common:
                    dc = x.astype(lo.LD) - np.mean(x.astype(lo.LD))
                    tot = float(np.sum(dc * dc))
                    e = abs(float(np.sum(st[:, 0]) - np.sum(dc * dc))) / (4 * (lo.reduction_depth(n) + 3) * 2.0 ** -53 * tot + 1e-300)
                    assert e <= 1.0, e
                    return e
                d = x.astype(lo.LD) - np.mean(x.astype(lo.LD), axis=0)
                ss = np.sum(d * d, axis=0)
                shift = b * np.max(np.abs(x), axis=0)
                e = max(float(np.max(np.abs(st[:, 0] - ss) / (b * ss + n * shift ** 2))),
                        float(np.max(np.abs(st[:, 1] - np.max(np.abs(d), axis=0)) / shift)))
                assert e <= 1.0, e
                return e
            return [plane], run, judge
        return Case("ds_level_stats", "n4097_common" if common else "n4097_mean", build)
    return [make(False), make(True)]


def _level_apply_cases():
    out = []
    for n in list(range(1, 10)) + [1003]:
        def build(n=n):
            l_fade = max(1, n // 3)
            fade = np.linspace(0.0, 1.0, l_fade + 1)[1:] ** 2
            gain = np.array([0.5, -1.25, 2.0])

            def run(ctx, devs):
                from dsptoolbox_amd import backend
                return _planars(backend.level_apply(devs[0], gain=gain, fade=fade, at_start=True, at_end=True))
            return [_level32(460 + n, n, 3)], run
        out.append(Case("ds_level_apply", f"n{n}_gain_fades", build))

    def norm():
        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return _planars(backend.level_apply(devs[0], order=1, norm="rms_all", norm_factor=0.1))
        plane = _level32(470, SPAN + 1, 3)

        def judge(out):
            """(x - line) 0.1 / rms of all channels about their common mean.  The three steps' bounds of test_levels_gpu, each
            of the channel's peak: the detrend's FLOOR (64 u), the gain's reduction bound, one rounding to float32."""
            import levels_cases as lc
            import levels_oracle as lo
            x = _level_x(plane)
            want = lo.detrend(x, 1) * (lo.LD(0.1) / lo.rms(x, common=True)[0])
            e = lo.relative_to_peak(_rows(out), want) / (64 * lc.U + _depth_bound(len(x)) + 2.0 ** -24)
            assert e <= 1.0, e
            return e
        return [plane], run, judge
    out.append(Case("ds_level_apply", "n4097_detrend_rms_all", norm))
    return out


def _moving_rms_cases():
    out = []
    for name, n, w in (("w_tile_plus_1", 2 * TILE + 5, TILE + 1), ("w_past_n", 700, 705)):
        def build(n=n, w=w):
            def run(ctx, devs):
                from dsptoolbox_amd import backend
                return (backend.moving_rms(devs[0], w),)
            plane = _level32(480 + w, n, 3)

            def judge(out):  # test_levels_gpu.test_moving_window_edges: 64 u of the peak mean square
                import levels_cases as lc
                import levels_oracle as lo
                got, want = out[0], lo.moving_mean_square(_level_x(plane), w)
                e = float(np.max(np.max(np.abs(got.astype(lo.LD) ** 2 - want), axis=0) / np.max(want, axis=0))) / (64 * lc.U)
                assert got.shape == want.shape and np.isfinite(got).all() and (got >= 0).all() and e <= 1.0, e
                return e
            return [plane], run, judge
        out.append(Case("ds_moving_rms", name, build))
    return out


def _loudness_case():
    def build():
        import levels_cases as lc
        fs, extra = 8000, 2049
        tg, step = lc.lufs_blocks(fs)
        x = lc.programme(90, fs, 2, [(tg + extra - 1500, "tone", 0.4), (1500, "noise", 0.05)])

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            from dsptoolbox_amd.standard import gain_and_level as gl
            return (backend.loudness_blocks(devs[0], gl._k_weighting_sos(fs), tg, step),)
        return [_f32(x)], run
    return Case("ds_loudness_blocks", "fs8000_extra2049", build)


def _envelope_case():
    def build():
        import levels_cases as lc
        seed, n, n_ch = lc.ENVELOPE_ANALYTIC["n4095"]

        def run(ctx, devs):
            from dsptoolbox_amd import backend
            return (backend.envelope_analytic(devs[0]),)
        plane = _level32(seed, n, 3)

        def judge(out):  # test_levels_gpu.test_analytic_envelope's bound at this length, per channel
            import fft64_cases as f64c
            import levels_oracle as lo
            with np.load(os.path.join(ROOT, "tests", "golden", "levels", "cases.npz"), allow_pickle=False) as z:
                measured = json.loads(str(z["meta"]))["measured"]["env_analytic"]["n4095"]
            ref = f64c.oracle_hilbert(lo.detrend(_level_x(plane), 1))
            err = np.max(np.abs(out[0].astype(lo.LD) - np.abs(ref)), axis=0)
            pk, scale = np.max(np.abs(ref), axis=0), np.sqrt(np.mean(np.abs(ref) ** 2, axis=0))
            bound = np.maximum(4 * measured * pk, f64c.tolerance(("hilbert", f64c.plan(n)[1])) * scale)
            e = float(np.max(err / bound))
            assert out[0].shape == ref.shape and e <= 1.0, e
            return e
        return [plane], run, judge
    return Case("ds_envelope_analytic", "n4095", build)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _entries():
    e = OrderedDict()

    def add(cases):
        for c in cases if isinstance(cases, list) else [cases]:
            e.setdefault(c.entry, []).append(c)

    add(_welch_cases("tf"))
    add(_welch_cases("psd"))
    add([_stft_case(nfft, short) for nfft in stft_nffts() for short in (False, True)])
    add([_csm_case("ds_csm_dev", W, 3) for W in csm_windows("all")] + [_csm_case("ds_csm_dev", 1024, 65)])
    add([_csm_case("ds_csm_bins_dev", W, 3) for W in csm_windows("part")] + [_csm_case("ds_csm_bins_dev", 1024, 65)])
    add([_rfft_case(n, short) for n in xform_nffts("rfft") for short in (False, True)])
    # one inverse spectrum for all channels has every launch-name set of one per channel, and the 8192-point kernel's
    add([_deconv_case(n, short, 0) for n in xform_nffts("deconv", 0) for short in (False, True)])
    add(_deconv_case(xform_nffts("deconv", 1)[1], True, 1))
    add([_fir_case(k) for k in fir_taps()])
    add([_iir_case(m) for m in ("PARALLEL", "SUMMED", "SEQUENTIAL")])
    add([_sfilt_case(k) for k in SFILT_KINDS])
    add([_rtfilt_case(k) for k in RTFILT_KINDS] + [_rtfilt_case("parallel", 33), _rtfilt_case("parallel", 2049, True)])
    add([_rtfir_case(63), _rtfir_case(4095)])
    add(_pair_moments_case())
    add(_fw_snr_case())
    add(_delay_sum_case())
    add(_cwt_case())
    add(_dft_cases())
    add(_lpc_cases())
    add(_allpass_case())
    add([_vqt_case("tile_c1_771", 1), _vqt_case("tile_195", 5)])
    add(_resample_cases())
    add(_fx_compress_case())
    add(_fx_detect_case())
    add([_fx_delay_case(d) for d in (1, 255, 256, 257)])
    add(_fx_chorus_case())
    add(_fx_distort_case())
    add(_fx_tremolo_case())
    add(_fx_specsub_case())
    add(_level_project_case())
    add(_level_stats_cases())
    add(_level_apply_cases())
    add(_moving_rms_cases())
    add(_loudness_case())
    add(_envelope_case())
    return e


ENTRIES = _entries()
# what the library builds on the entries and hands views itself: not C-ABI entries, run by the same test
LIBRARY = OrderedDict([("backend.stack_device", [_stack_case()]), ("effects._stack", [_fx_band_stack_case()])])


def all_cases():
    return [c for cases in list(ENTRIES.values()) + list(LIBRARY.values()) for c in cases]


def case_id(c):
    return f"{c.entry}-{c.name}"
