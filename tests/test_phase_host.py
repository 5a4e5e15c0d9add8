"""The analytic signal, the cepstra, the minimum-phase family and the group delays without a GPU: numpy restatements
of the reference's functions are held to every case of tests/golden/phase/cases.npz within 5e-13 of the channel's
largest magnitude (phases as exp(i phi)); a long-double DFT with exactly reduced phase shows that numpy itself stays
below 1e-11 on these inputs (measured: 2e-15 on the transforms, 3e-15 on the minimum phase of ir255), which leaves the
device bound of 1e-9 room; the fold, the mask and the gradient are checked at even and odd lengths; the Python bounds are the
header's; every argument that is not built raises NotImplementedError before the device is touched; the eight public
functions and the two not-built ones carry the reference's signatures; a frequency step of exactly 1 Hz gives radians
per bin as in the reference."""

import inspect
import json
import os

import numpy as np
import pytest
from scipy.fft import fft as sfft, ifft as sifft, next_fast_len
from scipy.interpolate import interp1d

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DevicePlanar
from test_smoothing_host import channel_error, ref_smoothing

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 5e-13
_GOLDEN = None


def make_ir(n, channels, delay, decay, seed):
    """tools/gen_golden_phase.py:make_ir."""
    rng = np.random.default_rng(seed)
    k = np.arange(n) - delay
    env = np.where(k > 0, np.exp(-np.maximum(k, 0) / decay), 0.0)
    x = 0.03 * rng.standard_normal((n, channels)) * env[:, None]
    x[delay, :] = 1.0
    if channels > 1:
        x[:, -1] *= 1e-3
    return x.astype(np.float32).astype(np.float64)


def golden():
    """(arrays, meta) of tests/golden/phase/cases.npz, loaded once: the stored signals widened to float64, the long
    ones rebuilt from their seeds and proved by their probes, the long frequency vectors rebuilt from their three
    numbers."""
    global _GOLDEN
    if _GOLDEN is None:
        f = np.load(os.path.join(HERE, "golden", "phase", "cases.npz"))
        meta = json.loads(str(f["meta"]))
        z = {k: f[k] for k in f.files if k != "meta"}
        for name, p in meta["signals"].items():
            if name in z:
                z[name] = z[name].astype(np.float64)
            else:
                x = make_ir(**p)
                assert np.array_equal(np.concatenate([x[:16, 0], [x.sum()]]), z[name + "_probe"]), "the seeded signal changed"
                z[name] = x
        for case in meta["cases"]:
            key = case["out"] + "_f"
            if key in z and len(z[key]) == 3 and len(z[case["out"]]) != 3:
                n, step, last = z[key]
                fv = np.arange(int(n)) * step
                assert abs(fv[-1] - last) <= 1e-9 * last
                z[key] = fv
        _GOLDEN = (z, meta)
    return _GOLDEN


def cases(fn, **match):
    z, meta = golden()
    for case in meta["cases"]:
        if case["fn"] == fn and all(case.get(k) == v for k, v in match.items()):
            yield case, z[case["sig"]], z[case["out"]], z.get(case["out"] + "_f")


def phase_error(out, ref):
    """max |exp(i out) - exp(i ref)|: phases that differ by a turn are the same phase."""
    return float(np.abs(np.exp(1j * out) - np.exp(1j * ref)).max())


# ---- restatements ---------------------------------------------------------------------------------------------------
def fold_weights(n):
    """helpers/minimum_phase.py:38-46 (and the mask of transforms.hilbert) as a vector."""
    w = np.zeros(n)
    w[0] = 1.0
    if n % 2 == 0:
        w[1:n // 2] = 2.0
        w[n // 2] = 1.0
    else:
        w[1:(n + 1) // 2] = 2.0
    return w


def ref_hilbert(x):
    return np.fft.ifft(np.fft.fft(x, axis=0) * fold_weights(len(x))[:, None], axis=0)


def ref_cepstrum(x, complex=True):
    sp = np.fft.fft(x, axis=0)
    return np.fft.ifft(np.log(sp) if complex else np.log(np.abs(sp)), axis=0)


def ref_from_cepstrum(c):
    return np.fft.ifft(np.exp(np.fft.fft(c, axis=0)), axis=0).real


def ref_min_phase_spectrum(x, padding_factor):
    n_fft = next_fast_len(max(x.shape[0] * padding_factor, x.shape[0]))
    y = np.real(sifft(np.log(np.abs(sfft(x, n=n_fft, axis=0))), axis=0))
    return np.exp(sfft(y * fold_weights(n_fft)[:, None], axis=0))


def ref_min_phase_ir(x, padding_factor=8, alpha=1.0):
    td = x.copy()
    if alpha != 1.0:
        td *= (alpha ** np.arange(len(td)))[:, None]
    td = np.real(np.fft.ifft(ref_min_phase_spectrum(td, padding_factor), axis=0))
    if alpha != 1.0:
        td *= (alpha ** (-np.arange(len(td))))[:, None]
    return td[:len(x)]


def ref_minimum_phase(x, fs, padding_factor=8):
    sp = ref_min_phase_spectrum(x, padding_factor)
    f = np.fft.fftfreq(len(sp), 1 / fs)
    if len(sp) % 2 == 0:
        f[len(sp) // 2] *= -1
    return f[f >= 0], np.angle(sp[f >= 0])


def ref_group_delay_direct(phase, delta_f):
    """_group_delay_direct (standard/_standard_backend.py:57-63): a step of exactly 1 means "no step given" there, and
    the result is radians per bin."""
    if delta_f != 1:
        return -np.gradient(np.unwrap(phase, axis=0), delta_f, axis=0) / np.pi / 2
    return -np.gradient(np.unwrap(phase, axis=0), axis=0)


def ref_gradient(v, h):
    """np.gradient's rule written out: centred differences, one-sided at the ends."""
    g = np.empty_like(v)
    g[1:-1] = (v[2:] - v[:-2]) / (2.0 * h)
    g[0] = (v[1] - v[0]) / h
    g[-1] = (v[-1] - v[-2]) / h
    return g


def ref_minimum_group_delay(x, fs, padding_factor=8, smoothing=0):
    f, ph = ref_minimum_phase(x, fs, padding_factor)
    gd = ref_group_delay_direct(ph, f[1] - f[0])
    return f, ref_smoothing(gd, None, smoothing) if smoothing else gd


def analytic_spectra(b, n_freq):
    """(numerator, denominator) of _group_delay_filter (classes/filter_helpers.py:189-196) for one column."""
    omega = np.linspace(0, np.pi, n_freq)
    e = np.exp(1j * omega)
    return np.polyval(b * np.arange(len(b)), e), np.polyval(b, e)


def ref_group_delay(x, fs, analytic=True, smoothing=0, latency=False):
    n = next_fast_len(x.shape[0] * 8, True) if latency else x.shape[0]
    td = np.concatenate([x, np.zeros((n - len(x), x.shape[1]))]) if n > len(x) else x[:n]
    f = np.fft.rfftfreq(n, 1 / fs)
    if not analytic:
        gd = ref_group_delay_direct(np.angle(np.fft.rfft(td, axis=0)), f[1] - f[0])
    else:
        gd = np.zeros((n // 2 + 1, x.shape[1]))
        for c in range(x.shape[1]):
            b = td[:, c]
            if latency:
                b = b[max(int(np.argmax(np.abs(b))) - 1, 0):]
            num, den = analytic_spectra(b, len(f))
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.real(num / den)
            g[~np.isfinite(g)] = 0
            gd[:, c] = g / fs
    return f, ref_smoothing(gd, None, smoothing) if smoothing else gd


def ref_excess_group_delay(x, fs, smoothing=0):
    f_min, min_gd = ref_minimum_group_delay(x, fs, 1)
    f, gd = ref_group_delay(x, fs, analytic=False)
    if len(f) != len(f_min):
        gd = interp1d(f, gd, kind="linear", copy=False, bounds_error=False, assume_sorted=True, fill_value=(0.0, 0.0),
                      axis=0)(f_min)
    ex = gd - min_gd
    return f_min, ref_smoothing(ex, None, smoothing) if smoothing else ex


def restate(case, x, fs):
    """(frequency vector or None, values) of the restatement of one golden case."""
    fn = case["fn"]
    if fn == "hilbert":
        return None, ref_hilbert(x)
    if fn == "cepstrum":
        return None, ref_cepstrum(x, case["complex"])
    if fn == "min_phase_ir":
        return None, ref_min_phase_ir(x, case["padding_factor"], case["alpha"])
    if fn == "minimum_phase":
        return ref_minimum_phase(x, fs, case["padding_factor"])
    if fn == "minimum_group_delay":
        return ref_minimum_group_delay(x, fs, case["padding_factor"], case["smoothing"])
    if fn == "group_delay":
        return ref_group_delay(x, fs, case["analytic_computation"], case["smoothing"], case["remove_ir_latency"])
    assert fn == "excess_group_delay"
    return ref_excess_group_delay(x, fs, case["smoothing"])


# ---- the long-double oracle -----------------------------------------------------------------------------------------
_PI_LD = np.longdouble(4) * np.arctan(np.longdouble(1))


def longdouble_dft(x, n_fft, inverse=False):
    """The transform of the columns of x (zero-padded to n_fft) as a direct sum in long double: the phase j k / n_fft is
    reduced to (j k) mod n_fft in integers first, so its error does not grow with the length."""
    n_in = min(len(x), n_fft)
    r = np.arange(n_fft, dtype=np.longdouble) * (2 * _PI_LD / n_fft)
    table = np.cos(r) + (1j if inverse else -1j) * np.sin(r)
    idx = np.outer(np.arange(n_fft, dtype=np.int64), np.arange(n_in, dtype=np.int64)) % n_fft
    out = table[idx] @ x[:n_in].astype(np.clongdouble)
    return out / n_fft if inverse else out


def longdouble_min_phase_spectrum(x, n_fft):
    y = np.real(longdouble_dft(np.log(np.abs(longdouble_dft(x, n_fft))), n_fft, inverse=True))
    return np.exp(longdouble_dft(y * fold_weights(n_fft).astype(np.longdouble)[:, None], n_fft))


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_restatements_match_every_golden_case():
    z, meta = golden()
    seen = set()
    for case in meta["cases"]:
        x, ref = z[case["sig"]], z[case["out"]]
        f, out = restate(case, x, case.get("fs", meta["fs"]))
        assert out.shape == ref.shape and out.dtype == ref.dtype, (case, out.shape, ref.shape)
        if f is not None:
            assert np.allclose(f, z[case["out"] + "_f"], rtol=1e-12, atol=0.0), case
        e = phase_error(out, ref) if case["fn"] == "minimum_phase" else channel_error(out, ref)
        assert e <= TOL, (case, e)
        seen.add(case["fn"])
    assert seen == {"hilbert", "cepstrum", "min_phase_ir", "minimum_phase", "minimum_group_delay", "group_delay",
                    "excess_group_delay"}
    # the three group-delay functions are pinned at a frequency step of exactly 1 Hz too: radians per bin there
    assert {c["fn"] for c in meta["cases"] if "fs" in c} == {"minimum_group_delay", "group_delay", "excess_group_delay"}
    for case, x, ref, f in cases("minimum_group_delay", fs=2048):
        seconds = -np.gradient(np.unwrap(ref_minimum_phase(x, 2048)[1], axis=0), 1.0, axis=0) / np.pi / 2
        assert f[1] - f[0] == 1.0 and channel_error(ref, 2 * np.pi * seconds) <= TOL
    for name in ("ir255", "ir256", "ir1000", "ir6000"):
        assert channel_error(ref_from_cepstrum(ref_cepstrum(z[name])), z[name]) <= TOL, name


def test_numpy_stays_below_1e_11_of_a_long_double_oracle():
    z, _ = golden()
    for name in ("ir255", "ir256", "ir1000"):
        x = z[name]
        n = len(x)
        exact = longdouble_dft(x, n)
        e = channel_error(np.fft.fft(x, axis=0), exact.astype(np.complex128))
        h = longdouble_dft(exact * fold_weights(n).astype(np.longdouble)[:, None], n, inverse=True)
        (_, _, ref, _), = cases("hilbert", sig=name)
        e = max(e, channel_error(ref, h.astype(np.complex128)))
        c = longdouble_dft(np.log(np.abs(exact)), n, inverse=True)
        (_, _, ref, _), = cases("cepstrum", sig=name, complex=False)
        e = max(e, channel_error(ref, c.astype(np.complex128)))
        print(f"{name}: numpy against long double {e:.2e}")
        assert e <= 1e-11, (name, e)
    # the whole minimum-phase chain at its padded length (2048 points for 255 samples)
    (case, x, ref, _), = cases("minimum_phase", sig="ir255")
    sp = longdouble_min_phase_spectrum(x, next_fast_len(8 * len(x)))
    phase = np.arctan2(sp.imag, sp.real).astype(np.float64)[:len(ref)]
    e = phase_error(ref, phase)
    print(f"ir255 minimum phase: reference against long double {e:.2e}")
    assert e <= 1e-11, e


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 254, 255])
def test_fold_mask_and_gradient_at_even_and_odd_lengths(n):
    rng = np.random.default_rng(n)
    # the fold / mask against the reference's own statements (helpers/minimum_phase.py:38-46, transforms.py:794-800)
    y = rng.standard_normal((n, 2))
    want = y.copy()
    if n % 2 == 0:
        want[1:n // 2, ...] *= 2.0
        want[n // 2 + 1:, ...] = 0.0
    else:
        want[1:(n + 1) // 2, ...] *= 2.0
        want[(n + 1) // 2:, ...] = 0.0
    assert np.array_equal(y * fold_weights(n)[:, None], want)
    # the analytic signal keeps the signal as its real part
    assert np.abs(ref_hilbert(y).real - y).max() <= 1e-13 * max(1.0, np.abs(y).max())
    if n >= 2:
        v = np.cumsum(rng.standard_normal((n, 2)), axis=0)
        assert np.array_equal(ref_gradient(v, 23.4375), np.gradient(v, 23.4375, axis=0))


def test_python_bounds_are_the_headers():
    text = open(os.path.join(HERE, "..", "dsptoolbox_amd", "csrc", "size_guards.hpp")).read()
    assert "kFft64MaxPow2 = (int64_t)1 << 22;" in text and backend.FFT64_MAX_POW2 == 1 << 22
    assert "kFft64MaxAny = (int64_t)1 << 21;" in text and backend.FFT64_MAX_ANY == 1 << 21
    header = open(os.path.join(HERE, "..", "include", "dsptoolbox_amd.h")).read()
    for i, name in enumerate(("SPECTRUM", "PHASE", "IR", "GROUP_DELAY")):
        assert f"#define DS_MIN_PHASE_{name} {i}" in header
        assert backend.MIN_PHASE_OUTPUTS[i] == name.lower()
    for n in (1, 1000, 1 << 21, (1 << 21) - 1, 1 << 22):
        backend._fft64_guard(n)
    for n in ((1 << 21) + 1, 3 << 20, (1 << 22) + 2, 1 << 23):
        with pytest.raises(NotImplementedError, match="beyond the device kernels' bounds"):
            backend._fft64_guard(n)
    assert backend.min_phase_fft_length(255, 8) == 2048 and backend.min_phase_fft_length(1000, 8) == 8000
    assert backend.min_phase_fft_length(6000, 8) == 48000


def test_arguments_that_are_not_built_raise():
    tf = dsp.transfer_functions
    ir = dsp.ImpulseResponse(None, np.eye(64)[:, 3:4] + 0.0, 48000)
    for call in (lambda: tf.min_phase_ir(ir, use_real_cepstrum=False),
                 lambda: tf.minimum_phase(ir, use_real_cepstrum=False),
                 lambda: tf.group_delay(ir, analytic_computation=False, remove_ir_latency=True),
                 lambda: tf.min_phase_from_mag(None, 48000),
                 lambda: tf.lin_phase_from_mag(None, 48000)):
        with pytest.raises(NotImplementedError, match="not built"):
            call()
    planar = object.__new__(DevicePlanar)  # never touched: the type alone is refused
    for call in (lambda: backend.hilbert(planar), lambda: backend.cepstrum(planar), lambda: backend.fft_c128(planar),
                 lambda: backend.min_phase(planar, 64, "ir", 8), lambda: backend.group_delay_phase(planar, 1.0)):
        with pytest.raises(NotImplementedError, match="not built"):
            call()
    # the reference's own assertions come first
    sig = dsp.Signal(None, np.ones((64, 1)), 48000)
    for call in (lambda: tf.min_phase_ir(sig), lambda: tf.minimum_phase(sig), lambda: tf.minimum_group_delay(sig),
                 lambda: tf.excess_group_delay(sig)):
        with pytest.raises(AssertionError, match="only valid for an impulse response"):
            call()
    with pytest.raises(AssertionError, match="Padding factor"):
        tf.min_phase_ir(ir, padding_factor=1)
    with pytest.raises(AssertionError, match="Alpha"):
        tf.min_phase_ir(ir, alpha=1.5)
    with pytest.raises(TypeError, match="valid type"):
        dsp.transforms.hilbert(np.ones(8))


def test_public_names_carry_the_reference_signatures():
    tr, tf = dsp.transforms, dsp.transfer_functions
    want = {
        tr.hilbert: [("signal", inspect.Parameter.empty)],
        tr.cepstrum: [("signal", inspect.Parameter.empty), ("complex", True)],
        tr.from_complex_cepstrum: [("cepstrum", inspect.Parameter.empty), ("sampling_rate_hz", inspect.Parameter.empty)],
        tf.min_phase_ir: [("sig", inspect.Parameter.empty), ("use_real_cepstrum", True), ("padding_factor", 8),
                          ("alpha", 1.0)],
        tf.minimum_phase: [("signal", inspect.Parameter.empty), ("use_real_cepstrum", True), ("padding_factor", 8)],
        tf.minimum_group_delay: [("signal", inspect.Parameter.empty), ("smoothing", 0), ("padding_factor", 8)],
        tf.group_delay: [("signal", inspect.Parameter.empty), ("analytic_computation", True), ("smoothing", 0),
                         ("remove_ir_latency", False)],
        tf.excess_group_delay: [("signal", inspect.Parameter.empty), ("smoothing", 0), ("remove_ir_latency", False),
                                ("analytic_computation", False)],
        # the two that only raise NotImplementedError keep the reference's signatures as well
        tf.min_phase_from_mag: [("spectrum", inspect.Parameter.empty), ("sampling_rate_hz", inspect.Parameter.empty),
                                ("ir_length_samples", None)],
        tf.lin_phase_from_mag: [("spectrum", inspect.Parameter.empty), ("sampling_rate_hz", inspect.Parameter.empty),
                                ("group_delay_ms", None), ("check_causality", True), ("minimum_group_delay_factor", 1.0)],
    }
    assert len(want) == 10  # eight functions that compute, two that say they are not built
    for fn, params in want.items():
        got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
        assert got == params, (fn.__name__, got)
        module = tr if fn.__module__.endswith("transforms") else tf
        assert fn.__name__ in module.__all__
