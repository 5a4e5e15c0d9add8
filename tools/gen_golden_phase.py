"""Golden vectors for the analytic signal, the cepstra, the minimum-phase family and the group delays, made by RUNNING
THE REFERENCE (dsptoolbox 0.8: transforms.hilbert / cepstrum / from_complex_cepstrum, transforms/transforms.py:59-110,
763-809; transfer_functions.min_phase_ir / group_delay / minimum_phase / minimum_group_delay / excess_group_delay,
transfer_functions.py:789-1083):
    python tools/gen_golden_phase.py

Writes tests/golden/phase/cases.npz.  `meta` is a JSON string:
- `signals`: {name: {"n", "channels", "delay", "decay", "seed"}}.  Signals up to 1000 samples are stored (float32);
  the longer ones are rebuilt by `make_ir` from their seed, and the fixture holds `<name>_probe`, the first 16 samples
  of channel 0 and the sum, to prove the rebuild.
- `cases`: a list of {"fn", "sig", keyword arguments ..., "out"} (`fs`, where a case does not use the file's 48000); `out` names the stored float64 / complex128 result
  (for the functions that return (f, values), the values; the frequency vector is `<out>_f`, or for more than 1100
  bins its length, second and last value).

Every signal is a unit impulse after an EVEN leading delay plus Gaussian noise under an exponential envelope after it,
rounded to float32; the last channel of a multichannel signal is scaled by 1e-3.  The delay makes the minimum-phase
result differ visibly from the input, and an even delay keeps the Nyquist bin of an even length positive: the
principal logarithm of a negative real bin hangs on the sign of a rounding-level imaginary part (numpy's own fft gives
either sign there).

The script ASSERTS on the reference's own numbers and fails otherwise:
- every channel's magnitude spectrum, at the signal's length and at every padded length a case uses, spans less than
  60 dB: log|X| is well conditioned;
- no adjacent-bin phase step that a group-delay case unwraps lies within 1e-3 of +-pi: unwrap is not decided by
  rounding, so a test may compare every bin;
- no bin's phase that a complex-cepstrum case takes lies within 1e-6 of +-pi."""

import json
import os
import sys
import warnings

import numpy as np
from scipy.fft import next_fast_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "phase", "cases.npz")
FS = 48000
STORED_UP_TO = 1000

SIGNALS = {
    "ir255": dict(n=255, channels=3, delay=6, decay=30.0, seed=255),
    "ir256": dict(n=256, channels=2, delay=8, decay=30.0, seed=256),
    "ir1000": dict(n=1000, channels=1, delay=12, decay=120.0, seed=1000),
    "ir4097": dict(n=4097, channels=1, delay=40, decay=500.0, seed=4097),
    "ir6000": dict(n=6000, channels=1, delay=100, decay=700.0, seed=6000),
}


def make_ir(n, channels, delay, decay, seed):
    """Unit impulse at `delay`, noise of 0.03 under exp(-(k - delay) / decay) after it; the last of several channels
    scaled by 1e-3; float32 values."""
    rng = np.random.default_rng(seed)
    k = np.arange(n) - delay
    env = np.where(k > 0, np.exp(-np.maximum(k, 0) / decay), 0.0)
    x = 0.03 * rng.standard_normal((n, channels)) * env[:, None]
    x[delay, :] = 1.0
    if channels > 1:
        x[:, -1] *= 1e-3
    return x.astype(np.float32).astype(np.float64)


def probe(x):
    return np.concatenate([x[:16, 0], [x.sum()]])


def span_db(x, n_fft):
    mag = np.abs(np.fft.fft(x, n=n_fft, axis=0))
    return float((20 * np.log10(mag.max(axis=0) / mag.min(axis=0))).max())


def assert_steps_clear(phase, what):
    d = np.diff(phase, axis=0)
    dm = np.mod(d + np.pi, 2 * np.pi) - np.pi
    gap = float(np.abs(np.abs(dm) - np.pi).min())
    assert gap > 1e-3, f"{what}: a phase step within {gap:.2e} of pi"


def main():
    dsp = import_reference()
    tf, tr = dsp.transfer_functions, dsp.transforms
    warnings.simplefilter("ignore")
    z, cases = {}, []
    sig = {name: make_ir(**p) for name, p in SIGNALS.items()}
    for name, x in sig.items():
        if len(x) <= STORED_UP_TO:
            z[name] = x.astype(np.float32)
        else:
            z[name + "_probe"] = probe(x)

    def ir_of(name):
        return dsp.ImpulseResponse(None, sig[name].copy(), FS, constrain_amplitude=False)

    def check_span(name, n_fft):
        s = span_db(sig[name], n_fft)
        assert s < 60.0, f"{name} at {n_fft} points spans {s:.1f} dB"

    def add(fn, name, out, f=None, **kw):
        key = f"{fn}_{len(cases)}"
        z[key] = np.ascontiguousarray(out)
        if f is not None:  # long frequency vectors as (length, second, last value): they are evenly spaced from 0
            assert f[0] == 0.0 and np.allclose(np.diff(f), f[1], rtol=1e-12, atol=0.0)
            z[key + "_f"] = np.ascontiguousarray(f) if len(f) <= 1100 else np.array([len(f), f[1], f[-1]])
        cases.append(dict(fn=fn, sig=name, out=key, **kw))

    # ---- the transforms and the minimum-phase pair at the four lengths
    for name in ("ir255", "ir256", "ir1000", "ir6000"):
        x, n = sig[name], len(sig[name])
        check_span(name, n)
        check_span(name, next_fast_len(8 * n))
        ph = np.angle(np.fft.fft(x, axis=0))
        assert float(np.abs(np.abs(ph) - np.pi).min()) > 1e-6, f"{name}: a bin's phase at the branch cut"
        h = tr.hilbert(ir_of(name))
        add("hilbert", name, h.time_data + 1j * h.time_data_imaginary)
        for cplx in (True, False):
            add("cepstrum", name, tr.cepstrum(ir_of(name), complex=cplx), complex=cplx)
        back = tr.from_complex_cepstrum(tr.cepstrum(ir_of(name), complex=True), FS).time_data
        assert np.abs(back - x).max() < 1e-12  # (the test compares with the signal itself)
        for alpha in (1.0, 1.0 - 1e-6):
            add("min_phase_ir", name, tf.min_phase_ir(ir_of(name), alpha=alpha).time_data, alpha=alpha, padding_factor=8)
        f, mp = tf.minimum_phase(ir_of(name))
        add("minimum_phase", name, mp, f=f, padding_factor=8)

    # ---- padding_factor 2 at 4097 samples
    check_span("ir4097", next_fast_len(2 * 4097))
    add("min_phase_ir", "ir4097", tf.min_phase_ir(ir_of("ir4097"), padding_factor=2).time_data, alpha=1.0, padding_factor=2)
    f, mp = tf.minimum_phase(ir_of("ir4097"), padding_factor=2)
    add("minimum_phase", "ir4097", mp, f=f, padding_factor=2)

    # ---- group delays
    def min_phase_steps(name, padding_factor):
        _, mp = tf.minimum_phase(ir_of(name), padding_factor=padding_factor)
        assert_steps_clear(mp, f"{name} minimum phase, padding {padding_factor}")

    def spectrum_steps(name):
        assert_steps_clear(np.angle(np.fft.rfft(sig[name], axis=0)), f"{name} spectrum")

    for name in ("ir255", "ir1000"):
        min_phase_steps(name, 8)
        f, gd = tf.minimum_group_delay(ir_of(name))
        add("minimum_group_delay", name, gd, f=f, smoothing=0, padding_factor=8)
    for name in ("ir255", "ir256", "ir1000"):
        spectrum_steps(name)
        f, gd = tf.group_delay(ir_of(name), analytic_computation=False)
        add("group_delay", name, gd, f=f, analytic_computation=False, smoothing=0, remove_ir_latency=False)
    for name in ("ir255", "ir256"):
        check_span(name, next_fast_len(len(sig[name])))
        min_phase_steps(name, 1)
        f, gd = tf.excess_group_delay(ir_of(name))
        add("excess_group_delay", name, gd, f=f, smoothing=0, remove_ir_latency=False, analytic_computation=False)
        for latency in (False, True):
            f, gd = tf.group_delay(ir_of(name), analytic_computation=True, remove_ir_latency=latency)
            add("group_delay", name, gd, f=f, analytic_computation=True, smoothing=0, remove_ir_latency=latency)
    f, gd = tf.group_delay(ir_of("ir256"), analytic_computation=False, smoothing=3)
    add("group_delay", "ir256", gd, f=f, analytic_computation=False, smoothing=3, remove_ir_latency=False)
    f, gd = tf.minimum_group_delay(ir_of("ir256"), smoothing=3)
    min_phase_steps("ir256", 8)
    add("minimum_group_delay", "ir256", gd, f=f, smoothing=3, padding_factor=8)
    f, gd = tf.excess_group_delay(ir_of("ir256"), smoothing=3)
    add("excess_group_delay", "ir256", gd, f=f, smoothing=3, remove_ir_latency=False, analytic_computation=False)

    # ---- a frequency step of exactly 1 Hz: _group_delay_direct takes its "no step given" branch and returns radians
    # per bin, not seconds (standard/_standard_backend.py:59-62).  Same signal, sampling rate = transform length.
    def ir_at(name, fs):
        return dsp.ImpulseResponse(None, sig[name].copy(), fs, constrain_amplitude=False)

    f, gd = tf.minimum_group_delay(ir_at("ir256", 2048))
    assert f[1] - f[0] == 1.0
    add("minimum_group_delay", "ir256", gd, f=f, smoothing=0, padding_factor=8, fs=2048)
    f, gd = tf.group_delay(ir_at("ir256", 256), analytic_computation=False)
    assert f[1] - f[0] == 1.0
    add("group_delay", "ir256", gd, f=f, analytic_computation=False, smoothing=0, remove_ir_latency=False, fs=256)
    f, gd = tf.excess_group_delay(ir_at("ir256", 256))
    assert f[1] - f[0] == 1.0
    add("excess_group_delay", "ir256", gd, f=f, smoothing=0, remove_ir_latency=False, analytic_computation=False, fs=256)

    z["meta"] = np.array(json.dumps({"signals": SIGNALS, "cases": cases, "fs": FS}))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases")
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
