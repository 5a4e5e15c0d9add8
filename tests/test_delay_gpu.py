"""Fractional delays and the time-domain delay-and-sum beamformer on the device (csrc/kernels_delay.hpp through
ds_delay_sum / ds_delay_sum_dev): the reference's own outputs (tests/golden/delay, tests/golden/beamformers/
das_time.npz), the device-built taps against the reference's formula, a 64-microphone beamformer against a float64
np.convolve restatement, the device-resident route and the order limit."""

import os
import warnings

import numpy as np
import pytest
from scipy.special import iv

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd.beamforming import BeamformerDASTime, MonopoleSource, mix_sources_on_array

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
TOL_HOST, TOL_DEV = 1e-11, 1e-6


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


class StoredPoints:
    """Geometry stand-in: hands back the distances the reference computed (mics x points)."""

    def __init__(self, distances, coordinates=None):
        self.d = np.asarray(distances)
        self.number_of_points = self.d.shape[0]
        self.coordinates = np.zeros((self.d.shape[1] if self.d.ndim == 2 else 1, 3)) if coordinates is None \
            else coordinates

    def get_distances_to_point(self, point):
        return self.d


class StoredGrid:
    def __init__(self, n):
        self.number_of_points = n
        self.coordinates = np.zeros((n, 3))


def ref_filter(delay_samples, order, db=60):
    """_fractional_delay_filter (standard/_standard_backend.py:430-492 of the reference), restated."""
    d_int = int(delay_samples)
    frac = delay_samples - d_int
    m_opt = int(frac) - (order - 1) / 2 if order % 2 else np.round(frac) - order / 2
    sinc = np.sinc(np.arange(order + 1) + m_opt - frac)
    beta = backend._kaiser_window_beta(db)
    alpha = order / 2
    L = np.arange(order + 1).astype(float) - frac
    if order % 2:
        L += 0.5
    elif frac > 0.5:
        L += 1
    Z = beta * np.sqrt(np.array(1 - ((L - alpha) / alpha) ** 2, dtype="complex"))
    return int(d_int + m_opt), sinc * np.real(iv(0, Z)) / iv(0, beta)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "delay", "cases.npz"))


@pytest.fixture(scope="module")
def bf_golden():
    return np.load(os.path.join(HERE, "golden", "beamformers", "das_time.npz"))


def _fd_case(golden, i, resident):
    d, fs, order, keep, name, ch, constrained = golden[f"fd_{i}_args"]
    x = golden[["x_noise", "x_hot"][int(name)]]
    if resident:
        if constrained:
            return None, None
        s = dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T), int(fs))
    else:
        s = dsp.Signal(None, x.astype(np.float64), int(fs), constrain_amplitude=bool(constrained))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = dsp.fractional_delay(s, float(d), channels=None if ch < 0 else int(ch), keep_length=bool(keep),
                                   order=int(order))
    return out, golden[f"fd_{i}"]


@pytest.mark.parametrize("resident", [False, True])
def test_fractional_delay_golden(golden, resident):
    n_cases = sum(1 for k in golden.files if k.startswith("fd_") and k.endswith("_args"))
    assert n_cases >= 30
    for i in range(n_cases):
        out, want = _fd_case(golden, i, resident)
        if out is None:
            continue
        if resident and float(golden[f"fd_{i}_args"][0]) != 0.0:
            assert out.on_device and not out._has_host_copy
        got = out.time_data
        assert relmax(got, want) <= (TOL_DEV if resident else TOL_HOST), (i, golden[f"fd_{i}_args"])


def test_fractional_delay_multiband(golden):
    x = golden["x_noise"].astype(np.float64)
    fs = 1024
    mb = dsp.MultiBandSignal([dsp.Signal(None, x[:, :2], fs), dsp.Signal(None, 0.5 * x[:, 1:], fs)])
    out = dsp.standard.fractional_delay(mb, 5.6 / fs, order=30)
    assert isinstance(out, dsp.MultiBandSignal)
    for k in range(2):
        assert relmax(out.bands[k].time_data, golden[f"mb_{k}"]) <= TOL_HOST


def test_device_taps_against_reference_formula():
    """The taps built on the device, read back as the fractional delay of a unit impulse."""
    rng = np.random.default_rng(7)
    fracs = np.concatenate([rng.uniform(0, 1, 10000), [0.0, 0.5, 0.5 - 1e-15, 0.5 + 1e-15, 1e-300, 1 - 1e-16,
                                                       0.25, 0.75]])
    fracs = fracs[fracs < 1]
    n = 64
    imp = np.zeros((n, 1))
    imp[0] = 1.0
    for order in (30, 31, 8, 1, 2, 255):
        for db in (60, 30, 10):
            shift = np.zeros((len(fracs), 1), dtype=np.int64)
            y, _ = backend.delay_sum(imp, n, np.zeros((len(fracs), 1), dtype=np.int32), shift, fracs[:, None], 1.0,
                                     order, db, order + 1)
            want = np.stack([ref_filter(f, order, db)[1] for f in fracs], axis=1)
            err = np.max(np.abs(y - want))
            assert err <= 1e-13, (order, db, err)


def test_monopole_and_mix_golden(bf_golden):
    b = bf_golden
    fs = int(b["fs"])
    for resident in (False, True):
        def sig(v):
            if resident:
                return dsp.Signal.from_planar_f32(np.ascontiguousarray(v[None, :]), fs)
            return dsp.Signal(None, v.astype(np.float64), fs)
        tol = TOL_DEV if resident else TOL_HOST
        one = MonopoleSource(sig(b["s1"]), [0.3, -0.2, 1.2]).get_signals_on_array(StoredPoints(b["d_src1"]))
        assert one.on_device == resident
        assert relmax(one.time_data, b["one_source"]) <= tol
        for key, order in (("two_sources", (("s1", "d_src1"), ("s2", "d_src2"))),
                           ("two_sources_short_first", (("s2", "d_src2"), ("s1", "d_src1")))):
            srcs = [_DistSource(sig(b[s]), b[d]) for s, d in order]
            mics = _MicsFor(srcs)
            keep = list(srcs)
            with pytest.warns(UserWarning, match="differ in length"):
                out = mix_sources_on_array(srcs, mics)
            assert len(srcs) == 1  # the reference's pop(0) on the caller's list
            assert keep[1].emitted_signal.length_samples == 600
            assert out.on_device == resident
            assert relmax(out.time_data, b[key]) <= tol, (key, resident)


def _DistSource(signal, distances):
    """A MonopoleSource (the exact type: mix_sources_on_array asserts it) that carries its stored distances."""
    s = MonopoleSource(signal, [0.0, 0.0, 0.0])
    s.distances = distances
    return s


class _MicsFor:
    """The microphones as seen from each source (the stored distances of whichever source asks)."""

    def __init__(self, srcs):
        self.by_source = {id(s.coordinates): s.distances for s in srcs}
        self.number_of_points = len(srcs[0].distances)

    def get_distances_to_point(self, point):
        return self.by_source[id(point)]


@pytest.mark.parametrize("constrained", [False, True])
def test_das_time_golden(bf_golden, constrained):
    b = bf_golden
    fs = int(b["fs"])
    x = b["array_signal"].astype(np.float64) * (4.0 if constrained else 1.0)
    s = dsp.Signal(None, x, fs, constrain_amplitude=constrained)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = BeamformerDASTime(s, StoredPoints(b["d_grid"]), StoredGrid(b["d_grid"].shape[1])).get_beamformer_output()
    want = b["das_time_constrained" if constrained else "das_time"]
    assert relmax(out.time_data, want) <= TOL_HOST
    if not constrained:
        r = BeamformerDASTime(dsp.Signal.from_planar_f32(np.ascontiguousarray(b["array_signal"].T), fs),
                              StoredPoints(b["d_grid"]), StoredGrid(b["d_grid"].shape[1])).get_beamformer_output()
        assert r.on_device and r._has_host_copy is False
        assert relmax(r.time_data, want) <= TOL_DEV


def test_das_time_64_mics_against_float64_oracle():
    rng = np.random.default_rng(11)
    fs, n, m, g = 48000, 48000, 64, 104
    mic = np.stack([rng.uniform(-0.5, 0.5, m), rng.uniform(-0.5, 0.5, m), np.zeros(m)], axis=1)
    gx, gy = np.meshgrid(np.linspace(-1, 1, 13), np.linspace(-1, 1, 8))
    pts = np.stack([gx.ravel(), gy.ravel(), np.full(g, 1.0)], axis=1)
    ds = np.sqrt(((mic[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    ds[3, 5] = ds.max() + 0.01  # one pass-through pair (delay exactly 0)
    x = rng.standard_normal((n, m)).astype(np.float32).astype(np.float64)
    s = dsp.Signal(None, x, fs)
    out = BeamformerDASTime(s, StoredPoints(ds), StoredGrid(g)).get_beamformer_output().time_data
    cols = [0, 5, 50, 103]
    want = _das_time_oracle(x, ds, fs, cols)
    assert relmax(out[:, cols], want) <= TOL_HOST


def _das_time_oracle(x, ds, fs, cols, c=343.0, order=30):
    """BeamformerDASTime restated in float64 with np.convolve, one filter per pair, for the grid columns cols."""
    n, m = x.shape
    r0, dmin = ds.max(), ds.min()
    total = n + int((r0 - dmin) / c * fs + 2)
    out = np.zeros((total, len(cols)))
    for k, ig in enumerate(cols):
        delays = (r0 - ds[:, ig]) / c
        for im in range(m):
            if delays[im] == 0:
                y = x[:, im].copy()
            else:
                integer_delay, h = ref_filter(delays[im] * fs, order)
                y = np.convolve(x[:, im], h)
                y = np.concatenate([np.zeros(integer_delay), y]) if integer_delay >= 0 else y[-integer_delay:]
            y = y * ds[im, ig]
            out[:, k] += np.concatenate([y, np.zeros(max(0, total - len(y)))])[:total]
        out[:, k] /= m
    return out


def test_resident_in_resident_out():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 5000)).astype(np.float32)
    s = dsp.Signal.from_planar_f32(x, 48000)
    out = dsp.fractional_delay(s, 12.3 / 48000)
    assert out.on_device and not out._has_host_copy
    want = dsp.fractional_delay(dsp.Signal(None, x.T.astype(np.float64), 48000), 12.3 / 48000).time_data
    assert relmax(out.time_data, want) <= TOL_DEV


def test_order_limit():
    s = dsp.Signal(None, np.random.default_rng(0).standard_normal((300, 2)), 48000)
    assert dsp.fractional_delay(s, 1.7 / 48000, order=255).length_samples == 300 + 255 + \
        backend._delay_split(1.7, 255)[0]
    with pytest.raises(NotImplementedError):
        dsp.fractional_delay(s, 1.7 / 48000, order=256)
    with pytest.raises(NotImplementedError):  # the device entry itself refuses it (DS_ERR_UNSUP)
        backend.delay_sum(np.ones((10, 1)), 10, np.zeros((1, 1), dtype=np.int32), 0, 0.3, 1.0, 256, 60, 10)
