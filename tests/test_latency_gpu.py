"""Latency estimation on the device against the reference's results of tests/golden/latency/cases.npz.
Integer lags: exactly.  The 2 p + 2 values around every peak: within 1e-9 of the largest |h| of the window (the bound of
the float64 transform family, TOL of test_phase_gpu.py).  Sub-sample lags: what a perturbation of that size can do to the
root -- for one point a side 2 TOL max|h| / |h[d] - h[d + 1]| samples, the conditioning of the linear root; for two and
three points twice the largest shift of the oracle's root when any one of the 2 p fitted values moves by +-TOL max|h|;
1e-12 on top for the subtraction from the length.  Correlation coefficients: 4 n 2^-53 + 1e-15, n the overlapped length
(2 n eps is the forward bound of the centred sums through Cauchy-Schwarz, doubled).  Group delays: 1e-9 N_padded / fs per
bin.  The peak search's ties, the guards, run-to-run identity and the launch names."""

import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import get_context
import latency_cases as lc
import latency_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-9
EPS = 2.0 ** -53
tf = dsp.transfer_functions
POS = [p for p in lc.POINTS if p > 0]


def sig_of(x):
    return None if x is None else dsp.Signal(None, x.copy(), lc.FS, constrain_amplitude=False)


def ir_of(x):
    return dsp.ImpulseResponse(None, x.copy(), lc.FS, constrain_amplitude=False)


def overlap(in1, in2, lags):
    """The samples each coefficient is taken over (_get_correlation_of_latencies)."""
    n1, n2 = len(in1), len(in1 if in2 is None else in2)
    r = np.round(lags, 0).astype(int)
    return np.where(r > 0, np.minimum(n1 - np.abs(r), n2), np.minimum(n2 - np.abs(r), n1))


def check_correlations(corr, ref, in1, in2, lags, what):
    bound = 4 * overlap(in1, in2, lags) * EPS + 1e-15
    err = np.abs(corr - ref)
    print(f"{what}: correlation error {err.max():.2e}, {(err / bound).max():.2e} of the bound")
    assert (err <= bound).all(), (what, err, bound)


def root_bound(near, hmax, p):
    """The allowed error of one channel's root, from the reference's neighbourhood values alone."""
    mb = int(near[p] * near[p + 1] > 0)
    if p == 1:
        return 2 * TOL * hmax / abs(near[1 - mb] - near[2 - mb]) + 1e-12
    d = p + 4
    col = np.zeros(2 * p + 10)
    col[d - p:d + p + 2] = near
    base = orc.root_of(col, d, p)
    shift = 0.0
    for j in range(d - mb - p + 1, d - mb + p + 1):  # the 2 p fitted rows
        for s in (-1.0, 1.0):
            moved = col.copy()
            moved[j] += s * TOL * hmax
            shift = max(shift, abs(orc.root_of(moved, d, p) - base))
    return 2 * shift + 1e-12


def device_peaks(in1, in2, p, **kw):
    """backend.latency_peaks in the order of the oracle's correlation columns."""
    if in2 is not None:
        return backend.latency_peaks(in1, in2, p, **kw)
    peaks, window, near, r = backend.latency_peaks(in1[:, 1:], in1[:, :1], p, reverse_pairs=True, **kw)
    return peaks[::-1], window, None if near is None else near[::-1], r


@pytest.mark.parametrize("name", list(lc.CASES))
def test_integer_lags_are_the_references(name):
    z, meta = lc.golden()
    in1, in2 = lc.pair_of(z, name)
    lags, corr = dsp.latency(sig_of(in1), sig_of(in2))
    ref = z[f"{name}_p0_lags"]
    assert lags.dtype == ref.dtype and lags.dtype.kind == "i" and np.array_equal(lags, ref), (lags, ref)
    check_correlations(corr, z[f"{name}_p0_corr"], in1, in2, ref, f"{name} p=0")
    peaks = device_peaks(in1, in2, 0)[0]
    assert list(peaks) == meta["latency"][name]["0"]["peaks"]


@pytest.mark.parametrize("name", list(lc.CASES))
def test_neighbourhoods_and_fractional_lags(name):
    z, meta = lc.golden()
    in1, in2 = lc.pair_of(z, name)
    for p in POS:
        info = meta["latency"][name][str(p)]
        ref_near, hmax = z[f"{name}_p{p}_near"], float(z[f"{name}_p{p}_hmax"])
        peaks, window, near, _ = device_peaks(in1, in2, p)
        assert list(peaks) == info["peaks"] and window == (info["lo"], info["m"])
        e_near = np.abs(near - ref_near).max() / hmax
        assert e_near <= TOL, (name, p, e_near)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            lags, corr = dsp.latency(sig_of(in1), sig_of(in2), polynomial_points=p)
        ref = z[f"{name}_p{p}_lags"]
        assert lags.dtype == np.float64 and lags.shape == ref.shape
        bound = np.array([root_bound(ref_near[c], hmax, p) for c in range(len(ref))])
        err = np.abs(lags - ref)
        print(f"{name} p={p}: neighbourhood {e_near:.2e} of max|h|, lag error {err.max():.2e} samples "
              f"({(err / bound).max():.2e} of the bound)")
        assert (err <= bound).all(), (name, p, err, bound)
        check_correlations(corr, z[f"{name}_p{p}_corr"], in1, in2, ref, f"{name} p={p}")


def test_reversed_order_and_its_correlations():
    z, _ = lc.golden()
    x = z["c8_in1"]
    lags, corr = dsp.latency(sig_of(x))
    assert list(lags) == [25, 12, 3] and np.abs(corr - z["c8_p0_corr"]).max() <= 4 * 500 * EPS + 1e-15
    mb_lags, mb_corr = dsp.latency(dsp.MultiBandSignal([sig_of(x), sig_of(x[:, ::-1].copy())]), polynomial_points=1)
    assert mb_lags.shape == mb_corr.shape == (2, 3) and mb_lags.dtype == np.float64
    assert np.abs(mb_lags[0] - z["c8_p1_lags"]).max() <= 1e-6 and np.all(mb_lags[1] < 0)
    two = lc.pair_of(z, "c2")
    mb_lags, _ = dsp.latency(dsp.MultiBandSignal([sig_of(two[0])]), dsp.MultiBandSignal([sig_of(two[1])]))
    assert mb_lags.dtype.kind == "i" and np.array_equal(mb_lags[0], z["c2_p0_lags"])


def test_lag_pearson_entry():
    z, _ = lc.golden()
    in1, in2 = lc.pair_of(z, "c7")
    lags = np.array([7, -5, 40, 0])
    cols = np.array([0, 1, 2, 1])
    ref = orc.correlation_of_latencies(in2[:, cols], in1[:, cols], lags)
    out = backend.lag_pearson(in2, in1, lags, cols, cols)
    assert (np.abs(out - ref) <= 4 * 4096 * EPS + 1e-15).all(), (out, ref)
    flat = in1.copy()
    flat[:, 1] = 0.25
    sel = [0, 1, 2, 0]
    out = backend.lag_pearson(in2, flat, [3, 3, 3276, -4096], sel, sel)  # a constant channel, one sample left, none left
    assert np.isfinite(out[0]) and np.isnan(out[1:]).all()


# ---- the peak search ---------------------------------------------------------------------------------------------------
def test_peak_search_ties_and_edges():
    rng = np.random.default_rng(11)
    n = 12000  # three workgroups of 4096 rows
    x = 0.1 * rng.standard_normal((n, 6))
    x[3000, 0], x[8000, 0] = 1.5, -1.5  # equal magnitudes 5000 rows apart: the first
    x[0, 1] = -2.0
    x[n - 1, 2] = 2.0
    x[4095, 3] = 2.0  # the last row of the first workgroup's span
    x[4096, 4] = -2.0  # the first row of the second one's
    x[4095, 5], x[4096, 5] = -3.0, 3.0  # a tie across the two
    peaks = backend.latency_peaks(x, None, 0)[0]
    assert list(peaks) == [3000, 0, n - 1, 4095, 4096, 4095] == list(np.argmax(np.abs(x), axis=0))
    y = np.zeros((300, 1))
    y[[7, 70, 263]] = [[-1.0], [1.0], [1.0]]  # within one lane's rows and across waves
    assert list(backend.latency_peaks(y, None, 0)[0]) == [7]


def test_find_ir_latency():
    z, meta = lc.golden()
    for name in lc.IRS:
        x, e = z[name], meta["ir"][name]
        for compare, key in ((True, "find_min"), (False, "find_peak")):
            src = orc.xcorr(x, orc.min_phase_rows(x, 8)[:len(x)]) if compare else x
            _, d, lo, h = orc.fractional_peak(src, 1, detail=True)
            near, hmax = orc.neighbourhood(h, d - lo, 1), np.abs(h).max()
            bound = np.array([root_bound(near[c], hmax, 1) for c in range(x.shape[1])])
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                out = tf.find_ir_latency(ir_of(x), compare)
            err = np.abs(out - z[e[key]])
            print(f"find_ir_latency {name} compare={compare}: {err.max():.2e} samples ({(err / bound).max():.2e} of the bound)")
            assert out.shape == (x.shape[1],) and (err <= bound).all(), (name, compare, err, bound)


def test_latency_free_group_delays():
    z, meta = lc.golden()
    for name in lc.IRS:
        x, e = z[name], meta["ir"][name]
        calls = ((e["gd"], lambda: tf._group_delay(ir_of(x), analytic_computation=False, remove_ir_latency=True)),
                 (e["egd"], lambda: tf._excess_group_delay(ir_of(x), remove_ir_latency=True)),
                 (e["egd_analytic"], lambda: tf.excess_group_delay(ir_of(x), remove_ir_latency=True, analytic_computation=True)))
        n_pad = 1.0 / z[e["gd"] + "_f"][1]  # N_padded / fs
        for key, call in calls:
            f, out = call()
            n_f, step, _ = z[key + "_f"]
            assert len(f) == int(n_f) and np.allclose(f, np.arange(int(n_f)) * step, rtol=1e-9) and out.shape == z[key].shape
            err = np.abs(out - z[key]).max()
            print(f"{key}: worst bin {err:.2e} s, {err / (TOL * n_pad):.2e} of the bound")
            assert err <= TOL * n_pad, (key, err)


# ---- guards, identity, launch names ------------------------------------------------------------------------------------
def test_guards_answer_with_nothing_launched_after_them():
    ctx = get_context()
    ctx.routes()
    x = np.ones((8, 1))
    peaks, window, near = np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(40)
    ptr = backend._ptr

    def raw_call(n_a, n_b, p):
        return ctx.lib.ds_latency(ctx.handle, ptr(x), n_a, 1, ptr(x), n_b, 1, p, 0, ptr(peaks), ptr(window), ptr(near), None)

    for n_a, n_b, p in (((1 << 21) + 1, (1 << 21) + 1, 0), (8, 8, 17)):  # never read: the entry answers first
        with pytest.raises(NotImplementedError, match="not built"):
            ctx.check(raw_call(n_a, n_b, p), "ds_latency")
        assert ctx.routes() == set()
    with pytest.raises(NotImplementedError, match="beyond the device kernels' bounds"):
        backend.latency_peaks(np.ones((64, 1)), np.ones((64, 1)), 17)
    # a peak in the last row of a 64-row array: the value at row 64 is not there, the host refuses to fit
    y = np.zeros((64, 1))
    y[63], y[20] = 1.0, 0.5
    pk, win, nr, _ = backend.latency_peaks(y, None, 1)
    assert list(pk) == [63] and win == (0, 64) and np.isnan(nr[0, 2:]).all() and np.isfinite(nr[0, :2]).all()
    with pytest.raises(ValueError, match="within 2 rows of an end"):
        tf.find_ir_latency(ir_of(y), compare_to_min_phase_ir=False)
    # a window that is too long for the any-length transform, found after the peak search: nothing runs after it
    n = (1 << 21) + 500
    far = np.zeros((n, 2))
    far[100, 0], far[n - 100, 1] = 1.0, -1.0
    ctx.routes()
    with pytest.raises(NotImplementedError, match="window around the peaks"):
        backend.latency_peaks(far, None, 1)
    assert ctx.routes() == {"lat_peak", "lat_peak_final"}


def test_the_same_call_returns_the_same_bits_and_names_its_launches():
    z, _ = lc.golden()
    in1, in2 = lc.pair_of(z, "c3")
    ctx = get_context()
    ctx.routes()
    first = backend.latency_peaks(in1, in2, 1, pearson=True)
    names = ctx.routes()
    assert {"lat_xmul", "lat_peak", "lat_peak_final", "lat_window", "lat_near", "lag_partial", "lag_final",
            "lag_partial@moments", "lag_final@moments"} <= names
    assert {"fft64_lds", "fft64_transpose", "fft64_blue", "fft64_point"} <= names  # 16384 points four-step, the window Bluestein
    second = backend.latency_peaks(in1, in2, 1, pearson=True)
    assert np.array_equal(first[0], second[0]) and first[1] == second[1]
    assert np.array_equal(first[2], second[2]) and np.array_equal(first[3], second[3])
    a, b = dsp.latency(sig_of(in1), sig_of(in2), 3), dsp.latency(sig_of(in1), sig_of(in2), 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
