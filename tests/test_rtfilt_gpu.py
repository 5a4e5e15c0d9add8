"""The realtime filters on the device (csrc/kernels_rtfilt.hpp through ds_rtfilt / ds_rtfilt_dev / ds_rtfir /
ds_rtfir_dev): every case of rtfilt_cases.py against the long-double oracle within the case's bound (block, group and
state-count edges; the four bands of the state-variable filter; the parallel filter's delays and FIR part; entry states;
final states from the lane that holds the last sample), the direct FIR sum within its forward error bound, successive
calls against one call over the joined signal, bit-identical repeats, the guards, the reference's golden vectors through
the classes, process_sample continuing after filter_signal, the chain, and device-resident signals."""

import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import rtfilt_cases as rc
import rtfilt_oracle as ro
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import get_context
from dsptoolbox_amd.filterbanks import (FilterChain, FIRFilter, IIRFilter, ParallelFilter, StateSpaceFilter,
                                        StateVariableFilter)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = 2.0 ** -24 * 1.001


def run(name, x=None, zi="case", want_zf=True):
    s, x0, zi0, _, _ = rc.problem(name)
    kind, coef, d, aux, delay, fir = rc.pack(s)
    return backend.rtfilt_filter(x0 if x is None else x, kind, coef, d, aux, delay, fir,
                                 zi=zi0 if isinstance(zi, str) else zi, want_zf=want_zf)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_against_the_oracle(name):
    y, zf = run(name)
    spec = rc.CASES[name]
    shape = (spec["n"], spec["n_ch"])
    assert y.shape == ((4,) + shape if spec["kind"] == "svf" else shape) and y.dtype == np.float64
    assert zf.shape == (spec["d"], spec["n_ch"])
    e, tol = rc.error(name, y, zf), rc.tolerance(name)
    print(f"{name}: {e:.2e} of the peak (bound {tol:.2e}, emulation {rc.RTFILT_EMULATION[name] * rc.EPS:.2e})")
    assert e <= tol, (name, e, tol)


@pytest.mark.parametrize("name", list(rc.FIR_CASES))
def test_fir_sum_within_its_forward_error_bound(name):
    b, x, hist, y_ref, bound = rc.fir_problem(name)
    y = backend.rtfir_filter(x, b, hist)
    assert y.shape == x.shape and y.dtype == np.float64
    err = np.abs(y.astype(ro.LD) - y_ref)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{name}: worst error {worst:.3f} of the element's bound")
    assert np.all(err <= bound)
    assert np.array_equal(backend.rtfir_filter(x, b, hist), y)  # one writer per sample: the same bits
    if hist is None:
        assert np.array_equal(backend.rtfir_filter(x, b, np.zeros((x.shape[1], len(b) - 1))), y)


@pytest.mark.parametrize("name,cut", [("tdf2_d63_n2049_zi", 31), ("tdf2_d64_n4097_zi", rc.G + 7),
                                      ("state_space_d64_n4097_zi", rc.G), ("state_space_d63_n2049_zi", rc.G - 1),
                                      ("parallel_d64_n4097_delay0_zi", 2 * rc.G), ("svf_d2_n4097_zi", rc.G + 7),
                                      ("svf_d2_n2049_zi", 31)])
def test_two_calls_with_state_equal_one_joined_call(name, cut):
    x = rc.problem(name)[1]
    y1, z1 = run(name, x[:cut])
    y2, z2 = run(name, x[cut:], zi=z1)
    e = rc.error(name, np.concatenate([y1, y2], axis=-2), z2)
    tol = rc.tolerance(name)  # (the bound of the joined case)
    print(f"{name} cut at {cut}: {e:.2e} (bound {tol:.2e})")
    assert e <= tol


def test_repeats_are_bit_identical_and_no_state_is_zero_state():
    for name in ("tdf2_d5_n4097", "state_space_d64_n4097_zi", "parallel_d64_n4097_delay33_fir", "svf_d2_n4097_zi"):
        (a, za), (b, zb) = run(name), run(name)
        assert np.array_equal(a, b) and np.array_equal(za, zb)
    for name in ("svf_d2_n2049", "tdf2_d5_n2049", "state_space_d5_n2049", "parallel_d2_n2049"):
        d = rc.CASES[name]["d"]
        (a, za), (b, zb) = run(name), run(name, zi=np.zeros((d, 1)))
        assert np.array_equal(a, b) and np.array_equal(za, zb)
        assert np.array_equal(run(name, want_zf=False), a)  # (without the final state)


def test_guards_refuse_before_the_device():
    ctx = get_context()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    x, y = np.zeros((8, 1)), np.empty((4, 8, 1))

    def call(kind, coef, d, aux=0, n_ch=1, n=8, delay=0, fir=None):
        return ctx.lib.ds_rtfilt(ctx.handle, p(x), n_ch, n, kind, p(coef), d, aux, delay, p(fir), 0 if fir is None else len(fir),
                                 None, p(y), None)

    with pytest.raises(NotImplementedError, match="more than 64 states"):
        ctx.check(call(backend.RTFILT_TDF2, np.zeros(132), 65), "ds_rtfilt")
    tdf2_64 = np.zeros(130)
    tdf2_64[0] = tdf2_64[65] = 1.0
    assert call(backend.RTFILT_TDF2, tdf2_64, 64) == 0
    with pytest.raises(NotImplementedError, match="carry gain"):  # an unstable first-order recursion
        ctx.check(call(backend.RTFILT_TDF2, np.array([1.0, 0.0, 1.0, -1.5]), 1), "ds_rtfilt")
    with pytest.raises(NotImplementedError, match="carry gain"):  # stable but ill-conditioned: above the companion limit
        from scipy.signal import butter
        b, a = butter(12, 0.05)
        ctx.check(call(backend.RTFILT_TDF2, np.concatenate([b, a]), 12), "ds_rtfilt")
    ss1 = np.array([0.5, 1.0, 1.0, 0.0])
    for bad in (dict(kind=4), dict(kind=-1), dict(d=0), dict(n_ch=0), dict(n=0), dict(kind=backend.RTFILT_SVF, d=3),
                dict(kind=backend.RTFILT_PARALLEL, d=2, aux=0), dict(kind=backend.RTFILT_PARALLEL, d=3, aux=1),
                dict(aux=1), dict(delay=1), dict(fir=np.ones(3)), dict(kind=backend.RTFILT_PARALLEL, d=2, aux=1, delay=-1)):
        a = dict(kind=backend.RTFILT_STATE_SPACE, d=1, aux=0, n_ch=1, n=8, delay=0, fir=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ctx.check(call(a["kind"], np.concatenate([ss1, np.zeros(32)]), a["d"], a["aux"], a["n_ch"], a["n"], a["delay"],
                           a["fir"]), "ds_rtfilt")
    with pytest.raises(ValueError, match="finite"):
        ctx.check(call(backend.RTFILT_STATE_SPACE, np.array([0.5, np.nan, 1.0, 0.0]), 1), "ds_rtfilt")
    sec = np.array([1.0, 0.0, 0.0, -0.5, 0.1])
    with pytest.raises(NotImplementedError, match="4096 taps"):
        ctx.check(call(backend.RTFILT_PARALLEL, sec, 2, 1, fir=np.ones(4097)), "ds_rtfilt")
    fir_call = lambda b: ctx.lib.ds_rtfir(ctx.handle, p(x), 1, 8, p(b), len(b), None, p(y))
    with pytest.raises(NotImplementedError, match="4096 taps"):
        ctx.check(fir_call(np.ones(4097)), "ds_rtfir")
    with pytest.raises(ValueError, match="finite"):
        ctx.check(fir_call(np.array([1.0, np.inf])), "ds_rtfir")
    assert fir_call(np.ones(4096)) == 0
    with pytest.raises(NotImplementedError, match="2\\^40"):
        ctx.check(ctx.lib.ds_rtfir(ctx.handle, p(x), 1, 2 ** 29, p(np.ones(4096)), 4096, None, p(y)), "ds_rtfir")


# ---- the golden vectors through the classes --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "rtfilt", "cases.npz"))
    return z, json.loads(str(z["meta"]))


def emulation_error(s, x):
    """The float64 emulation of the blocked algorithm against the long-double recursion on this very filter and input,
    outputs and final states."""
    y_ref, zf_ref = ro.serial(s, x)
    y, zf = ro.blocked_f64(s, x)
    return max(ro.stream_error(y, y_ref), ro.stream_error(zf.reshape(-1, 1), zf_ref.reshape(-1, 1)))


def golden_tolerance(meta, family, emulation):
    """The reference's own distance to the long-double recursion, as tools/gen_golden_rtfilt.py measured it for the
    family, x HOST_MARGIN, plus the device's: 4 x HOST_MARGIN x the emulation's error, the rule of rtfilt_cases.py."""
    return rc.HOST_MARGIN * meta["worst"][family] + 4.0 * rc.HOST_MARGIN * emulation


def signal(td, fs):
    return dsp.Signal(None, np.array(td, dtype=np.float64), fs, constrain_amplitude=False)


def continue_by_samples(f, x, start, count=8):
    return np.array([[f.process_sample(x[start + n, c], c) for c in range(x.shape[1])] for n in range(count)])


def test_golden_state_variable_filter(golden):
    z, meta = golden
    x, fs = z["x"].astype(np.float64), meta["fs"]
    svf = StateVariableFilter(*meta["svf"], fs)
    s = ro.svf_structure(*meta["svf"], fs)
    tol = golden_tolerance(meta, "svf", emulation_error(s, x))
    mb = svf.filter_signal(signal(x, fs))  # (re-dimensions to two channels silently, as the reference does)
    assert type(mb) is dsp.MultiBandSignal and len(mb.bands) == 4 and all(type(b) is dsp.Signal for b in mb.bands)
    got = np.stack([b.time_data for b in mb.bands])
    e = max(ro.stream_error(got, z["svf_y"]), ro.stream_error(svf.state.reshape(-1, 1), z["svf_state"].reshape(-1, 1)))
    print(f"svf: {e:.2e} (bound {tol:.2e})")
    assert e <= tol
    ps = np.array([svf.process_sample(x[i, 0], 0) for i in range(5)])  # goes on from the state filter_signal left
    assert np.max(np.abs(ps - z["svf_ps"])) <= tol * np.max(np.abs(z["svf_y"]))
    # two calls continue the recursion
    svf.reset_state()
    a = svf.filter_signal(signal(x[:100], fs))
    b = svf.filter_signal(signal(x[100:], fs))
    joined = np.stack([np.concatenate([p.time_data, q.time_data]) for p, q in zip(a.bands, b.bands)])
    assert ro.stream_error(joined, z["svf_y"]) <= tol
    with pytest.raises(ValueError, match="fewer samples than channels"):  # (only a resident signal can be that shape)
        svf.filter_signal(dsp.Signal.from_planar_f32(np.ones((3, 2), dtype=np.float32), fs))
    ir = svf.get_ir(64)
    assert len(ir.bands) == 4 and type(ir.bands[0]) is dsp.ImpulseResponse and ir.bands[0].time_data.shape == (64, 1)


def test_golden_iir_fir_state_space_and_process_sample_goes_on(golden):
    z, meta = golden
    x, fs = z["x"].astype(np.float64), meta["fs"]
    cut = 333
    b, a = z["iir_b"], z["iir_a"]
    s_iir = dict(kind="tdf2", b=b / a[0], a=a / a[0])
    s_ss = dict(kind="state_space", A=z["ss_A"], B=z["ss_B"], C=z["ss_C"], Dd=float(z["ss_D"]))
    ss = StateSpaceFilter.from_filter(dsp.Filter.from_ba(b.copy(), a.copy(), fs))
    for f, s, family, key, state in ((IIRFilter(b.copy(), a.copy()), s_iir, "iir", "iir", "state"), (ss, s_ss, "ss", "ss", "x")):
        tol = golden_tolerance(meta, family, emulation_error(s, x))
        with pytest.warns(UserWarning, match="Number of channels"):
            y1 = f.filter_signal(signal(x[:cut], fs))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            y2 = f.filter_signal(signal(x[cut:], fs))
        final = z[f"{key}_state" if state == "state" else "ss_x"]
        assert type(y1) is dsp.Signal and getattr(f, state).shape == final.shape
        e = max(ro.stream_error(np.concatenate([y1.time_data, y2.time_data]), z[f"{key}_y"]),
                ro.stream_error(getattr(f, state).reshape(-1, 1), final.reshape(-1, 1)))
        f.reset_state()
        f.filter_signal(signal(x[:cut], fs))
        nxt = continue_by_samples(f, x, cut)
        e = max(e, float(np.max(np.abs(nxt - z[f"{key}_y"][cut:cut + 8]) / np.max(np.abs(z[f"{key}_y"]), axis=0))))
        print(f"{family}: {e:.2e} (bound {tol:.2e})")
        assert e <= tol
    # FIRFilter: the output within the dot product's bound; the state holds input samples, so it is exact
    fb = z["fir_b"]
    fir = FIRFilter(fb.copy())
    with pytest.warns(UserWarning, match="Number of channels"):
        y1 = fir.filter_signal(signal(x[:cut], fs))
    y2 = fir.filter_signal(signal(x[cut:], fs))
    got = np.concatenate([y1.time_data, y2.time_data])
    bound = len(fb) * rc.EPS * ro.fir_direct(np.abs(fb), np.abs(x)).astype(np.float64)
    assert np.all(np.abs(got - z["fir_y"]) <= 2 * bound)  # (the reference's own sum has the same bound)
    assert np.array_equal(fir.state, z["fir_state"]) and np.array_equal(fir.current_state_ind, z["fir_ind"])
    fir.reset_state()
    fir.set_n_channels(2)
    fir.filter_signal(signal(x[:cut], fs))
    nxt = continue_by_samples(fir, x, cut)
    assert np.all(np.abs(nxt - z["fir_y"][cut:cut + 8]) <= 2 * bound[cut:cut + 8])
    short = FIRFilter(fb.copy())  # fewer samples than the order: the older entries of the buffer stay
    short.set_n_channels(2)
    ref_state = FIRFilter(fb.copy())
    ref_state.set_n_channels(2)
    for piece in (x[:5], x[5:8], x[8:30]):
        short.filter_signal(signal(piece, fs))
        for c in range(2):
            for v in piece[:, c]:
                ref_state.process_sample(v, c)
        assert np.array_equal(short.state, ref_state.state) and np.array_equal(short.current_state_ind, ref_state.current_state_ind)
    y0 = FIRFilter(np.array([0.5])).filter_signal(signal(x[:, :1], fs)).time_data
    assert np.array_equal(y0, 0.5 * x[:, :1])


def test_golden_parallel_filter(golden):
    z, meta = golden
    x, fs = z["x"].astype(np.float64), meta["fs"]
    par = ParallelFilter(z["par_poles"], meta["par"]["n_fir"], fs).set_parameters(delay_iir_samples=meta["par"]["delay"])
    par._sos = z["par_sos"].copy()
    par.set_coefficients(z["par_sos"][:, :2], z["par_fir"])
    s = dict(kind="parallel", sos=z["par_sos"][:, [0, 1, 2, 4, 5]], delay=meta["par"]["delay"], fir=z["par_fir"])
    tol = golden_tolerance(meta, "parallel", emulation_error(s, x))
    y = par.filter_signal(signal(x, fs))
    e = ro.stream_error(y.time_data, z["par_y"])
    print(f"parallel: {e:.2e} (bound {tol:.2e})")
    assert type(y) is dsp.Signal and e <= tol
    d = np.zeros((64, 1))
    d[0] = 1.0
    ir = par.get_ir(64)
    want = z["par_get_ir"]
    assert type(ir) is dsp.ImpulseResponse
    assert ro.stream_error(ir.time_data, want) <= golden_tolerance(meta, "parallel", emulation_error(s, d))


def test_filter_chain_against_the_oracles_composition(golden):
    z, meta = golden
    x, fs = z["x"].astype(np.float64), meta["fs"]
    b, a = z["iir_b"], z["iir_a"]
    make = lambda: FilterChain([IIRFilter(b.copy(), a.copy()), FIRFilter(z["fir_b"].copy()),
                                StateSpaceFilter.from_filter(dsp.Filter.from_ba(b.copy(), a.copy(), fs))])
    chain = make()
    chain.set_n_channels(2)
    s_iir = dict(kind="tdf2", b=b / a[0], a=a / a[0])
    s_ss = dict(kind="state_space", A=z["ss_A"], B=z["ss_B"], C=z["ss_C"], Dd=float(z["ss_D"]))
    stage1 = ro.serial(s_iir, x)[0]
    stage2 = ro.fir_direct(z["fir_b"], stage1)
    want = ro.serial(s_ss, stage2)[0]
    # A member's error is carried through the members behind it: through the FIR member it grows by at most sum |b|,
    # through the state-space member by at most the l1 norm of its impulse response.  Per channel, in absolute terms:
    # the first member's bound; that carried plus the FIR sum's own forward bound; that carried plus the last member's.
    peak = lambda a: np.max(np.abs(a), axis=0).astype(np.float64)
    d = np.zeros((len(x), 1))
    d[0] = 1.0
    l1_fir, l1_ss = float(np.sum(np.abs(z["fir_b"]))), float(np.sum(np.abs(ro.serial(s_ss, d)[0])))
    fir_own = float(np.max(len(z["fir_b"]) * rc.EPS * ro.fir_direct(np.abs(z["fir_b"]), np.abs(stage1))))

    def carried(own1, own2, own3):
        return float(np.max((l1_ss * (l1_fir * own1 * peak(stage1) + own2) + own3 * peak(want)) / peak(want)))

    tol = carried(4.0 * rc.HOST_MARGIN * emulation_error(s_iir, x), fir_own,
                  4.0 * rc.HOST_MARGIN * emulation_error(s_ss, stage2.astype(np.float64)))
    y = chain.filter_signal(signal(x, fs))
    e = ro.stream_error(y.time_data, want)
    print(f"chain: {e:.2e} (bound {tol:.2e}); golden {ro.stream_error(y.time_data, z['chain_y']):.2e}")
    assert e <= tol and ro.stream_error(y.time_data, z["chain_y"]) <= tol + rc.HOST_MARGIN * meta["worst"]["chain"]
    resident = make()
    resident.set_n_channels(2)
    out = resident.filter_signal(dsp.Signal.from_planar_f32(np.ascontiguousarray(z["x"].T), fs))
    # rounded to float32 once per member: 2^-24 of each member's peak, carried like the members' own errors
    tol32 = carried(F32, F32 * float(np.max(peak(stage2))), F32) + tol
    e32 = ro.stream_error(out.time_data, y.time_data)
    print(f"chain resident: {e32:.2e} (bound {tol32:.2e})")
    assert out.on_device and e32 <= tol32


# ---- device-resident signals -----------------------------------------------------------------------------------------
def test_resident_fp32_signals_are_filtered_where_they_lie(golden):
    """A resident signal against the host entry on the same fp32-rounded samples: the same float64 recursion, the output
    rounded to fp32 once (2^-24 of the sample, so of the peak)."""
    z, meta = golden
    fs = meta["fs"]
    planar = np.ascontiguousarray(z["x"].T)  # (2, N) float32
    x = z["x"].astype(np.float64)
    b, a = z["iir_b"], z["iir_a"]

    def parallel():
        par = ParallelFilter(z["par_poles"], 3, fs).set_parameters(delay_iir_samples=2)
        par._sos = z["par_sos"].copy()
        return par.set_coefficients(z["par_sos"][:, :2], z["par_fir"])

    makers = [lambda: IIRFilter(b.copy(), a.copy()), lambda: FIRFilter(z["fir_b"].copy()),
              lambda: StateSpaceFilter.from_filter(dsp.Filter.from_ba(b.copy(), a.copy(), fs)), parallel,
              lambda: StateVariableFilter(*meta["svf"], fs)]
    for make in makers:
        on_host, resident = make(), make()
        for f in (on_host, resident):
            if not isinstance(f, ParallelFilter):  # (its filter_signal runs from rest and holds no state)
                f.set_n_channels(2)
        for call in range(2):  # the second call enters with the state the first left: only the states cross
            want = on_host.filter_signal(signal(x, fs))
            out = resident.filter_signal(dsp.Signal.from_planar_f32(planar, fs))
            if isinstance(resident, StateVariableFilter):
                assert all(bd.on_device and type(bd) is dsp.Signal for bd in out.bands)
                got, ref = np.stack([bd.time_data for bd in out.bands]), np.stack([bd.time_data for bd in want.bands])
            else:
                assert out.on_device and type(out) is dsp.Signal
                got, ref = out.time_data, want.time_data
            e = ro.stream_error(got, ref)
            print(f"{type(resident).__name__} call {call}: resident against host entry {e:.2e}")
            assert e <= F32
            for attr in ("state", "x", "current_state_ind"):
                if hasattr(resident, attr) and not isinstance(resident, ParallelFilter):
                    assert np.array_equal(getattr(resident, attr), getattr(on_host, attr))
