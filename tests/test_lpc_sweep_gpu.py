"""The linear-prediction kernels (csrc/kernels_lpc.hpp) against a long-double oracle at their lane, wave, block and
LDS edges: the problems of tests/lpc_cases.py, which tests/test_lpc_sweep_host.py shows to be within 1e-12 of the
oracle in plain float64 arithmetic, so what is measured here is the kernels'.

Every estimator problem runs three ways -- backend.lpc on the float64 host array, backend.lpc on the samples of a
device-resident Signal, and ds_lpc_dev through the C ABI with a row stride of n_samples + 13 whose padding is NaN (a NaN
in a live pair means the padding was read) -- with both methods, and every pair is compared.  The Levinson-Durbin and
synthesis problems run through backend.levinson_durbin and backend.lpc_synthesize, the singular flag through the raw
entry as well.  The bound is the family's own (BOUND of tests/test_lpc_gpu.py, 1e-9) with its error functions: a relative
to each pair's largest |a|, var relatively, NaN and zero positions equal, the synthesis relative to each channel's peak.
Every test prints the largest error it measured."""

import ctypes as C

import numpy as np
import pytest

import dsptoolbox_amd as dsp
import lpc_cases as lc
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import get_context
from feature_cases import Dev, call
from lpc_oracle import channel_error, coefficient_error, variance_error
from test_lpc_gpu import BOUND

pytestmark = pytest.mark.gpu

FS = 48000
ENTRIES = ("host", "resident", "strided")


def run_estimator(case, kind, method, entry):
    """(a of order + 1 rows, var) from one of the three entries."""
    x32 = lc.case_signal(case, kind)
    order, window = lc.order_of(case, method), lc.hann(case["L"])
    name = backend.LPC_METHODS[lc.METHODS.index(method)]
    if entry == "host":
        return backend.lpc(x32.astype(np.float64), order, window, case["hop"], name)
    if entry == "resident":
        s = dsp.Signal.from_planar_f32(np.ascontiguousarray(x32.T), FS)
        assert s.on_device
        return backend.lpc(s.device_samples, order, window, case["hop"], name)
    n, n_ch = x32.shape
    n_frames = -(-n // case["hop"])
    rows = lc.strided_rows(x32)
    assert rows.shape == (n_ch, n + lc.PAD) and np.isnan(rows[:, n:]).all()
    args = [("x", Dev(rows)), ("n_ch", n_ch), ("ldx", n + lc.PAD), ("n_samples", n), ("window", window),
            ("window_length", case["L"]), ("hop", case["hop"]), ("order", order), ("method", lc.METHODS.index(method)),
            ("a", np.zeros((order + 1, n_frames, n_ch))), ("var", np.zeros((n_frames, n_ch))),
            ("singular", np.zeros(1, np.int32))]
    rc, err, _, got = call(get_context(), "ds_lpc_dev", args, ["a", "var", "singular"])
    assert rc == 0 and not got["singular"][0], (rc, err, got.get("singular"))
    return got["a"], got["var"]


@pytest.mark.parametrize("name,kind", lc.ESTIMATOR_RUNS)
def test_estimators(name, kind):
    case = lc.estimator_case(name)
    worst = {}
    for method in case["methods"]:
        ref_a, ref_var = lc.estimator_oracle(case, kind, method)
        for entry in ENTRIES:
            a, var = run_estimator(case, kind, method, entry)
            assert a.dtype == np.float64 and var.dtype == np.float64
            ea, ev = coefficient_error(a, ref_a), variance_error(var, ref_var)  # (NaN and zero positions asserted)
            worst[method] = tuple(max(p) for p in zip(worst.get(method, (0.0, 0.0)), (ea, ev)))
            print(f"{name} {kind} {method} {entry}: L {case['L']}, hop {case['hop']}, order {lc.order_of(case, method)}, "
                  f"{var.size} pairs: a {ea:.2e}, var {ev:.2e}")
            assert ea <= BOUND and ev <= BOUND
    print(f"WORST estimators {name} {kind}:", {m: f"a {e[0]:.2e}, var {e[1]:.2e}" for m, e in worst.items()})


@pytest.mark.parametrize("order", lc.LEVINSON_ORDERS)
def test_levinson_durbin(order):
    for n_cols in lc.LEVINSON_COLUMNS:
        ref_a, ref_var, _ = lc.levinson_oracle(order, n_cols)
        r = lc.levinson_problem(order, n_cols)
        a, var = backend.levinson_durbin(r)
        ea, ev = coefficient_error(a, ref_a), variance_error(var, ref_var)
        print(f"WORST levinson_durbin order {order}, {n_cols} columns: a {ea:.2e}, var {ev:.2e}")
        assert a.shape == r.shape and ea <= BOUND and ev <= BOUND


def test_levinson_durbin_singular_at_the_last_order_of_a_late_column():
    r = lc.singular_problem()
    with pytest.raises(ValueError, match="Singular Matrix"):
        backend.levinson_durbin(r)
    others = np.delete(np.arange(lc.SINGULAR_COLUMNS), lc.SINGULAR_AT)
    backend.levinson_durbin(np.ascontiguousarray(r[:, others]))  # without that column: regular
    backend.levinson_durbin(np.ascontiguousarray(r[:-1]))          # one order less: regular, that column too
    ctx = get_context()
    a, var, flag = np.zeros_like(r), np.zeros(r.shape[1]), C.c_int(0)
    rc = ctx.lib.ds_levinson(ctx.handle, backend._ptr(r), lc.SINGULAR_ORDER, r.shape[1], backend._ptr(a),
                             backend._ptr(var), C.byref(flag))
    assert rc == 0 and flag.value == 1
    ref_a, ref_var, singular = lc.singular_oracle()
    assert singular
    ea, ev = coefficient_error(a[:, others], ref_a[:, others]), variance_error(var[others], ref_var[others])
    print(f"WORST levinson singular problem, the {len(others)} regular columns: a {ea:.2e}, var {ev:.2e}")
    assert ea <= BOUND and ev <= BOUND
    # the singular column itself: k = 0 until the last order, then -1 and a prediction error of exactly 0
    assert np.array_equal(a[:, lc.SINGULAR_AT], ref_a[:, lc.SINGULAR_AT].astype(np.float64)) and var[lc.SINGULAR_AT] == 0.0


@pytest.mark.parametrize("name", lc.SYNTHESIS_NAMES)
def test_synthesis(name):
    case = lc.synthesis_case(name)
    a, src, window = lc.synthesis_inputs(case)
    _, ref = lc.synthesis_oracle(case)
    y = backend.lpc_synthesize(a, src, window, case["hop"], case["n_out"])
    e = channel_error(y, ref)
    print(f"WORST lpc_synthesize {name}: order {case['order']}, L {case['L']}, hop {case['hop']}, "
          f"{case['n_frames']} x {case['n_ch']} pairs, {case['n_out']} samples: {e:.2e}")
    assert y.dtype == np.float64 and e <= BOUND
    assert not y[lc.uncovered(case)].any()  # between frames and past the last one: exactly 0
    if name == "ola_floor":
        assert not y[::case["hop"]].any()   # w[0] = 0 over the 1e-4 floor


def test_repeats_are_bit_identical():
    case = lc.estimator_case("chunks_o255")
    for method in case["methods"]:
        for entry in ("host", "resident"):
            first, again = run_estimator(case, "coloured", method, entry), run_estimator(case, "coloured", method, entry)
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    syn = lc.synthesis_case("seven_pairs")
    a, src, window = lc.synthesis_inputs(syn)
    assert syn["order"] == 255
    first = backend.lpc_synthesize(a, src, window, syn["hop"], syn["n_out"])
    assert np.array_equal(first, backend.lpc_synthesize(a, src, window, syn["hop"], syn["n_out"]))
