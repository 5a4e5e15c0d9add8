"""The linear-prediction sweep without a GPU: the problems of tests/lpc_cases.py are fit to judge a device with.

The device tests (tests/test_lpc_sweep_gpu.py) hold the kernels to 1e-9 of a long-double oracle.  That says something
about a kernel only where the arithmetic itself, in float64 and in any order, stays far below 1e-9 on the same inputs.
So every problem is run through the float64 restatement of tests/lpc_oracle.py as well, and the two must agree within
CAP = 1e-12, three decades below the device bound, with the error functions the device tests use.  This is a condition
on the inputs: a problem that misses it is replaced by another seed or signal, not excused.

Then the plain-numpy models of the kernels' arrangements (tests/test_lpc_host.py: Burg's two error rows updated in
place, the transposed direct form II with four states per lane, the overlap-add gathered per output sample) at the new
edges, within what test_lpc_host.py asserts of them, and the singular column of the Levinson-Durbin problem.
Every test prints what it measured."""

import numpy as np
import pytest
from scipy.signal import lfilter

import lpc_cases as lc
import lpc_oracle as lo
from test_lpc_host import burg_in_place, df2t_blocked, ola_gather

CAP = 1e-12
F64 = np.float64


def test_the_oracle_is_wider_than_float64():
    print("oracle dtype:", np.dtype(lc.ORACLE_DTYPE).name, "eps", float(np.finfo(lc.ORACLE_DTYPE).eps))
    assert lc.ORACLE_DTYPE is np.longdouble or np.finfo(np.longdouble).eps >= 1e-18


def test_case_tables_hold_the_edges():
    orders = lambda prefix: sorted(c["order"] for c in lc.ESTIMATOR_CASES if c["name"].startswith(prefix))
    assert orders("lags_") == [2, 3, 4, 15, 16] and orders("chunks_") == [127, 129, 130, 191, 192, 193, 194, 254, 255]
    for c in lc.ESTIMATOR_CASES:
        assert ("burg" in c["methods"]) == (c["burg_order"] <= c["L"] // 4) and c["order"] < c["L"]
    by = lc.estimator_case
    assert by("quarter_window")["order"] * 4 == by("quarter_window")["L"] and "burg" in by("quarter_window")["methods"]
    assert "burg" in by("largest_lds")["methods"] and by("largest_lds")["L"] == 8192
    assert -(-by("many_pairs")["n"] // by("many_pairs")["hop"]) > 65535
    assert sorted(c["order"] for c in lc.SYNTHESIS_CASES if c["name"].startswith("orders_")) == \
        [1, 3, 4, 5, 63, 64, 65, 252, 253, 254, 255]
    assert {64, 65, 128, 129, 192, 193, 255} <= set(lc.LEVINSON_ORDERS)
    pairs = {c["n_frames"] * c["n_ch"] for c in lc.SYNTHESIS_CASES}
    assert {1, 5, 7} <= pairs
    assert len({(n, k) for n, k in lc.ESTIMATOR_RUNS}) == len(lc.ESTIMATOR_RUNS)


@pytest.mark.parametrize("name,kind", lc.ESTIMATOR_RUNS)
def test_estimator_problems_meet_the_cap(name, kind):
    case = lc.estimator_case(name)
    x = lc.case_signal(case, kind)
    assert x.dtype == np.float32 and x.shape == (case["n"], case["n_ch"])
    for method in case["methods"]:
        a, var = lc.estimator_oracle(case, kind, method)
        a64, var64 = lc.estimator_oracle(case, kind, method, F64)
        n_frames = -(-case["n"] // case["hop"])
        assert a.shape == (lc.order_of(case, method) + 1, n_frames, case["n_ch"]) and var.shape == a.shape[1:]
        ea, ev = lo.coefficient_error(a64, a), lo.variance_error(var64, var)
        print(f"{name} {kind} {method}: float64 against the oracle: a {ea:.2e}, var {ev:.2e}, "
              f"silent pairs {int((np.isnan(var) | (var == 0)).sum())} of {var.size}")
        assert ea <= CAP and ev <= CAP
        if case["silent"] is not None:  # the silent channel's patterns, its neighbours live
            s = case["silent"]
            live = [c for c in range(case["n_ch"]) if c != s]
            assert np.isfinite(np.asarray(a[:, :, live], dtype=F64)).all() and (a[0] == 1).all()
            if method == "yw":
                assert np.isnan(a[1:, :, s]).all() and np.isnan(var[:, s]).all()
            else:
                assert not a[1:, :, s].any() and not var[:, s].any()


@pytest.mark.parametrize("order", lc.LEVINSON_ORDERS)
def test_levinson_problems_meet_the_cap(order):
    for n_cols in lc.LEVINSON_COLUMNS:
        a, var, singular = lc.levinson_oracle(order, n_cols)
        a64, var64, singular64 = lc.levinson_oracle(order, n_cols, F64)
        assert not singular and not singular64 and a.shape == (order + 1, n_cols)
        ea, ev = lo.coefficient_error(a64, a), lo.variance_error(var64, var)
        print(f"levinson order {order}, {n_cols} columns: float64 against the oracle: a {ea:.2e}, var {ev:.2e}")
        assert ea <= CAP and ev <= CAP


def test_singular_column_is_the_only_one():
    r = lc.singular_problem()
    assert r.shape == (lc.SINGULAR_ORDER + 1, lc.SINGULAR_COLUMNS)
    for dtype in (lc.ORACLE_DTYPE, F64):
        a, var, singular = lo.levinson(r, dtype)
        assert singular
        assert var[lc.SINGULAR_AT] == 0 and a[-1, lc.SINGULAR_AT] == -1 and not a[1:-1, lc.SINGULAR_AT].any()
        others = np.delete(np.arange(lc.SINGULAR_COLUMNS), lc.SINGULAR_AT)
        assert (var[others] > 0).all()
        _, _, singular_others = lo.levinson(r[:, others], dtype)
        assert not singular_others
        # the prediction error reaches 0 at the last order only: one order less is regular in every column
        assert not lo.levinson(r[:-1], dtype)[2]
    a, var, _ = lc.singular_oracle()
    a64, var64, _ = lc.singular_oracle(F64)
    ea, ev = lo.coefficient_error(a64, a), lo.variance_error(var64, var)
    print(f"singular problem: float64 against the oracle: a {ea:.2e}, var {ev:.2e}")
    assert ea <= CAP and ev <= CAP


@pytest.mark.parametrize("name", lc.SYNTHESIS_NAMES)
def test_synthesis_problems_meet_the_cap(name):
    case = lc.synthesis_case(name)
    a, src, window = lc.synthesis_problem(case)
    assert a.shape == (case["order"] + 1, case["n_frames"], case["n_ch"]) and src.shape == (case["L"],) + a.shape[1:]
    filtered, out = lc.synthesis_oracle(case)
    filtered64, out64 = lc.synthesis_oracle(case, F64)
    ef = lo.channel_error(filtered64.reshape(case["L"], -1), filtered.reshape(case["L"], -1))
    eo = lo.channel_error(out64, out)
    peak = float(np.abs(filtered).max())
    print(f"synthesis {name}: float64 against the oracle: all-pole filter {ef:.2e}, output {eo:.2e}; filtered peak {peak:.2f}")
    assert ef <= CAP and eo <= CAP and peak < 100.0
    assert out.shape == (case["n_out"], case["n_ch"]) and not out[lc.uncovered(case)].any()
    if case["scaled"]:  # the scaled inputs state the same problem
        sa, ssrc, _ = lc.synthesis_inputs(case)
        assert not (sa[0] == 1.0).all() and set(np.unique(sa[0])) == set(lc.A0_SCALES)
        e = lo.channel_error(lo.all_pole(sa, ssrc, lc.ORACLE_DTYPE).reshape(case["L"], -1), filtered.reshape(case["L"], -1))
        print(f"synthesis {name}: the scaled inputs against the unscaled oracle: {e:.2e}")
        assert e <= CAP
    else:
        assert lc.synthesis_inputs(case)[0] is a


def test_synthesis_edges_are_what_the_table_says():
    floor = lc.synthesis_case("ola_floor")
    w = lc.hann(floor["L"])
    assert w[0] == 0.0 and (w[:3] ** 2 < 1e-4).all()  # no overlap: the envelope of these samples is below the floor
    _, out = lc.synthesis_oracle(floor)
    assert not out[::floor["hop"]].any()
    gaps = lc.synthesis_case("ola_gaps")
    assert lc.uncovered(gaps).sum() == 3 * (gaps["hop"] - gaps["L"])
    padded, trimmed = lc.synthesis_case("ola_padded"), lc.synthesis_case("ola_trimmed")
    assert padded["n_out"] == padded["total"] + 50 and lc.uncovered(padded).sum() == 50
    assert trimmed["n_out"] < trimmed["total"] and not lc.uncovered(trimmed).any()


# ---- the kernels' arrangements at the new edges (models and tolerances of tests/test_lpc_host.py) -------------------
@pytest.mark.parametrize("name", [f"orders_o{o}" for o in (252, 253, 254, 255)]
                         + [f"blocks_L{L}_o{o}" for L in (63, 65, 130) for o in (3, 5)])
def test_blocked_filter_arrangement(name):
    case = lc.synthesis_case(name)
    a, src, _ = lc.synthesis_problem(case)
    worst = 0.0
    for f, c in ((0, 0), (case["n_frames"] - 1, case["n_ch"] - 1)):
        want = lfilter([1.0], a[:, f, c], src[:, f, c])
        got = df2t_blocked(a[:, f, c], src[:, f, c])
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())
    print(f"df2t_blocked {name}: {worst:.2e} of the peak off lfilter")


def test_blocked_filter_normalises_by_a0():
    case = lc.synthesis_case("scaled_a0")
    a, src, _ = lc.synthesis_problem(case)
    sa, ssrc, _ = lc.synthesis_inputs(case)
    for f in range(case["n_frames"]):
        want = lfilter([1.0], a[:, f, 0], src[:, f, 0])
        assert np.allclose(df2t_blocked(sa[:, f, 0], ssrc[:, f, 0]), want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_burg_in_place_arrangement_at_a_quarter_of_the_window():
    case = lc.estimator_case("quarter_window")
    td = lo.windowed_frames(lc.case_signal(case, "coloured"), lc.hann(case["L"]), case["hop"])
    a, den = lc.estimator_oracle(case, "coloured", "burg", F64)
    for f, c in ((0, 0), (td.shape[1] - 1, 1)):
        a1, den1 = burg_in_place(td[:, f, c], case["order"])
        ea = float(np.abs(a1 - a[:, f, c]).max() / np.abs(a[:, f, c]).max())
        ed = float(abs(den1 - den[f, c]) / abs(den[f, c]))
        print(f"burg_in_place L = {case['L']}, order {case['order']}, frame {f}, channel {c}: a {ea:.2e}, den {ed:.2e}")
        assert np.allclose(a1, a[:, f, c], rtol=0, atol=1e-12 * np.abs(a[:, f, c]).max())
        assert abs(den1 - den[f, c]) <= 1e-11 * abs(den[f, c])


@pytest.mark.parametrize("name", ["ola_gaps", "ola_hop1", "ola_padded", "ola_trimmed", "ola_floor"])
def test_gathered_overlap_add_arrangement(name):
    case = lc.synthesis_case(name)
    filtered, want = lc.synthesis_oracle(case, F64)
    got = ola_gather(filtered, lc.hann(case["L"]), case["hop"], case["n_out"])
    print(f"ola_gather {name}: {float(np.abs(got - want).max() / np.abs(want).max()):.2e} of the peak off overlap_add")
    assert np.allclose(got, want, rtol=0, atol=1e-13 * np.abs(want).max())
    assert not got[lc.uncovered(case)].any()
