"""The delay-and-sum kernels (csrc/kernels_delay.hpp) against a float64 numpy oracle, at the shapes where they split
their work.

tests/test_delay_gpu.py checks ds_delay_sum through the features built on it, at the shapes those produce.  Here a
plain restatement of

    y[g, t] = sum_j w[g,j] (h(frac[g,j]) * x_src[g,j])[t - shift[g,j]],   0 <= t < out_len

with np.convolve, one term at a time, is first checked without a GPU against the reference's own time-domain
delay-and-sum output (tests/golden/beamformers/das_time.npz), and then judges k_delay_sum where it can go wrong: both
sides of the switch between the workgroup-wide and the wave-by-wave filling of the LDS windows, row counts that leave
a workgroup partly empty, workgroups whose rows share the source of one term and not of the next, sources shorter
than their buffer (NaN behind the valid samples: one read too far shows) and of length 0, negative and far shifts,
every output-tail length around a lane and a tile, orders on both sides of a multiple of 8 taps, pass-through terms,
zero and negative weights, the peak output and the peak-only mode over several tiles.

The bound is |y - oracle| <= tol * scale[g] with scale[g] = sum_j |w[g,j]| sum_k |h_k| max|x_src|, tol = 1e-11 for the
float64 host entry and 1e-6 for the float32 device entry (oracle on the float32-rounded input).  The oracle itself is
within 1.7e-16 of scale of a long-double evaluation.  A row whose oracle is identically zero must be exactly zero;
only a row whose weights are all zero has scale 0, and that rule covers it.

Every GPU test prints its worst row error as a fraction of the bound.  No MI355X figures are recorded here yet: the
sweep has only been checked without a GPU, where a numpy emulation of k_delay_sum's staging and tap loop stays within
5e-16 of scale of the oracle on every case of the table."""

import functools
import os
import zlib

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import DeviceBuffer, DevicePlanar
from dsptoolbox_amd.beamforming import BeamformerDASTime
from test_delay_gpu import TOL_DEV, TOL_HOST, StoredGrid, StoredPoints, ref_filter

HERE = os.path.dirname(__file__)
DB = 60.0  # side lobe suppression of every case (fractional_delay's default)
N = 1500   # samples per source buffer unless a case says otherwise
LD_PAD = 36  # NaN columns behind the N samples of the planar float32 buffer of the device entry

# mirrors of csrc/kernels_delay.hpp
TT = 512    # outputs per row and workgroup
R = 8       # outputs per lane; the taps are padded to a multiple of it
WAVES = 4   # rows per workgroup
SHARED_SPAN_MAX = WAVES * (TT + 256)


# ---- the oracle --------------------------------------------------------------------------------------------------
def oracle(x, src_len, src, shift, frac, weight, order, out_len):
    """x (samples, sources) float64, source c valid over [0, src_len[c]) and zero outside; src, shift, frac, weight
    (rows, terms) -> y (out_len, rows) float64 and the row scale (rows,)."""
    n_rows, n_terms = src.shape
    y = np.zeros((out_len, n_rows))
    scale = np.zeros(n_rows)
    for g in range(n_rows):
        for j in range(n_terms):
            xs = x[:src_len[src[g, j]], src[g, j]]
            h = np.ones(1) if frac[g, j] < 0 else ref_filter(float(frac[g, j]), order, DB)[1]
            w, s = float(weight[g, j]), int(shift[g, j])
            if xs.size == 0:
                continue
            scale[g] += abs(w) * np.sum(np.abs(h)) * np.max(np.abs(xs))
            full = np.convolve(xs, h)  # sample i of it lands on output s + i
            lo, hi = max(0, s), min(out_len, s + full.size)
            if hi > lo:
                y[lo:hi, g] += w * full[lo - s:hi - s]
    return y, scale


# ---- the kernel's choice of staging pass, restated ---------------------------------------------------------------
def staging_passes(case):
    """{(workgroup row block, tile, term): "shared" | "waves"} as k_delay_sum decides it"""
    src, shift = case["src"], case["shift"]
    ntp = -(-(case["order"] + 1) // R) * R
    wl = TT + ntp
    out = {}
    for wg in range(-(-src.shape[0] // WAVES)):
        rows = slice(wg * WAVES, min(src.shape[0], (wg + 1) * WAVES))  # the absent rows take no part
        for tile in range(-(-case["out_len"] // TT)):
            for j in range(src.shape[1]):
                b = [tile * TT - int(s) - (ntp - 1) for s in shift[rows, j]]
                same = len(set(src[rows, j].tolist())) == 1
                out[wg, tile, j] = "shared" if same and max(b) - min(b) + wl <= SHARED_SPAN_MAX else "waves"
    return out


def shift_spread(case, wg=0, j=0):
    s = case["shift"][wg * WAVES:(wg + 1) * WAVES, j]
    return int(s.max()) - int(s.min())


# ---- the case table ----------------------------------------------------------------------------------------------
def _case(name, item, order, out_len, src, shift, frac, weight, src_len=(N,), n=N, peaks=False, spikes=None):
    src = np.asarray(src, dtype=np.int32)
    assert src.ndim == 2

    def bc(a, t):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=t), src.shape))

    return dict(name=name, item=item, order=order, out_len=int(out_len), src=src, shift=bc(shift, np.int64),
                frac=bc(frac, np.float64), weight=bc(weight, np.float64), src_len=tuple(src_len), n=n, peaks=peaks,
                spikes=spikes)


def _mixed_terms(rng, n_terms):
    """8 rows over sources of length (1500, 700, 0): an even term has one source per workgroup (the empty one among
    them), an odd term a source per row; the first workgroup's even terms keep their shifts within 200 samples of
    each other (the shared pass), everything else is drawn from the whole range"""
    shared = {0: (1, 0), 2: (2, 1), 4: (0, 2)}
    src = np.empty((8, n_terms), dtype=np.int32)
    shift = rng.integers(-40, 3001, (8, n_terms))
    for j in range(n_terms):
        if j % 2 == 0:
            src[:4, j], src[4:, j] = shared[j]
            shift[:4, j] = rng.integers(-40, 2801) + rng.integers(0, 201, 4)
        else:
            src[:, j] = (rng.permutation(8) + j) % 3  # eight rows over three sources: no workgroup agrees
    return src, shift


def _cases():
    rng = np.random.default_rng(20240611)

    def fr(*shape):
        return rng.uniform(0.02, 0.98, shape)

    out = []
    # 1. the staging switch: 4 rows of one source, shifts spread over s
    for order, spreads in ((30, (0, 1, 2527, 2528, 2529, 5000)), (255, (2303, 2304, 2305))):
        for s in spreads:
            n = N if s < 5000 else 960  # out_len stays at 6000
            out.append(_case(f"switch-order{order}-s{s}", 1, order, n + s + order + 10, np.zeros((4, 1)),
                             [[0], [s // 3], [2 * s // 3], [s]], fr(4, 1), rng.standard_normal((4, 1)),
                             src_len=(n,), n=n))
    # 2. row remainders, one source for all rows and a source per row; the first term's shifts lie close together,
    #    the second's far apart
    for n_rows in (1, 2, 3, 5, 6, 7):
        for kind in ("shared", "own"):
            src = np.zeros((n_rows, 2)) if kind == "shared" else \
                (np.arange(n_rows)[:, None] + np.arange(2)[None, :]) % n_rows
            shift = np.stack([rng.integers(0, 200, n_rows), np.arange(n_rows) % WAVES * 900 + rng.integers(0, 50, n_rows)],
                             axis=1)
            n_src = 1 if kind == "shared" else n_rows
            out.append(_case(f"rows{n_rows}-{kind}", 2, 30, N + 2800, src, shift, fr(n_rows, 2),
                             rng.standard_normal((n_rows, 2)), src_len=(N,) * n_src))
    # 3. mixed terms over sources of three lengths
    for n_terms in (2, 5):
        src, shift = _mixed_terms(rng, n_terms)
        out.append(_case(f"mixed-terms{n_terms}", 3, 30, N + 3040, src, shift, fr(8, n_terms),
                         rng.standard_normal((8, n_terms)), src_len=(N, 700, 0)))
    # 4. shifts: rows 3 to 6 lie wholly outside the output
    order, out_len = 30, N + 30 + 10
    out.append(_case("shifts", 4, order, out_len, np.zeros((8, 1)),
                     [[-1], [-7], [-(N + order) + 1], [-(N + order)], [out_len], [10**12], [-10**12], [0]],
                     fr(8, 1), rng.uniform(0.5, 2.0, (8, 1))))
    # 5. the output tail around a lane's 8 outputs and a tile's 512
    for out_len in (1, 7, 8, 9, 511, 512, 513, 1024, 1031):
        out.append(_case(f"tail-{out_len}", 5, 30, out_len, np.zeros((3, 2)), rng.integers(-5, 40, (3, 2)), fr(3, 2),
                         rng.standard_normal((3, 2))))
    # 6. orders with order + 1 on both sides of a multiple of 8
    for order in (1, 2, 6, 7, 8, 30, 31, 254, 255):
        out.append(_case(f"order-{order}", 6, order, N + order + 20, np.zeros((2, 2)), rng.integers(-3, 11, (2, 2)),
                         fr(2, 2), rng.standard_normal((2, 2))))
    # 7. pass-through terms
    out.append(_case("through-alone", 7, 30, N + 10, [[0]], [[0]], [[-1.0]], [[1.0]]))
    out.append(_case("through-mixed", 7, 30, N + 60, [[0, 0, 0]], [[3, 0, 17]], [[-1.0, 0.3, 0.81]], [[0.7, -1.2, 0.4]]))
    # 8. weights: zero and negative within a row, and a row of zeros
    out.append(_case("weights", 8, 30, N + 60, np.zeros((2, 3)), rng.integers(0, 20, (2, 3)), fr(2, 3),
                     [[0.0, -1.5, 1.0], [0.0, 0.0, 0.0]], peaks=True))
    # 9. peaks over four tiles: rows 0 to 2 carry a spike in tiles 0, 1 and 2, row 3 is shifted out of the output
    out.append(_case("peaks", 9, 30, 1600, [[0, 3], [1, 3], [2, 3], [0, 3]],
                     [[0, 5], [2, 9], [1, 0], [10**6, 10**6]], fr(4, 2), [[1.0, 0.5], [-1.0, 0.5], [1.0, -0.5], [1.0, 1.0]],
                     src_len=(N,) * 4, peaks=True, spikes=((0, 100), (1, 700), (2, 1300))))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
DEVICE_CASES = [c for c in CASES if c["item"] <= 8]


def _id(c):
    return c["name"]


@functools.lru_cache(maxsize=None)
def problem(name, entry):
    """the case's samples and its oracle, computed once: x (n, sources) float64 with NaN from src_len on (for the
    device entry rounded to float32 first), oracle y (out_len, rows), row scales"""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal((c["n"], len(c["src_len"])))
    if c["spikes"]:
        x *= 0.01
        for col, at in c["spikes"]:
            x[at, col] = 100.0
    if entry == "device":
        x = x.astype(np.float32).astype(np.float64)
    for col, n_valid in enumerate(c["src_len"]):
        x[n_valid:, col] = np.nan
    y, scale = oracle(x, c["src_len"], c["src"], c["shift"], c["frac"], c["weight"], c["order"], c["out_len"])
    for a in (x, y, scale):
        a.setflags(write=False)
    return x, y, scale


def judge(c, y, ref, scale, tol):
    """the worst row error as a fraction of its bound; rows whose oracle is zero must be zero exactly"""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert np.all(np.isfinite(y)), ("not finite at (t, row)", np.argwhere(~np.isfinite(y))[:8])
    worst = 0.0
    for g in range(ref.shape[1]):
        err = np.abs(y[:, g].astype(np.float64) - ref[:, g])
        if not ref[:, g].any():
            assert not y[:, g].any(), (c["name"], "row", g, "must be zero, is not at t =", np.flatnonzero(y[:, g])[:8])
            continue
        t = int(np.argmax(err))
        ratio = err[t] / (tol * scale[g])
        worst = max(worst, ratio)
        assert ratio <= 1.0, (c["name"], "row", g, "t", t, "tile", t // TT, "error / scale", err[t] / scale[g])
    return worst


# ---- 1. without a GPU: the table and the oracle ------------------------------------------------------------------
def test_cases_are_well_posed_and_cover_the_grid():
    # the largest spread the shared pass takes, and one more, at both orders
    for order, edge in ((30, 2528), (255, 2304)):
        ntp = -(-(order + 1) // R) * R
        assert edge + TT + ntp == SHARED_SPAN_MAX
        at = {shift_spread(c): c for c in CASES if c["item"] == 1 and c["order"] == order}
        assert edge in at and edge + 1 in at, (order, sorted(at))
        assert set(staging_passes(at[edge]).values()) == {"shared"}
        assert set(staging_passes(at[edge + 1]).values()) == {"waves"}
    # some workgroup fills its windows both ways within one call; so does every mixed-terms case
    both = [c["name"] for c in CASES
            if any({"shared", "waves"} <= {p for (wg, _, _), p in staging_passes(c).items() if wg == w}
                   for w in range(-(-c["src"].shape[0] // WAVES)))]
    assert both and {c["name"] for c in CASES if c["item"] == 3} <= set(both), both
    for c in CASES:
        if c["item"] == 3:  # within one workgroup a term with one source and a term with several
            one = [[len(set(c["src"][w:w + WAVES, j].tolist())) == 1 for j in range(c["src"].shape[1])]
                   for w in (0, WAVES)]
            assert all(any(o) and not all(o) for o in one), c["name"]
            assert c["shift"].min() >= -40 and c["shift"].max() <= 3000
    assert {c["src"].shape[0] % WAVES for c in CASES} == {0, 1, 2, 3}
    assert {c["name"] for c in CASES if c["item"] == 2} == \
        {f"rows{r}-{kind}" for r in (1, 2, 3, 5, 6, 7) for kind in ("shared", "own")}
    for c in CASES:
        if c["item"] == 2:
            assert c["name"] == f"rows{c['src'].shape[0]}-{'shared' if len(c['src_len']) == 1 else 'own'}" or \
                c["name"] == "rows1-own"
    assert sorted(c["src"].shape for c in CASES if c["item"] == 3) == [(8, 2), (8, 5)]
    assert [c["src_len"] for c in CASES if c["item"] == 3] == [(N, 700, 0)] * 2
    assert {c["out_len"] for c in CASES if c["item"] == 5} == {1, 7, 8, 9, 511, 512, 513, 1024, 1031}
    assert {c["order"] for c in CASES if c["item"] == 6} == {1, 2, 6, 7, 8, 30, 31, 254, 255}
    assert {c["item"] for c in CASES} == set(range(1, 10))
    for c in CASES:
        assert c["src"].shape[0] <= 8 and c["out_len"] <= 6000 and c["n"] <= N, c["name"]
        assert np.all((c["frac"] < 0) | ((c["frac"] > 0) & (c["frac"] < 1)))
        for entry in ("host", "device"):
            x, ref, scale = problem(c["name"], entry)
            assert np.all(np.isfinite(ref)) and np.all(np.isfinite(scale)), c["name"]
            # the scale vanishes only where every weight of the row is zero: the row the exact-zero rule judges
            assert np.array_equal(scale > 0, c["weight"].any(axis=1)), (c["name"], scale)
            for col, n_valid in enumerate(c["src_len"]):
                assert np.all(np.isfinite(x[:n_valid, col])) and np.all(np.isnan(x[n_valid:, col]))
    # what the named rows are there for
    _, ref, _ = problem("shifts", "host")
    assert ref[:, 0].any() and ref[:, 1].any() and ref[:, 7].any()
    assert np.flatnonzero(ref[:, 2]).tolist() == [0]  # only the last filtered sample survives
    assert not ref[:, 3:7].any()
    _, ref, _ = problem("weights", "host")
    assert ref[:, 0].any() and not ref[:, 1].any()
    _, ref, _ = problem("peaks", "host")
    assert BY_NAME["peaks"]["out_len"] >= 3 * TT + 1
    assert (np.argmax(np.abs(ref[:, :3]), axis=0) // TT).tolist() == [0, 1, 2] and not ref[:, 3].any()


def test_oracle_reproduces_the_reference_das_time():
    """the oracle on the terms BeamformerDASTime builds for the reference's own scene gives the reference's output"""
    b = np.load(os.path.join(HERE, "golden", "beamformers", "das_time.npz"))
    x = b["array_signal"].astype(np.float64)
    n, n_mics = x.shape
    n_grid = b["d_grid"].shape[1]
    bf = BeamformerDASTime(dsp.Signal(None, x, int(b["fs"])), StoredPoints(b["d_grid"]), StoredGrid(n_grid))
    shift, frac, ds, total = bf._terms()
    src = np.broadcast_to(np.arange(n_mics, dtype=np.int32), (n_grid, n_mics))
    y, scale = oracle(x, (n,) * n_mics, src, shift, frac, ds.T / n_mics, 30, total)
    want = b["das_time"]
    assert y.shape == want.shape
    ratio = np.max(np.abs(y - want), axis=0) / scale
    print(f"oracle against das_time.npz: worst row error {ratio.max():.2e} of scale")
    assert np.all(ratio <= TOL_HOST)
    assert np.max(np.abs(y - want)) <= TOL_HOST * np.max(np.abs(want))


# ---- 2. the host entry -------------------------------------------------------------------------------------------
def run_host(c, x, **kw):
    return backend.delay_sum(x, np.array(c["src_len"]), c["src"], c["shift"], c["frac"], c["weight"], c["order"], DB,
                             c["out_len"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_host_entry_against_oracle(case):
    x, ref, scale = problem(case["name"], "host")
    y, pk = run_host(case, x, want_peaks=case["peaks"])
    assert y.dtype == np.float64
    worst = judge(case, y, ref, scale, TOL_HOST)
    print(f"{case['name']}: worst row error {worst:.3f} of the bound {TOL_HOST:.0e} * scale")
    if case["name"] == "through-alone":
        assert np.array_equal(y[:case["n"], 0], x[:, 0]) and not y[case["n"]:].any()
    if case["peaks"]:
        assert np.array_equal(pk, np.abs(y).max(axis=0)), (pk, np.abs(y).max(axis=0))
        only = run_host(case, x, want_samples=False, want_peaks=True)
        assert only[0] is None and np.array_equal(only[1], pk)
        assert pk[[not r.any() for r in ref.T]].tolist() == [0.0]  # one all-zero row in each of these cases


# ---- 3. the device entry -----------------------------------------------------------------------------------------
def run_device(c, x):
    """x as planar float32 with NaN in the ld padding too -> (out_len, rows) float32"""
    planar = np.full((x.shape[1], c["n"] + LD_PAD), np.nan, dtype=np.float32)
    planar[:, :c["n"]] = x.T
    ctx = backend.get_context()
    dev = DevicePlanar(DeviceBuffer.from_array(ctx, planar), x.shape[1], c["n"], planar.shape[1])
    out = backend.delay_sum_device(dev, np.array(c["src_len"]), c["src"], c["shift"], c["frac"], c["weight"],
                                   c["order"], DB, c["out_len"])
    assert (out.n_ch, out.n_samples) == (c["src"].shape[0], c["out_len"])
    return out.to_planar().T


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEVICE_CASES, ids=_id)
def test_device_entry_against_oracle(case):
    x, ref, scale = problem(case["name"], "device")
    y = run_device(case, x)
    assert y.dtype == np.float32
    worst = judge(case, y, ref, scale, TOL_DEV)
    print(f"{case['name']}: worst row error {worst:.3f} of the bound {TOL_DEV:.0e} * scale")
    if case["name"] == "through-alone":
        assert np.array_equal(y[:case["n"], 0], x[:, 0].astype(np.float32)) and not y[case["n"]:].any()


# ---- 4. repeatability, workspace reuse, the shift bound ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c["item"] == 3], ids=_id)
def test_repeatable(case):
    """the windows are not cleared between terms or calls: a sample left unfilled would differ from run to run"""
    for entry, run in (("host", lambda c, x: run_host(c, x)[0]), ("device", run_device)):
        x = problem(case["name"], entry)[0]
        assert np.array_equal(run(case, x), run(case, x)), entry


@pytest.mark.gpu
def test_workspace_reuse():
    """small, then the largest case (the io and ws buffers grow), then small again: bit for bit the same"""
    small = BY_NAME["tail-9"]
    large = max(CASES, key=lambda c: c["out_len"] * c["src"].shape[0] * c["src"].shape[1])
    assert large["item"] == 3
    for entry, run in (("host", lambda c, x: run_host(c, x)[0]), ("device", run_device)):
        first = run(small, problem(small["name"], entry)[0])
        run(large, problem(large["name"], entry)[0])
        assert np.array_equal(run(small, problem(small["name"], entry)[0]), first), entry


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [2**62, -2**62, np.iinfo(np.int64).min, 2**61, -2**61])
def test_shift_beyond_a_quarter_of_int64_is_refused(bad):
    """the host refuses it before anything is carved or launched; the largest shifts it takes are +-(2^61 - 1)"""
    c = BY_NAME["tail-9"]
    x = problem(c["name"], "host")[0]
    shift = c["shift"].copy()
    shift[-1, -1] = bad
    with pytest.raises(ValueError, match="shift"):
        backend.delay_sum(x, np.array(c["src_len"]), c["src"], shift, c["frac"], c["weight"], c["order"], DB, c["out_len"])
