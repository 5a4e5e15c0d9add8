"""The device beamformers (csrc/kernels_beamform.hpp) against a float64 numpy oracle, beyond the fixture's one geometry.

tests/test_beamformers.py checks the reference's own maps at 16 microphones, 36 grid points and 1 or 7 bins.  Here a
plain numpy restatement of the four methods is first checked against those same reference maps without a
GPU, and then judges the kernels where they split their work: more than one workgroup along the grid (G > 256), the
16-column and 16-row chunks for C that is not a multiple of 16, up to 64 microphones, 40 bins, unnormalised steering
vectors, indefinite CSMs, the argmax tie rule, the eigensolver's edges and the device-pointer entries.

Every random case is checked to be well posed before it is run (clear argmaxes, separated eigenvalues, a bounded
condition number, a stopping rule away from equality); a seed that is not is replaced in CASES, never skipped."""

import ctypes as C

import numpy as np
import pytest
from scipy.integrate import simpson

from dsptoolbox_amd import backend
from conftest import load_golden

TIE = 1e-6  # smallest relative gap between the best and the second-best grid point of any argmax


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.nanmax(np.abs(a - b)) / np.nanmax(np.abs(b)))


def gap(v):
    """relative distance between the largest and the second-largest entry of v (inf for a single entry)"""
    if v.size < 2:
        return np.inf
    top = np.sort(v)[-2:]
    return (top[1] - top[0]) / max(abs(top[1]), 1e-300)


# ---- the oracle: csm (F, C, C), h (F, C, G) -> (G, F), float64 ---------------------------------------------------
def _proj(csm_b, h_b):
    """eigh of one bin (ascending, the lower triangle) and P[g, k] = |v_k^H h_g|^2"""
    w, v = np.linalg.eigh(csm_b)
    return w, np.abs(h_b.conj().T @ v) ** 2


def _proj_all(csm, h):
    """_proj for every bin at once: w (F, C), P (F, G, C)"""
    w, v = np.linalg.eigh(csm)
    return w, np.abs(np.einsum("fig,fik->fgk", h.conj(), v)) ** 2


def mvdr(csm, h):
    w, P = _proj_all(csm, h)
    return (1.0 / np.sum(P / w[:, None, :], axis=2)).T


def functional(csm, h, gamma):
    """(h^H A h / |h|^2)^gamma |h|^2 with A = sum_k sign(lambda_k)|lambda_k|^(1/gamma) v_k v_k^H (the reference's SVD
    form); a negative base with a non-integer gamma gives NaN, as numpy's ** does"""
    w, P = _proj_all(csm, h)
    q = np.einsum("fgk,fk->fg", P, np.sign(w) * np.abs(w) ** (1.0 / gamma))
    hn = np.sum(np.abs(h) ** 2, axis=1)
    with np.errstate(invalid="ignore"):
        return ((q / hn) ** gamma * hn).T


def orthogonal(csm, h, n_eig):
    """for the n_eig largest signed eigenvalues, largest first: map[argmax P_e] = P_e[argmax] lambda_e, assigned"""
    m = np.zeros((h.shape[2], csm.shape[0]))
    for b in range(csm.shape[0]):
        w, P = _proj(csm[b], h[b])
        for e in range(n_eig):
            k = len(w) - 1 - e
            i = np.argmax(P[:, k])
            m[i, b] = P[i, k] * w[k]
    return m


def cleansc(csm, h, max_iter, safety, remove_diag, trace=None):
    """CLEAN-SC per bin with the dirty map updated in rank-1 form:
    r -= s p (|h_^H h_g|^2 - [remove_diag] sum_i |h_gi|^2 |h__i|^2).  `trace` (a list) collects, per bin, every
    argmax's residual map and every stopping comparison, for the well-posedness checks."""
    m = np.zeros((h.shape[2], csm.shape[0]))
    for b in range(csm.shape[0]):
        D = csm[b].copy()
        if remove_diag:
            np.fill_diagonal(D, 0)
        hb = h[b]
        r = np.real(np.sum(hb.conj() * (D @ hb), axis=0))
        n_prev, n_cur = 2 * np.linalg.norm(D, 1), np.linalg.norm(D, 1)
        t = dict(maps=[], norms=[], stop="max_iter")
        for _ in range(max_iter):
            t["maps"].append(r.copy())
            i = np.argmax(r)
            p = r[i]
            m[i, b] += p * safety
            t["norms"].append((n_cur, n_prev))
            if n_cur >= n_prev:
                t["stop"] = "norm"
                break
            w = hb[:, i]
            h_, w2, Dw = w.copy(), np.abs(w) ** 2, D @ w / p
            for _ in range(20):
                H = np.abs(h_) ** 2
                h_ = (Dw + H * w) / np.sqrt(1 + H @ w2)
            upd = np.abs(h_.conj() @ hb) ** 2
            if remove_diag:
                upd -= (np.abs(h_) ** 2) @ (np.abs(hb) ** 2)
            r = r - safety * p * upd
            G = np.outer(h_, h_.conj()) * p
            if remove_diag:
                np.fill_diagonal(G, 0)
            D = D - safety * G
            n_prev, n_cur = n_cur, np.linalg.norm(D, 1)
        if trace is not None:
            trace.append(t)
    return m


def oracle_map(method, csm, h, prm, trace=None):
    if method == "mvdr":
        return mvdr(csm, h)
    if method == "functional":
        return functional(csm, h, prm["gamma"])
    if method == "orthogonal":
        return orthogonal(csm, h, prm["n_eig"])
    return cleansc(csm, h, prm["max_iter"], prm["safety"], prm["remove_diag"], trace)


def device_map(method, csm, h, prm):
    if method == "cleansc":
        return backend.beamformer_cleansc_map(csm, h, prm["max_iter"], prm["safety"], prm["remove_diag"])
    return backend.beamformer_eig_map(csm, h, method, gamma=prm.get("gamma", 10.0), n_eig=prm.get("n_eig", 0))


# ---- 1. the oracle against the reference's maps (no GPU) ---------------------------------------------------------
def test_oracle_matches_reference_fixture():
    meta, z = load_golden("beamformers/cases")
    n_mic = meta["n_mics"]
    for i, c in enumerate(meta["cases"]):
        f, h, csm = z[f"f_{c['band']}"], z[f"h_{c['band']}"], z[f"csm_{c['scaling']}_{c['band']}"]
        kw = c["kwargs"]
        prm = dict(gamma=kw.get("gamma", 10), n_eig=kw.get("number_eigenvalues", n_mic // 2),
                   max_iter=kw.get("maximum_iterations", 2 * n_mic), safety=kw.get("safety_factor", 0.5),
                   remove_diag=kw.get("remove_csm_diagonal", False))
        m = oracle_map(c["method"], csm, h, prm)
        m = simpson(m, dx=f[1] - f[0], axis=1) if len(f) > 1 else m.squeeze()
        ref = z[f"map_{i}"].ravel()
        assert relmax(m, ref) <= 1e-9, (i, c, relmax(m, ref))
        if c["method"] in ("orthogonal", "cleansc"):
            assert np.array_equal(np.flatnonzero(m), np.flatnonzero(ref)), (i, c)


# ---- random, seeded problems -------------------------------------------------------------------------------------
def make_problem(C, G, F, kind, seed):
    """steering vectors complex Gaussian, not normalised; CSMs either PSD and full rank (2C + 3 frames) or
    indefinite (Hermitian with mixed-sign eigenvalues)"""
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal((F, C, G)) + 1j * rng.standard_normal((F, C, G))) * np.sqrt(0.5)
    x = rng.standard_normal((F, C, 2 * C + 3)) + 1j * rng.standard_normal((F, C, 2 * C + 3))
    if kind == "psd":
        csm = x @ np.conj(np.swapaxes(x, 1, 2)) / x.shape[2]
    else:
        y = x[:, :, :C]
        csm = y + np.conj(np.swapaxes(y, 1, 2))
        if C == 2:  # a 2 x 2 random Hermitian may have both signs the same: make it certain
            csm = csm - np.trace(csm, axis1=1, axis2=2).real[:, None, None] / 2 * np.eye(2)
    return csm, h


CS = [2, 3, 15, 16, 17, 31, 32, 33, 47, 63, 64]
GS = [1, 255, 256, 257, 600, 4099]
FS = [1, 3, 40]
MAX_ELEMS = 2_500_000  # F * C * G: the steering vectors stay below 40 MB


def _cases():
    """(method, C, G, F, kind, params, seed): for every method each C and each G appears (Latin-square pairing)"""
    out = []
    for mi, method in enumerate(("mvdr", "functional", "orthogonal", "cleansc")):
        for i, C in enumerate(CS):
            G = GS[(i + mi) % len(GS)]
            F = FS[(i + 2 * mi) % len(FS)]
            while F * C * G > MAX_ELEMS or (method == "cleansc" and F > 3 and C * G > 20_000):
                F = FS[FS.index(F) - 1]
            kind = "psd" if (i + mi) % 2 == 0 else "indefinite"
            if method == "mvdr":
                prm = {}
            elif method == "functional":
                prm = dict(gamma=(1.0, 2.5, 10.0)[i % 3])
            elif method == "orthogonal":
                prm = dict(n_eig=min((1, 15, 16, 17, C)[i % 5], C))
            else:
                prm = dict(max_iter=(1, 2 * C, 300)[i % 3], safety=(0.05, 0.5, 1.0)[(i // 3 + i) % 3],
                           remove_diag=i % 4 in (1, 2))
            out.append((method, C, G, F, kind, prm, SEEDS.get((method, i), 1000 * mi + i)))
    return out


# seeds that replace the default 1000 * method + i where that case was not well posed
SEEDS = {("mvdr", 5): 500005, ("mvdr", 9): 100009, ("functional", 4): 101004, ("functional", 10): 701010,
         ("orthogonal", 1): 102001}


def well_posed(method, csm, h, prm, trace):
    """assert that the case has one answer to well below the tolerance; returns the tolerance the arithmetic gives"""
    F = csm.shape[0]
    if method == "cleansc":
        for t in trace:
            for r in t["maps"]:
                assert gap(r) > TIE, ("cleansc near-tie", gap(r))
            for n_cur, n_prev in t["norms"]:
                assert abs(n_cur - n_prev) > 1e-9 * n_prev, "cleansc stopping rule near equality"
        return 1e-10
    tol = 0.0 if method == "mvdr" else 1e-10
    for b in range(F):
        w, P = _proj(csm[b], h[b])
        na = np.max(np.abs(w))
        if method == "mvdr":
            kappa = na / np.min(np.abs(w))
            terms = P / w
            cancel = np.max(np.sum(np.abs(terms), axis=1) / np.abs(np.sum(terms, axis=1)))
            assert kappa * cancel <= 1e6, ("mvdr condition", kappa, cancel)
            tol = max(tol, 1e-12 * kappa * cancel)
        elif method == "functional":
            c = np.sign(w) * np.abs(w) ** (1.0 / prm["gamma"])
            q = P @ c
            cancel = np.max(np.abs(P) @ np.abs(c) / np.abs(q))
            if prm["gamma"] != int(prm["gamma"]):  # the sign of q decides NaN or not
                assert cancel <= 1e4, ("functional base near 0", cancel)
        else:
            n_eig = prm["n_eig"]
            lead = w[::-1][:min(n_eig + 1, len(w))]
            if len(lead) > 1:
                assert np.min(-np.diff(lead)) > 1e-4 * na, ("orthogonal eigenvalues not separated", np.diff(lead))
            for e in range(n_eig):
                assert gap(P[:, len(w) - 1 - e]) > TIE, ("orthogonal near-tie", b, e)
    return tol


CASES = _cases()


def _id(c):
    return f"{c[0]}-C{c[1]}-G{c[2]}-F{c[3]}-{c[4]}"


def test_sweep_cases_are_well_posed_and_cover_the_grid():
    """(no GPU) every sweep case passes its well-posedness checks, every C and every G meets every method, and
    CLEAN-SC both stops on its norm rule and runs out of iterations somewhere"""
    stops = set()
    for method, C, G, F, kind, prm, seed in CASES:
        csm, h = make_problem(C, G, F, kind, seed)
        if kind == "indefinite":
            w = np.linalg.eigvalsh(csm)
            assert np.all((w < 0).any(axis=1) & (w > 0).any(axis=1))
        trace = []
        oracle_map(method, csm, h, prm, trace)
        well_posed(method, csm, h, prm, trace)
        stops |= {t["stop"] for t in trace}
    assert stops == {"norm", "max_iter"}
    for method in ("mvdr", "functional", "orthogonal", "cleansc"):
        cs = {c[1] for c in CASES if c[0] == method}
        gs = {c[2] for c in CASES if c[0] == method}
        fs = {c[3] for c in CASES if c[0] == method}
        assert cs == set(CS) and gs == set(GS), method
        assert fs == set(FS), (method, fs)


# ---- 2. the device against the oracle over shapes and parameters -------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_sweep_against_oracle(case):
    method, C, G, F, kind, prm, seed = case
    csm, h = make_problem(C, G, F, kind, seed)
    trace = []
    ref = oracle_map(method, csm, h, prm, trace)
    tol = well_posed(method, csm, h, prm, trace)
    assert tol <= 1e-6
    m = device_map(method, csm, h, prm)
    assert m.shape == (G, F) and m.dtype == np.float64
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(m), nan), (np.flatnonzero(np.isnan(m))[:8], np.flatnonzero(nan)[:8])
    if method == "functional" and kind == "indefinite" and prm["gamma"] != int(prm["gamma"]):
        assert nan.any() and not nan.all()  # the NaN rule is exercised, not vacuous
    else:
        assert not nan.any()
    e = relmax(m[~nan], ref[~nan])
    print(f"{_id(case)} {prm}: relative max error {e:.2e} (tolerance {tol:.1e})")
    assert e <= tol, (e, tol)
    if method in ("orthogonal", "cleansc"):  # the sources land on the same grid points, bin by bin
        assert np.array_equal(m != 0, ref != 0)


# ---- 3. tie rule, determinism, bin isolation, workspace reuse ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dup", [70, 200, 300, 517])
def test_argmax_tie_takes_the_lowest_index(dup):
    """grid points 5 and `dup` have the same steering vector, the clear maximum of the map: their values come out
    of the same arithmetic, so the tie is exact, and the lower index must win.  dup = 70 and 200 sit in other
    waves, 300 in another thread's second stride (and another k_bf_project workgroup), 517 in thread 5's own third
    stride."""
    C, G = 17, 600
    csm, h = make_problem(C, G, 1, "psd", 77)
    w, v = np.linalg.eigh(csm[0])
    h[0, :, 5] = 8.0 * v[:, -1]  # along the leading eigenvector: the largest P and the largest dirty-map value
    h[0, :, dup] = h[0, :, 5]
    P = np.abs(h[0].conj().T @ v[:, -1]) ** 2
    r = np.real(np.sum(h[0].conj() * (csm[0] @ h[0]), axis=0))
    for x in (P, r):  # a clear maximum over every other point
        assert np.sort(x)[-3] < 0.5 * x[5] and x[5] == np.max(x)
    m = backend.beamformer_eig_map(csm, h, "orthogonal", n_eig=3)
    assert m[5, 0] > 0 and m[dup, 0] == 0.0
    for it in (1, 2 * C):
        m = backend.beamformer_cleansc_map(csm, h, it, 0.5, False)
        assert m[5, 0] > 0 and m[dup, 0] == 0.0, it


def _mid_problem(F=40, G=700, C=33, seed=5):
    return make_problem(C, G, F, "psd", seed)


METHOD_PRM = [("mvdr", {}), ("functional", dict(gamma=2.5)), ("orthogonal", dict(n_eig=5)),
              ("cleansc", dict(max_iter=40, safety=0.5, remove_diag=True))]


@pytest.mark.gpu
@pytest.mark.parametrize("method,prm", METHOD_PRM, ids=[m for m, _ in METHOD_PRM])
def test_deterministic_and_bins_isolated(method, prm):
    """two identical calls agree bitwise, and bin b of a 40-bin call equals bitwise the same bin run alone"""
    csm, h = _mid_problem()
    a = device_map(method, csm, h, prm)
    assert np.array_equal(a, device_map(method, csm, h, prm), equal_nan=True)
    for b in (0, 1, 17, 39):
        one = device_map(method, csm[b:b + 1], h[b:b + 1], prm)
        assert np.array_equal(one[:, 0], a[:, b], equal_nan=True), b


@pytest.mark.gpu
@pytest.mark.parametrize("method,prm", METHOD_PRM, ids=[m for m, _ in METHOD_PRM])
def test_workspace_reuse(method, prm):
    """small, then large (the io and ws buffers grow), then small again: the last result equals the first bitwise"""
    small = make_problem(5, 37, 2, "indefinite", 11)
    large = make_problem(64, 4099, 9, "psd", 12)
    first = device_map(method, *small, prm)
    device_map(method, *large, prm)
    assert np.array_equal(device_map(method, *small, prm), first, equal_nan=True)


# ---- 4. eigensolver edges ----------------------------------------------------------------------------------------
def _check_eigh(a, w, v):
    """the bounds of test_beamformers.py::test_hermitian_eigh_indefinite; they hold for degenerate spectra too"""
    n = a.shape[0]
    na = np.linalg.norm(a, 2)
    assert np.all(np.diff(w) >= 0)
    assert np.max(np.abs(w - np.linalg.eigvalsh(a))) <= 1e-12 * na
    assert np.linalg.norm(a @ v - v * w) <= 1e-12 * na
    assert np.linalg.norm(v.conj().T @ v - np.eye(n)) <= 1e-12


def _herm(rng, n):
    x = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return x + x.conj().T


def _unitary(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q


def _edge_matrices():
    rng = np.random.default_rng(2024)
    out = {"C1": np.array([[-2.5 + 0j]]), "C2": _herm(rng, 2), "zero": np.zeros((7, 7), complex)}
    u = rng.standard_normal(20) + 1j * rng.standard_normal(20)
    out["identity_plus_rank1"] = np.eye(20) + np.outer(u, u.conj())
    q = _unitary(rng, 24)
    out["repeated"] = (q * np.repeat([-1.0, 0.5, 2.0, 3.0], 6)) @ q.conj().T
    x = rng.standard_normal((64, 10)) + 1j * rng.standard_normal((64, 10))
    out["rank10_C64"] = x @ x.conj().T / 10
    r = rng.standard_normal((30, 30))
    out["real"] = (r + r.T).astype(complex)
    s = rng.standard_normal((30, 30))
    out["imaginary"] = np.diag(rng.standard_normal(30)) + 1j * (s - s.T)
    q = _unitary(rng, 64)
    out["cluster_C64"] = (q * (1.0 + np.arange(64) * 1e-10)) @ q.conj().T
    return out


EDGES = _edge_matrices()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGES))
def test_hermitian_eigh_edges(name):
    a = EDGES[name]
    w, v = backend.hermitian_eigh(a[None])
    _check_eigh(a, w[0], v[0])
    if name == "zero":
        assert np.all(w == 0.0)


@pytest.mark.gpu
def test_hermitian_eigh_diagonal_is_exact():
    """a diagonal matrix needs no rotation: the eigenvalues are the sorted diagonal exactly, V a permutation"""
    d = np.array([3.0, -1.0, 0.25, 7.5, -1.0, 0.0, 2.0])
    w, v = backend.hermitian_eigh(np.diag(d).astype(complex)[None])
    assert np.array_equal(w[0], np.sort(d))
    order = np.argsort(d, kind="stable")
    assert np.array_equal(v[0], np.eye(7)[:, order].astype(complex))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2.0 ** 500, 2.0 ** -500, 1e160, 1e-160], ids=["2^500", "2^-500", "1e160", "1e-160"])
def test_hermitian_eigh_scale(scale):
    """eigenvalues scale with the matrix (exactly for a power of two), eigenvectors do not change"""
    rng = np.random.default_rng(31)
    a = _herm(rng, 33)
    w1, v1 = backend.hermitian_eigh(a[None])
    ws, vs = backend.hermitian_eigh((a * scale)[None])
    na = np.linalg.norm(a, 2)
    assert np.all(np.isfinite(ws))
    assert np.max(np.abs(ws[0] / scale - np.linalg.eigvalsh(a))) <= 1e-12 * na
    assert np.linalg.norm(a @ vs[0] - vs[0] * (ws[0] / scale)) <= 1e-12 * na  # (a unscaled: no overflow here)
    assert np.linalg.norm(vs[0].conj().T @ vs[0] - np.eye(33)) <= 1e-12
    if np.log2(scale) == int(np.log2(scale)):
        assert np.array_equal(ws, w1 * scale) and np.array_equal(vs, v1)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e160, 1e-160])
def test_eig_maps_at_extreme_scale(scale):
    """the maps go through the eigensolver unscaled: MVDR scales with the CSM, Orthogonal with it too"""
    csm, h = make_problem(16, 300, 2, "psd", 41)
    for method, prm in (("mvdr", {}), ("orthogonal", dict(n_eig=4))):
        trace = []
        ref = oracle_map(method, csm, h, prm, trace)
        tol = well_posed(method, csm, h, prm, trace)
        m = device_map(method, csm * scale, h, prm) / scale
        assert relmax(m, ref) <= max(tol, 1e-10), method
        if method == "orthogonal":
            assert np.array_equal(m != 0, ref != 0)


# ---- 5. device-pointer entries and limits ------------------------------------------------------------------------
@pytest.mark.gpu
def test_dev_entries_match_host_entries():
    csm, h = make_problem(24, 333, 5, "indefinite", 9)
    F, n, G = h.shape
    ctx = backend.get_context()
    lib = ctx.lib
    bufs = []

    def dev(arr):
        bufs.append(ctx.to_device(arr))
        return bufs[-1]

    def out(nbytes):
        bufs.append(ctx.malloc(nbytes))
        return bufs[-1]

    try:
        d_csm, d_h = dev(csm), dev(h)
        d_w, d_v, d_m = out(F * n * 8), out(F * n * n * 16), out(G * F * 8)
        w_ref, v_ref = backend.hermitian_eigh(csm)
        ctx.check(lib.ds_bf_eigh_dev(ctx.handle, C.c_void_p(d_csm), F, n, C.c_void_p(d_w), C.c_void_p(d_v)),
                  "ds_bf_eigh_dev")
        w, v = np.empty_like(w_ref), np.empty_like(v_ref)
        ctx.download(d_w, w)
        ctx.download(d_v, v)
        assert np.array_equal(w, w_ref) and np.array_equal(v, v_ref)
        for method, gamma, n_eig in (("mvdr", 10.0, 0), ("functional", 3.0, 0), ("orthogonal", 10.0, 7)):
            ref = backend.beamformer_eig_map(csm, h, method, gamma=gamma, n_eig=n_eig)
            ctx.check(lib.ds_bf_eig_map_dev(ctx.handle, C.c_void_p(d_csm), C.c_void_p(d_h), F, n, G,
                                            backend.BF_METHODS[method], gamma, n_eig, C.c_void_p(d_m)),
                      "ds_bf_eig_map_dev")
            m = np.empty((G, F))
            ctx.download(d_m, m)
            assert np.array_equal(m, ref, equal_nan=True), method
        ref = backend.beamformer_cleansc_map(csm, h, 48, 0.5, True)
        ctx.check(lib.ds_bf_cleansc_dev(ctx.handle, C.c_void_p(d_csm), C.c_void_p(d_h), F, n, G, 48, 0.5, 1,
                                        C.c_void_p(d_m)), "ds_bf_cleansc_dev")
        m = np.empty((G, F))
        ctx.download(d_m, m)
        assert np.array_equal(m, ref)
    finally:
        for d in bufs:
            ctx.free(d)


@pytest.mark.gpu
def test_65535_bins_and_no_more():
    rng = np.random.default_rng(65535)
    F = 65535
    x = rng.standard_normal((F, 2, 5)) + 1j * rng.standard_normal((F, 2, 5))
    csm = x @ np.conj(np.swapaxes(x, 1, 2)) / 5
    h = rng.standard_normal((F, 2, 1)) + 1j * rng.standard_normal((F, 2, 1))
    assert np.max(np.linalg.cond(csm)) < 1e6
    m = backend.beamformer_eig_map(csm, h, "mvdr")
    assert m.shape == (1, F)
    kappa = np.max(np.linalg.cond(csm))
    assert relmax(m, mvdr(csm, h)) <= 1e-12 * kappa
    m = backend.beamformer_cleansc_map(csm, h, 1, 0.5, False)  # one grid point: the first pick is the whole map
    assert relmax(m[0], 0.5 * np.real(np.einsum("fi,fij,fj->f", h[:, :, 0].conj(), csm, h[:, :, 0]))) <= 1e-12
    big_csm = np.concatenate([csm, csm[:1]])
    big_h = np.concatenate([h, h[:1]])
    for call in (lambda: backend.beamformer_eig_map(big_csm, big_h, "mvdr"),
                 lambda: backend.beamformer_cleansc_map(big_csm, big_h, 1, 0.5, False),
                 lambda: backend.hermitian_eigh(big_csm)):
        with pytest.raises(NotImplementedError, match="65535 bins"):
            call()


@pytest.mark.gpu
def test_invalid_arguments_raise_value_error():
    csm, h = make_problem(6, 10, 1, "psd", 3)
    for n_eig in (0, 7):
        with pytest.raises(ValueError, match="n_eig"):
            backend.beamformer_eig_map(csm, h, "orthogonal", n_eig=n_eig)
    with pytest.raises(ValueError, match="max_iter"):
        backend.beamformer_cleansc_map(csm, h, 0, 0.5, False)
