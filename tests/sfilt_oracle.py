"""Oracles and emulations for the structure filters (csrc/kernels_sfilt.hpp): FIR lattice, IIR lattice-ladder,
second-order-section lattice-ladder, warped FIR, warped IIR and Kautz.

A structure is a dict: `kind` and its float64 coefficients, exactly the numbers the device is given --
    fir_lattice  k (D,)                 iir_lattice  k (D,), c (D + 1,)        sos_lattice  k (K, 2), c (K, 3)
    warped_fir   lam, b (D,)            warped_iir   lam, b (D,) zero-padded, sigma (M + 1,)
    kautz        p (R,), g (R,), c (R,) for the real poles; q, r (P,), g2 (P, 2), c2 (P, 2) for the pole pairs
and a state is (D, streams) in the layout of the device (the reference's layouts for the lattice and warped classes;
for Kautz one direct-form-II value per real pole and two per pair).

The steps are restated from the formulas:
    FIR lattice     f_0 = g_0 = x;  f_i = f_{i-1} - k_i g_{i-1}[n-1];  g_i = g_{i-1}[n-1] - k_i f_{i-1};  y = f_D
    lattice-ladder  from the last stage down  f_{i} = f_{i+1} + k_i g_i[n-1];  g_{i+1} = g_i[n-1] - k_i f_i;
                    y = c_0 f_0 + sum c_{i+1} g_{i+1}
    warped FIR      s_0 = x;  s_{i+1}[n] = lam (s_{i+1}[n-1] - s_i[n]) + s_i[n-1];  y = sum b_i s_i
    warped IIR      x' = sigma_0 (x + sum_{i<M} sigma_{i+1} state_i), then the warped FIR chain on x'
    Kautz           real pole p: w = x + p w[n-1], tap g w, next x = w[n-1] - p w;  pair (q, r): w = x - q w[n-1] - r w[n-2],
                    taps g (w -+ w[n-1]), next x = r w + q w[n-1] + w[n-2];  y = sum c tap
`serial` runs them sample by sample in any dtype (np.longdouble: the oracle, eps 1.1e-19 on x86-64); `blocked_f64` is the
kernels' blocked algorithm in float64 numpy: blocks of L samples from zero state, the scan over the B blocks of a group
with Phi = A^L (A probed with the step itself on the unit vectors, then squared), the carry over the groups with Phi^B,
the rerun of every block from its entry state.  Its distance to the oracle is the size of error the algorithm itself
allows; the bound of a case is four times that (sfilt_cases.py)."""

import numpy as np

LD = np.longdouble
KINDS = ("fir_lattice", "iir_lattice", "sos_lattice", "warped_fir", "warped_iir", "kautz")


def n_states(s):
    kind = s["kind"]
    if kind in ("fir_lattice", "iir_lattice"):
        return len(s["k"])
    if kind == "sos_lattice":
        return 2 * len(s["k"])
    if kind in ("warped_fir", "warped_iir"):
        return len(s["b"])
    return len(s["p"]) + 2 * len(s["q"])


def cast(s, dtype):
    return {key: (v if key == "kind" else np.asarray(v, dtype=np.float64).astype(dtype)) for key, v in s.items()}


def warped_sigmas(a, lam):
    """Karjalainen et al. 1997: with S_N = a_N and S_{i-1} = a_{i-1} - lam S_i, sigma_i = lam S_{i-1} + S_i for
    1 < i < N, sigma_N = lam a_N, sigma_1 = S_1; stored negated behind sigma_0 = 1 / (1 - lam S_1).  a (N,), a[0] = 1,
    indices as in the paper shifted by one -> (N + 1,)."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    sig = np.zeros(n + 1)
    sig[n] = lam * a[n - 1]
    s = a[n - 1]
    for i in range(n - 1, 1, -1):
        s_new = a[i - 1] - lam * s
        sig[i] = lam * s_new + s
        s = s_new
    sig[1] = s
    sig[0] = 1.0 / (1.0 - lam * s)
    sig[1:] *= -1.0
    return sig


def kautz_structure(poles, c_real=None, c_complex=None):
    """The Kautz structure of poles (real ones, and one of each conjugate pair), unit weights unless given."""
    poles = np.asarray(poles, dtype=np.complex128)
    real = poles.imag == 0.0
    p = poles[real].real
    pc = poles[~real]
    q, r = -2.0 * pc.real, np.abs(pc) ** 2.0
    g2 = np.stack([((1.0 - r) * (1.0 + r - q) / 2.0) ** 0.5, ((1.0 - r) * (1.0 + r + q) / 2.0) ** 0.5], axis=1)
    c = np.ones(len(p)) if c_real is None else np.asarray(c_real, dtype=np.float64)
    c2 = np.ones((len(pc), 2)) if c_complex is None else np.asarray(c_complex, dtype=np.float64).reshape(len(pc), 2)
    return dict(kind="kautz", p=p, g=(1.0 - p ** 2.0) ** 0.5, c=c, q=q, r=r, g2=g2.reshape(len(pc), 2), c2=c2)


def kautz_taps(s, state):
    """The weighted-by-one taps at the sample the state was left after: g w for a real pole, g (w -+ w[n-1]) for a pair.
    state (D, streams) -> (D, streams), real poles first."""
    n_real = len(s["p"])
    out = [s["g"][i] * state[i] for i in range(n_real)]
    for j in range(len(s["q"])):
        w, w1 = state[n_real + 2 * j], state[n_real + 2 * j + 1]
        out += [s["g2"][j, 0] * (w - w1), s["g2"][j, 1] * (w + w1)]
    return np.array(out)


def step(s, x, st):
    """One sample of every stream: x (m,), st (D, m) updated in place -> y (m,)."""
    kind = s["kind"]
    if kind == "fir_lattice":
        k = s["k"]
        f, g = x, x
        for i in range(len(k)):
            old = st[i].copy()
            st[i] = g
            f, g = f - k[i] * old, old - k[i] * f
        return f
    if kind == "iir_lattice":
        k, c = s["k"], s["c"]
        d = len(k)
        f, low = x, 0.0
        for i in range(d - 1, -1, -1):
            old = st[i].copy()
            f = f + k[i] * old
            g = old - k[i] * f
            if i != d - 1:
                st[i + 1] = g
            low = low + c[i + 1] * g
        st[0] = f
        return c[0] * f + low
    if kind == "sos_lattice":
        for j, (k, c) in enumerate(zip(s["k"], s["c"])):
            s0, s1 = st[2 * j].copy(), st[2 * j + 1].copy()
            f = x + k[1] * s1
            low = c[2] * (s1 - k[1] * f)
            f = f + k[0] * s0
            g = s0 - k[0] * f
            st[2 * j + 1] = g
            st[2 * j] = f
            x = c[0] * f + (low + c[1] * g)
        return x
    if kind in ("warped_fir", "warped_iir"):
        lam, b = s["lam"], s["b"]
        d = len(b)
        if kind == "warped_iir":
            sig = s["sigma"]
            fb = 0.0
            for i in range(len(sig) - 1):
                fb = fb + sig[i + 1] * st[i]
            x = (x + fb) * sig[0]
        y, res = b[0] * x, x
        for i in range(d - 1):
            new = lam * (st[i + 1] - res) + st[i]
            st[i] = res
            res = new
            y = y + b[i + 1] * new
        st[d - 1] = res
        return y
    assert kind == "kautz"
    y = 0.0
    n_real = len(s["p"])
    for i, p in enumerate(s["p"]):
        w1 = st[i].copy()
        w = x + p * w1
        y = y + s["g"][i] * w * s["c"][i]
        x = w1 - p * w
        st[i] = w
    for j in range(len(s["q"])):
        q, r = s["q"][j], s["r"][j]
        w1, w2 = st[n_real + 2 * j].copy(), st[n_real + 2 * j + 1].copy()
        w = x - q * w1 - r * w2
        y = y + s["g2"][j, 0] * (w - w1) * s["c2"][j, 0]
        y = y + s["g2"][j, 1] * (w + w1) * s["c2"][j, 1]
        x = r * w + q * w1 + w2
        st[n_real + 2 * j + 1] = w1
        st[n_real + 2 * j] = w
    return y


def serial(s, x, zi=None, dtype=LD):
    """The serial recursion over x (N, C) from zi (D, C) or zero -> y (N, C), zf (D, C), in dtype."""
    sc = cast(s, dtype)
    x = np.asarray(x).astype(dtype)
    n, n_ch = x.shape
    st = np.zeros((n_states(s), n_ch), dtype=dtype) if zi is None else np.asarray(zi).astype(dtype).copy()
    y = np.empty((n, n_ch), dtype=dtype)
    for i in range(n):
        y[i] = step(sc, x[i], st)
    return y, st


def transition(s, dtype=np.float64):
    """The zero-input state transition A (D, D): column j is one step from the unit state e_j."""
    d = n_states(s)
    st = np.eye(d, dtype=dtype)  # stream j starts from e_j
    step(cast(s, dtype), np.zeros(d, dtype=dtype), st)
    return st


def _squarings(m, count):
    for _ in range(count):
        m = m @ m
    return m


def carry_tables(s, L=32, B=64):
    lg_l, lg_b = int(np.log2(L)), int(np.log2(B))
    assert 1 << lg_l == L and 1 << lg_b == B
    phi = _squarings(transition(s), lg_l)
    return phi, _squarings(phi, lg_b)


def carry_gain(s, L=32, B=64):
    """The largest magnitude in Phi = A^L and Phi^B: what the host entry holds against its limit."""
    with np.errstate(all="ignore"):
        phi, phig = carry_tables(s, L, B)
        g = max(np.max(np.abs(phi)), np.max(np.abs(phig)))
    return float(g) if np.isfinite(g) else float("inf")


def _blocks(s, w, nv, state):
    """Every block (rows of w, (n_blocks, L)) from `state` (D, n_blocks); only the first nv[b] samples of block b move
    its state.  Returns the outputs and the final states."""
    st = state.copy()
    out = np.zeros_like(w)
    for i in range(w.shape[1]):
        live = i < nv
        trial = st.copy()
        yi = step(s, w[:, i], trial)
        st = np.where(live, trial, st)
        out[:, i] = np.where(live, yi, 0.0)
    return out, st


def blocked_f64(s, x, zi=None, L=32, B=64, phi_power_offset=0, drop_state=None):
    """One structure over x (N, C) by the kernels' algorithm in float64 -> y (N, C), zf (D, C).  phi_power_offset and
    drop_state break it on purpose (Phi one power off; one carried state value dropped): what the bound must reject."""
    s = cast(s, np.float64)
    d = n_states(s)
    n, n_ch = x.shape
    G = L * B
    n_groups = -(-n // G)
    phi, _ = carry_tables(s, L, B)
    if phi_power_offset:
        phi = phi @ np.linalg.matrix_power(transition(s), phi_power_offset)
    phig = _squarings(phi, int(np.log2(B)))
    y = np.zeros((n, n_ch))
    zf = np.zeros((d, n_ch))
    for c in range(n_ch):
        xp = np.zeros(n_groups * G)
        xp[:n] = x[:, c]
        w = xp.reshape(n_groups * B, L)
        nv = np.clip(n - np.arange(n_groups * B) * L, 0, L)
        _, sb = _blocks(s, w, nv, np.zeros((d, n_groups * B)))
        sb = sb.T.reshape(n_groups, B, d)
        t = np.zeros((n_groups, d))
        for g in range(n_groups - 1):
            st = np.zeros(d)
            for b in range(B):
                st = phi @ st + sb[g, b]
            t[g] = st
        T = np.zeros((n_groups, d))
        st = np.zeros(d) if zi is None else np.asarray(zi, dtype=np.float64)[:, c].copy()
        for g in range(n_groups):
            T[g] = st
            st = phig @ st + t[g]
        entry = np.zeros((n_groups, B, d))
        for g in range(n_groups):
            st = T[g]
            for b in range(B):
                entry[g, b] = st
                st = phi @ st + sb[g, b]
        if drop_state is not None:
            entry[:, 1:, drop_state] = 0.0
        out, fin = _blocks(s, w, nv, entry.reshape(n_groups * B, d).T.copy())
        y[:, c] = out.reshape(-1)[:n]
        zf[:, c] = fin[:, (n - 1) // L]
    return y, zf


def stream_error(out, ref):
    """Worst |out - ref| over the samples of a column, as a multiple of that column's largest |ref| -> max over columns
    (axis 0 is the sample axis)."""
    out, ref = np.asarray(out), np.asarray(ref)
    peak = np.max(np.abs(ref), axis=0)
    err = np.max(np.abs(out.astype(LD) - ref), axis=0)
    assert np.all(peak > 0)
    return float(np.max(err / peak))
