"""Oracles and emulations for the realtime filters (csrc/kernels_rtfilt.hpp): the state-variable filter, the transposed
direct form II, the parallel second-order sections, the state-space filter and the direct FIR sum.

A filter is a dict: `kind` and its float64 coefficients, exactly the numbers the device is given --
    svf          g, r, h = 1 / (1 + r g + g^2)                tdf2         b (D + 1,), a (D + 1,), a[0] = 1
    parallel     sos (K, 5) rows b0 b1 b2 a1 a2, delay (int), fir (taps,) or None
    state_space  A (D, D), B (D,), C (D,), Dd
and a state is (D, streams) in the layout of the device (the reference's layouts; for the parallel filter sosfilt's
(z1, z2) per section).

The steps are restated from the formulas:
    svf          yh = (x - (r + g) s0 - s1) h;  yb = g yh + s0;  s0' = g yh + yb;  yl = g yb + s1;  s1' = g yb + yl;
                 outputs yl, yh, yb, yl - r yb + yh
    tdf2         y = b0 x + s0;  s_i' = b_{i+1} x - a_{i+1} y + s_{i+1};  s_{D-1}' = b_D x - a_D y
    parallel     per section y_k = b0 u + z1;  z1' = b1 u - a1 y_k + z2;  z2' = b2 u - a2 y_k, u[n] = x[n - delay];
                 y = base + y_0 + y_1 + ..., base[n] = sum_i fir_i x[n - i]
    state_space  y = C s + Dd x;  s' = A s + B x
`serial` runs them sample by sample in any dtype (np.longdouble: the oracle); `blocked_f64` is the kernels' blocked
algorithm in float64 numpy, as sfilt_oracle.blocked_f64.  `fir_direct` is the direct FIR sum in any dtype."""

import numpy as np

LD = np.longdouble
KINDS = ("svf", "tdf2", "parallel", "state_space")


def n_states(s):
    kind = s["kind"]
    if kind == "svf":
        return 2
    if kind == "tdf2":
        return len(s["b"]) - 1
    if kind == "parallel":
        return 2 * len(s["sos"])
    return len(s["B"])


def n_bands(s):
    return 4 if s["kind"] == "svf" else 1


def cast(s, dtype):
    keep = ("kind", "delay")
    return {key: (v if key in keep or v is None else np.asarray(v, dtype=np.float64).astype(dtype)) for key, v in s.items()}


def svf_structure(frequency_hz, resonance, sampling_rate_hz):
    g = float(np.tan(np.pi * frequency_hz / sampling_rate_hz))
    return dict(kind="svf", g=g, r=float(resonance), h=float(1 / (1 + resonance * g + g ** 2)))


def step(s, x, st, base=0.0):
    """One sample of every stream: x (m,), st (D, m) updated in place -> y (bands, m)."""
    kind = s["kind"]
    if kind == "svf":
        g, r, h = s["g"], s["r"], s["h"]
        s0, s1 = st[0].copy(), st[1].copy()
        yh = (x - (r + g) * s0 - s1) * h
        yb = g * yh + s0
        st[0] = g * yh + yb
        yl = g * yb + s1
        st[1] = g * yb + yl
        return np.stack([yl, yh, yb, yl - r * yb + yh])
    if kind == "tdf2":
        b, a = s["b"], s["a"]
        d = len(b) - 1
        y = b[0] * x + st[0]
        for i in range(d - 1):
            st[i] = x * b[i + 1] - y * a[i + 1] + st[i + 1]
        st[d - 1] = x * b[d] - y * a[d]
        return y[None]
    if kind == "parallel":
        acc = base + 0.0 * x
        for k, q in enumerate(s["sos"]):
            y = q[0] * x + st[2 * k]
            st[2 * k] = q[1] * x - q[3] * y + st[2 * k + 1]
            st[2 * k + 1] = q[2] * x - q[4] * y
            acc = acc + y
        return acc[None]
    assert kind == "state_space"
    old = st.copy()
    y = s["C"] @ old + s["Dd"] * x
    st[:] = s["A"] @ old + s["B"][:, None] * x
    return y[None]


def fir_direct(b, x, hist=None, dtype=LD):
    """y[n] = b[0] x[n] + sum_i b[i + 1] x[n - 1 - i] over x (N, C) in dtype, summed in that order.  hist (C, order):
    the samples before the first one, oldest first (None: zeros)."""
    b = np.asarray(b, dtype=np.float64).astype(dtype)
    x = np.asarray(x).astype(dtype)
    n, n_ch = x.shape
    order = len(b) - 1
    ext = np.zeros((order + n, n_ch), dtype=dtype)
    if hist is not None and order:
        ext[:order] = np.asarray(hist).astype(dtype).T
    ext[order:] = x
    y = np.zeros((n, n_ch), dtype=dtype)
    for i in range(order + 1):
        y = y + b[i] * ext[order - i:order - i + n]
    return y


def _inputs(s, x, dtype):
    """(the samples the recursion reads, the samples its output is added to) of x (N, C) in dtype."""
    x = np.asarray(x).astype(dtype)
    base = np.zeros_like(x)
    if s["kind"] == "parallel":
        if s.get("fir") is not None:
            base = fir_direct(s["fir"], x, None, dtype)
        delay = int(s.get("delay", 0))
        if delay:
            u = np.zeros_like(x)
            u[delay:] = x[:max(len(x) - delay, 0)]
            x = u
    return x, base


def serial(s, x, zi=None, dtype=LD):
    """The serial recursion over x (N, C) from zi (D, C) or zero -> y (N, C) (svf: (4, N, C)), zf (D, C), in dtype."""
    sc = cast(s, dtype)
    u, base = _inputs(s, x, dtype)
    n, n_ch = u.shape
    st = np.zeros((n_states(s), n_ch), dtype=dtype) if zi is None else np.asarray(zi).astype(dtype).copy()
    y = np.empty((n_bands(s), n, n_ch), dtype=dtype)
    for i in range(n):
        y[:, i] = step(sc, u[i], st, base[i])
    return (y if n_bands(s) > 1 else y[0]), st


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


def _blocks(s, w, wb, nv, state):
    """Every block (rows of w, (n_blocks, L); wb the samples the outputs are added to) from `state` (D, n_blocks); only
    the first nv[b] samples of block b move its state.  Returns the outputs (bands, n_blocks, L) and the final states."""
    st = state.copy()
    out = np.zeros((n_bands(s),) + w.shape)
    for i in range(w.shape[1]):
        live = i < nv
        trial = st.copy()
        yi = step(s, w[:, i], trial, wb[:, i])
        st = np.where(live, trial, st)
        out[:, :, i] = np.where(live, yi, 0.0)
    return out, st


def blocked_f64(s, x, zi=None, L=32, B=64, phi_power_offset=0, drop_state=None):
    """One filter over x (N, C) by the kernels' algorithm in float64 -> y (N, C) (svf: (4, N, C)), zf (D, C).
    phi_power_offset and drop_state break it on purpose (Phi one power off; one carried state value dropped): what the
    bound must reject."""
    s = cast(s, np.float64)
    d = n_states(s)
    u, base = _inputs(s, x, np.float64)
    n, n_ch = u.shape
    G = L * B
    n_groups = -(-n // G)
    phi, _ = carry_tables(s, L, B)
    if phi_power_offset:
        phi = phi @ np.linalg.matrix_power(transition(s), phi_power_offset)
    phig = _squarings(phi, int(np.log2(B)))
    y = np.zeros((n_bands(s), n, n_ch))
    zf = np.zeros((d, n_ch))
    for c in range(n_ch):
        xp, bp = np.zeros(n_groups * G), np.zeros(n_groups * G)
        xp[:n], bp[:n] = u[:, c], base[:, c]
        w, wb = xp.reshape(n_groups * B, L), bp.reshape(n_groups * B, L)
        nv = np.clip(n - np.arange(n_groups * B) * L, 0, L)
        _, sb = _blocks(s, w, wb, nv, np.zeros((d, n_groups * B)))
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
        out, fin = _blocks(s, w, wb, nv, entry.reshape(n_groups * B, d).T.copy())
        y[:, :, c] = out.reshape(n_bands(s), -1)[:, :n]
        zf[:, c] = fin[:, (n - 1) // L]
    return (y if n_bands(s) > 1 else y[0]), zf


def stream_error(out, ref):
    """Worst |out - ref| over the samples of a column, as a multiple of that column's largest |ref| -> max over columns
    (the sample axis is the last but one; leading axes are further streams)."""
    out, ref = np.asarray(out), np.asarray(ref)
    peak = np.max(np.abs(ref), axis=-2)
    err = np.max(np.abs(out.astype(LD) - ref), axis=-2)
    assert np.all(peak > 0)
    return float(np.max(err / peak))
