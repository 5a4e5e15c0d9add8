"""Oracles and emulations for the complex-coefficient recursion (csrc/kernels_ciir.hpp) and the distance kernels
(csrc/kernels_dist.hpp).

The oracle is the serial definition in numpy.clongdouble / longdouble (eps 1.1e-19 on x86-64): sosfilt's transposed
direct form II section by section, sample by sample; the segmental SNR frame by frame as
_fw_snr_seg_per_channel (distances/_distances.py:104-195 of the reference) states it, with scipy.fft keeping the long
double; the pair sums term by term.

The emulation is the kernels' BLOCKED algorithm in float64 numpy: blocks of L samples from zero state, the scan over
the B blocks of a group with Phi = A^L, the carry over the groups with Phi^(L B), the rerun of every block from its
entry state.  It rounds where the kernels round up to the order inside one complex product (numpy does not fuse), so
its distance to the oracle is the size of error the algorithm itself allows; the bound of a case is four times that
(ciir_cases.py)."""

import numpy as np
import scipy.fft

CLD = np.clongdouble
LD = np.longdouble


def normalised(sos, dtype):
    """(K, 6) sections -> (K, 5) b0 b1 b2 a1 a2 divided by a0."""
    s = np.asarray(sos).astype(dtype)
    return np.concatenate([s[:, :3], s[:, 4:]], axis=1) / s[:, 3:4]


def bank_ld(sos, x, zi=None):
    """The serial cascades of F filters in clongdouble, all filters and channels side by side.  sos (F, K, 6); x (N, C)
    real; zi (F, K, 2, C) or None -> y (F, N, C), zf (F, K, 2, C)."""
    s = np.asarray(sos).astype(CLD)
    cf = np.concatenate([s[..., :3], s[..., 4:]], axis=-1) / s[..., 3:4]  # (F, K, 5)
    n, n_ch = np.shape(x)
    y = np.broadcast_to(np.asarray(x).astype(CLD), (len(cf), n, n_ch)).copy()
    zf = np.zeros((len(cf), cf.shape[1], 2, n_ch), dtype=CLD)
    for k in range(cf.shape[1]):
        b0, b1, b2, a1, a2 = (cf[:, k, i][:, None] for i in range(5))
        z1 = np.zeros((len(cf), n_ch), dtype=CLD) if zi is None else np.asarray(zi)[:, k, 0].astype(CLD)
        z2 = np.zeros((len(cf), n_ch), dtype=CLD) if zi is None else np.asarray(zi)[:, k, 1].astype(CLD)
        for i in range(n):
            xi = y[:, i].copy()
            yi = b0 * xi + z1
            z1 = b1 * xi - a1 * yi + z2
            z2 = b2 * xi - a2 * yi
            y[:, i] = yi
        zf[:, k, 0], zf[:, k, 1] = z1, z2
    return y, zf


def sosfilt_ld(sos, x, zi=None):
    """One filter: sos (K, 6), zi (K, 2, C) or None -> y (N, C), zf (K, 2, C)."""
    y, zf = bank_ld(np.asarray(sos)[None], x, None if zi is None else np.asarray(zi)[None])
    return y[0], zf[0]


# ---- the blocked algorithm in float64 ------------------------------------------------------------------------------
def transition(cf):
    """The zero-input state transition A (D, D) of the cascade, as the host builds it: column j is one step from e_j."""
    k_sec = len(cf)
    d = 2 * k_sec
    a = np.zeros((d, d), dtype=cf.dtype)
    for j in range(d):
        inp = 0.0
        for k, (b0, b1, b2, a1, a2) in enumerate(cf):
            z1, z2 = float(j == 2 * k), float(j == 2 * k + 1)
            y = b0 * inp + z1
            a[2 * k, j] = b1 * inp - a1 * y + z2
            a[2 * k + 1, j] = b2 * inp - a2 * y
            inp = y
    return a


def _squarings(m, count):
    for _ in range(count):
        m = m @ m
    return m


def _blocks(cf, w, nv, state):
    """Every block (rows of w, (n_blocks, L)) through the cascade from `state` (n_blocks, D); only the first nv[b]
    samples of block b move its state.  Returns the outputs and the final states."""
    w = w.astype(np.complex128)
    out_state = state.copy()
    for k, (b0, b1, b2, a1, a2) in enumerate(cf):
        z1, z2 = out_state[:, 2 * k].copy(), out_state[:, 2 * k + 1].copy()
        for i in range(w.shape[1]):
            live = i < nv
            xi = w[:, i]
            yi = b0 * xi + z1
            n1 = b1 * xi - a1 * yi + z2
            n2 = b2 * xi - a2 * yi
            z1, z2 = np.where(live, n1, z1), np.where(live, n2, z2)
            w[:, i] = np.where(live, yi, xi)
        out_state[:, 2 * k], out_state[:, 2 * k + 1] = z1, z2
    return w, out_state


def blocked_f64(sos, x, zi=None, L=32, B=64, phi_power_offset=0, drop_imag_state=False):
    """One filter over x (N, C) by the kernels' algorithm in float64 / complex128 -> y (N, C), zf (K, 2, C).
    phi_power_offset and drop_imag_state break it on purpose (Phi one power off; the carried state's imaginary part
    dropped): what the bound must reject."""
    cf = normalised(sos, np.complex128)
    d = 2 * len(cf)
    n, n_ch = x.shape
    G = L * B
    n_groups = -(-n // G)
    a = transition(cf)
    lg_l, lg_b = int(np.log2(L)), int(np.log2(B))
    assert 1 << lg_l == L and 1 << lg_b == B
    phi = _squarings(a, lg_l)
    if phi_power_offset:
        phi = phi @ np.linalg.matrix_power(a, phi_power_offset)
    phig = _squarings(phi, lg_b)
    y = np.zeros((n, n_ch), dtype=np.complex128)
    zf = np.zeros((len(cf), 2, n_ch), dtype=np.complex128)
    for c in range(n_ch):
        xp = np.zeros(n_groups * G)
        xp[:n] = x[:, c]
        w = xp.reshape(n_groups * B, L)
        nv = np.clip(n - np.arange(n_groups * B) * L, 0, L)
        _, s = _blocks(cf, w, nv, np.zeros((n_groups * B, d), dtype=np.complex128))
        s = s.reshape(n_groups, B, d)
        # group pass: the zero-entry state of every group but the last
        t = np.zeros((n_groups, d), dtype=np.complex128)
        for g in range(n_groups - 1):
            st = np.zeros(d, dtype=np.complex128)
            for b in range(B):
                st = phi @ st + s[g, b]
            t[g] = st
        # carry pass
        T = np.zeros((n_groups, d), dtype=np.complex128)
        st = np.zeros(d, dtype=np.complex128) if zi is None else np.asarray(zi)[:, :, c].reshape(d).astype(np.complex128)
        for g in range(n_groups):
            T[g] = st
            st = phig @ st + t[g]
        # apply pass: the entry state of every block, then the rerun
        entry = np.zeros((n_groups, B, d), dtype=np.complex128)
        for g in range(n_groups):
            st = T[g]
            for b in range(B):
                entry[g, b] = st
                st = phi @ st + s[g, b]
        if drop_imag_state:
            entry = entry.real.astype(np.complex128)
        out, fin = _blocks(cf, w, nv, entry.reshape(n_groups * B, d))
        y[:, c] = out.reshape(-1)[:n]
        zf[:, :, c] = fin[(n - 1) // L].reshape(len(cf), 2)
    return y, zf


def stream_error(out, ref):
    """Worst |out - ref| over the samples of a column, as a multiple of that column's largest |ref| -> max over columns
    (axis 0 is the sample axis)."""
    out, ref = np.asarray(out), np.asarray(ref)
    peak = np.max(np.abs(ref), axis=0)
    err = np.max(np.abs(out.astype(CLD) - ref), axis=0)
    assert np.all(peak > 0)
    return float(np.max(err / peak))


# ---- pair sums ------------------------------------------------------------------------------------------------------------
def snr_ld(s, n):
    """20 log10(std(s) / std(n)) per channel in long double; a one-channel n is everyone's noise."""
    s, n = np.asarray(s).astype(LD), np.asarray(n).astype(LD)
    sd = lambda v: np.sqrt(np.mean((v - np.mean(v, axis=0)) ** 2, axis=0))
    return 20 * np.log10(sd(s) / sd(n)) * np.ones(s.shape[1], dtype=LD)


def si_sdr_ld(s, shat):
    s, shat = np.asarray(s).astype(LD), np.asarray(shat).astype(LD)
    out = np.empty(shat.shape[1], dtype=LD)
    for c in range(shat.shape[1]):
        a = s[:, 0 if s.shape[1] == 1 else c]
        alpha = (a @ shat[:, c]) / (a @ a)
        out[c] = 10 * np.log10(np.sum((alpha * a) ** 2) / np.sum((alpha * a - shat[:, c]) ** 2))
    return out


def pair_sums_f64(a, b, par, nt=256, per_lane=16):
    """The kernels' summation order in float64 for ONE channel pair: lanes stride NT inside a span, a halving tree over
    the lanes, the spans' partial sums lane-strided and the same tree -> the six sums."""
    al, ma, mb = par

    def tree(v):
        v = v.copy()
        s = nt // 2
        while s:
            v[:s] += v[s:2 * s]
            s //= 2
        return v[0]

    span = nt * per_lane
    parts = []
    for n0 in range(0, len(a), span):
        v = np.zeros((6, nt))
        for i in range(per_lane):
            xs, ys = a[n0 + i * nt:n0 + (i + 1) * nt][:nt], b[n0 + i * nt:n0 + (i + 1) * nt][:nt]
            if len(xs) == 0:
                break
            m = len(xs)
            r = al * xs - ys
            v[0, :m] += (xs - ma) ** 2
            v[1, :m] += (ys - mb) ** 2
            v[2, :m] += xs * ys
            v[3, :m] += xs
            v[4, :m] += ys
            v[5, :m] += r * r
        parts.append([tree(v[k]) for k in range(6)])
    parts = np.array(parts)
    acc = np.zeros((6, nt))
    for w in range(len(parts)):
        acc[:, w % nt] += parts[w]
    return np.array([tree(acc[k]) for k in range(6)])


# ---- the segmental measure ----------------------------------------------------------------------------------------------
def fw_frames_ld(xb, xhb, window, snr_range_db, gamma, perturb=0.0, seed=0, dtype=LD):
    """One channel: xb, xhb (N, bands) band signals -> (unclipped frame values, the clipped mean), in `dtype`.
    Frames of len(window) at half overlap, zeros past the end, ceil(N / hop) of them.  With perturb > 0 every combined
    frame spectrum Z = FFT((x + i xhat) w) is moved by perturb max|Z| in a random direction per bin, and X, Xhat are
    taken from its conjugate-even and -odd parts as the device does."""
    cdt = CLD if dtype is LD else np.complex128
    lw = len(window)
    hop = lw // 2
    n = len(xb)
    n_frames = -(-n // hop)
    pad = n_frames * hop + lw
    xb = np.concatenate([np.asarray(xb).astype(dtype), np.zeros((pad - n, xb.shape[1]), dtype=dtype)])
    xhb = np.concatenate([np.asarray(xhb).astype(dtype), np.zeros((pad - n, xhb.shape[1]), dtype=dtype)])
    w = np.asarray(window).astype(dtype)[:, None]
    rng = np.random.default_rng(seed)
    eps = dtype(1e-30)
    vals = np.empty(n_frames, dtype=dtype)
    for m in range(n_frames):
        fx, fh = xb[m * hop:m * hop + lw] * w, xhb[m * hop:m * hop + lw] * w
        if perturb:
            z = scipy.fft.fft((fx + 1j * fh).astype(cdt), axis=0)
            z = z + perturb * np.max(np.abs(z), axis=0) * np.exp(2j * np.pi * rng.random(z.shape))
            zr = np.conj(np.roll(z[::-1], 1, axis=0))  # conj Z[N - k]
            X = np.abs((z + zr) / 2)[:lw // 2 + 1]
            Xh = np.abs((z - zr) / 2)[:lw // 2 + 1]
        else:
            X = np.abs(scipy.fft.rfft(fx, axis=0))
            Xh = np.abs(scipy.fft.rfft(fh, axis=0))
        W = X ** dtype(gamma)
        X = X / np.sum(X, axis=0)
        Xh = Xh / np.sum(Xh, axis=0)
        snr = np.sum(np.log10(X ** 2 / (X - Xh + eps) ** 2) * W, axis=1)
        vals[m] = np.mean(10 * snr / np.sum(W, axis=1))
    return vals, np.mean(np.clip(vals, dtype(snr_range_db[0]), dtype(snr_range_db[1])))
