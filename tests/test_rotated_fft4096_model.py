"""Float64 model of welch4096::fft4096_wr, the rotated 16 x 16 x 16 register transform of the headline Welch loop
(kernels_welch4096w.hpp).  Host only: it checks the index and twiddle work the kernel does, with the kernel's own
conventions, against np.fft.fft.

Thread tid = 16 n2 + n3 holds v[n1] = z[tid + 256 n1].  Pass 1 is a DFT over n1, twiddled by W4096^(tid k1) and, in
the rotated form, by W16^(n2 n3).  Pass 2 (lane n3 of row k1) reads the column, and its DFT output m then holds
X2[(m + n3) mod 16]; the W256 twiddle comes from the rotated table tw2r[m 16 + n3] = W256^(n3 ((m + n3) mod 16)).  The
exchange is a DPP row_ror:m of register m, so lane L receives lane (L - m) mod 16's register m.  Pass 3 is the plain
DFT over the registers; its output m is bin k3 = -m mod 16 times the unit phase W16^(-k2 k3), which cancels in
conj(W) Z and |Z|^2, the only quantities the Welch loop keeps.
"""
import numpy as np

N = 4096


def W(n, e):
    return np.exp(-2j * np.pi * np.asarray(e, dtype=np.float64) / n)


def pos16(k):
    """register of DFT output k in dft16 / dft16_h"""
    return 4 * (k & 3) + (k >> 2)


def posr16(k3):
    """register of bin k3 after pass 3 of the rotated transform (kernels_welch4096w.hpp)"""
    return pos16((16 - k3) & 15)


def dft16_regs(x):
    """x[..., n] -> out[..., m] = sum_n x[n] W16^(n m) (natural output order; pos16 is a storage detail)"""
    n = np.arange(16)
    return x @ W(16, np.outer(n, n))


def tw2r_table():
    m, n3 = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    return W(256, n3 * ((m + n3) % 16)).reshape(256)  # [m 16 + n3]


def fft4096_wr(z):
    """z: (4096,) complex.  Returns out[tid, k3]: thread tid's value for bin k3 (as the kernel relabels it), and the
    raw register file regs[tid, pos] after pass 3."""
    tid = np.arange(256)
    n2, n3 = tid >> 4, tid & 15
    v = z.reshape(16, 256).T  # v[tid, n1] = z[tid + 256 n1]
    # pass 1, with the rotation W16^(n2 n3) folded into the per-thread twiddles
    X1 = dft16_regs(v)  # [tid, k1]
    k1 = np.arange(16)
    X1 = X1 * W(N, np.outer(tid, k1)) * W(16, n2 * n3)[:, None]
    img = X1.T  # pass-1 image: row k1, column tid
    # pass 2: lane (k1u, n3) reads row k1u at columns 16 n2 + n3
    regs = np.empty((256, 16), dtype=np.complex128)
    tw2r = tw2r_table()
    for t in range(256):
        k1u, l = t >> 4, t & 15
        x = img[k1u, 16 * np.arange(16) + l]
        y = dft16_regs(x)  # y[m] = X2[(m + l) mod 16]
        regs[t] = y * tw2r[np.arange(16) * 16 + l]
    # exchange: DPP row_ror:m on register m (rows of 16 lanes; lane L <- lane (L - m) mod 16)
    ex = np.empty_like(regs)
    for t in range(256):
        row, L = t & ~15, t & 15
        for m in range(16):
            ex[t, m] = regs[row | ((L - m) & 15), m]
    # pass 3: plain DFT over the registers
    out3 = dft16_regs(ex)  # out3[tid, m]
    stored = np.empty_like(out3)
    for m in range(16):
        stored[:, pos16(m)] = out3[:, m]
    by_bin = np.stack([stored[:, posr16(k3)] for k3 in range(16)], axis=1)
    return by_bin, stored


def bin_thread(tid):
    return ((tid & 15) << 4) | (tid >> 4)


def phase(k):
    k2, k3 = (k >> 4) & 15, k >> 8
    return W(16, -(k2 * k3))


def bins_of_threads():
    tid = np.arange(256)
    return bin_thread(tid)[:, None] + 256 * np.arange(16)[None, :]  # [tid, k3]


def test_rotated_transform_is_the_fft_up_to_the_per_bin_phase():
    rng = np.random.default_rng(7)
    z = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    by_bin, _ = fft4096_wr(z)
    k = bins_of_threads()
    ref = np.fft.fft(z)
    err = np.abs(by_bin - phase(k) * ref[k]).max() / np.abs(ref).max()
    assert err < 1e-13, err
    # every bin exactly once; the phase is 1 on bin 0 (the one detrend clears)
    assert sorted(k.ravel().tolist()) == list(range(N))
    assert phase(np.array([0]))[0] == 1.0


def test_the_phase_cancels_in_what_the_welch_loop_keeps():
    rng = np.random.default_rng(11)
    n_pairs = 3
    T = np.zeros((256, 16), dtype=np.complex128)
    P = np.zeros((256, 16))
    Tr = np.zeros(N, dtype=np.complex128)
    Pr = np.zeros(N)
    for _ in range(n_pairs):
        # two real frames ride one complex sequence, for the input (w) and the output (z) channel
        w = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        z = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        Wb, _ = fft4096_wr(w)
        Zb, _ = fft4096_wr(z)
        T += np.conj(Wb) * Zb
        P += np.abs(Zb) ** 2
        Wf, Zf = np.fft.fft(w), np.fft.fft(z)
        Tr += np.conj(Wf) * Zf
        Pr += np.abs(Zf) ** 2
    k = bins_of_threads()
    # the chunk-end fold k <-> N - k of k_y3, on the bin-ordered image
    t_img = np.empty(N, dtype=np.complex128)
    p_img = np.empty(N)
    t_img[k] = T
    p_img[k] = P
    nb = N // 2 + 1
    kk = np.arange(nb)
    fold_t = 0.5 * (t_img[kk] + np.conj(t_img[(N - kk) & (N - 1)]))
    fold_p = 0.5 * (p_img[kk] + p_img[(N - kk) & (N - 1)])
    ref_t = 0.5 * (Tr[kk] + np.conj(Tr[(N - kk) & (N - 1)]))
    ref_p = 0.5 * (Pr[kk] + Pr[(N - kk) & (N - 1)])
    assert np.abs(fold_t - ref_t).max() / np.abs(ref_t).max() < 1e-14
    assert np.abs(fold_p - ref_p).max() / np.abs(ref_p).max() < 1e-14


def test_static_output_relabelling():
    """A unit impulse of bin k (z = W4096^(-k n) / N) lands in thread t = bin_thread^-1(k mod 256), register
    posr16(k >> 8), and nowhere else."""
    rng = np.random.default_rng(3)
    n = np.arange(N)
    for k in rng.choice(N, size=24, replace=False):
        z = W(N, -k * n) / N
        _, stored = fft4096_wr(z)
        t, r = np.unravel_index(np.argmax(np.abs(stored)), stored.shape)
        assert bin_thread(t) == (k & 255) and r == posr16(k >> 8), (k, t, r)
        assert abs(abs(stored[t, r]) - 1.0) < 1e-12
        mask = np.ones_like(stored, dtype=bool)
        mask[t, r] = False
        assert np.abs(stored[mask]).max() < 1e-12
    # the relabelling is a permutation of the 16 registers, and bin k3 = 0 stays in register 0
    assert sorted(posr16(k3) for k3 in range(16)) == list(range(16)) and posr16(0) == 0


def test_rotated_twiddle_table():
    """tw2r as host_tables() appends it: row m of lane n3 is W256^(n3 ((m + n3) mod 16)); for n3 = 0 it is all 1
    (the unrotated table's k2 = 0 row is 1 for every lane instead)."""
    t = tw2r_table().reshape(16, 16)
    assert np.allclose(t[:, 0], 1.0)
    for m in range(16):
        for n3 in range(16):
            assert np.isclose(t[m, n3], np.exp(-2j * np.pi * n3 * ((m + n3) % 16) / 256))
