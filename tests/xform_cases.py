"""The float32 whole-signal transforms (ds_rfft / ds_rfft_dev, ds_deconv / ds_deconv_dev) beyond one workgroup's LDS:
the four-step transform at every power of two it is built for and Bluestein's chirp-z on every M it can run on -- the
cases, a restatement of the host plan, a float32 restatement of the device algorithm and the recorded bounds.
test_xform_sweep_host.py checks all of this on the CPU, test_xform_sweep_gpu.py holds the kernels to it.

The code under test: csrc/kernels_bigfft.hpp, csrc/kernels_bluestein.hpp and, in csrc/api.hip, big_cols, big_rows,
big_rows_ct, blue_len, blue_dft, xform_blue_run, xform_big_run, xform_check.

Problems are built like route_cases.rfft_problem / deconv_problem (seeded; `ident` names a problem and is what its
oracle is cached under), but the signals are ZERO-MEAN: 0.5 x standard normal, rounded to float32, no offset.  On an
offset of 0.25 the DC bin of a 2^24-point spectrum is 2000 times the rms of the bins and its float32 rounding alone
sets the bound (route_oracles: emulation 29.5 at rfft 2^20); without it the rms of the bins is the size of every bin.
No float64-layout entry runs here, so `x` / `y` of a problem are the float32 rows themselves.  The oracles are
route_oracles.rfft and route_oracles.deconv in float64, the judge is route_oracles.judge with its rule unchanged:
|out - oracle| <= tol x rms of the oracle over the transform axis of that row, every element.

FOUR   N = 2^15 ... 2^24, all ten: N = 1024 x n2, and k_big_rows<n2> is one kernel per n2 = 32 ... 16384, each with its
       own rows per workgroup (four_plan restates big_rows_ct and ch_stride).  At 2^23 and 2^24 one row per workgroup
       on 70 KB and 140 KB of dynamic LDS.  Signal lengths n in {N, N/2 + 1}; channels {1, 3} up to 2^21 (the odd count
       leaves a last pair without a second channel), {2} above.  Deconvolution: r_per_channel in {0, 1}, n_out in
       {N, N/2 + 3} (the two share one oracle), one item of 3 channels and, at N <= 2^17, two; above 2^21 one item of
       2 channels with r_per_channel = 1.
BLUE   length L -> the M it must run on.  5; 1001 (odd composite); 1009 (prime); 100003 (prime, M = 2^18); 1572864 =
       3 x 2^19 (even: the Nyquist branch of k_mul_r; M = 2^22); the fullest length of every M, L = M/2 - 1 (2L - 1 =
       M - 3) for M = 2^15 ... 2^24, the last being the largest length the library takes; the emptiest, L = M/4 + 1,
       for M = 2^16, 2^17, 2^18 and 2^24.  Channels {1, 3} for L < 2^20, {2} above; n in {L, (L + 1) // 2}.
       Deconvolution at 1001, 1009, 16383, 16385, 1572864 and 8388607 with n_out in {L, L // 2 + 3}.
REFUSED  n_fft = 2^23 + 1 and 3 x 2^22 (not powers of two, 2L - 1 > 2^24) and 2^25: DS_ERR_UNSUP, xform_check's words,
       no launch, nothing written.

The bound.  EMULATION[(family, length)] is the worst error of a float32 emulation as a multiple of 1e-6 x scale over
the problems of that length, measured on the CPU against the float64 oracle (tools/measure_xform_emulation.py prints the
table; the host test measures every entry again).  tolerance() is route_oracles' rule: 1e-6 where EMULATION x
HOST_MARGIN <= 0.25, else 4 x EMULATION x HOST_MARGIN x 1e-6.  For powers of two the emulation is
route_oracles.compute(p, numpy.float32): scipy's transform in single precision.  For Bluestein lengths it is the larger
of that and Restatement(numpy.float32): the chirp exp(-i pi (n^2 mod 2L) / L) with n^2 mod 2L in int64, the phase in
float64, rounded to complex64; three complex64 transforms of M = max(2^15, next power of two >= 2L - 1) points; the
products with the chirp and the pair unpack / multiply in float32 -- a mixed-radix float32 FFT of L points alone
understates what three transforms of M points cost.  The library's output sets no bound.

Restatement also states the four-step split itself (four=True: N = 1024 x n2, the twiddle W_N^(j2 k1) from (j2 k1) mod N
in float64 rounded to complex64), and, in float64, four ways of being subtly wrong (WRONG): the host test shows that
the bound rejects each at least ten times over."""

import zlib
from collections import OrderedDict

import numpy as np
import scipy.fft as sfft

import route_oracles as ros

# ---- the host plan restated (csrc/api.hip, csrc/fft_lds.hpp, csrc/kernels_bigfft.hpp) ---------------------------------
MAX_FFT = 16384            # kMaxFft: the longest transform of one workgroup's LDS
MAX_BIG = 1 << 24          # kMaxBigFft
N1 = 1024                  # the columns transform of every four-step length
BLUE_MIN = 1 << 15         # blue_len's smallest M
LDS_LIMIT = 160 << 10      # LDS of a gfx950 workgroup
LDS_BUDGET = 70 << 10      # big_rows_ct: rows are packed into a workgroup up to this many bytes
DS_ERR_UNSUP = -2


def threads_for(n):
    return max(64, min(512, n // 16))


def lds_len(n):
    return n + n // 16 + 2


def ch_stride(n):
    return (lds_len(n) + 30) // 32 * 32 + 1


def big_rows_ct(n2):
    ct = min(16, 1024 // threads_for(n2), max(1, LDS_BUDGET // (ch_stride(n2) * 8)))
    while ct & (ct - 1):
        ct &= ct - 1
    return ct


def four_plan(N):
    """the two launches of one N-point four-step transform"""
    n2 = N // N1
    ct1, ct2 = min(8, n2), big_rows_ct(n2)
    return dict(n2=n2, cols_ct=ct1, cols_lds=ct1 * ch_stride(N1) * 8, cols_threads=ct1 * threads_for(N1),
                rows_ct=ct2, rows_lds=ct2 * ch_stride(n2) * 8, rows_threads=ct2 * threads_for(n2))


def blue_len(L):
    m = BLUE_MIN
    while m < 2 * L - 1:
        m <<= 1
    return m


def refusal(n_fft):
    """what xform_check says of a length it does not take (after the entry's name and " n_fft: "), or None"""
    pow2 = n_fft & (n_fft - 1) == 0
    if not pow2 and 2 * n_fft - 1 > MAX_BIG:
        return "non-power-of-two lengths above 2^23 are not built yet"
    if pow2 and n_fft > MAX_BIG:
        return "lengths above 2^24 are not built yet"
    return None


# ---- the cases ---------------------------------------------------------------------------------------------------------
FOUR = tuple(1 << k for k in range(15, 25))
BLUE = OrderedDict(
    [(5, 1 << 15), (1001, 1 << 15), (1009, 1 << 15), (100003, 1 << 18), (3 << 19, 1 << 22)]
    + [((1 << k) // 2 - 1, 1 << k) for k in range(15, 25)]
    + [((1 << k) // 4 + 1, 1 << k) for k in (16, 17, 18, 24)])
BLUE_DECONV = (1001, 1009, 16383, 16385, 3 << 19, (1 << 23) - 1)
REFUSED = ((1 << 23) + 1, 3 << 22, 1 << 25)
ENTRIES = {"rfft": ("rfft", "rfft_dev"), "deconv": ("deconv", "deconv_dev")}
WIDE = 1 << 21   # four-step lengths above this run two channels, one item
LONG = 1 << 20   # Bluestein lengths from this on run two channels, one item

# worst error of the float32 emulation / (1e-6 * scale) per (family, length), as measured on the CPU
EMULATION = {
    ('rfft', 32768): 0.597, ('rfft', 65536): 0.555, ('rfft', 131072): 0.64, ('rfft', 262144): 0.669,
    ('rfft', 524288): 0.722, ('rfft', 1048576): 0.743, ('rfft', 2097152): 0.731, ('rfft', 4194304): 0.785,
    ('rfft', 8388608): 0.875, ('rfft', 16777216): 0.888, ('rfft', 5): 0.193, ('rfft', 1001): 0.547,
    ('rfft', 1009): 0.704, ('rfft', 100003): 1.21, ('rfft', 1572864): 1.33, ('rfft', 16383): 0.924,
    ('rfft', 32767): 1.02, ('rfft', 65535): 1.01, ('rfft', 131071): 1.14, ('rfft', 262143): 1.29,
    ('rfft', 524287): 1.39, ('rfft', 1048575): 1.39, ('rfft', 2097151): 1.41, ('rfft', 4194303): 1.51,
    ('rfft', 8388607): 1.61, ('rfft', 16385): 0.845, ('rfft', 32769): 1.22, ('rfft', 65537): 1.33,
    ('rfft', 4194305): 1.53,
    ('deconv', 32768): 1.05, ('deconv', 65536): 1.09, ('deconv', 131072): 1.13, ('deconv', 262144): 1.21,
    ('deconv', 524288): 1.53, ('deconv', 1048576): 1.27, ('deconv', 2097152): 1.43, ('deconv', 4194304): 1.42,
    ('deconv', 8388608): 1.54, ('deconv', 16777216): 1.56, ('deconv', 1001): 1.28, ('deconv', 1009): 1.36,
    ('deconv', 16383): 2.31, ('deconv', 16385): 1.85, ('deconv', 1572864): 2.39, ('deconv', 8388607): 3.29,
}


def tolerance(tk):
    """route_oracles.tolerance's rule on this file's table"""
    e = EMULATION[tk] * ros.HOST_MARGIN
    return ros.BASE_TOL if e <= 0.25 else 4.0 * e * ros.BASE_TOL


def _rows(rows, n, *seed):
    rng = np.random.default_rng(zlib.crc32(repr(seed).encode()))
    return np.ascontiguousarray(0.5 * rng.standard_normal((rows, n)), dtype=np.float32)


def rfft_problem(n_fft, n, n_ch):
    """One whole-signal spectrum of n samples (zero padded to n_fft) of n_ch channels; xp is (channels, samples)."""
    xp = _rows(n_ch, n, "rfft", n_fft, n, n_ch)
    return dict(family="rfft", ident=("xform", "rfft", n_fft, n, n_ch), x=xp, xp=xp, n=n, n_fft=n_fft, n_ch=n_ch,
                B=n_fft // 2 + 1, scale=np.float32(1.0 / n_fft))


def deconv_problem(n_fft, n, r_per_channel, n_items, n_ch):
    """One batch of deconvolutions with ALL n_fft output samples (a call keeps the first n_out: calls()); yp is
    (items x channels, samples), r as route_cases.deconv_problem draws it."""
    yp = _rows(n_items * n_ch, n, "deconv", n_fft, n, r_per_channel, n_items, n_ch)
    B, n_r = n_fft // 2 + 1, (n_ch if r_per_channel else 1)
    rng = np.random.default_rng(n_fft)
    r = np.empty((n_r, B), np.complex64)
    for k in range(n_r):  # (row by row: the same draws as one (n_r, B) call, without its float64 copy of 2^24 bins)
        r[k].real = rng.standard_normal(B)
    for k in range(n_r):
        r[k].imag = rng.standard_normal(B)
    return dict(family="deconv", ident=("xform", "deconv", n_fft, n, r_per_channel, n_items, n_ch), y=yp, yp=yp, r=r, n=n,
                n_fft=n_fft, n_ch=n_ch, n_items=n_items, r_per_channel=r_per_channel, B=B, n_out=n_fft)


def short(n_fft):
    """the ragged signal length of a transform length"""
    return n_fft // 2 + 1 if n_fft & (n_fft - 1) == 0 else (n_fft + 1) // 2


def channels(n_fft):
    pow2 = n_fft & (n_fft - 1) == 0
    return (1, 3) if (n_fft <= WIDE if pow2 else n_fft < LONG) else (2,)


def rfft_specs(n_fft):
    """the builder arguments of the spectra of one length"""
    return [(n_fft, n, n_ch) for n in (n_fft, short(n_fft)) for n_ch in channels(n_fft)]


def deconv_specs(n_fft):
    """[(builder arguments, the n_out of its calls)] of one length"""
    outs = (n_fft, n_fft // 2 + 3)
    if len(channels(n_fft)) == 1:
        return [((n_fft, n, 1, 1, 2), outs) for n in (n_fft, short(n_fft))]
    return [((n_fft, n, rpc, n_items, 3), outs) for n in (n_fft, short(n_fft)) for rpc in (0, 1)
            for n_items in ((1, 2) if n_fft <= 1 << 17 else (1,))]


_problems: OrderedDict = OrderedDict()


def problem(family, spec):
    """the problem of (family, builder arguments); the last few are kept (the host tests walk a length several times)"""
    key = (family,) + tuple(spec)
    p = _problems.get(key)
    if p is None:
        p = _problems[key] = (rfft_problem if family == "rfft" else deconv_problem)(*spec)
        while len(_problems) > 4:
            _problems.popitem(last=False)
    return p


def calls(family, n_fft):
    """[(key, entry, problem with the call's n_out)] of one length, the calls of one problem in a row"""
    if family == "rfft":
        return [(f"{e}|{n_fft}|{s[1]}|{s[2]}", e, ("rfft", s), None) for s in rfft_specs(n_fft) for e in ENTRIES["rfft"]]
    return [(f"{e}|{n_fft}|{s[1]}|{s[2]}|{s[3]}|{s[4]}|{n_out}", e, ("deconv", s), n_out)
            for s, outs in deconv_specs(n_fft) for n_out in outs for e in ENTRIES["deconv"]]


# ---- the oracle and the judge -----------------------------------------------------------------------------------------
def oracle(p):
    """route_oracles.rfft / deconv in float64 (a deconvolution with all n_fft samples), once per problem"""
    assert p["family"] == "rfft" or p["n_out"] == p["n_fft"]
    with sfft.set_workers(ros._threads()):
        return ros.oracle(p)


def target(p, ref, n_out=None):
    """(oracle in the layout of the float32 entries, scale, dtype of the output) of a call that keeps n_out samples"""
    if p["family"] == "rfft":
        return ref, ros._rms(ref, 0), np.complex64
    ref = ref[..., :n_out]
    return ref, ros._rms(ref, 2), np.float32


def judge_call(key, p, out, n_out=None, tol=None):
    """what one call returned against the problem's oracle -> the worst error as a fraction of the bound"""
    tol = tolerance((p["family"], p["n_fft"])) if tol is None else tol
    ref, scale, dtype = target(p, oracle(p), n_out)
    return ros.judge(key, out, ref, scale, tol, dtype)


def fraction(p, out, n_outs=(None,)):
    """the worst error of `out` (a deconvolution: all n_fft samples) / (1e-6 * scale), over the calls' n_out"""
    worst = 0.0
    for n_out in n_outs:
        ref, scale, _ = target(p, oracle(p), n_out)
        o = out if n_out is None else out[..., :n_out]
        s = np.broadcast_to(scale, ref.shape)
        assert np.all(s > 0), p["ident"]
        worst = max(worst, float(np.max(np.abs(o - ref) / (ros.BASE_TOL * s))))
    return worst


# ---- the device algorithm restated ------------------------------------------------------------------------------------
WRONG = {
    "wrap": "a circular convolution of M / 2 points: the chirp filter's two halves overlap and the products wrap around"
            " (a blue_len that stops one doubling early)",
    "pair_sign": "the second channel of a pair unpacked with the wrong sign of its imaginary part (k_big_unpack's B)",
    "edge_imag": "a deconvolution that keeps the imaginary part of the DC / Nyquist product, which leaks into the other"
                 " channel of the pair (k_big_mul / k_mul_r without their km == k branch)",
    "twiddle": "an off-by-one in the inter-stage twiddle of the four-step transform, W_N^((j2 + 1) k1) (k_big_cols)",
}


def chirp(L, cdt):
    """w[n] = exp(-i pi (n^2 mod 2L) / L): dsblue::chirp"""
    n = np.arange(L, dtype=np.int64)
    return np.exp(-1j * np.pi * (((n * n) % (2 * L)).astype(np.float64) / float(L))).astype(cdt)


class Restatement:
    """What xform_big_run / xform_blue_run do to a problem, in precision dt.  The power-of-two transforms are scipy's
    (four=False) or the four-step split (four=True).  `wrong` names the one thing it gets wrong (WRONG), None nothing."""

    def __init__(self, dt=np.float32, four=False, wrong=None):
        assert wrong is None or wrong in WRONG, wrong
        self.dt, self.cdt, self.wrong = dt, ros._cdt(dt), wrong
        self.four = four or wrong == "twiddle"

    def four_step(self, z):
        """k_big_cols, k_big_rows: z (batch, N) -> (batch, N)"""
        b, N = z.shape
        n2 = N // N1
        t = sfft.fft(z.reshape(b, N1, n2), axis=1)                                           # [k1][j2]
        j2 = np.arange(n2, dtype=np.int64)[None, :] + (1 if self.wrong == "twiddle" else 0)
        m = (np.arange(N1, dtype=np.int64)[:, None] * j2) % N
        t *= np.exp(-2j * np.pi * (m.astype(np.float64) / float(N))).astype(self.cdt)       # W_N^(j2 k1)
        t = sfft.fft(t, axis=2)                                                              # [k1][k2]
        return np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(b, N)                      # bin k1 + N1 k2

    def pow2(self, z):
        assert z.dtype == self.cdt
        return self.four_step(z) if self.four else sfft.fft(z, axis=1)

    def chirpz(self, z, L):
        """blue_filter, blue_dft: z (batch, L) -> its L-point DFT"""
        M = blue_len(L) // (2 if self.wrong == "wrap" else 1)
        w = chirp(L, self.cdt)
        bf = np.zeros((1, M), self.cdt)
        bf[0, :L] = w.conj()
        bf[0, M - np.arange(1, L)] = w[1:].conj()
        bf = self.pow2(bf)
        a = np.zeros((len(z), M), self.cdt)
        a[:, :L] = z * w                                                                     # k_pre
        q = (self.pow2(a) * bf).conj()                                                       # k_mul_filter
        c = self.pow2(q)
        return (c[:, :L].conj() * self.dt(1.0 / M)) * w                                      # k_post

    def dft(self, z):
        L = z.shape[1]
        return self.pow2(z) if L & (L - 1) == 0 else self.chirpz(z, L)

    def pairs(self, xp, n_items, n_ch, L):
        """the channel pairs xa + i xb of every item, zero padded to L: (items x pairs, L)"""
        npair = (n_ch + 1) // 2
        z = np.zeros((n_items, npair, L), self.cdt)
        x = xp.reshape(n_items, n_ch, -1)
        z.real[:, :, :x.shape[2]] = x[:, 0::2]
        z.imag[:, :n_ch // 2, :x.shape[2]] = x[:, 1::2]
        return z.reshape(n_items * npair, L)

    def unpack(self, Z):
        """the spectra A, B of the two real channels of each pair, bins 0 ... L/2"""
        L = Z.shape[1]
        k = np.arange(L // 2 + 1)
        P, Qc = Z[:, k], Z[:, (L - k) % L].conj()
        half = self.dt(0.5)
        A, B = (P + Qc) * half, (P - Qc) * self.cdt(-0.5j)
        return A, (B.conj() if self.wrong == "pair_sign" else B)

    def rfft(self, p):
        """-> (n_fft/2 + 1, C)"""
        L, C = p["n_fft"], p["n_ch"]
        A, B = self.unpack(self.dft(self.pairs(p["xp"], 1, C, L)))
        out = np.empty((L // 2 + 1, C), self.cdt)
        out[:, 0::2] = A.T
        out[:, 1::2] = B.T[:, :C // 2]
        return out * self.dt(p["scale"])

    def deconv(self, p):
        """-> (items, C, n_fft)"""
        L, C, items = p["n_fft"], p["n_ch"], p["n_items"]
        npair, nb = (C + 1) // 2, L // 2 + 1
        A, B = self.unpack(self.dft(self.pairs(p["yp"], items, C, L)))
        r = np.asarray(p["r"], self.cdt)
        ca = 2 * np.arange(npair)
        cb = np.minimum(ca + 1, C - 1)
        Ra, Rb = (r[ca], r[cb]) if p["r_per_channel"] else (r[[0] * npair], r[[0] * npair])
        VA = (A.reshape(items, npair, nb) * Ra[None]).reshape(-1, nb)
        VB = (B.reshape(items, npair, nb) * Rb[None]).reshape(-1, nb)
        V = np.empty((len(VA), L), self.cdt)
        V[:, :nb] = VA + 1j * VB
        k = np.arange(1, (L - 1) // 2 + 1)
        V[:, L - k] = VA[:, k].conj() + 1j * VB[:, k].conj()
        if self.wrong != "edge_imag":
            for e in ((0,) if L % 2 else (0, L // 2)):
                V[:, e] = VA[:, e].real + 1j * VB[:, e].real
        F = self.dft(V.conj()).reshape(items, npair, L) * self.dt(1.0 / L)                   # k_big_store / k_store
        out = np.empty((items, C, L), self.dt)
        out[:, 0::2] = F.real
        out[:, 1::2] = -F.imag[:, :C // 2]
        return out

    def run(self, p):
        return self.rfft(p) if p["family"] == "rfft" else self.deconv(p)


def emulations(p):
    """{name: the float32 emulation's output} of one problem: scipy in single precision and, for a Bluestein length, the
    float32 chirp-z"""
    with sfft.set_workers(ros._threads()):
        emus = {"plain": ros.compute(p, np.float32)}
        if p["n_fft"] & (p["n_fft"] - 1):
            emus["chirp-z"] = Restatement(np.float32).run(p)
    return emus


def emulation_fractions(family, n_fft):
    """{name: worst error / (1e-6 * scale) over the problems and calls of one length}"""
    worst = {}
    specs = [(s, (None,)) for s in rfft_specs(n_fft)] if family == "rfft" else deconv_specs(n_fft)
    for spec, n_outs in specs:
        p = problem(family, spec)
        for name, out in emulations(p).items():
            worst[name] = max(worst.get(name, 0.0), fraction(p, out, n_outs))
    return worst
