"""The float64 any-length transform (ds_fft_c128, ds_hilbert; kernels in csrc/kernels_fft64.hpp, host code fft64_pow2 /
fft64_plan / fft64_blue_tables in csrc/api.hip) route by route: the cases, their oracle, a float64 emulation of the
device algorithm, the bound and the judge.  test_fft64_host.py checks all of this on the CPU, test_fft64_gpu.py holds the
kernels to it.

The oracle.  scipy.fft.fft / ifft on numpy.clongdouble along axis 0 (it keeps long double: eps 1.1e-19 on x86-64) of the
float64 or complex128 array the entry is handed, zero-padded or cropped to n as ds_fft_c128 does.  For n <= 1024 the host
test also holds it to test_phase_host.longdouble_dft, the direct sum with integer-reduced phases, so it does not rest
on one library's Bluestein.  hilbert: transform, test_phase_host.fold_weights, inverse, all in long double.

The emulation.  Emulation.fft / hilbert restate in numpy float64 exactly what the device does: k_load's planar columns;
bit-reversed radix-2 decimation in time with the strided 4096-entry table exp(-2 pi i k / 8192); the four-step split
with lg1 = floor(lg / 2) and the outgoing twiddle from (j2 k1) mod n; Bluestein with k^2 mod 2n, the circular filter, the
transform of the filter, the 1 / M at the product and the conjugate tables for the inverse; the 1 / n of k_store as a
product with the rounded reciprocal.  Table values are long-double sin / cos rounded to double where the device calls
sincospi.  `perturb` makes it subtly wrong in one of five ways (PERTURBATIONS): the host test shows that the bound
rejects each.

The error rule is route_oracles.judge's: |out - oracle| <= tol * scale elementwise, scale = the rms of the oracle column
over all n bins; every bin of every column is judged, and a column that is identically zero must come back exactly
zero.  (No pure tones: a tone's spectrum is one bin of size n, its rms sqrt(n), and the emulation itself errs by 200 to
600 eps of that.)

The bound.  FFT64_EMULATION[(route, points of the power-of-two transform)] holds the emulation's worst error over the
cases of that key as a multiple of eps64 * scale, measured on the CPU (tools/measure_fft64_emulation.py prints the
table; the host test measures every entry up to 2^18 points again).  tolerance = 4 x max(that, 0.5) x HOST_MARGIN x
eps64: four for another equally valid rounding of sincospi and of the products, a tenth for another host's numpy
(x64_cases.tolerance's reasoning), and never below the half ulp of one rounding (at one point the emulation is exact).
No bound may exceed CAP = 1e-13 of the column rms, and the emulation alone has to stay within a quarter of that.

Inputs, per column: seeded Gaussian noise (real or complex), a unit impulse at the last kept row, one noise column
scaled by 1e-3, and in the 300-column case one column of zeros.  hilbert runs noise and scaled noise only: the analytic
signal of an impulse is the impulse again, one sample of size 1 in a column whose rms is sqrt(2 / n), so the half ulp
of that sample alone is 64 eps of the rms at 2^15 points (measured: 64 at 2^15, 106 at 5001).

The cases sit on the edges of the kernels, which depend on the constants mirrored below (the host test reads them out
of the sources and fails when they differ).  A length whose power-of-two transform (n, or Bluestein's M) has fewer than
2^20 points runs the cross of (1, 3) channels, n_in in {n - 7, n, n + 5}, real and complex, forward and inverse; from
2^20 on two calls of two channels: forward on complex noise with n_in = n, inverse on real input with n_in = n - 7 and
the impulse in the second column.  (That puts the prime 1048573 = 2^20 - 3 with its neighbours on M = 2^21 and 2^22: 24
long-double oracles of a prime that long take 22 s.)

  LDS route    1, 2 (the lg = 0 branch and one stage), 4, 256 and 512 (butterflies per stage below and equal to the 256
               lanes), 1024, 8192 (the whole 128 KB)
  four-step    2^14 (128 x 128), 2^15 (128 x 256: the smallest with n1 != n2), 2^16, 2^19 (512 x 1024), 2^21 (1024 x 2048),
               2^22 (2048 x 2048, the ceiling)
  Bluestein    BLUE_CASES: the length -> the M it runs on.  3 and 5 (less than one workgroup of k_chirp); 129 and 255
               (bottom and top of M = 512); 2049 and 4095 (of M = 8192, the last M on the LDS route); 4097 and 8191 (of M =
               16384, the first on the four-step); 46341 (the first k with k^2 > 2^31); 65537 and 1048573 (primes);
               1048577 and 2097151 (bottom and top of M = 2^22; the longest length accepted)
  many columns 8 points x 4096 channels; 1000 x 300 (rows and channels off any power of two in the flat-index divisions
               of k_load, k_store and k_blue); 2^14 x 33 (k_transpose and k_fft_lds with blockIdx.z / y > 32)
  hilbert      2^15 (even, four-step); 5000 and 5001 (even and odd mask, Bluestein on a four-step M); 4095 (Bluestein on
               the LDS route): two channels each
"""

import zlib
from collections import OrderedDict

import numpy as np
import scipy.fft as sfft

import route_oracles as ros
from test_phase_host import fold_weights

# ---- the constants the case list depends on (csrc/kernels_fft64.hpp, csrc/size_guards.hpp, csrc/api.hip) ------------
LDS_MAX = 8192                # points of the transform one workgroup holds; the twiddle table has LDS_MAX / 2 entries
NT = 256                      # lanes of every kernel
TRANSPOSE_TILE = 32
MAX_POW2 = 1 << 22            # kFft64MaxPow2
MAX_ANY = 1 << 21             # kFft64MaxAny
BLUE_CAP_BYTES = 256 << 20    # kBlue64CapBytes
BIG = 1 << 20                 # a length whose power-of-two transform has this many points or more runs two calls, not the cross

EPS = float(np.finfo(np.float64).eps)
CAP = 1e-13
HOST_MARGIN = ros.HOST_MARGIN
LD, CLD = np.longdouble, np.clongdouble

# worst error of the float64 emulation / (eps64 * scale) per (route, points of the power-of-two transform), as measured
# on the CPU by tools/measure_fft64_emulation.py
FFT64_EMULATION = {
    ("lds", 1): 0.0, ("lds", 2): 0.587, ("lds", 4): 0.771, ("lds", 8): 2.2, ("lds", 256): 2.92, ("lds", 512): 2.96,
    ("lds", 1024): 3.68, ("lds", 8192): 4.62,
    ("four", 16384): 6.28, ("four", 32768): 5.91, ("four", 65536): 7.05, ("four", 524288): 7.41, ("four", 2097152): 7.12,
    ("four", 4194304): 7.41,
    ("blue", 8): 3.34, ("blue", 16): 2.88, ("blue", 512): 6.78, ("blue", 2048): 9.5, ("blue", 8192): 9.68,
    ("blue", 16384): 10.2, ("blue", 131072): 10.9, ("blue", 262144): 10.4, ("blue", 2097152): 12.4, ("blue", 4194304): 13.2,
    ("hilbert", 8192): 10.8, ("hilbert", 16384): 11.6, ("hilbert", 32768): 6.55,
}

BLUE_CASES = OrderedDict([(3, 8), (5, 16), (129, 512), (255, 512), (2049, 8192), (4095, 8192), (4097, 16384), (8191, 16384),
                          (46341, 1 << 17), (65537, 1 << 18), (1048573, 1 << 21), (1048577, 1 << 22), (2097151, 1 << 22)])
LDS_CASES = (1, 2, 4, 256, 512, 1024, 8192)
FOUR_CASES = (1 << 14, 1 << 15, 1 << 16, 1 << 19, 1 << 21, 1 << 22)
COLUMN_CASES = ((8, 4096), (1000, 300), (1 << 14, 33))
HILBERT_CASES = (1 << 15, 5000, 5001, 4095)


def plan(n):
    """fft64_plan's rule -> (route, M, lg): the power-of-two transform that runs has M = 2^lg points."""
    pow2 = n & (n - 1) == 0
    M, lg = 1, 0
    while M < (n if pow2 else 2 * n - 1):
        M, lg = M << 1, lg + 1
    return ("blue" if not pow2 else "lds" if n <= LDS_MAX else "four"), M, lg


def tolerance(tk):
    return 4.0 * max(FFT64_EMULATION[tk], 0.5) * HOST_MARGIN * EPS


# ---- the cases ---------------------------------------------------------------------------------------------------------------
_specs = OrderedDict()


def call_spec(n_ch, n_in, cplx, inverse, impulse=None, small=None, zero=None):
    return dict(n_ch=n_ch, n_in=n_in, cplx=cplx, inverse=inverse, impulse=impulse, small=small, zero=zero)


def cross(n):
    """the calls of one length below 2^20: three channels are noise, the impulse, noise scaled by 1e-3"""
    return [call_spec(n_ch, n_in, cplx, inverse, impulse=1 if n_ch == 3 else None, small=2 if n_ch == 3 else None)
            for n_ch in (1, 3) for n_in in sorted({max(1, n - 7), n, n + 5}) for cplx in (False, True)
            for inverse in (False, True)]


def _add(ident, fn, n, calls):
    assert ident not in _specs, ident
    route, M, _ = plan(n)
    _specs[ident] = dict(ident=ident, fn=fn, n=n, calls=calls, key=("hilbert" if fn == "hilbert" else route, M))


def _build():
    for n in LDS_CASES + FOUR_CASES + tuple(BLUE_CASES):
        if plan(n)[1] < BIG:
            calls = cross(n)
        else:
            calls = [call_spec(2, n, True, False, small=1), call_spec(2, n - 7, False, True, impulse=1)]
        _add(f"{plan(n)[0]}|{n}", "fft", n, calls)
    for n, C in COLUMN_CASES:
        _add(f"cols|{n}x{C}", "fft", n, [call_spec(C, n, True, False, impulse=1, small=C - 1, zero=2 if C >= 100 else None),
                                        call_spec(C, max(1, n - 7), False, True, impulse=1, small=C - 1)])
    for n in HILBERT_CASES:
        _add(f"hilbert|{n}", "hilbert", n, [call_spec(2, n, False, False, small=1)])


_build()
IDENTS = list(_specs)


def case(ident):
    return _specs[ident]


def adhoc(n, calls):
    """a case outside the list (the host test's wrong emulations at 50000), with the bound of its route and M"""
    route, M, _ = plan(n)
    return dict(ident=f"adhoc|{n}", fn="fft", n=n, calls=calls, key=(route, M))


def call_input(c, i):
    """The (n_in, n_ch) array call i of the case hands the entry: float64 or complex128, C-contiguous; its own seed."""
    q = c["calls"][i]
    rng = np.random.default_rng(zlib.crc32(f"{c['ident']}|{i}".encode()))
    x = rng.standard_normal((q["n_in"], q["n_ch"]))
    if q["cplx"]:
        x = x + 1j * rng.standard_normal((q["n_in"], q["n_ch"]))
    if q["small"] is not None:
        x[:, q["small"]] *= 1e-3
    if q["impulse"] is not None:
        x[:, q["impulse"]] = 0.0
        x[min(q["n_in"], c["n"]) - 1, q["impulse"]] = 0.6 - 0.8j if q["cplx"] else 1.0
    if q["zero"] is not None:
        x[:, q["zero"]] = 0.0
    return np.ascontiguousarray(x)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def oracle_fft(x, n, inverse):
    """fft / ifft(x, n, axis=0) in long double"""
    kept = min(len(x), n)
    a = np.zeros((n, x.shape[1]), CLD)
    a[:kept] = x[:kept]
    return (sfft.ifft if inverse else sfft.fft)(a, axis=0, workers=min(x.shape[1], 8))


def oracle_hilbert(x):
    X = sfft.fft(x.astype(CLD), axis=0, workers=min(x.shape[1], 8))
    X *= fold_weights(len(x)).astype(LD)[:, None]
    return sfft.ifft(X, axis=0, workers=min(x.shape[1], 8))


def oracle(c, i, x):
    ref = oracle_hilbert(x) if c["fn"] == "hilbert" else oracle_fft(x, c["n"], c["calls"][i]["inverse"])
    assert ref.dtype == CLD
    return ref


# ---- the emulation: float64, the device's own steps ---------------------------------------------------------------------------
PERTURBATIONS = ("chirp_float", "twiddle_f32_phase", "table_f32", "scale_one_column", "filter_shift")
_PI = LD(4) * np.arctan(LD(1))
_bitrev_cache = {}


def sincospi(q):
    """(sin, cos)(pi q) of a float64 array as long-double values rounded to double; q is first reduced mod 2, which is
    exact in float64"""
    q = np.fmod(np.asarray(q, np.float64), 2.0)
    a = q.astype(LD) * _PI
    s, c = np.sin(a).astype(np.float64), np.cos(a).astype(np.float64)
    h = 2.0 * q                         # exact at the multiples of pi / 2, as the device's sincospi is
    whole = h == np.rint(h)
    s[whole & (np.fmod(h, 2.0) == 0.0)] = 0.0
    c[whole & (np.fmod(h, 2.0) != 0.0)] = 0.0
    return s, c


def _bitrev(lg):
    rev = _bitrev_cache.get(lg)
    if rev is None:
        rev = np.zeros(1, np.int64)
        for _ in range(lg):
            rev = np.concatenate([2 * rev, 2 * rev + 1])
        _bitrev_cache[lg] = rev
    return rev


class Emulation:
    """One float64 restatement of the device algorithm; perturb names the one thing it gets wrong, None nothing."""

    def __init__(self, perturb=None):
        assert perturb is None or perturb in PERTURBATIONS, perturb
        self.perturb = perturb
        s, c = sincospi(-np.arange(LDS_MAX // 2) / (LDS_MAX // 2))  # f64c::k_twiddles
        self.tw = c + 1j * s
        if perturb == "table_f32":
            self.tw = self.tw.astype(np.complex64).astype(np.complex128)
        self._four = (None, None)
        self._blue = (None, None)

    # k_fft_lds without its outgoing twiddle: the rows of a (batches, 2^lg), f64c::radix2_lds
    def radix2(self, a, lg, inv):
        if lg == 0:
            return a
        n = 1 << lg
        a = a[:, _bitrev(lg)]
        tw = self.tw.conj() if inv else self.tw
        for s in range(lg):
            half = 1 << s
            w = tw[(np.arange(half) << (lg - 1 - s)) * (LDS_MAX >> lg)]
            v = a.reshape(len(a), n // (2 * half), 2, half)
            u = v[:, :, 0, :].copy()
            t = v[:, :, 1, :] * w
            v[:, :, 0, :] = u + t
            v[:, :, 1, :] = u - t
        return a

    def _four_twiddle(self, n, n1, n2, inv):
        if self._four[0] != n:
            r = (np.arange(n2, dtype=np.int64)[:, None] * np.arange(n1, dtype=np.int64)[None, :]) % n
            if self.perturb == "twiddle_f32_phase":  # the phase in radians formed in float32
                a = (np.float32(2.0 * np.pi) * r.astype(np.float32) / np.float32(n)).astype(np.float64)
                s, c = np.sin(a), np.cos(a)
            else:
                s, c = sincospi(2.0 * r.astype(np.float64) / float(n))
            self._four = (n, c - 1j * s)
        return self._four[1].conj() if inv else self._four[1]

    # fft64_pow2: the rows of a (C, 2^lg), unnormalised
    def pow2(self, a, lg, inv):
        n = 1 << lg
        if n <= LDS_MAX:
            return self.radix2(a, lg, inv)
        C, lg1 = len(a), lg // 2
        n1, n2 = 1 << lg1, 1 << (lg - lg1)
        t = np.ascontiguousarray(a.reshape(C, n1, n2).transpose(0, 2, 1)).reshape(C * n2, n1)       # [j2][j1]
        t = self.radix2(t, lg1, inv).reshape(C, n2, n1) * self._four_twiddle(n, n1, n2, inv)        # [j2][k1] w_n^(j2 k1)
        t = np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(C * n1, n2)                          # [k1][j2]
        t = self.radix2(t, lg - lg1, inv).reshape(C, n1, n2)                                        # [k1][k2]
        return np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(C, n)                             # bin k1 + n1 k2

    # k_chirp and the transform of the filter (fft64_blue_tables) -> w [n], B [M]
    def _blue_tables(self, n, M, lg):
        if self._blue[0] != n:
            j = np.arange(n, dtype=np.int64)
            if self.perturb == "chirp_float":  # k^2 / n as a double quotient, no integer reduction
                q = (j * j).astype(np.float64) / float(n)
            else:
                q = ((j * j) % (2 * n)).astype(np.float64) / float(n)
            s, c = sincospi(q)
            b = np.zeros(M, np.complex128)
            b[:n] = c + 1j * s
            b[M - j[1:] - (1 if self.perturb == "filter_shift" else 0)] = b[1:n]
            self._blue = (n, (c - 1j * s, self.pow2(b[None, :], lg, False)[0]))
        return self._blue[1]

    # Fft64Run::fft on the planar (C, ld) array; the first n of every row are the result
    def transform(self, a, n, inv):
        route, M, lg = plan(n)
        if route != "blue":
            return self.pow2(a, lg, inv)
        w, B = self._blue_tables(n, M, lg)
        if inv:
            w, B = w.conj(), B.conj()
        a = a.copy()
        a[:, :n] *= w
        a[:, n:] = 0.0
        a = self.pow2(a, lg, False) * B
        scale = np.full((len(a), 1), 1.0 / M)
        if self.perturb == "scale_one_column":
            scale[0] = 1.0
        a = self.pow2(a * scale, lg, True)
        a[:, :n] *= w
        return a

    def load(self, x, n):
        kept = min(len(x), n)
        a = np.zeros((x.shape[1], plan(n)[1]), np.complex128)
        a[:, :kept] = x[:kept].T
        return a

    def fft(self, x, n, inverse):
        """ds_fft_c128"""
        a = self.transform(self.load(x, n), n, inverse)
        return np.ascontiguousarray(a[:, :n].T) * (1.0 / float(n) if inverse else 1.0)

    def hilbert(self, x):
        """ds_hilbert: load, transform, k_point's mask, inverse, 1 / n at the store"""
        n = len(x)
        a = self.transform(self.load(x, n), n, False)
        a[:, :n] *= fold_weights(n)
        a = self.transform(a, n, True)
        return np.ascontiguousarray(a[:, :n].T) * (1.0 / float(n))

    def run(self, c, i, x):
        return self.hilbert(x) if c["fn"] == "hilbert" else self.fft(x, c["n"], c["calls"][i]["inverse"])


# ---- the judge ------------------------------------------------------------------------------------------------------------------
def call_name(c, i):
    q = c["calls"][i]
    return (f"{c['ident']} {q['n_ch']}ch n_in={q['n_in']} {'complex' if q['cplx'] else 'real'} "
            f"{'inverse' if q['inverse'] else 'forward'}")


def judge_call(c, i, out, ref, tol=None):
    """what one call returned against its oracle -> the worst error as a fraction of the bound"""
    tol = tolerance(c["key"]) if tol is None else tol
    return ros.judge(call_name(c, i), out, ref, ros._rms(ref, 0), tol, np.complex128)


def fraction(out, ref):
    """the worst error of out / (eps64 * scale) over the columns that are not identically zero"""
    scale = np.broadcast_to(ros._rms(ref, 0), ref.shape)
    err = np.abs(out.astype(ref.dtype) - ref)
    return float(np.max(err[scale > 0] / (EPS * scale[scale > 0]), initial=0.0))


def emulation_fraction(c, perturb=None, calls=None):
    """the (perturbed) emulation's worst error / (eps64 * scale) over the calls of the case"""
    emu = Emulation(perturb)
    worst = 0.0
    for i in (range(len(c["calls"])) if calls is None else calls):
        x = call_input(c, i)
        worst = max(worst, fraction(emu.run(c, i, x), oracle(c, i, x)))
    return worst
