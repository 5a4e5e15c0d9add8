"""Long-double oracles of the fractional-octave smoothing kernels (csrc/kernels_smooth.hpp), one function per stage.
Pure numpy, no device.  Every function returns (value, bound): `value` in np.longdouble (eps 1.1e-19 on x86-64), `bound`
a per-element forward error bound of a float64 implementation of the same stage, derived in the function's docstring
from the roundings the stage performs -- nothing is fitted to the device.  u = 2^-53 is the unit roundoff of float64;
a library function that is good to 2 ulp errs by at most 4 u of its result.

An input may come with a bound `e` of its own (the previous stage's); it is carried through the stage's condition
(the convolution carries sum |w| e, the interpolations the weighted neighbours, the unwrap and the recombination pass
it on) and added to the stage's own roundings.  Second-order terms (u^2, u e) are covered by the slack of the integer
constants, which are all rounded up."""

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
ULD = LD(np.finfo(LD).eps)
PI = LD(4) * np.arctan(LD(1))
TWO_PI = 2 * PI


def _ld(a):
    return np.asarray(a, dtype=LD)


def _zero_like(a):
    return np.zeros(np.shape(a), dtype=LD)


# ---- k_smooth ---------------------------------------------------------------------------------------------------------
def smooth(v, window, e=None):
    """out[i] = sum_m wr[m] v[clamp(i - L / 2 + m, 0, N - 1)], wr the window over its long-double sum, reversed: the
    reference's edge padding (L / 2 rows in front, L / 2 - 1 behind for an even L, L / 2 for an odd one) and valid-mode
    convolution.  v: (N, C) float64 (or long double with its bound e).

    Bound.  The host forms wr in float64: the sum of L taps errs by (L - 1) u kappa relatively, kappa = sum |w| /
    |sum w| (1 for taps of one sign), the division adds u, so every tap carries the common factor (1 + delta), |delta|
    <= ((L - 1) kappa + 1) u <= (L + 1) kappa u.  A dot product of L terms accumulated in any order, with or without
    FMA, errs by at most gamma_L A = L u A / (1 - L u), A[i] = sum_m |wr[m]| |v[row]| over the clamped rows.  Together
    (L kappa + kappa + L) u A <= 2 (L + 2) kappa u A.  That worst case is all but attained when the roundings are few
    (two taps: four of them), and the host test wants every correct float64 implementation within a quarter of the
    bound, so the constant is doubled: c = 4.  The oracle's own long-double sum adds (L + 2) eps_ld A.  An input
    bound e comes out as sum |wr| e and joins |v| inside A.

    L = 1: w / w is 1 exactly and fma(1, v, 0) is v, so the stage is the identity and its own bound is zero."""
    v = _ld(v)
    e = _zero_like(v) if e is None else _ld(e)
    w = _ld(window)
    L, N = len(w), v.shape[0]
    if L == 1:
        return v.copy(), e.copy()
    wr = (w / w.sum())[::-1]
    kappa = np.abs(w).sum() / abs(w.sum())
    rows = np.arange(N) - L // 2
    out, A, E = _zero_like(v), _zero_like(v), _zero_like(v)
    av = np.abs(v) + e
    for m in range(L):
        src = np.clip(rows + m, 0, N - 1)
        out += wr[m] * v[src]
        A += abs(wr[m]) * av[src]
        E += abs(wr[m]) * e[src]
    return out, (4 * (L + 2) * kappa * U + (L + 2) * ULD) * A + E


# ---- k_to_log ---------------------------------------------------------------------------------------------------------
def _sgn(x):
    return np.sign(x)


def pchip_edge(m0, m1, second_branch=True):
    """scipy's PchipInterpolator._edge_case at unit spacing, elementwise"""
    d = (3 * m0 - m1) / 2
    first = _sgn(d) != _sgn(m0)
    second = (_sgn(m0) != _sgn(m1)) & (np.abs(d) > 3 * np.abs(m0)) & ~first
    d = np.where(first, 0, d)
    return np.where(second, 3 * m0, d) if second_branch else d


def edge_branch(m0, m1):
    """which branch pchip_edge takes: 0 (d and m0 differ in sign: 0), 1 (the slopes differ in sign and |d| > 3 |m0|:
    3 m0), 2 (d as it is)"""
    d = (3 * m0 - m1) / 2
    first = _sgn(d) != _sgn(m0)
    second = (_sgn(m0) != _sgn(m1)) & (np.abs(d) > 3 * np.abs(m0)) & ~first
    return np.where(first, 0, np.where(second, 1, 2))


def pchip_mid(ma, mb, zero_rule=True):
    """the interior derivative at unit spacing.  zero_rule False: the harmonic mean as 2 ma mb / (ma + mb) guarded by
    the sign rule alone -- two zero slopes side by side then divide 0 by 0"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if zero_rule:
            d = 1 / ((3 / ma + 3 / mb) / 6)
            return np.where((_sgn(ma) != _sgn(mb)) | (ma == 0) | (mb == 0), 0, d)
        return np.where(_sgn(ma) != _sgn(mb), 0, 2 * ma * mb / (ma + mb))


def pchip_terms(v, k_log, dtype=LD, zero_rule=True, second_branch=True):
    """k_to_log's quantities in `dtype`: (s, y0, d0, c1, t, V) per (query, channel); V = the largest |v| of the four
    knots the interval reads.  The interval index comes from the float64 k_log, as on the device."""
    v = np.asarray(v, dtype=dtype)
    k_log = np.asarray(k_log, dtype=np.float64)
    N = v.shape[0]
    i = np.clip(np.floor(k_log).astype(np.int64) - 1, 0, N - 2)
    s = (k_log.astype(dtype) - (i + 1).astype(dtype))[:, None]
    ym, y0, y1, yp = v[np.maximum(i - 1, 0)], v[i], v[i + 1], v[np.minimum(i + 2, N - 1)]
    m_prev, m, m_next = y0 - ym, y1 - y0, yp - y1
    if N > 2:
        first, last = (i == 0)[:, None], (i + 2 == N)[:, None]
        d0 = np.where(first, pchip_edge(m, m_next, second_branch), pchip_mid(m_prev, m, zero_rule))
        d1 = np.where(last, pchip_edge(m, m_prev, second_branch), pchip_mid(m, m_next, zero_rule))
    else:
        d0, d1 = m, m
    t = d0 + d1 - 2 * m
    c1 = (m - d0) - t
    V = np.maximum(np.maximum(np.abs(ym), np.abs(y0)), np.maximum(np.abs(y1), np.abs(yp)))
    return s, y0, d0, c1, t, V


def pchip_eval(s, y0, d0, c1, t):
    return y0 + d0 * s + c1 * (s * s) + t * (s * s * s)


def to_log(v, k_log):
    """PCHIP through the knots (1 .. N, v) at the points k_log: interior derivative the harmonic mean of the two
    neighbouring slopes, 0 where they differ in sign or one is 0; scipy's three-branch end rule; N = 2: the straight
    line; evaluated as y0 + d0 s + c1 s^2 + t s^3 on the interval i = clamp(floor(k_log) - 1, 0, N - 2), s = k_log -
    (i + 1), which extrapolates below knot 1 and above knot N.  v: (N, C) float64.

    The branches.  The sign of a rounded difference of two float64 numbers is the sign of the exact one, so the sign
    and zero tests of the interior rule, and sgn(m0) != sgn(m1) of the end rule, come out as in the oracle.  The end
    rule's two tests on d = (3 m0 - m1) / 2 can flip, but the rule is continuous there (d against 0 at d = 0; d against
    3 m0 at |d| = 3 |m0|), so a flip costs no more than the error of d itself.

    Bound, with V the largest |v| of the four knots read (every slope is at most 2 V, one rounding each):
      interior d   five roundings of a cancellation-free expression that is homogeneous and monotone in the slopes:
                   6 u |d|, |d| <= 2 min(|ma|, |mb|) <= 4 V: 24 u V
      end d        3 m0 - m1 and the halving, on slopes that carry u each: u (6 |m0| + |m1| + 2 |d|) <= 22 u V
      t            d0 + d1 - 2 m: 24 + 24 + 4 from its inputs, two roundings of at most 8 V and 12 V: 72 u V
      c1           (m - d0) - t: 2 + 24 + 72 from its inputs, roundings of at most 6 V and 18 V: 122 u V
      s            one subtraction, u |s| (exact for the axes of the sweep); it enters through the cubic's
                   derivative, at most 3 companion / |s|, so 3 u companion
      evaluation   two roundings for s^2 and s^3, one per product, one per addition: 6 u companion, companion =
                   |y0| + |d0 s| + |c1 s^2| + |t s^3|
    Together u (V (24 |s| + 122 s^2 + 72 |s|^3) + 10 companion), the oracle's own roundings (the same expression at
    eps_ld) added."""
    s, y0, d0, c1, t, V = pchip_terms(v, k_log)
    a = np.abs(s)
    comp = np.abs(y0) + np.abs(d0) * a + np.abs(c1) * a * a + np.abs(t) * a * a * a
    return pchip_eval(s, y0, d0, c1, t), (U + ULD) * (V * (24 * a + 122 * a * a + 72 * a * a * a) + 10 * comp)


# ---- k_to_lin ---------------------------------------------------------------------------------------------------------
def lin_bracket(k_log):
    """lo[l - 1] for the linear bins l = 1 .. N: the last index with k_log[lo] < l, within [0, N - 2]; found by exact
    comparison on the float64 axis"""
    k_log = np.asarray(k_log, dtype=np.float64)
    N = len(k_log)
    l = np.arange(1, N + 1, dtype=np.float64)
    return np.clip(np.searchsorted(k_log, l, side="left") - 1, 0, N - 2)


def to_lin(y, k_log, e=None, clip_ch=0):
    """Linear interpolation of (k_log, y) at the bins l = 1 .. N: r = y_lo + (y_hi - y_lo) (l - x_lo) / (x_hi - x_lo) on
    the bracket of lin_bracket; negative results of the first clip_ch columns become 0.

    Bound.  The weight w = (l - x_lo) / (x_hi - x_lo) lies in [0, 1] because k_log spans 1 .. N.  The device rounds
    y_hi - y_lo, x_hi - x_lo, the quotient, l - x_lo and the product (five roundings on the term w (y_hi - y_lo)) and
    the final addition (u |r|): at most 5 u |y_hi - y_lo| w + u |r| <= 6 u (|y_lo| + |y_hi|).  Six roundings that can
    all but align (neighbours of opposite sign, w near 1), and the host test wants every correct float64
    implementation within a quarter of the bound: the constant is doubled to 12.  The inputs' bounds come out as
    (1 - w) e_lo + w e_hi.  The clip is 1-Lipschitz: it moves the value, not the bound."""
    y = _ld(y)
    e = _zero_like(y) if e is None else _ld(e)
    k = _ld(np.asarray(k_log, dtype=np.float64))
    N = len(k)
    lo = lin_bracket(k_log)
    l = np.arange(1, N + 1).astype(LD)
    w = ((l - k[lo]) / (k[lo + 1] - k[lo]))[:, None]
    y_lo, y_hi = y[lo], y[lo + 1]
    r = y_lo + (y_hi - y_lo) * w
    b = (12 * U + 6 * ULD) * (np.abs(y_lo) + e[lo] + np.abs(y_hi) + e[lo + 1]) + (1 - w) * e[lo] + w * e[lo + 1]
    if clip_ch:
        r[:, :clip_ch] = np.maximum(r[:, :clip_ch], 0)
    return r, b


def clip(y, e, clip_ch):
    """k_clip: negative values of the first clip_ch columns become 0; exact, and 1-Lipschitz on the input's bound"""
    y = _ld(y).copy()
    y[:, :clip_ch] = np.maximum(y[:, :clip_ch], 0)
    return y, _ld(e)


def pipeline(v, k_log, window, clip_ch=0):
    """the three stages on linear bins (k_log given) or k_smooth and the clip alone (k_log None), each stage's bound
    carried through the next"""
    if k_log is None:
        y, e = smooth(v, window)
        return clip(y, e, clip_ch) if clip_ch else (y, e)
    y, e = to_log(v, k_log)
    y, e = smooth(y, window, e)
    return to_lin(y, k_log, e, clip_ch)


# ---- k_unwrap ---------------------------------------------------------------------------------------------------------
def unwrap_turns(ph):
    """(turns, d): the whole turns numpy.unwrap takes off at every step d = ph[b] - ph[b - 1] of float64 wrapped
    phases along axis 0, with pi in long double: floor((d + pi) / 2 pi) where |d| >= pi, none below; a rising step
    that lands exactly on -pi stays at +pi (one turn less)."""
    p = _ld(ph)
    d = np.diff(p, axis=0)
    q = np.floor((d + PI) / TWO_PI)
    on_edge = (d + PI - q * TWO_PI == 0) & (d > 0)
    q = np.where(on_edge, q - 1, q)
    q = np.where(np.abs(d) < PI, 0, q)
    return np.concatenate([np.zeros((1,) + p.shape[1:], dtype=LD), q], axis=0), d


def unwrap(ph, e=None, exact=None):
    """ph[b] - 2 pi (turns accumulated up to b): the mathematical unwrap of float64 phases (`exact`: the long-double
    phases the float64 ones were rounded from, which then are what the turns are taken off).  A float64 step of exactly
    +-fl(pi) lies inside the long-double pi, so it takes no turn -- what numpy's rule for +-pi comes to.

    Bound.  One correction is fl(pi)-arithmetic on a step |d| <= 2 pi: d itself (u |d|), d + pi (3 pi u), the exact
    fmod, + 2 pi (2 pi u), - pi (pi u), dm - d (2 pi u) and the two rounded constants (2 pi u): 12 pi u = 6 u |corr|.
    K_b nonzero corrections summed in any order (zeros add exactly) cost (K_b - 1) u S_b, S_b = sum |corr| up to b;
    carry + lane prefix, prefix + own, and the final addition to ph (u |out| <= 1.5 u S_b once anything was
    corrected) three more.  Together (K_b + 9.5) u S_b <= 4 (K_b + 2) u S_b for K_b >= 1: c = 4.  Before the first
    correction the output is the input, bit for bit, and the bound is zero.  An input bound passes through
    unchanged as long as it keeps every step on its side of pi (the cases keep a margin)."""
    p = _ld(ph if exact is None else exact)
    e = _zero_like(p) if e is None else _ld(e)
    q, _ = unwrap_turns(ph)
    K = np.cumsum(q != 0, axis=0)
    S = TWO_PI * np.cumsum(np.abs(q), axis=0)
    return p - TWO_PI * np.cumsum(q, axis=0), 4 * (K + 2) * (U + ULD) * S + e


def step_margin(ph):
    """the smallest distance of a step's magnitude from pi"""
    _, d = unwrap_turns(ph)
    return float(np.abs(np.abs(d) - PI).min()) if d.size else np.inf


# ---- k_polar, k_recombine ----------------------------------------------------------------------------------------------
def polar(z):
    """(|z|, its bound, atan2(im, re), its bound) of complex128 z.  hypot and atan2 of the device library are good
    to 2 ulp: 4 u of the result; atan2 of a zero imaginary part is 0 or +-fl(pi) exactly (C99 Annex F), which the
    oracle reproduces by rounding its long-double pi to float64 there."""
    z = np.asarray(z, dtype=np.complex128)
    re, im = _ld(z.real), _ld(z.imag)
    mag = np.hypot(re, im)
    ph = np.arctan2(im, re)
    on_axis = z.imag == 0
    ph = np.where(on_axis, _ld(np.arctan2(z.imag, z.real)), ph)
    return mag, 4 * U * mag, ph, np.where(on_axis, 0, 4 * U * np.abs(ph))


def recombine(mag, e_mag, ph, e_ph):
    """mag (cos ph, sin ph) -> (re, im, bound); the bound holds for either component.

    Bound.  |d z| <= |d mag| + |mag| |d ph| + |mag| (sincos, 4 u, and the product, u): with the device's phase within
    e_ph of the oracle's this is e_mag + |z| (e_ph + 6 u (1 + |ph|)) -- the |ph| term allows the library's argument
    reduction 6 u |ph| on top of the 6 u of the result."""
    mag, ph = _ld(mag), _ld(ph)
    a = np.abs(mag) + e_mag
    return mag * np.cos(ph), mag * np.sin(ph), e_mag + a * (e_ph + 6 * (U + ULD) * (1 + np.abs(ph)))


def complex_pipeline(z, k_log, window, clip_magnitude=False):
    """ds_octave_smooth_complex: |z| and the unwrapped phase smoothed as the 2 C columns of one real array, the first
    C clipped at 0 if asked, recombined.  Returns (re, im, bound, stages) with the stages' values for the tests."""
    mag, e_mag, ph, e_ph = polar(z)
    C = mag.shape[1]
    un, e_un = unwrap(np.asarray(ph, dtype=np.float64), e_ph, exact=ph)
    both, e_both = np.concatenate([mag, un], axis=1), np.concatenate([e_mag, e_un], axis=1)
    assert k_log is None, "the sweep runs the complex entry on logarithmic bins"
    sm, e_sm = smooth(both, window, e_both)
    if clip_magnitude:
        sm, e_sm = clip(sm, e_sm, C)
    re, im, b = recombine(sm[:, :C], e_sm[:, :C], sm[:, C:], e_sm[:, C:])
    return re, im, b, dict(mag=mag, wrapped=ph, unwrapped=un, e_unwrapped=e_un, smoothed=sm)


# ---- the judge ---------------------------------------------------------------------------------------------------------
def ratio(out, value, bound):
    """the worst |out - value| / bound over every element; where the bound is zero the error has to be zero (inf
    otherwise), and a value that is not finite counts as inf"""
    out = _ld(out)
    value, bound = np.broadcast_to(_ld(value), out.shape), np.broadcast_to(_ld(bound), out.shape)
    if out.size == 0:
        return 0.0
    if not np.isfinite(out.astype(np.float64)).all():
        return np.inf
    err = np.abs(out - value)
    zero = bound == 0
    if (err[zero] != 0).any():
        return np.inf
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
