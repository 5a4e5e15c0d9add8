"""The cases of the latency sweep (tests/test_latency_sweep_host.py, tests/test_latency_sweep_gpu.py): the constants of
csrc/kernels_latency.hpp, csrc/kernels_dist.hpp and csrc/size_guards.hpp restated, the inputs (built from seeds and
from lists of spikes: no golden file), each case's exact or long-double oracle with its bound, and a float64 numpy
emulation of every entry that can be made subtly wrong in eleven ways (FAULTS).  Pure numpy / scipy, no device.

Families, by the name's head:
  direct    k_peak, k_peak_final through backend.latency_peaks(x, None, 0) against np.argmax(np.abs(x), axis=0), exactly:
            lengths on both sides of one lane round (NT), of one workgroup (PEAK_SPAN) and of the final kernel's first
            round (256 and 257 workgroups and one row); equal magnitudes of opposite sign within a lane, across lanes,
            waves, workgroups and the final kernel's rounds; an all-zero column; a peak in the very last row
  corr      k_xmul, the rotated RowView, k_peak, k_peak_final through latency_peaks(td1, td2, 0): spike trains with
            small integer amplitudes, td1 = sum a_i delta[n - p_i], td2 = sum b_j delta[n - q_j], whose full correlation
            is exactly r[q_j - p_i + Na - 1] += a_i b_j in int64 (corr_rows; the dense arrays are only built to be
            uploaded).  The unique largest value sits in turn on row 0, L - 1, Na - 2, Na - 1, 4095, 4096 and, in the long
            shape, in workgroup 256 with smaller rivals below it; td2 has three channels or one.  With Na = 1 and one
            channel of td2 every pair has the same peak row (there is one lag per row of td2): the channels then differ
            in sign only.
            NO TIES in this family: the float64 transform returns equal integers differing in their last bits, so which
            of two equal magnitudes wins is not defined.  Every case's runner-up is at least 1 below its peak (the host
            test asserts it), against a transform error of about 1e-15.
  pearson   k_lag_partial, k_lag_final through backend.lag_pearson (and once through latency_peaks(..., pearson=True))
            against a two-pass long-double oracle.  Bound: each centred sum passes depth(n) = min(16, ceil(n / 256)) + 8
            + ceil(n_wg / 256) + 8 additions (levels_oracle.reduction_depth) and each term carries a few roundings of
            its own, so |r^ - r| <= 2 (depth(n) + 5) 2^-53 (A + |r|), A = sum |x'y'| / sqrt(sum x'^2 sum y'^2) from the
            oracle.
  window    the shared window's bounds, exactly, and the 2 p + 2 values of k_near around every peak: the NaN pattern
            exactly, the finite values against imag of fft64_cases.oracle_hilbert of the window.  Direct mode: the window
            is the input itself, the bound is hilbert_tolerance(M) times the rms of the oracle's analytic column, M the
            window's length.  Correlation mode: the window comes out of three power-of-two transforms of n_fft points
            first, so its own error is added: bound = hilbert_tolerance(M) rms(analytic window column) +
            pow2_tolerance(n_fft) rms(circular correlation column, n_fft rows), both taken from the long-double oracle.
  phase     k_lat_phase through backend.group_delay_phase(x, df, tau, fs) - group_delay_phase(x, df), which is -tau / fs
            per channel as long as both calls unwrap alike (precondition, asserted by the host test for every case:
            max |dphi| + 2 pi |tau| / n <= pi - 0.5).  Bound: PHASE_C 2^-53 (1 + |tau| + P / pi) / df, P the largest
            unwrapped phase of either call: the roundings of the shifted phase and of the unwrap's running sum, through
            the gradient.  What this cannot see: a slip of exactly 2 pi in the wrap is taken out again by the unwrap
            behind it; it is not visible through this entry (nor is it a defect of the entry), and no coverage of it is
            claimed.

LATENCY_EMULATION records the emulation's worst error / bound per family as measured on the CPU (run this module to
print it); the host test holds every case to a quarter of its bound."""

import functools
import zlib

import numpy as np
from scipy.signal import correlate, hilbert

import fft64_cases as fc

LD = np.longdouble
U = 2.0 ** -53

# ---- csrc/kernels_latency.hpp, csrc/kernels_dist.hpp, csrc/size_guards.hpp, csrc/api.hip ------------------------------
NT = 256
PEAK_SPAN = 4096       # rows per workgroup of the peak search
SPAN = 4096            # dsdist::SPAN = NT * PER_LANE, samples per workgroup of the Pearson sums
PER_LANE = 16
WINDOW_MARGIN = 200
MAX_POINTS = 16        # kLatencyMaxPoints
FINAL_ROUND = NT * PEAK_SPAN  # rows (samples) the first round of a final kernel covers: 2^20

# One rounding per operation gives (1.5 (1 + |tau|) + P / pi) 2^-53 / df: three roundings of pi (1 + |tau|) in the shifted
# phase and one of P in the unwrapped one, at both bins of the central difference over 4 pi df.  The device adds the
# unwrap's corrections as a lane's, a wave's and a tile's prefix instead of one running sum and takes three products for
# the shift: four times the analysis.  Numpy's float64 emulation measures PHASE_EMULATION_UNITS of that unit at worst,
# less than a quarter of PHASE_C.
PHASE_C = 8.0
PHASE_EMULATION_UNITS = 0.67
# the float64 emulation's worst error / bound per family (the exact families have none)
LATENCY_EMULATION = {"pearson": 0.0411, "window": 0.121, "phase": 0.0838}


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def family(name: str) -> str:
    return name.split("-")[0]


# ---- tolerances of the transform family -----------------------------------------------------------------------------------
def hilbert_tolerance(m: int) -> float:
    """fft64_cases' bound of a Hilbert transform of m rows, relative to the column's rms: the table's entry for the
    power-of-two transform it runs on (M of fft64_cases.plan), else the largest entry at or above that M (the error
    grows with the number of butterfly stages, and Bluestein's exceeds the plain route's)."""
    M = fc.plan(m)[1]
    if ("hilbert", M) in fc.FFT64_EMULATION:
        return fc.tolerance(("hilbert", M))
    return max(fc.tolerance(k) for k in fc.FFT64_EMULATION if k[0] == "hilbert" and k[1] >= M)


def pow2_tolerance(n_fft: int) -> float:
    """the bound of the power-of-two transform of n_fft points, the nearest larger entry of its route standing in"""
    route = fc.plan(n_fft)[0]
    sizes = sorted(m for r, m in fc.FFT64_EMULATION if r == route and m >= n_fft)
    return fc.tolerance((route, sizes[0]))


def pow2_at_least(n: int) -> int:
    m = 1
    while m < n:
        m <<= 1
    return m


# ==== A. the peak search ====================================================================================================
DIRECT_LENGTHS = (1, 255, 256, 257, PEAK_SPAN - 1, PEAK_SPAN + 1, 256 * PEAK_SPAN + 1, 257 * PEAK_SPAN + 1)
LONGEST = 257 * PEAK_SPAN + 1
TIES_N = 3 * PEAK_SPAN + 5
# column -> (the row that wins, the later row of the same magnitude); the earlier value is negative in every other one
TIES = {"lane": (7, 7 + NT), "lanes": (70, 75), "waves": (70, 200), "workgroups": (100, PEAK_SPAN + 50)}
ROUND_TIES = {"direct-rounds-lane": (PEAK_SPAN + 9, 257 * PEAK_SPAN),        # workgroups 1 and 257: lane 1, rounds 0 and 1
              "direct-rounds-lanes": (5 * PEAK_SPAN + 77, 256 * PEAK_SPAN + 3)}  # workgroup 5 (lane 5), 256 (lane 0, round 1)


def direct_cases():
    return [f"direct-len-n{n}" for n in DIRECT_LENGTHS] + ["direct-ties"] + list(ROUND_TIES) + ["direct-last-row"]


def _quiet(rng, shape):
    """noise well below the spikes"""
    return np.clip(0.1 * rng.standard_normal(shape), -0.9, 0.9)


def direct_problem(name: str) -> dict:
    rng = _rng(name)
    must = None
    if name.startswith("direct-len-"):
        n = int(name.split("-n")[1])
        x = rng.standard_normal((n, 1 if n > FINAL_ROUND else 3))
    elif name == "direct-ties":
        x = _quiet(rng, (TIES_N, len(TIES) + 1))
        for c, (first, later) in enumerate(TIES.values()):
            s = -1.0 if c % 2 == 0 else 1.0
            x[first, c], x[later, c] = 2.0 * s, -2.0 * s
        x[:, len(TIES)] = 0.0
        must = [first for first, _ in TIES.values()] + [0]
    elif name in ROUND_TIES:
        x = _quiet(rng, (LONGEST, 1))
        first, later = ROUND_TIES[name]
        x[first, 0], x[later, 0] = -2.0, 2.0
        must = [first]
    elif name == "direct-last-row":
        x = _quiet(rng, (LONGEST, 1))
        x[LONGEST - 1, 0] = -2.0
        must = [LONGEST - 1]
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x)
    expect = np.argmax(np.abs(x), axis=0).astype(np.int64)
    return dict(x=x, expect=expect, must=must)


def emu_direct_peaks(x, fault=None):
    a = np.abs(x)
    if fault == "final_drop":  # the final kernel reads the first 256 partials only
        a = a[:FINAL_ROUND]
    if fault == "tie_later":
        return (len(a) - 1 - np.argmax(a[::-1], axis=0)).astype(np.int64)
    return np.argmax(a, axis=0).astype(np.int64)


# ---- correlation mode -------------------------------------------------------------------------------------------------------
LONG_SHAPE = (1 << 20, 4098)
CORR_SHAPES = ((1, 7), (7, 1), (2049, 2048), (2049, 2049), (4096, 4097), LONG_SHAPE)
LONG_ROW = FINAL_ROUND + 99  # in workgroup 256 of the long shape
N_CH = 3


def corr_targets(Na: int, Nb: int) -> list:
    L = Na + Nb - 1
    rows = {0, L - 1, Na - 2, Na - 1, 4095, 4096}
    if (Na, Nb) == LONG_SHAPE:
        rows.add(LONG_ROW)
    return sorted(k for k in rows if 0 <= k < L)


def _q_range(rows, Na, Nb):
    """the positions of a shared td2 spike that put the peaks of three channels on `rows`"""
    return max(0, max(rows) - (Na - 1)), min(Nb - 1, min(rows))


def corr_row_sets(Na: int, Nb: int, cb: int) -> list:
    """the peak rows of the three channels, case by case: every target row of the shape turns up"""
    T = corr_targets(Na, Nb)
    sets = []
    if cb == N_CH:
        for i in range(0, len(T), N_CH):
            sets.append([T[(i + c) % len(T)] for c in range(N_CH)])
        return sets
    i = 0
    while i < len(T):  # one channel of td2: neighbouring targets that one spike of td2 can serve
        rows = [T[i]]
        while len(rows) < N_CH and i + len(rows) < len(T):
            lo, hi = _q_range(rows + [T[i + len(rows)]], Na, Nb)
            if lo > hi:
                break
            rows.append(T[i + len(rows)])
        i += len(rows)
        for d in (-1, -2, 1, 2):  # too few targets left: rows next to the first one, so that every channel has its own
            k = rows[0] + d
            if len(rows) < N_CH and Na > 1 and 0 <= k < Na + Nb - 1 and k not in rows:
                lo, hi = _q_range(rows + [k], Na, Nb)
                if lo <= hi:
                    rows.append(k)
        sets.append([rows[c % len(rows)] for c in range(N_CH)])
    return sets


def corr_cases():
    return [f"corr-{Na}x{Nb}-b{cb}-s{i}" for Na, Nb in CORR_SHAPES for cb in (N_CH, 1)
            for i in range(len(corr_row_sets(Na, Nb, cb)))]


def _corr_fields(name: str):
    _, shape, b, s = name.split("-")
    Na, Nb = (int(v) for v in shape.split("x"))
    return Na, Nb, int(b[1:]), int(s[1:])


def _other(rng, n, taken):
    """a position in [0, n) that is not `taken`"""
    return int((taken + 1 + rng.integers(0, n - 1)) % n)


def corr_spikes(name: str):
    """(sp1, sp2, rows): per channel of td1 and of td2 the list of (position, integer amplitude), and the row every
    channel's peak has to be on.  td1: the main spike +-3 and a lesser one of 1; td2: the main spike 4 and a lesser one
    of 2.  The peak is 12; the other products are 6, 4 and 2 and add up to 10 at most where they fall on one row."""
    Na, Nb, cb, s = _corr_fields(name)
    rows = corr_row_sets(Na, Nb, cb)[s]
    rng = _rng(name)
    shared_q = _q_range(rows, Na, Nb)[0] if cb == 1 else None
    sp1, sp2 = [], []
    for c, k in enumerate(rows):
        if cb == 1:
            q = shared_q
            p = q + Na - 1 - k
        else:
            p = max(0, Na - 1 - k)
            q = k - (Na - 1) + p
        assert 0 <= p < Na and 0 <= q < Nb, (name, c, p, q)
        one = [(p, 3 if c % 2 == 0 else -3)]
        if Na > 1:
            one.append((_other(rng, Na, p), 1))
        sp1.append(one)
        if cb == N_CH or c == 0:
            two = [(q, 4)]
            if Nb > 1:
                two.append((_other(rng, Nb, q), 2))
            sp2.append(two)
    return sp1, sp2, rows


def corr_rows(one, two, Na: int, rot_off: int = 0, n_fft: int = 0, L: int = 0) -> dict:
    """{row: int64 value} of the full correlation of two spike lists: r[q - p + Na - 1] += a b.  With n_fft: through the
    circular correlation and the rotated view as the device reads it, the rotation off by rot_off."""
    out = {}
    for p, a in one:
        for q, b in two:
            k = q - p + Na - 1
            if n_fft:
                m = (q - p) % n_fft                       # where the circular correlation holds the product
                k = (m - (n_fft - (Na - 1) + rot_off)) % n_fft  # the row whose view reads it
                if k >= L:
                    continue
            out[k] = out.get(k, 0) + a * b
    return out


def peak_of(rows: dict):
    """(row, |value|, runner-up's |value|) of the largest magnitude, the lowest row among equal ones"""
    order = sorted(rows.items(), key=lambda kv: (-abs(kv[1]), kv[0]))
    return order[0][0], abs(order[0][1]), (abs(order[1][1]) if len(order) > 1 else 0)


def dense(spikes, n: int) -> np.ndarray:
    x = np.zeros((n, len(spikes)))
    for c, one in enumerate(spikes):
        for p, a in one:
            x[p, c] += a
    return x


def corr_problem(name: str) -> dict:
    Na, Nb, cb, _ = _corr_fields(name)
    sp1, sp2, rows = corr_spikes(name)
    full = [corr_rows(sp1[c], sp2[c if cb == N_CH else 0], Na) for c in range(N_CH)]
    expect = np.array([peak_of(r)[0] for r in full], dtype=np.int64)
    return dict(Na=Na, Nb=Nb, cb=cb, sp1=sp1, sp2=sp2, must=rows, full=full, expect=expect)


def corr_inputs(p: dict):
    return dense(p["sp1"], p["Na"]), dense(p["sp2"], p["Nb"])


def emu_corr_peaks(p: dict, fault=None):
    Na, Nb, cb = p["Na"], p["Nb"], p["cb"]
    L = Na + Nb - 1
    out = []
    for c in range(N_CH):
        rows = corr_rows(p["sp1"][c], p["sp2"][c if cb == N_CH else 0], Na, 1 if fault == "rot_off" else 0,
                         pow2_at_least(L), L)
        if fault == "final_drop":
            rows = {k: v for k, v in rows.items() if k < FINAL_ROUND}
        if fault == "tie_later":
            rows = {-k: v for k, v in rows.items()}
        k = peak_of(rows)[0] if rows else 0
        out.append(-k if fault == "tie_later" else k)
    return np.array(out, dtype=np.int64)


# ==== B. Pearson's r at a lag =================================================================================================
PEARSON_LENGTHS = (0, 1, 2, 3, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1, 256 * SPAN + 1, (1 << 20) + 4097)
RHOS = {"r95": 0.95, "r50": 0.5, "r05": 0.05, "rm70": -0.7}
OFFSETS = {"plain": (0.0, 0.0), "offset": (1000.0, 500.0)}  # added to every column of t, of o
# way -> (lag, how much longer than the overlap the undelayed signal is; None: the delayed one is, by 3, after the lag)
WAYS = {"pos_short": (3, 5), "pos_long": (7, None), "neg_short": (-3, 5), "neg_long": (-7, None), "zero_t": (0, 5),
        "zero_o": (0, None)}
CHANNELS = ((1, 2), (2, 5), (5, 1), (2, 1), (1, 5), (5, 2))  # (n_ch_t, n_ch_o): the strides differ
PEARSON_ENTRY = "pearson-latency"


def depth(n: int) -> int:
    n_wg = -(-n // SPAN)
    return min(PER_LANE, -(-n // NT)) + 8 + -(-n_wg // NT) + 8


def pearson_ways(n: int):
    if n == 0:  # the undelayed signal has a sample at least: only the delayed one can run out
        return ("pos_short", "neg_short")
    if n > FINAL_ROUND:
        return ("pos_short", "neg_long", "zero_t")
    return tuple(WAYS)


def pearson_kinds(n: int):
    if n > FINAL_ROUND:  # one channel each: 8.4 MB per array
        return ("r95-offset", "r05-plain", "rm70-offset", "special-offset")
    return tuple(f"{r}-{o}" for r in RHOS for o in OFFSETS) + ("special-plain", "special-offset")


def pearson_cases(n=None):
    return [f"pearson-n{m}-{way}-{kind}" for m in (PEARSON_LENGTHS if n is None else (n,)) for way in pearson_ways(m)
            for kind in pearson_kinds(m)]


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def pearson_problem(name: str) -> dict:
    """t (n_t, n_ch_t), o (n_o, n_ch_o), rows (col_t, col_o, lag).  Column k of o is rho times column k mod n_ch_t of t,
    as the lag aligns them, plus noise, all float32-valued.  special: o's columns are 2 x, -0.5 x (exactly), noise against
    a constant column of t, and a constant column."""
    _, nn, way, what, off = name.split("-")
    n, rng = int(nn[1:]), _rng(name)
    lag, extra = WAYS[way]
    s = abs(lag)
    if lag == 0:
        n_t, n_o = (n, n + 5) if way == "zero_t" else (n + 3, n)
    else:
        n_del, n_und = (n + s, n + extra) if extra is not None else (n + s + 3, n)
        n_t, n_o = (n_und, n_del) if lag > 0 else (n_del, n_und)
    n_t, n_o = max(n_t, 1), max(n_o, 1)
    off_t, off_o = OFFSETS[off]
    long = n > FINAL_ROUND
    start_t, start_o = max(lag, 0), max(-lag, 0)  # t[i] and o[i + lag] are the same instant
    size = max(n_t + start_t, n_o + start_o)

    def base():
        return rng.standard_normal(size)

    if what == "special":
        g = _f32(_f32(base()) + off_t)
        if long:
            t = g[start_t:start_t + n_t, None]
            o = (-0.5 * g)[start_o:start_o + n_o, None]
            rows = [(0, 0, lag)]
        else:
            t = np.stack([g, np.full(size, 0.25 + off_t)], axis=1)[start_t:start_t + n_t]
            o = np.stack([2.0 * g, -0.5 * g, _f32(_f32(base()) + off_o), np.full(size, 0.25 + off_o), _f32(base())],
                         axis=1)[start_o:start_o + n_o]
            rows = [(0, 0, lag), (0, 1, lag), (1, 2, lag), (0, 3, lag), (0, 4, lag)]
    else:
        rho = RHOS[what]
        n_ch_t, n_ch_o = (1, 1) if long else CHANNELS[zlib.crc32(name.encode()) % len(CHANNELS)]
        tt = [_f32(base()) for _ in range(n_ch_t)]
        oo = [_f32(rho * tt[k % n_ch_t] + np.sqrt(1.0 - rho * rho) * base()) for k in range(n_ch_o)]
        t = np.stack([_f32(v + off_t) for v in tt], axis=1)[start_t:start_t + n_t]
        o = np.stack([_f32(v + off_o) for v in oo], axis=1)[start_o:start_o + n_o]
        rows = [(k % n_ch_t, k, lag) for k in range(n_ch_o)]
    t, o = np.ascontiguousarray(t), np.ascontiguousarray(o)
    value, bound = pearson_oracle_rows(t, o, rows)
    return dict(t=t, o=o, rows=np.array(rows, dtype=np.int64), n=n, value=value, bound=bound)


def overlap(t, o, ct, co, lag):
    """(x, y): the delayed column from its first kept sample and the undelayed one, both cut to the shorter
    (_get_correlation_of_latencies)"""
    s = abs(lag)
    dl, und = (o[:, co], t[:, ct]) if lag > 0 else (t[:, ct], o[:, co])
    dl = dl[s:]
    n = min(len(dl), len(und))
    return dl[:n], und[:n]


def pearson_oracle(x, y):
    """(r, bound) in long double, two passes; NaN below two samples or for a constant column"""
    n = len(x)
    if n < 2:
        return LD(np.nan), LD(0)
    x, y = x.astype(LD), y.astype(LD)
    xc, yc = x - x.sum() / n, y - y.sum() / n
    sxx, syy, sxy = (xc * xc).sum(), (yc * yc).sum(), (xc * yc).sum()
    if sxx == 0 or syy == 0:
        return LD(np.nan), LD(0)
    den = np.sqrt(sxx * syy)
    r = sxy / den
    return r, 2 * (depth(n) + 5) * LD(U) * (np.abs(xc * yc).sum() / den + abs(r))


def pearson_oracle_rows(t, o, rows):
    got = [pearson_oracle(*overlap(t, o, ct, co, lag)) for ct, co, lag in rows]
    return np.array([g[0] for g in got], dtype=LD), np.array([g[1] for g in got], dtype=LD)


def _tree(v):
    """dsdist::tree over the last axis (NT lanes)"""
    v = v.copy()
    s = NT // 2
    while s > 0:
        v[..., :s] += v[..., s:2 * s]
        s >>= 1
    return v[..., 0]


def kernel_sum(terms, drop=False):
    """the sum of a vector in the kernels' order: lane t of workgroup w adds the terms w SPAN + i NT + t in turn, a tree
    over the lanes, then lane t adds the partials t, t + NT, ... and the same tree.  drop: partials from NT on are lost"""
    n = len(terms)
    n_wg = max(1, -(-n // SPAN))
    v = np.zeros(n_wg * SPAN)
    v[:n] = terms
    v = v.reshape(n_wg, PER_LANE, NT)
    acc = np.zeros((n_wg, NT))
    for i in range(PER_LANE):
        acc = acc + v[:, i, :]
    part = _tree(acc)
    if drop:
        part = part[:NT]
    rounds = -(-len(part) // NT)
    w = np.zeros(rounds * NT)
    w[:len(part)] = part
    w = w.reshape(rounds, NT)
    acc = np.zeros(NT)
    for i in range(rounds):
        acc = acc + w[i]
    return float(_tree(acc))


def emu_pearson_row(t, o, ct, co, lag, fault=None):
    if fault == "lag_sign":
        lag = -lag
    s = abs(lag)
    o_delayed = lag > 0
    n_t, n_o = len(t), len(o)
    n_del, n_und = (n_o, n_t) if o_delayed else (n_t, n_o)
    n = max(min(n_del - s, n_und), 0)
    if n < 1:
        return np.nan
    st, so = t.shape[1], o.shape[1]
    if fault == "stride_swap":
        st, so = so, st
    ft, fo = t.reshape(-1), o.reshape(-1)
    idx = np.arange(n)
    if o_delayed:
        x, y = fo[(co + (s + idx) * so) % fo.size], ft[(ct + idx * st) % ft.size]
    else:
        x, y = ft[(ct + (s + idx) * st) % ft.size], fo[(co + idx * so) % fo.size]
    drop = fault == "final_drop"
    if fault == "means_uncut":
        mx, my = (o[:, co].mean(), t[:, ct].mean()) if o_delayed else (t[:, ct].mean(), o[:, co].mean())
    else:
        mx, my = kernel_sum(x, drop) / n, kernel_sum(y, drop) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        if fault == "raw_moment":
            sxx = kernel_sum(x * x) - n * mx * mx
            syy = kernel_sum(y * y) - n * my * my
            sxy = kernel_sum(x * y) - n * mx * my
        else:
            xc, yc = x - mx, y - my
            sxx, syy, sxy = kernel_sum(xc * xc, drop), kernel_sum(yc * yc, drop), kernel_sum(xc * yc, drop)
        r = np.float64(sxy) / np.sqrt(np.float64(sxx) * np.float64(syy))
    if n < 2:
        r = np.nan
    return float(np.clip(r, -1.0, 1.0))


def emu_pearson(p: dict, fault=None):
    return np.array([emu_pearson_row(p["t"], p["o"], int(ct), int(co), int(lag), fault) for ct, co, lag in p["rows"]])


def judge_pearson(p: dict, out) -> float:
    """worst |out - r| / bound; NaN exactly where the oracle has it; every finite value in [-1, 1]"""
    value, bound = p["value"], p["bound"]
    assert out.shape == value.shape and out.dtype == np.float64
    nan = np.isnan(value)
    if not np.array_equal(np.isnan(out), nan):
        return float("inf")
    if not (np.abs(out[~nan]) <= 1.0).all():
        return float("inf")
    return float(np.max(np.abs(out[~nan].astype(LD) - value[~nan]) / bound[~nan], initial=0.0))


def pearson_entry_problem() -> dict:
    """latency_peaks(td1, td2, 0, pearson=True): one channel of td2 (zero-mean float32-valued noise) against three delayed,
    scaled and noisy copies of it"""
    rng = _rng(PEARSON_ENTRY)
    Nb, Na, delays = 5000, 5003, (3, 17, 40)
    td2 = _f32(rng.standard_normal((Nb, 1)))
    td1 = np.zeros((Na, 3))
    for c, d in enumerate(delays):
        td1[d:, c] = (0.9 - 0.2 * c) * td2[:Na - d, 0]
    td1 = np.ascontiguousarray(_f32(td1 + 0.3 * rng.standard_normal(td1.shape)))
    full = np.stack([correlate(td2[:, 0], td1[:, c]) for c in range(3)], axis=1)
    peaks = np.argmax(np.abs(full), axis=0).astype(np.int64)
    rows = [(0, c, int(Na - 1 - peaks[c])) for c in range(3)]
    value, bound = pearson_oracle_rows(td2, td1, rows)
    return dict(td1=td1, td2=td2, expect=peaks, t=td2, o=td1, rows=np.array(rows, dtype=np.int64), value=value, bound=bound,
                delays=delays)


# ==== C. the shared window and the neighbourhood ===========================================================================
NOISE = 1e-3
DIRECT_L = 6000
NEAR_L = 3000                      # direct mode, four channels: the window is the array, its Bluestein M = 8192
NEAR_SHAPES = ((2049, 2049), (2049, 2048))  # L = 4097 (window M = 16384, n_fft = 8192) and L = n_fft = 4096
NEAR_P = (1, 3, MAX_POINTS)
# layout -> the peak rows of the two channels of a (DIRECT_L, 2) array, p = 1
WINDOW_LAYOUTS = {
    "ends": (0, DIRECT_L - 1),
    "e198": (198, DIRECT_L - 199), "e199": (199, DIRECT_L - 200), "e200": (200, DIRECT_L - 201),
    "pow2": (700, 700 + 4096 - 2 * WINDOW_MARGIN), "pow2p1": (700, 700 + 4097 - 2 * WINDOW_MARGIN),
}


def near_rows(L: int, p: int):
    return (0, p, L - 2 - p, L - 1)


def window_cases():
    out = [f"window-direct-{k}" for k in WINDOW_LAYOUTS]
    for p in NEAR_P:
        out.append(f"window-near-direct-p{p}")
        out += [f"window-near-first-p{p}", f"window-near-last-p{p}"]
        out += [f"window-near-corr{Na}x{Nb}-p{p}" for Na, Nb in NEAR_SHAPES]
    return out


def _spiky(rng, n, rows):
    """(n, C): +-3 at the channel's row, n // 4 lesser spikes of +-1 and +-2 and the noise.  The lesser spikes give the
    column an rms of about 0.8: the transform family's bounds are relative to the rms, and the values next to a lone
    spike in a silent column are a hundred times the rms (fft64_cases leaves impulses out of its Hilbert cases for that
    reason)"""
    x = NOISE * rng.standard_normal((n, len(rows)))
    for c, k in enumerate(rows):
        at = rng.choice(n, size=n // 4, replace=False)
        x[at, c] += rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(at))
        x[k, c] = 3.0 if c % 2 == 0 else -3.0
    return np.ascontiguousarray(x)


def window_of(peaks, L: int):
    lo = max(int(min(peaks)) - WINDOW_MARGIN, 0)
    return lo, min(int(max(peaks)) + WINDOW_MARGIN, L) - lo


def near_pattern(peaks, lo: int, m: int, p: int) -> np.ndarray:
    """(C, 2 p + 2) bool: True where the row lies outside the window"""
    row = np.asarray(peaks)[:, None] - lo - p + np.arange(2 * p + 2)[None, :]
    return (row < 0) | (row >= m)


def window_problem(name: str) -> dict:
    parts = name.split("-")
    rng = _rng(name)
    if parts[1] == "direct":
        rows, p = WINDOW_LAYOUTS[parts[2]], 1
        td1, td2, L = _spiky(rng, DIRECT_L, rows), None, DIRECT_L
    else:
        p = int(parts[3][1:])
        if parts[2] == "direct":
            L = NEAR_L
            rows = near_rows(L, p)
        elif parts[2] in ("first", "last"):
            L = NEAR_L
            rows = (0,) if parts[2] == "first" else (L - 1,)
        if parts[2].startswith("corr"):
            Na, Nb = (int(v) for v in parts[2][4:].split("x"))
            L = Na + Nb - 1
            rows = near_rows(L, p)
            pq = [(max(0, Na - 1 - k), k - (Na - 1) + max(0, Na - 1 - k)) for k in rows]
            td1 = NOISE * rng.standard_normal((Na, len(rows)))
            for c, (pp, _) in enumerate(pq):
                td1[pp, c] += 3.0 if c % 2 == 0 else -3.0
            td2 = _spiky(rng, Nb, [q for _, q in pq])
            td2[[q for _, q in pq], np.arange(len(rows))] = 4.0
            td1, td2 = np.ascontiguousarray(td1), np.ascontiguousarray(td2)
        else:
            td1, td2 = _spiky(rng, L, rows), None
    lo, m = window_of(rows, L)
    nan = near_pattern(rows, lo, m, p)
    # the long-double oracle of the window and of its Hilbert transform
    if td2 is None:
        win = td1[lo:lo + m].astype(LD)
        extra = np.zeros(td1.shape[1], dtype=LD)
    else:
        n_fft = pow2_at_least(L)
        A, B = fc.oracle_fft(td1, n_fft, False), fc.oracle_fft(td2, n_fft, False)
        circ = fc.sfft.ifft(B * np.conj(A), axis=0).real
        full = np.roll(circ, Na - 1, axis=0)[:L]  # full[k] = circ[(k - (Na - 1)) mod n_fft]
        win = full[lo:lo + m]
        extra = LD(pow2_tolerance(n_fft)) * np.sqrt(np.mean(circ * circ, axis=0))
    h = fc.oracle_hilbert(win)
    bound = LD(hilbert_tolerance(m)) * np.sqrt(np.mean(np.abs(h) ** 2, axis=0)) + extra
    value = np.full(nan.shape, np.nan, dtype=LD)
    for c, k in enumerate(rows):
        for j in range(2 * p + 2):
            if not nan[c, j]:
                value[c, j] = h[k - lo - p + j, c].imag
    return dict(td1=td1, td2=td2, p=p, L=L, must=list(rows), expect=np.array(rows, dtype=np.int64), window=(lo, m), nan=nan,
                value=value, bound=np.asarray(bound, dtype=LD))


def emu_latency(td1, td2, p: int, fault=None):
    """(peaks, window, near) of latency_peaks in float64 numpy: the circular correlation on n_fft points, the rotated
    view, the shared window scaled by 1 / n_fft, scipy's hilbert, the neighbourhood"""
    if td2 is None:
        full = td1
    else:
        Na, L = len(td1), len(td1) + len(td2) - 1
        n_fft = pow2_at_least(L)
        circ = np.fft.ifft(np.fft.fft(td2, n_fft, axis=0) * np.conj(np.fft.fft(td1, n_fft, axis=0)), axis=0).real
        rot = n_fft - (Na - 1) + (1 if fault == "rot_off" else 0)
        full = circ[(np.arange(L) + rot) % n_fft]
    L = len(full)
    peaks = np.argmax(np.abs(full), axis=0).astype(np.int64)
    lo, m = window_of(peaks[:1] if fault == "window_first_channel" else peaks, L)
    h = hilbert(full[lo:lo + m], axis=0).imag
    row = peaks[:, None] - lo - p + np.arange(2 * p + 2)[None, :]
    inside = (row >= 0) & (row < m)
    near = h[np.clip(row, 0, m - 1), np.arange(len(peaks))[:, None]]
    if fault != "near_clamp":
        near = np.where(inside, near, np.nan)
    return peaks, (lo, m), near


def judge_window(p: dict, out) -> float:
    """peaks and window exactly, NaN where the pattern says so and nowhere else, the finite values within the bound"""
    peaks, window, near = out
    if not np.array_equal(peaks, p["expect"]) or tuple(window) != p["window"]:
        return float("inf")
    assert near.shape == p["nan"].shape and near.dtype == np.float64
    if not np.array_equal(np.isnan(near), p["nan"]):
        return float("inf")
    err = np.abs(near.astype(LD) - p["value"]) / p["bound"][:, None]
    return float(np.max(err[~p["nan"]], initial=0.0))


# ==== D. the latency taken out of the phase =================================================================================
FS = 48000.0
PHASE_NS = (64, 1000, 4097, 32768)
PHASE_TAUS = ("d", "neg", "frac", "zero", "each")


def phase_cases():
    return [f"phase-n{n}-{t}" for n in PHASE_NS for t in PHASE_TAUS]


def phase_problem(name: str) -> dict:
    _, nn, kind = name.split("-")
    n, rng = int(nn[1:]), _rng(name)
    d = max(2, n // 64)
    n_ch = 3 if kind == "each" else 2
    x = NOISE * rng.standard_normal((n, n_ch))
    x[d] += 1.0
    x = np.ascontiguousarray(x)
    tau = {"d": [d, d], "neg": [-3.0, -3.0], "frac": [d + 0.37, d + 0.37], "zero": [0.0, 0.0],
           "each": [d, -2.5, 0.5 * d + 0.25]}[kind]
    tau = np.array(tau, dtype=np.float64)
    df = FS / n
    ph = np.unwrap(np.angle(np.fft.rfft(x, axis=0)), axis=0)
    k = np.arange(len(ph))[:, None]
    shifted = ph + 2 * np.pi * k * tau[None, :] / n
    margin = np.pi - 0.5 - (np.abs(np.diff(ph, axis=0)).max(axis=0) + 2 * np.pi * np.abs(tau) / n)
    P = np.maximum(np.abs(ph).max(axis=0), np.abs(shifted).max(axis=0))
    bound = PHASE_C * U * (1.0 + np.abs(tau) + P / np.pi) / df
    return dict(x=x, n=n, d=d, tau=tau, df=df, fs=FS, margin=margin, value=(-tau / FS).astype(LD), bound=bound.astype(LD))


def wrap(x):
    return (x + np.pi) % (2 * np.pi) - np.pi


def emu_phase(p: dict, fault=None):
    """group_delay_phase(x, df, tau, fs) - group_delay_phase(x, df) with numpy, k_lat_phase's order of operations"""
    ang = np.angle(np.fft.rfft(p["x"], axis=0))
    k = np.arange(len(ang), dtype=np.float64)[:, None]
    tau = p["tau"]
    if fault == "latency_channel0":
        tau = np.full_like(tau, tau[0])
    df, fs = (p["fs"], p["df"]) if fault == "fs_df_swapped" else (p["df"], p["fs"])
    shifted = wrap(ang + (2 * np.pi) * (k * df) * (tau / fs)[None, :])

    def gd(ph):
        return -np.gradient(np.unwrap(ph, axis=0), p["df"], axis=0) / (2 * np.pi)

    return gd(shifted) - gd(ang)


def judge_phase(p: dict, diff) -> float:
    assert diff.shape == (p["n"] // 2 + 1, len(p["tau"])) and diff.dtype == np.float64
    if not np.isfinite(diff).all():
        return float("inf")
    return float(np.max(np.abs(diff.astype(LD) - p["value"][None, :]) / p["bound"][None, :]))


def phase_units(p: dict, diff) -> float:
    """the worst error in units of 2^-53 (1 + |tau| + P / pi) / df"""
    return judge_phase(p, diff) * PHASE_C


# ==== all families ==========================================================================================================
def all_cases():
    return direct_cases() + corr_cases() + pearson_cases() + [PEARSON_ENTRY] + window_cases() + phase_cases()


@functools.lru_cache(maxsize=24)
def problem(name: str) -> dict:
    fam = family(name)
    if name == PEARSON_ENTRY:
        return pearson_entry_problem()
    return {"direct": direct_problem, "corr": corr_problem, "pearson": pearson_problem, "window": window_problem,
            "phase": phase_problem}[fam](name)


PEAK_FAULTS = ("final_drop", "tie_later", "rot_off")
PEARSON_FAULTS = ("raw_moment", "means_uncut", "lag_sign", "stride_swap", "final_drop")
WINDOW_FAULTS = ("rot_off", "window_first_channel", "near_clamp")
PHASE_FAULTS = ("fs_df_swapped", "latency_channel0")
FAULTS = ("raw_moment", "means_uncut", "lag_sign", "stride_swap", "final_drop", "tie_later", "rot_off",
          "window_first_channel", "near_clamp", "fs_df_swapped", "latency_channel0")


def emulate(name: str, fault=None):
    """the case's entry in float64 numpy, in the shape judge takes"""
    p, fam = problem(name), family(name)
    if fam == "direct":
        return emu_direct_peaks(p["x"], fault)
    if fam == "corr":
        return emu_corr_peaks(p, fault)
    if name == PEARSON_ENTRY:
        peaks = emu_latency(p["td1"], p["td2"], 1, fault)[0]
        q = dict(p, rows=np.array([(0, c, len(p["td1"]) - 1 - int(peaks[c])) for c in range(3)], dtype=np.int64))
        return peaks, emu_pearson(q, fault)
    if fam == "pearson":
        return emu_pearson(p, fault)
    if fam == "window":
        return emu_latency(p["td1"], p["td2"], p["p"], fault)
    return emu_phase(p, fault)


def judge(name: str, out) -> float:
    """error / bound at worst; the exact families give 0 or infinity"""
    p, fam = problem(name), family(name)
    if fam in ("direct", "corr"):
        assert out.shape == p["expect"].shape and out.dtype == np.int64
        return 0.0 if np.array_equal(out, p["expect"]) else float("inf")
    if name == PEARSON_ENTRY:
        return judge_pearson(p, out[1]) if np.array_equal(out[0], p["expect"]) else float("inf")
    if fam == "pearson":
        return judge_pearson(p, out)
    if fam == "window":
        return judge_window(p, out)
    return judge_phase(p, out)


if __name__ == "__main__":  # prints the tables above
    worst = {}
    for case in pearson_cases() + [PEARSON_ENTRY] + window_cases() + phase_cases():
        worst[family(case)] = max(worst.get(family(case), 0.0), judge(case, emulate(case)))
    print("LATENCY_EMULATION = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in worst.items()) + "}")
    print(f"PHASE_EMULATION_UNITS = {worst['phase'] * PHASE_C:.3g}")
