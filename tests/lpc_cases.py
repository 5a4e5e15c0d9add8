"""The problems of the linear-prediction sweep (tests/test_lpc_sweep_host.py, tests/test_lpc_sweep_gpu.py), built
without a device, and their oracle.

Every builder is pure numpy with a fixed seed.  The case tables are laid out against csrc/kernels_lpc.hpp: the lag
groups of k_lpc_yw (KB = 4 lags per wave, 16 per sweep), the four 64-lag register chunks of levinson_wave, the lane per
coefficient of k_lpc_burg, the four states per lane and the 64-sample blocks of k_lpc_filter, the row stride of
ds_lpc_dev, the singular flag of k_levinson, and the largest LDS either estimator declares.

Signals are white noise, and the same noise through lfilter([1], [1, -0.9, 0.5]) (poles at radius 0.71: the recursions
have a spectrum to fit and stay well conditioned), rounded through float32 so that the float64 host entry and the
float32 resident entries see the same samples.  The oracle is tests/lpc_oracle.py as it is, run in long double (x87,
80 bit); ORACLE_DTYPE falls back to float64, and says so, where long double is no wider than that.  Oracles are cached
per problem: the host float64, resident and strided entries of a problem share one."""

import numpy as np
from scipy.signal import get_window, lfilter

import lpc_oracle as lo

if np.finfo(np.longdouble).eps < 1e-18:
    ORACLE_DTYPE = np.longdouble
else:  # (a platform whose long double is float64 or double-double)
    ORACLE_DTYPE = np.float64
    print("lpc_cases: np.longdouble is not an 80-bit type here; the oracle falls back to float64")

KINDS = ("white", "coloured")
METHODS = ("yw", "burg")  # backend.LPC_METHODS in the same order
COLOUR = [1.0, -0.9, 0.5]
PAD = 13  # floats behind every row of the strided ds_lpc_dev call

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def hann(L):
    """The periodic Hann window transforms.lpc hands to the entries."""
    return get_window("hann", L, fftbins=True)


def signal(kind, n, n_ch, seed, silent=None):
    """(n, n_ch) float32; `silent`: a channel of zeros."""
    x = np.random.default_rng(seed).standard_normal((n, n_ch))
    if kind == "coloured":
        x = lfilter([1.0], COLOUR, x, axis=0)
    else:
        assert kind == "white"
    if silent is not None:
        x[:, silent] = 0.0
    return x.astype(np.float32)


# ---- estimator problems ----------------------------------------------------------------------------------------------
def _est(name, L, hop, order, n_ch, n=3000, kinds=KINDS, silent=None, burg_order=None):
    # Burg keeps tools/gen_golden_lpc.py's rule order <= L // 4 (beyond it the recursion itself loses its digits);
    # burg_order: the order Burg runs at where the case's own breaks that rule
    b = order if burg_order is None else burg_order
    methods = ("yw", "burg") if b <= L // 4 else ("yw",)
    return dict(name=name, L=L, hop=hop, order=order, n_ch=n_ch, n=n, kinds=kinds, silent=silent, burg_order=b,
                methods=methods, seed=7919 * L + 31 * order + n_ch)


CHUNK_ORDERS = (127, 129, 130, 191, 192, 193, 194, 254, 255)
ESTIMATOR_CASES = (
    # lag-group edges of k_lpc_yw: 3, 4, 5, 16, 17 lags; a window that is no multiple of 64 or 256; pair % 5; 82 frames,
    # the last of which has 3 of its 100 samples
    [_est(f"lags_o{o}", 100, 37, o, 5) for o in (2, 3, 4, 15, 16)]
    # lane-chunk edges of levinson_wave and the waves 1 .. 3 of k_lpc_burg's coefficient update.  Step m of the
    # recursion updates the lags below m, so chunk upd[q] is first written at order 64 q + 2: 130 and 194 are the
    # smallest orders that need upd[2] and upd[3]
    + [_est(f"chunks_o{o}", 1024, 512, o, 2) for o in CHUNK_ORDERS]
    + [_est("quarter_window", 1020, 510, 255, 2),          # order = L / 4 exactly, L no multiple of 256
       _est("largest_lds", 8192, 8192, 255, 1, n=20000),   # 72 KB (Yule-Walker) and 135 KB (Burg) of LDS
       _est("long_window", 8192, 4096, 17, 2, n=20000),
       _est("smallest", 2, 1, 1, 2),                        # two lags, a window of [0, 1]; the last frame is silent
       _est("mostly_zeros", 64, 64, 8, 2, n=40),            # one frame, 40 of its 64 samples
       # 70000 workgroups (past 65535); the last frame holds one sample times w[0] = 0: silent
       _est("many_pairs", 8, 1, 2, 1, n=70000, kinds=("coloured",)),
       # a channel of zeros between two live ones: NaN (Yule-Walker), [1, 0, ...] and 0 (Burg, at order L / 4)
       _est("silent_channel", 256, 128, 129, 3, silent=1, burg_order=64)])
ESTIMATOR_RUNS = [(c["name"], k) for c in ESTIMATOR_CASES for k in c["kinds"]]
_BY_NAME = {c["name"]: c for c in ESTIMATOR_CASES}


def estimator_case(name):
    return _BY_NAME[name]


def order_of(case, method):
    return case["burg_order"] if method == "burg" else case["order"]


def case_signal(case, kind):
    return cached(("sig", case["name"], kind),
                  lambda: signal(kind, case["n"], case["n_ch"], case["seed"], case["silent"]))


def strided_rows(x32, pad=PAD):
    """(n, n_ch) float32 -> (n_ch, n + pad) float32 rows, the padding NaN."""
    rows = np.full((x32.shape[1], x32.shape[0] + pad), np.nan, dtype=np.float32)
    rows[:, :x32.shape[0]] = x32.T
    return rows


def estimate(td, order, method, dtype):
    """(a of order + 1 rows, var) of windowed frames (L, frames, channels)."""
    if method == "yw":
        a, var, singular = lo.yule_walker(td, order, dtype)
        assert not singular
        return a, var
    return lo.burg(td, order, dtype)


def estimator_oracle(case, kind, method, dtype=None):
    dtype = ORACLE_DTYPE if dtype is None else dtype

    def make():
        td = lo.windowed_frames(case_signal(case, kind), hann(case["L"]), case["hop"])
        return estimate(td, order_of(case, method), method, dtype)
    return cached(("est", case["name"], kind, method, np.dtype(dtype).name), make)


# ---- Levinson-Durbin problems ----------------------------------------------------------------------------------------
LEVINSON_ORDERS = (64, 65, 66, 128, 129, 130, 192, 193, 194, 255)  # (64 q + 2: the first to write upd[q])
LEVINSON_COLUMNS = (1, 300)
LEVINSON_L, LEVINSON_HOP = 1024, 512
SINGULAR_ORDER, SINGULAR_COLUMNS, SINGULAR_AT = 130, 70, 69


def levinson_r():
    """(256, 300) float64: the long-double biased autocorrelations, lags 0 .. 255, of the frames (6 frames x 2
    channels) of the coloured L = 1024 signal drawn from 25 seeds."""
    def make():
        cols = []
        for seed in range(25):
            td = lo.windowed_frames(signal("coloured", 3000, 2, 4001 + seed), hann(LEVINSON_L), LEVINSON_HOP)
            cols.append(lo.autocorrelation(td, max(LEVINSON_ORDERS), ORACLE_DTYPE).reshape(max(LEVINSON_ORDERS) + 1, -1))
        r = np.concatenate(cols, axis=1).astype(np.float64)
        assert r.shape == (256, 300)
        return r
    return cached("levinson_r", make)


def levinson_problem(order, n_cols):
    return np.ascontiguousarray(levinson_r()[:order + 1, :n_cols])


def levinson_oracle(order, n_cols, dtype=None):
    """(a, var, singular) of levinson_problem(order, n_cols)."""
    dtype = ORACLE_DTYPE if dtype is None else dtype
    return cached(("lev", order, n_cols, np.dtype(dtype).name),
                  lambda: lo.levinson(levinson_problem(order, n_cols), dtype))


def singular_problem():
    """70 columns at order 130; column 69 is r = [1, 0, ..., 0, 1]: every reflection coefficient is 0 until the last,
    which is -1, so the prediction error reaches 0 at the last step only."""
    r = levinson_problem(SINGULAR_ORDER, SINGULAR_COLUMNS).copy()
    r[:, SINGULAR_AT] = 0.0
    r[0, SINGULAR_AT] = r[SINGULAR_ORDER, SINGULAR_AT] = 1.0
    return r


def singular_oracle(dtype=None):
    dtype = ORACLE_DTYPE if dtype is None else dtype
    return cached(("singular", np.dtype(dtype).name), lambda: lo.levinson(singular_problem(), dtype))


# ---- synthesis problems ----------------------------------------------------------------------------------------------
A0_SCALES = (2.0, -0.5, 1.0, 3.0, -0.125)


def _syn(name, order, L, n_frames, n_ch, hop=None, n_out=None, scaled=False):
    hop = L // 2 if hop is None else hop
    total = (n_frames - 1) * hop + L
    return dict(name=name, order=order, L=L, n_frames=n_frames, n_ch=n_ch, hop=hop, total=total,
                n_out=total if n_out is None else n_out, scaled=scaled, seed=104729 + 101 * L + order + 7 * n_frames)


SYNTHESIS_CASES = (
    # the four states per lane of k_lpc_filter: one lane, lanes 0 .. 1, 15 .. 16, and the last lane's live[] edge;
    # 5 pairs: the second workgroup holds one wave
    [_syn(f"orders_o{o}", o, 1024, 5, 1) for o in (1, 3, 4, 5, 63, 64, 65, 252, 253, 254, 255)]
    # its 64-sample blocks: one short of a block, one past it, two past two
    + [_syn(f"blocks_L{L}_o{o}", o, L, 3, 2) for L in (63, 65, 130) for o in (3, 5)]
    + [_syn("one_pair", 255, 1024, 1, 1),
       _syn("seven_pairs", 255, 1024, 7, 1),               # the last workgroup holds 3 of its 4 waves
       _syn("scaled_a0", 65, 1024, 5, 1, scaled=True),     # a and sources times a0 per pair: the same output
       # the overlap-add, order 5, 3 channels
       _syn("ola_gaps", 5, 100, 4, 3, hop=130),            # hop > L: the samples between two frames are exactly 0
       _syn("ola_hop1", 5, 100, 20, 3, hop=1),
       _syn("ola_padded", 5, 100, 4, 3, hop=50, n_out=300),   # 50 past the last frame: exactly 0
       _syn("ola_trimmed", 5, 100, 4, 3, hop=50, n_out=120),  # shorter than the frames
       _syn("ola_floor", 5, 100, 4, 3, hop=100)])          # no overlap: w[0] = 0 and its neighbours divide by 1e-4
SYNTHESIS_NAMES = [c["name"] for c in SYNTHESIS_CASES]
_SYN_BY_NAME = {c["name"]: c for c in SYNTHESIS_CASES}


def synthesis_case(name):
    return _SYN_BY_NAME[name]


def synthesis_problem(case):
    """(a float64 (order + 1, frames, channels), sources float64 (L, frames, channels), window).  a is the long-double
    Yule-Walker answer for the frames of a coloured signal (the biased autocorrelation makes it minimum phase: the
    filters are stable), the sources are standard normal deviates.  Unscaled: a[0] = 1."""
    def make():
        L, n_frames, n_ch = case["L"], case["n_frames"], case["n_ch"]
        own_hop = L // 2  # (the frames a was estimated from; the case's hop is the overlap-add's)
        x = signal("coloured", n_frames * own_hop, n_ch, case["seed"])
        td = lo.windowed_frames(x, hann(L), own_hop)
        assert td.shape == (L, n_frames, n_ch)
        a, _ = estimate(td, case["order"], "yw", ORACLE_DTYPE)
        a = a.astype(np.float64)
        assert np.isfinite(a).all() and (a[0] == 1.0).all()
        src = np.random.default_rng(case["seed"] + 1).standard_normal((L, n_frames, n_ch))
        return a, src, hann(L)
    return cached(("syn", case["name"]), make)


def a0_scales(case):
    """(frames, channels): A0_SCALES over the pairs."""
    n = case["n_frames"] * case["n_ch"]
    return np.resize(np.array(A0_SCALES), n).reshape(case["n_frames"], case["n_ch"])


def synthesis_inputs(case):
    """What the entry is handed: synthesis_problem, with a and the sources of every pair times its a0 where the case
    is the scaled one."""
    a, src, window = synthesis_problem(case)
    if case["scaled"]:
        s = a0_scales(case)
        a, src = a * s, src * s
    return a, src, window


def synthesis_oracle(case, dtype=None):
    """(filtered frames (L, frames, channels), output (n_out, channels)) of the UNSCALED problem."""
    dtype = ORACLE_DTYPE if dtype is None else dtype

    def make():
        a, src, window = synthesis_problem(case)
        filtered = lo.all_pole(a, src, dtype)
        return filtered, lo.overlap_add(filtered, window, case["hop"], case["n_out"], dtype)
    return cached(("syn_oracle", case["name"], np.dtype(dtype).name), make)


def uncovered(case):
    """The output samples no frame covers (between frames where hop > L, past the last frame): exactly 0."""
    n = np.arange(case["n_out"])
    return (n % case["hop"] >= case["L"]) | (n >= case["total"])
