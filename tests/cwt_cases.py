"""The cases of the wavelet-transform sweep (tests/test_cwt_sweep_host.py, tests/test_cwt_sweep_gpu.py): the plan of
`cwt_run` / `ds_cwt` (csrc/api.hip) restated in plain Python, the wavelets and signals the tests draw, and the case lists.
Pure numpy, no device.  Every case carries the edge it is there for as a predicate on plan(); the host test checks that
each case meets its predicate and that the constants below are the sources'.

A wavelet of L taps on n samples: h = (L - 1) // 2, cropped to the taps k in [h - n + 1, h + n - 1] (lc of them, hc = h
minus what was cut at the front), class M = max(MIN_M, 2^ceil(log2(2 lc))).  A class: cc = max(lc - 1 - hc), hmax =
max(hc), V = M - hmax - cc valid outputs per block, n_blocks = ceil(n / V); LDS route up to MAX_LDS_M, four-step beyond,
where the inverse walks n_items = nf * n_blocks * n_ch in chunks.  The host entry computes `rows` frequencies per pass.

hc = min(h, n - 1) and lc - 1 - hc = min(L - 1 - h, n - 1) both grow with L, so the longest wavelet of a class always
attains both maxima: hmax and cc cannot come from two wavelets that exclude each other.  What a class of both parities does
reach is cc = hmax + 1 (set by an even length, cc_f = h_f + 1) beside an odd wavelet that attains hmax with cc_f = h_f < cc:
mixed_parity() below, the predicate of the block-edge classes."""

from dataclasses import dataclass
from typing import Callable

import numpy as np

from dsptoolbox_amd.transforms import MorletWavelet, Wavelet
from dsptoolbox_amd.transforms._wavelets import _normalised_wavelets

# csrc/kernels_cwt.hpp
MIN_M, MAX_LDS_M, MAX_TAPS, BIG_N1 = 256, 16384, 1 << 18, 1024
# csrc/api.hip: cwt_run's four-step column buffer, the largest grid dimension, ds_cwt's device scalogram per pass
BIG_STAGE_BYTES, GRID_Y_MAX, HOST_PASS_BYTES = 256 << 20, 65535, 512 << 20

TOL = 1e-6  # every row within TOL * max_t |x_c|


def wavelet_plan(L: int, n: int) -> dict:
    h = (L - 1) // 2
    k0, k1 = max(0, h - n + 1), min(L - 1, h + n - 1)
    lc = k1 - k0 + 1
    m = MIN_M
    while m < 2 * lc:
        m *= 2
    return dict(L=L, k0=k0, lc=lc, hc=h - k0, M=m)


def plan(lengths, n: int, n_ch: int) -> dict:
    """cwt_run for one call with these wavelets (for the host entry: one frequency pass; `passes` lists them, and a
    pass's classes are plan(lengths[f0:f0 + nr], n, n_ch))."""
    wav = [wavelet_plan(int(L), n) for L in lengths]
    classes = {}
    for m in sorted({w["M"] for w in wav}):
        idx = [i for i, w in enumerate(wav) if w["M"] == m]
        cc = max(wav[i]["lc"] - 1 - wav[i]["hc"] for i in idx)
        hmax = max(wav[i]["hc"] for i in idx)
        v = m - hmax - cc
        n_blocks = -(-n // v)
        big = m > MAX_LDS_M
        n_items = len(idx) * n_blocks * n_ch
        chunk = min(n_items, GRID_Y_MAX, max(1, BIG_STAGE_BYTES // (8 * m))) if big else 0
        classes[m] = dict(idx=idx, cc=cc, hmax=hmax, V=v, n_blocks=n_blocks, route="four-step" if big else "lds",
                          n_items=n_items, chunk=chunk, j0=[wav[i]["hc"] + cc for i in idx])
    rows = max(1, min(len(wav), HOST_PASS_BYTES // (8 * n * n_ch)))
    passes = [(f0, min(rows, len(wav) - f0)) for f0 in range(0, len(wav), rows)]
    return dict(wavelets=wav, classes=classes, rows=rows, passes=passes)


def mixed_parity(p: dict, m: int) -> bool:
    """class m: cc is one more than hmax (an even length sets it) and an odd wavelet attains hmax with its own
    L - 1 - h below cc"""
    c = p["classes"][m]
    w = [p["wavelets"][i] for i in c["idx"]]
    return c["cc"] == c["hmax"] + 1 and any(v["hc"] == c["hmax"] and v["lc"] - 1 - v["hc"] < c["cc"] for v in w)


# ---- wavelets ---------------------------------------------------------------------------------------------------------
class Taps(Wavelet):
    """A wavelet of exactly int(f) random complex taps, seeded by the length; a fractional part of f (in 1/1024) seeds
    another wavelet of the same length."""

    def get_wavelet(self, f, fs):
        n = int(f)
        rng = np.random.default_rng(n if f == n else int(round(f * 1024)))
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)


class LevelBank(Wavelet):
    """The wavelets of the level cases: MorletWavelet(h=3, step=1e-3) below LEVEL_TAPS "Hz", Taps of that length at it."""

    def __init__(self):
        super().__init__()
        self.morlet = MorletWavelet(h=3, step=1e-3)

    def get_wavelet(self, f, fs):
        return Taps().get_wavelet(f, fs) if f == LEVEL_TAPS else self.morlet.get_wavelet(f, fs)


def normalised(wavelet, freqs, fs):
    """the taps transforms.cwt hands to the backend (sum of magnitudes 1), float64"""
    return _normalised_wavelets(wavelet, freqs, fs)


# ---- signals ----------------------------------------------------------------------------------------------------------
MAX_CH = 5


def signal(n: int, n_ch: int = MAX_CH, seed: int = 0) -> np.ndarray:
    """(n, n_ch) float64 holding float32 values; the first columns of a wider signal of the same n and seed are the same
    numbers"""
    rng = np.random.default_rng(9100 + 17 * seed + n)
    return rng.standard_normal((n, MAX_CH)).astype(np.float32).astype(np.float64)[:, :n_ch].copy()


def level_signal(levels_db, n: int, fs: int) -> np.ndarray:
    """(n, len(levels_db)) float32-valued float64: channel c is a sine of its own frequency plus 1 % noise, at
    levels_db[c] dB re full scale; None: all zeros"""
    rng = np.random.default_rng(4242)
    t = np.arange(n) / fs
    x = np.zeros((n, len(levels_db)))
    for c, db in enumerate(levels_db):
        tone = np.sin(2 * np.pi * LEVEL_TONES[c] * t + 0.3 * c) + 0.01 * rng.standard_normal(n)
        if db is not None:
            x[:, c] = 10.0 ** (db / 20.0) * tone
    return x.astype(np.float32).astype(np.float64)


# ---- oracles ----------------------------------------------------------------------------------------------------------
def direct_scalogram(td: np.ndarray, waves) -> np.ndarray:
    """S[f, t, c] = sum_k w_f[k] x_c[t + (L_f - 1) // 2 - k] as a float64 sum over the taps (short wavelets)"""
    n = td.shape[0]
    out = np.zeros((len(waves), n, td.shape[1]), dtype=np.complex128)
    for f, w in enumerate(waves):
        out[f] = direct_row(td, w)
    return out


def direct_row(td: np.ndarray, w: np.ndarray) -> np.ndarray:
    n, h = td.shape[0], (len(w) - 1) // 2
    row = np.zeros(td.shape, dtype=np.complex128)
    for k, wk in enumerate(w):
        s = h - k  # row[t] += wk x[t + s]
        lo, hi = max(0, -s), min(n, n - s)
        if lo < hi:
            row[lo:hi] += wk * td[lo + s:hi + s]
    return row


def row_ratios(S, ref, td) -> np.ndarray:
    """(F, C): max_t |S - ref| / (TOL max_t |x_c|) of every row and channel, every element counted; a silent channel is
    held to a peak of 1 here and to exact zeros by its own test"""
    peak = np.abs(td).max(axis=0)
    peak = np.where(peak == 0, 1.0, peak)
    return np.abs(S - ref).max(axis=1) / (TOL * peak[None, :])


# ---- cases ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    lengths: tuple       # the wavelets: Taps lengths (LevelBank frequencies for the level cases)
    n: int
    channels: tuple      # the channel counts the case runs at
    edge: Callable       # plan(lengths, n, n_ch) -> bool: the edge the case is there for
    why: str


# block edges on the LDS route: one class per M, four wavelets, N on either side of one and of two blocks
LDS_MS = [256, 512, 1024, 2048, 4096, 8192, 16384]
BLOCK_CHANNELS = (1, 2, 3, 5)
BLOCK_EDGES = [(1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1)]  # n = k V + d


def block_lengths(m: int) -> tuple:
    """the longest of the class (even), its odd neighbour (attains hmax), an even one in between, the shortest"""
    lo = 1 if m == MIN_M else m // 4 + 1
    mid = (lo + m // 2) // 2
    return (m // 2, lo, mid + (mid & 1), m // 2 - 1)


def block_v(m: int) -> int:
    return m - (m // 4 - 1) - m // 4  # hmax = M/4 - 1, cc = M/4


def block_cases():
    out = []
    for m in LDS_MS:
        for k, d in BLOCK_EDGES:
            n = k * block_v(m) + d

            def edge(p, m=m, k=k, d=d, n=n):
                c = p["classes"]
                return (list(c) == [m] and c[m]["route"] == "lds" and len(c[m]["idx"]) == 4 and n == k * c[m]["V"] + d
                        and c[m]["n_blocks"] == k + (d > 0) and mixed_parity(p, m)
                        and all(w["k0"] == 0 and w["lc"] == w["L"] for w in p["wavelets"]))

            out.append(Case(f"block-M{m}-{k}V{d:+d}", block_lengths(m), n, BLOCK_CHANNELS, edge,
                            "n = k V + d of one LDS class of both parities, uncropped"))
    return out


# every class boundary in one call, on signals short enough to crop most of the wavelets
MIXED_NS = [1, 2, 257, 1000]
MIXED_CHANNELS = (1, 3)


def mixed_lengths(n: int) -> tuple:
    return (1, 2, 3, 4, 127, 128, 129, 130, 255, 256, 257, 511, 512, 513, 4096, 4097, 8192, 8193, 8194, 5 * n + 1, 5 * n + 2)


def mixed_cases():
    out = []
    for n in MIXED_NS:
        def edge(p, n=n):
            w = p["wavelets"]
            cropped = [v for v in w if v["lc"] < v["L"]]
            want = {1: [256], 2: [256], 257: [256, 512, 1024, 2048], 1000: [256, 512, 1024, 2048, 4096]}[n]
            return (len(cropped) >= 2 and all(v["lc"] == 2 * n - 1 and v["hc"] == n - 1 for v in w if v["L"] >= 2 * n + 1)
                    and (n < 257 or any(v["lc"] == v["L"] for v in w)) and list(p["classes"]) == want
                    and all(c["n_blocks"] >= 1 and c["V"] >= 1 for c in p["classes"].values())
                    and (n < 257 or max(c["n_blocks"] for c in p["classes"].values()) > 1))

        out.append(Case(f"mixed-N{n}", mixed_lengths(n), n, MIXED_CHANNELS, edge,
                        "lengths on both sides of every class boundary, cropped and uncropped wavelets in one call"))
    return out


# the four-step route at every M it is built for: two blocks, the second holding one sample
BIG_MS = [1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19]
BIG_CHANNELS = (1, 2, 3)


def big_cases():
    out = []
    for m in BIG_MS:
        n = block_v(m) + 1

        def edge(p, m=m, n=n):
            c = p["classes"]
            return (list(c) == [m] and c[m]["route"] == "four-step" and c[m]["n_blocks"] == 2 and n == c[m]["V"] + 1
                    and c[m]["chunk"] == c[m]["n_items"])  # one chunk: the chunk cases are CHUNK_*

        out.append(Case(f"four-step-M{m}", (m // 2, m // 4 + 1), n, BIG_CHANNELS, edge,
                        "the four-step route at this M, two blocks, the last holding one sample"))
    return out


# the four-step inverse's item chunks entered twice
def _chunk_one_block():
    n = 98304
    lengths = tuple(range((1 << 18) - 12, (1 << 18) + 1))

    def edge(p):
        c = p["classes"]
        m = 1 << 19
        return (list(c) == [m] and c[m]["n_blocks"] == 1 and c[m]["chunk"] == 64 and c[m]["n_items"] == 65
                and all(w["lc"] == 2 * n - 1 for w in p["wavelets"]) and len(p["passes"]) == 1)

    return Case("chunk-one-block", lengths, n, (5,), edge, "65 items against a chunk of 64 at M = 2^19: item0 > 0")


def _chunk_blocks():
    lengths = tuple(range(32743, 32769))
    n = 3 * block_v(1 << 16) + 1

    def edge(p):
        c = p["classes"]
        m = 1 << 16
        if list(c) != [m]:
            return False
        q = c[m]
        fb, ch = divmod(q["chunk"], 5)  # the first item of the second chunk
        return (q["n_blocks"] == 4 and n == 3 * q["V"] + 1 and q["chunk"] == 512 and q["n_items"] == 520 and ch != 0
                and fb % q["n_blocks"] != 0 and len(p["passes"]) == 1)

    return Case("chunk-blocks", lengths, n, (5,), edge,
                "520 items against a chunk of 512 at M = 2^16; the boundary falls inside one block's channels")


CHUNK_ONE_BLOCK, CHUNK_BLOCKS = _chunk_one_block(), _chunk_blocks()


# the host entry's frequency passes entered twice: 44 distinct wavelets of 1 ... 9 taps
def _passes():
    n, n_f = 1 << 19, 44
    freqs = tuple(1 + i % 9 + (i + 1) / 1024 for i in range(n_f))

    def edge(p):
        return p["rows"] == 42 and p["passes"] == [(0, 42), (42, 2)] and n_f > p["rows"] and list(p["classes"]) == [MIN_M]

    return Case("host-passes", freqs, n, (3,), edge, "44 frequencies against 42 rows per pass: f0 > 0")


PASSES = _passes()

# channel selection, both entries against the oracle's gathered columns
SELECT_N, SELECT_CH, SELECT_LENGTHS = 3001, 5, (3, 130, 4097)
SELECTIONS = [[2, 0], [1, 1, 0], [4], None]

# channel levels and silent channels
LEVEL_N, LEVEL_FS, LEVEL_TAPS = 20000, 16000, 8193
LEVEL_FREQS = (80.0, 300.0, 1200.0, float(LEVEL_TAPS))
LEVEL_TONES = (440.0, 1310.0, 97.0, 2750.0, 620.0)  # per channel, Hz
LEVEL_SETS = [(0, -40), (0, -80), (0, -120), (0, -60, -120), (0, -120, -40, -80)]  # dB, each also reversed
SILENT_SETS = [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (5, 0), (5, 2), (5, 4)]  # (channels, the silent one)


def level_lengths() -> tuple:
    return tuple(len(w) for w in normalised(LevelBank(), LEVEL_FREQS, LEVEL_FS))


def level_edge(p) -> bool:
    c = p["classes"]
    routes = [q["route"] for q in c.values()]
    blocks = [q["n_blocks"] for q in c.values()]
    # odd and even block counts on the LDS route, and a single block (its partner all zeros) on the four-step route
    return (len(c) == 4 and routes == ["lds"] * 3 + ["four-step"] and min(blocks[:3]) >= 2 and blocks[3] == 1
            and any(b % 2 for b in blocks[:3]) and any(b % 2 == 0 for b in blocks[:3]))


ALL_PLANNED = block_cases() + mixed_cases() + big_cases() + [CHUNK_ONE_BLOCK, CHUNK_BLOCKS, PASSES]
