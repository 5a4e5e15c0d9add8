"""The cases of the shoebox room tests (tests/test_room_host.py, tests/test_room_gpu.py) and of the golden generator
(tools/gen_golden_room.py): numbers only, shared so that the reference, the oracle and the device see the same inputs.

Image-source cases are the smallest shapes at which the kernels can still go wrong: one cell; 27 cells; a cube with
symmetric positions (988 of 17576 sources are replaced inside their own cell: without that rule the result is wrong by
71 % of the peak); six different walls; one large room without max_order (1.33 M sources, 166375 cells: no multiple of
the 256-lane workgroup, as no odd cube is); a small room at a low rate whose bins hold up to 1327 sources (past every
wave, workgroup and sort-tile edge of the per-bin sum) and the same room at 250 Hz (up to 4614 per bin: several id
ranges per bin, found by halving); an output shorter and one longer than the reference's buffer;
three bands in one call."""

import functools

import numpy as np

import room_oracle

GOLDEN = ("tests", "golden", "room", "cases.npz")
GOLDEN_CROSSOVER = ("tests", "golden", "room", "crossover.npz")


def sabine_alpha(dim, t60):
    dim = np.asarray(dim, dtype=np.float64)
    return 0.161 * np.prod(dim) / (np.roll(dim, 1) @ dim * 2) / t60


_ROOM = dict(dim=(5.0, 4.0, 3.0), s=(1.1, 2.3, 1.2), r=(3.7, 0.9, 1.6), alpha=0.25, t60=0.3, sr=48000)
_WALLS = dict(dim=(3.2, 2.5, 2.4), s=(0.9, 1.7, 1.1), r=(2.6, 0.8, 1.9), alpha=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6), t60=0.3,
              sr=44100, max_order=8)
# name -> dim, s, r, alpha (one or six: north south east west floor ceiling), t60, sr, max_order, n_out (None: the buffer)
ISM_CASES = {
    "order0": dict(_ROOM, max_order=0, n_out=None),
    "order1": dict(_ROOM, max_order=1, n_out=None),
    "cube": dict(dim=(4.0, 4.0, 4.0), s=(1.0, 1.0, 1.0), r=(3.0, 3.0, 3.0), alpha=sabine_alpha((4, 4, 4), 0.25), t60=0.25,
                 sr=48000, max_order=6, n_out=None),
    "walls": dict(_WALLS, n_out=None),
    "large": dict(_ROOM, max_order=None, n_out=None),
    "crowded": dict(dim=(2.0, 2.2, 2.5), s=(0.7, 1.3, 0.9), r=(1.6, 0.4, 2.1), alpha=0.3, t60=0.3, sr=2000, max_order=20,
                    n_out=None),
    "packed": dict(dim=(2.0, 2.2, 2.5), s=(0.7, 1.3, 0.9), r=(1.6, 0.4, 2.1), alpha=0.3, t60=0.3, sr=250, max_order=20,
                   n_out=None),
    "short": dict(_WALLS, n_out=1469),   # the full response has sources in bins 1468 (kept) and 1469 (dropped)
    "long": dict(_WALLS, n_out=80000),   # the buffer has int(1.1 * 0.3 * 5 * 44100) = 72765 samples
}
# what the issue counted for these shapes: sources, sources replaced inside their own cell
ISM_COUNTS = {"order0": (8, None), "order1": (216, None), "cube": (17576, 988), "large": (1331000, 1974),
              "crowded": (551368, 61136)}
# three bands of six walls each in one call (rows: bands; columns: north south east west floor ceiling)
BAND_ALPHAS = np.array([[0.10, 0.20, 0.30, 0.40, 0.50, 0.60], [0.15, 0.15, 0.35, 0.25, 0.55, 0.45],
                        [0.30, 0.30, 0.30, 0.30, 0.30, 0.30]])
INDEX_MARGIN = 1e-9  # every d / c sr + 0.5 is at least this far from an integer; its rounding error is below 2e-11


def ism_args(case):
    """backend.image_source_rir's arguments for a case."""
    n_out = case["n_out"] if case["n_out"] is not None else int(case["t60"] * 1.1 * 5 * case["sr"])
    return dict(room_dim=case["dim"], alphas=np.atleast_1d(case["alpha"])[None, :], s_pos=case["s"], r_pos=case["r"],
                t60_s=case["t60"], max_order=case["max_order"], sr=case["sr"], n_out=n_out)


@functools.lru_cache(maxsize=None)
def ism_expected(name, band=None):
    """The oracle's (rir, terms per bin, replaced sources, sources) of a case, computed once and read-only; band: a row
    of BAND_ALPHAS on the 'walls' geometry.  Asserts the index-exactness premise."""
    case = ISM_CASES[name]
    alpha = case["alpha"] if band is None else BAND_ALPHAS[band]
    rir, terms, replaced, sources, margin = room_oracle.ism_oracle(case["dim"], alpha, case["s"], case["r"], case["t60"],
                                                                  case["max_order"], case["sr"], case["n_out"])
    assert margin >= INDEX_MARGIN, f"{name}: a source lies {margin:.3g} samples from a bin edge"
    rir.setflags(write=False)
    terms.setflags(write=False)
    return rir, terms, replaced, sources


def assert_ism_close(out, name, band=None, label=None):
    """Same support, and per bin |out - oracle| <= 4 k eps oracle with k the oracle's number of terms: k - 1 additions of
    positive terms cost at most (k - 1) eps, the rest allows an ulp per term for square root, division and products.
    Prints the worst ratio of error to bound."""
    rir, terms, _, _ = ism_expected(name, band)
    out = np.asarray(out)
    assert out.shape == rir.shape
    assert np.array_equal(out != 0, rir != 0), f"{label or name}: the sets of non-zero bins differ"
    hit = rir != 0
    ratio = np.abs(out[hit] - rir[hit]) / (4 * terms[hit] * room_oracle.EPS * rir[hit])
    worst = ratio.max() if hit.any() else 0.0
    print(f"{label or name}: {int(hit.sum())} bins, up to {int(terms.max())} terms, worst error / bound {worst:.3g}")
    assert worst <= 1.0, f"{label or name}: error {worst:.3g} times the bound 4 k eps"


# ---- generate_synthetic_rir against the reference: room, positions, rate, length and switches ----------------------
RIR_ROOM = dict(dim=(3.2, 2.5, 2.4), t60=0.25, s=(0.9, 1.7, 1.1), r=(2.6, 0.8, 1.9), sr=8000, length_s=0.25)
RIR_DETAILED = dict(north=[0.10, 0.20, 0.30], south=0.25, east=[0.30, 0.15], west=[0.20, 0.25, 0.35], floor=[0.40, 0.30, 0.20],
                    ceiling=0.5)
RIR_SEED = 1234
RIR_PATHS = {"plain": {}, "bandpass": dict(apply_bandpass=True), "noise": dict(add_noise_reverberant_tail=True),
             "detailed": dict(use_detailed_absorption=True, max_order=4)}

# ---- ShoeboxRoom attributes ------------------------------------------------------------------------------------------
ABSORPTION_SETS = {
    "short": dict(north=[0.1, 0.2, 0.3], south=0.25, east=[0.3, 0.15], west=[0.2, 0.25, 0.35], floor=[0.4, 0.3, 0.2],
                  ceiling=0.5),
    "scalar": dict(north=0.1, south=0.2, east=0.3, west=0.4, floor=0.5, ceiling=0.6),
    "eight": {w: list(np.linspace(0.05 + 0.05 * i, 0.4 + 0.05 * i, 8)) for i, w in
              enumerate(("north", "south", "east", "west", "floor", "ceiling"))},
}

# ---- the modal response ----------------------------------------------------------------------------------------------
MODAL_ROOM = dict(dim=(5.0, 4.0, 3.0), t60=0.6, s=(1.1, 2.3, 1.2), r=(3.7, 0.9, 1.6))
MODAL_ORDERS = (1, 3, 10)


def modal_freqs():
    """257 frequencies from 20 to 300 Hz, one of them 5e-4 Hz above the (1, 0, 0) mode at 343 / 2 / 5 = 34.3 Hz."""
    f = np.linspace(20.0, 300.0, 257)
    f[np.argmin(np.abs(f - 34.3))] = 34.3 + 5e-4
    return f


# ---- the crossover bank ------------------------------------------------------------------------------------------------
SOS_CASES = {"o2": (2, 1000.0, 48000), "o3": (3, 700.0, 16000), "o4": (4, 2500.0, 44100), "o12": (12, 125 * 2 ** 0.5, 8000)}
BANK = dict(freqs=(300.0, 1200.0, 3500.0), order=(4, 2, 3), sr=16000)  # three crossovers: the all-pass states are shared


def bank_signal():
    """(3000, 2) noise, the same in the generator and in the tests."""
    return np.random.default_rng(7).standard_normal((3000, 2)) * 0.2
