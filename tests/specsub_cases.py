"""The cases of the spectral-subtraction tests: the ones tools/gen_golden_specsub.py runs through the reference
(tests/golden/specsub), and the generated shapes the GPU tests hold against the long-double oracle of specsub_oracle.py.
Signals are rebuilt from seeds: fx_cases.burst, noise at -40 dB with a tone burst over the middle third, rounded to
float32, at FS = 8000 -- so the default threshold of -40 dB gates some noise frames and not others, and the tone is never
gated.  BLOCK_S = 0.008 gives windows of 64 samples.

Every case is used only when the oracle finds no frame level within 1e-6 dB of the threshold and no bin within 1e-6 of
its clip (specsub_oracle); a case that does not is given another seed here, never skipped."""

import numpy as np

import fx_cases as fc
import specsub_oracle as so

FS = fc.FS
BLOCK_S = 0.008
W = 64
N = 700
burst = fc.burst


def given_spectrum(seed: int, scale: float = 1.0) -> np.ndarray:
    """33 values around the squared magnitude the cases' noise has under a 64-sample Hann window (1e-4 x sum w^2)."""
    return scale * 2.4e-3 * (1 + 0.5 * np.random.default_rng(seed).random(W // 2 + 1))


def quiet_second_channel(x: np.ndarray) -> np.ndarray:
    """Channel 1 a thousand times softer (exactly representable steps stay float32): a given spectrum sized for the
    noise of channel 0 then subtracts all of it."""
    y = x.copy()
    y[:, 1] = (y[:, 1] * 2.0 ** -10).astype(np.float32)
    return y


# name: (seed, n, n_ch, constructor arguments, advanced arguments); "given": the seed of a spectrum to subtract
GOLDEN = {
    "default": (801, N, 2, dict(), dict()),
    "overlap75": (802, N, 2, dict(), dict(overlap_percent=75)),
    "overlap0": (803, N, 2, dict(), dict(overlap_percent=0)),
    "overlap30": (804, N, 2, dict(), dict(overlap_percent=30)),
    "exponent1": (805, N, 2, dict(), dict(subtraction_exponent=1)),
    "exponent1p5": (806, N, 2, dict(), dict(subtraction_exponent=1.5)),
    "hamming": (807, N, 2, dict(), dict(window_type="Hamming")),
    "forgetting1": (808, N, 2, dict(), dict(noise_forgetting_factor=1)),
    "no_gate": (809, N, 2, dict(threshold_rms_dbfs=-90), dict()),
    "short": (810, 5, 2, dict(), dict()),
    "one_channel": (811, N, 1, dict(), dict()),
    "three_channels": (812, N, 3, dict(), dict()),
    "static_given": (813, N, 2, dict(adaptive_mode=False, given=91), dict(subtraction_factor=1.5)),
    "static_detector": (814, N, 2, dict(adaptive_mode=False, threshold_rms_dbfs=-20), dict()),
    "silence": (815, N, 2, dict(adaptive_mode=False, given=92, quiet=True), dict()),
}
MULTIBAND = {"bands": ((816, 817), N, 2, dict(), dict())}  # a MultiBandSignal of two bands, adaptive mode


def samples(name: str) -> np.ndarray:
    seed, n, n_ch, ctor, _ = GOLDEN[name]
    x = burst(seed, n, n_ch)
    return quiet_second_channel(x) if ctor.get("quiet") else x


def effect(fx, enums, ctor: dict, adv: dict):
    """The SpectralSubtractor of a case, for either package (`enums` holds its Window)."""
    ctor = dict(ctor)
    given = ctor.pop("given", None)
    ctor.pop("quiet", None)
    if given is not None:
        ctor["spectrum_to_subtract"] = given_spectrum(given)
    e = fx.SpectralSubtractor(block_length_s=BLOCK_S, **ctor)
    adv = dict(adv)
    if "window_type" in adv:
        adv["window_type"] = getattr(enums.Window, adv["window_type"])
    e.set_advanced_parameters(**adv)
    return e


def oracle(x, ctor: dict, adv: dict, fs: int = FS):
    """specsub_oracle.subtract of a case -> (y, gate margins, clip margins, the detector's nearest level or inf)."""
    from scipy.signal.windows import get_window
    name = adv.get("window_type", "Hann").lower()
    overlap = adv.get("overlap_percent", 50) / 100
    e = adv.get("subtraction_exponent", 2)
    given = ctor.get("given")
    window_length = W if given is not None else so.closest_power_of_2(BLOCK_S * fs)
    plain = get_window(name, window_length)
    window = np.clip(plain, a_min=1e-6, a_max=None)
    step = int(window_length * (1 - overlap))
    common = dict(threshold_db=ctor.get("threshold_rms_dbfs", -40), forgetting=adv.get("noise_forgetting_factor", 0.9),
                  factor=adv.get("subtraction_factor", 2), exponent=e)
    nearest = np.inf
    if ctor.get("adaptive_mode", True):
        out = so.subtract(x, window, step, "adaptive", env_floor=1e-4, **common)
    else:
        if given is not None:
            table = np.abs(given_spectrum(given)).astype(so.LD) ** (so.LD(e) / 2)
        else:
            table, nearest = so.detector_table(x, fs, plain, window_length, overlap * 100, common["threshold_db"],
                                               adv.get("ad_release_time_ms", 30), e)
        out = so.subtract(x, window, step, "static", table=table, **common)
    return out + (nearest,)


def conditions(gate_margins, clip_margins, nearest=np.inf, adaptive=True):
    """The two conditions on a case's inputs (and the detector's, where it runs): -> the three smallest margins."""
    gate = float(np.min(gate_margins)) if adaptive else np.inf  # (static mode has no gate)
    clip = float(np.min(np.abs(clip_margins))) if len(clip_margins) else np.inf
    assert gate > so.MARGIN_DB, ("a frame level within 1e-6 dB of the threshold", gate)
    assert clip > so.MARGIN_CLIP, ("a bin within 1e-6 of its clip", clip)
    assert nearest > 1e-9, ("a detector level within 1e-9 dB of its threshold", nearest)
    return gate, clip, nearest


# ---- generated shapes for the GPU tests ----------------------------------------------------------------------------------
WINDOWS = (4, 8, 256, 4096, 16384)  # Hann at 50 % overlap, adaptive, defaults otherwise; FLOOR alone is the bound


def edge_lengths(window: int):
    """n % step = 0, 1 and step - 1 with 5 or 6 frames."""
    step = window // 2
    return sorted({step, step + 1, 2 * step - 1})


def tile_lengths(track_tile: int, ola_tile: int):
    """W = 64, step 32: frame counts on either side of one and two tiles of k_ss_track, lengths on either side of
    k_ss_ola's."""
    step = W // 2
    frames = [track_tile - 1, track_tile, track_tile + 1, 2 * track_tile, 2 * track_tile + 1]
    return sorted({(f - 4) * step for f in frames} | {ola_tile - 1, ola_tile, ola_tile + 1})


def generated(window: int, n: int, seed_shift: int = 0):
    """(x (n, 2), window table, step) of a generated shape."""
    from scipy.signal.windows import get_window
    x = burst(900 + seed_shift + (window % 251) + n % 89, n, 2)
    return x, np.clip(get_window("hann", window), a_min=1e-6, a_max=None), window // 2
