"""The cases of the audio-effects tests: the ones tools/gen_golden_fx.py runs through the reference (tests/golden/fx),
and the generated shapes the GPU tests hold against the long-double oracle of fx_oracle.py.  Signals are rebuilt from
seeds: a tone burst over low noise, rounded to float32, at FS = 8000, so that a compressor meets attack, release and all
three sections of its knee curve."""

import numpy as np

FS = 8000


def burst(seed: int, n: int, n_ch: int, level: float = 0.8, noise: float = 0.01) -> np.ndarray:
    """(n, n_ch) float64 holding float32 values: noise, and a tone over the middle third (channel c a little softer and
    at another frequency)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = noise * rng.standard_normal((n, n_ch))
    lo, hi = n // 3, max(n // 3 + 1, 2 * n // 3)
    for c in range(n_ch):
        x[lo:hi, c] += level / (1 + 0.5 * c) * np.sin(2 * np.pi * (440 + 130 * c) / FS * t[lo:hi] + 0.3 * c)
    if n < 8:  # (the shortest shapes have no room for a burst: keep them away from silence)
        x += 0.3 * rng.standard_normal((n, n_ch))
    return x.astype(np.float32).astype(np.float64)


# ---- golden cases: {name: (seed, n, n_ch, parameters)} ---------------------------------------------------------------
COMPRESSOR = {
    "default": (11, 420, 2, dict()),
    "knee_up_abs": (12, 420, 2, dict(threshold_dbfs=-14, attack_time_ms=1.0, release_time_ms=30, ratio=4, relative=False,
                                     knee_db=6, pre_gain_db=3, post_gain_db=-2, make_up=False, downward=False)),
    "attack0_knee": (13, 500, 1, dict(threshold_dbfs=-12, attack_time_ms=0.0, release_time_ms=50, ratio=8, knee_db=4,
                                      pre_gain_db=-1.5, post_gain_db=4)),
    "up_hard": (14, 420, 3, dict(threshold_dbfs=-20, attack_time_ms=2.0, release_time_ms=10, ratio=2, downward=False)),
}
# the case each deliberately wrong oracle is shown on (it must miss BOUND by a wide margin there)
WRONG_ORACLES = {"swap": "default", "knee": "attack0_knee", "post": "attack0_knee"}

DETECTOR = {  # channel 0 of the burst
    "relative": (21, 500, 2, dict(threshold_dbfs=-20, relative=True, release_time_ms=25)),
    "absolute": (22, 500, 1, dict(threshold_dbfs=-30, relative=False, release_time_ms=5)),
    "release0": (23, 300, 1, dict(threshold_dbfs=-25, relative=True, release_time_ms=0)),
    "empty": (24, 300, 1, dict(threshold_dbfs=-0.5, relative=False, release_time_ms=25)),
}

DELAY = {
    "digital": (31, 300, 2, dict(delay_ms=10, feedback=0.4, saturation="digital")),
    "arctan": (32, 300, 2, dict(delay_ms=3.3, feedback=0.1, saturation="arctan")),
}

# voices: (depth ms, base delay ms, LFO frequency, waveform, random phase, smooth); `seed` precedes the apply
CHORUS = {
    "default": (41, 700, 2, dict(voices=None, mix_percent=100, seed=5)),
    "three": (42, 700, 2, dict(voices=[(2, 5, 1.5, "harmonic", True, 0), (3, 8, 3.0, "triangle", True, 0),
                                       (4, 12, 0.7, "sawtooth", True, 0)], mix_percent=60, seed=6)),
    "negative": (43, 500, 1, dict(voices=[(8, 3, 6.0, "sawtooth", False, 0)], mix_percent=85, seed=7)),
}

# kinds, levels dB, mix percent, offsets dB, post gain dB
DISTORTION = {
    "arctan": (51, 300, 2, dict(kinds=["Arctan"], levels=[20], mix=[100], offsets=[-np.inf], post=0)),
    "hard": (52, 300, 2, dict(kinds=["HardClip"], levels=[12], mix=[70], offsets=[-np.inf], post=2)),
    "soft": (53, 300, 2, dict(kinds=["SoftClip"], levels=[6], mix=[100], offsets=[-20], post=0)),
    "clean": (54, 300, 1, dict(kinds=["NoDistortion"], levels=[0], mix=[40], offsets=[-np.inf], post=-3)),
    "combined": (55, 300, 2, dict(kinds=["Arctan", "HardClip", "SoftClip", "NoDistortion"], levels=[25, 10, 4, 0],
                                  mix=[50, 0, 30, 20], offsets=[-12, -np.inf, -30, -np.inf], post=1.5)),
}

# depth, LFO frequency, waveform, random phase, smooth, seed
TREMOLO = {f"{w}_{'smooth' if s else 'plain'}": (60 + i, 400, 2, dict(depth=0.3 + 0.1 * i, freq=30.0 + 7 * i, waveform=w,
                                                                        random_phase=bool(i % 2), smooth=s, seed=70 + i))
           for i, (w, s) in enumerate((w, s) for w in ("harmonic", "sawtooth", "square", "triangle") for s in (0, 5))}

LFOS = [(2.0, "harmonic", True, 0, 100, 1), (35.0, "sawtooth", True, 0, 300, 2), (35.0, "sawtooth", True, 3, 300, 3),
        (50.0, "square", False, 0, 250, 4), (50.0, "square", True, 4, 250, 5), (20.0, "triangle", True, 0, 300, 6),
        (20.0, "triangle", False, 6, 300, 7), (("eighth 3", 90), "harmonic", False, 0, None, 8)]  # (.., length, seed)
RHYTHMS = [("quarter", 120), ("half dotted", 90), ("eighth 3", 100.0), ("whole", 60), ("sixteenth", 140), ("32th", 80),
           ("quintuplet", 75)]


# ---- the effects of a case, for either package (the reference or this one) -------------------------------------------
def compressor(fx, p):
    e = fx.Compressor(p.get("threshold_dbfs", -10), p.get("attack_time_ms", 0.5), p.get("release_time_ms", 20),
                      p.get("ratio", 3), p.get("relative", True))
    e.set_advanced_parameters(knee_factor_db=p.get("knee_db", 0), pre_gain_db=p.get("pre_gain_db", 0),
                              post_gain_db=p.get("post_gain_db", 0), automatic_make_up_gain=p.get("make_up", True),
                              downward_compression=p.get("downward", True))
    return e


def delay(fx, p):
    e = fx.DigitalDelay(p["delay_ms"], p["feedback"])
    e.set_advanced_parameters(p["saturation"])
    return e


def chorus(fx, p):
    if p["voices"] is None:
        return fx.Chorus(mix_percent=p["mix_percent"])
    v = p["voices"]
    return fx.Chorus([q[0] for q in v], [q[1] for q in v], [fx.LFO(q[2], q[3], q[4], q[5]) for q in v], p["mix_percent"])


def distortion(fx, p):
    e = fx.Distortion()
    kinds = [getattr(fx.DistortionType, k) for k in p["kinds"]]
    single = len(kinds) == 1
    e.set_advanced_parameters(kinds[0] if single else kinds, p["levels"][0] if single else np.array(p["levels"]),
                              p["mix"][0] if single else np.array(p["mix"]),
                              p["offsets"][0] if single else np.array(p["offsets"]), p["post"])
    return e


def distortion_lists(p):
    """kinds, levels, mix fractions and offsets as the class expands them (a single curve gets the clean signal)."""
    kinds, levels, mix, offsets = list(p["kinds"]), list(p["levels"]), [m / 100 for m in p["mix"]], list(p["offsets"])
    if len(kinds) == 1:
        kinds, levels, mix, offsets = kinds + ["NoDistortion"], levels + [0], mix + [1 - mix[0]], offsets + [-np.inf]
    return kinds, levels, mix, offsets


def tremolo(fx, p):
    return fx.Tremolo(p["depth"], fx.LFO(p["freq"], p["waveform"], p["random_phase"], p["smooth"]))


# ---- generated shapes for the GPU tests (lengths around the follower's tile; see test_fx_gpu.py) ----------------------
def follower_lengths(tile: int):
    return [1, 2, tile - 1, tile, tile + 1, 3 * tile + 5]


def comb_delays(n: int):
    return [0, 1, 63, 64, 65, n - 1, n + 7]


def chorus_table(effect, n: int):
    """(the (n, voices) delays in samples as the effect's apply() rounds them, the smallest distance of an unrounded
    delay from a half-integer).  Draws the phases apply() would draw: seed before both."""
    mod = np.zeros((n, effect.number_of_voices))
    for i, m in enumerate(effect.modulators):
        mod[:, i] = m.get_waveform(FS, n) * effect.depths_ms[i] + effect.base_delays_ms[i]
    exact = mod * 1e-3 * FS
    return np.round(exact).astype(int), float(np.min(np.abs(exact - np.floor(exact) - 0.5)))
