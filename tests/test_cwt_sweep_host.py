"""The wavelet-transform sweep without a device: the plan restated in tests/cwt_cases.py against the constants of
csrc/kernels_cwt.hpp and csrc/api.hip, every case against the edge it is there for, the oracle (`ref_scalogram` of
tests/test_cwt_host.py) against a direct float64 sum and for its independence of the channels, and a float32 emulation of
the transform's channel pairing -- the measurement that made the kernels pair blocks of one channel instead."""

import os
import re

import numpy as np
import pytest
from scipy import fft as sfft

import cwt_cases as cc
from dsptoolbox_amd import backend
from test_cwt_host import ref_scalogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name):
    return open(os.path.join(ROOT, "dsptoolbox_amd", "csrc", name)).read()


def test_constants_match_the_sources():
    hdr = source("kernels_cwt.hpp")

    def const(name):
        return re.search(rf"constexpr \w+ {name} = ([^;]+);", hdr).group(1).strip()

    assert int(const("MIN_M")) == cc.MIN_M
    assert int(const("MAX_LDS_M")) == cc.MAX_LDS_M
    assert const("MAX_TAPS") == "1 << 18" and cc.MAX_TAPS == 1 << 18 == backend.CWT_MAX_TAPS
    assert int(const("BIG_N1")) == cc.BIG_N1
    api = source("api.hip")
    run = api[api.index("static int cwt_run("):api.index('extern "C" int ds_cwt_dev(')]
    m = re.search(r"chunk = big \? std::min<int64_t>\(\{n_items, (\d+), std::max<int64_t>\(1, \(\(int64_t\)(\d+) << 20\) / "
                  r"\(8 \* \(int64_t\)M\)\)\}\) : 0;", run)
    assert m and int(m.group(1)) == cc.GRID_Y_MAX and int(m.group(2)) << 20 == cc.BIG_STAGE_BYTES
    assert "while (M < 2 * lc) M *= 2;" in run and "const int64_t V = M - hmax - cc;" in run
    assert "k0 = std::max<int64_t>(0, h - N + 1), k1 = std::min<int64_t>(L - 1, h + N - 1);" in run
    assert "const bool big = M > dscwt::MAX_LDS_M;" in run
    host = api[api.index('extern "C" int ds_cwt('):api.index('extern "C" int ds_cwt_squeeze_dev(')]
    m = re.search(r"rows = \(int\)std::max<int64_t>\(1, std::min<int64_t>\(n_freq, \(\(int64_t\)(\d+) << 20\) / \(8 \* row\)\)\);", host)
    assert m and int(m.group(1)) << 20 == cc.HOST_PASS_BYTES
    assert "const int64_t row = n_samples * n_ch;" in host


def test_plan_on_known_shapes():
    # the chunks the sources' budgets give: 64 items at M = 2^19, 1024 at 2^15 (were the call that large)
    p = cc.plan([1 << 18], (1 << 18) + 3, 70)
    assert p["classes"][1 << 19]["chunk"] == 64 and p["classes"][1 << 19]["n_items"] == 140
    assert cc.BIG_STAGE_BYTES // (8 << 15) == 1024
    # cropping: a wavelet longer than the signal keeps 2 n - 1 taps around its centre
    w = cc.wavelet_plan(5001, 1000)
    assert (w["k0"], w["lc"], w["hc"], w["M"]) == (2500 - 999, 1999, 999, 4096)
    w = cc.wavelet_plan(8, 1000)
    assert (w["k0"], w["lc"], w["hc"], w["M"]) == (0, 8, 3, 256)
    # an even length gives cc = h + 1, an odd one cc = h
    assert cc.plan([128], 500, 1)["classes"][256]["cc"] == 64 and cc.plan([127], 500, 1)["classes"][256]["cc"] == 63
    assert cc.plan([128], 500, 1)["classes"][256]["hmax"] == 63 == cc.plan([127], 500, 1)["classes"][256]["hmax"]


@pytest.mark.parametrize("case", cc.ALL_PLANNED, ids=lambda c: c.name)
def test_case_meets_its_edge(case):
    for n_ch in case.channels:
        lengths = [int(v) for v in case.lengths]
        assert max(lengths) <= cc.MAX_TAPS
        assert case.edge(cc.plan(lengths, case.n, n_ch)), (case.name, n_ch, case.why)


def test_case_lists_are_the_issues():
    assert [c.n for c in cc.block_cases() if "M256-" in c.name] == [128, 129, 130, 257, 258, 259]
    assert cc.block_lengths(256) == (128, 1, 64, 127) and cc.block_lengths(16384) == (8192, 4097, 6144, 8191)
    for m in cc.LDS_MS:
        L = cc.block_lengths(m)
        assert L[0] == m // 2 and L[1] == (1 if m == 256 else m // 4 + 1) and L[2] % 2 == 0 and L[3] % 2 == 1
        assert L[1] < L[2] < L[0] and L[1] < L[3] < L[0]
    assert len(cc.block_cases()) == 7 * 6 and len(cc.big_cases()) == 5
    assert cc.CHUNK_ONE_BLOCK.n == 98304 and len(cc.CHUNK_ONE_BLOCK.lengths) == 13
    assert len(cc.CHUNK_BLOCKS.lengths) == 26 and cc.CHUNK_BLOCKS.n == 3 * 32769 + 1
    # the second chunk of the several-block case starts at (frequency 25, block 2, channel 2)
    q = cc.plan(cc.CHUNK_BLOCKS.lengths, cc.CHUNK_BLOCKS.n, 5)["classes"][1 << 16]
    fb, c = divmod(q["chunk"], 5)
    assert (fb // q["n_blocks"], fb % q["n_blocks"], c) == (25, 2, 2)
    # 44 distinct wavelets of 1 ... 9 taps
    waves = cc.normalised(cc.Taps(), cc.PASSES.lengths, 8000)
    assert sorted({len(w) for w in waves}) == list(range(1, 10)) and len(waves) == 44
    assert len({w.tobytes() for w in waves}) == 44
    assert 16 * 44 * cc.PASSES.n * 3 > 1.1e9  # the complex128 result
    # the level wavelets: three LDS classes and a four-step one, odd and even block counts
    for n_ch in (2, 3, 4, 5):
        assert cc.level_edge(cc.plan(cc.level_lengths(), cc.LEVEL_N, n_ch))
    assert cc.level_lengths()[3] == cc.LEVEL_TAPS
    assert len({cc.LEVEL_TONES[c] for c in range(cc.MAX_CH)}) == cc.MAX_CH


def test_signals_are_float32_valued_and_nested():
    x = cc.signal(257, 5)
    assert np.array_equal(x, x.astype(np.float32)) and np.array_equal(cc.signal(257, 3), x[:, :3])
    y = cc.level_signal((0, -120, None), 4000, cc.LEVEL_FS)
    assert np.array_equal(y, y.astype(np.float32)) and not y[:, 2].any()
    peaks = np.abs(y).max(axis=0)
    assert 0.95 < peaks[0] < 1.1 and 0.95e-6 < peaks[1] < 1.1e-6


def test_oracle_agrees_with_the_direct_sum():
    x = cc.signal(300, 3, seed=2)
    lengths = np.array([1, 2, 3, 8, 9, 130, 257, 601, 602], dtype=np.float64)  # shorter and longer than the signal
    ref = ref_scalogram(x, lengths, cc.Taps(), 8000)
    direct = cc.direct_scalogram(x, cc.normalised(cc.Taps(), lengths, 8000))
    assert np.abs(ref - direct).max() <= 1e-13 * np.abs(x).max()


def test_oracle_treats_channels_independently():
    x = cc.signal(1000, 3, seed=3)
    lengths = np.array([5, 130, 2501], dtype=np.float64)
    a = ref_scalogram(x, lengths, cc.Taps(), 8000)
    y = x.copy()
    y[:, 1] *= 2.0 ** -20
    b = ref_scalogram(y, lengths, cc.Taps(), 8000)
    assert np.array_equal(b[:, :, 1], a[:, :, 1] * 2.0 ** -20)
    assert b[:, :, [0, 2]].tobytes() == a[:, :, [0, 2]].tobytes()
    z = x.copy()
    z[:, 1] = 0
    assert not ref_scalogram(z, lengths, cc.Taps(), 8000)[:, :, 1].any()


# ---- the pairing emulation: a recorded measurement --------------------------------------------------------------------
EMU_M = 4096


def emulate_pair(a, b, w):
    """float32 throughout, scipy's single-precision FFT: z = a + i b, one M-point transform, unpack both spectra, multiply
    by the taps' spectrum (taps / M), inverse.  Returns the two circular convolutions (complex64)."""
    m = len(a)
    z = (a.astype(np.float32) + 1j * b.astype(np.float32)).astype(np.complex64)
    Z = sfft.fft(z)
    assert Z.dtype == np.complex64
    Zc = np.conj(np.roll(Z[::-1], 1))  # conj Z[(M - k) mod M]
    A = (np.float32(0.5) * (Z + Zc)).astype(np.complex64)
    B = (np.complex64(-0.5j) * (Z - Zc)).astype(np.complex64)
    wp = np.zeros(m, dtype=np.complex64)
    wp[:len(w)] = (w / m).astype(np.complex64)
    W = sfft.fft(wp)
    return sfft.ifft(A * W) * np.float32(m), sfft.ifft(B * W) * np.float32(m)


def exact_circular(a, w):
    m = len(a)
    wp = np.zeros(m, dtype=np.complex128)
    wp[:len(w)] = w.astype(np.complex64)  # the taps the device gets
    return np.fft.ifft(np.fft.fft(a.astype(np.float64)) * np.fft.fft(wp))


def emu_inputs(kind):
    rng = np.random.default_rng(77)
    t = np.arange(2 * EMU_M)
    if kind == "morlet":  # a Morlet-like wavelet on sines with 1 % noise
        k = np.arange(-1000, 1001)
        w = np.exp(2j * np.pi * k / 60.0) * np.exp(-(k / 400.0) ** 2)
        xs = [np.sin(2 * np.pi * f * t) + 0.01 * rng.standard_normal(len(t)) for f in (0.0313, 0.0871)]
    else:  # random taps on noise
        w = rng.standard_normal(2001) + 1j * rng.standard_normal(2001)
        xs = [rng.standard_normal(len(t)) for _ in range(2)]
    w = w / np.abs(w).sum()
    return w, [x.astype(np.float32).astype(np.float64) for x in xs]


def quiet_error(kind, db, same_channel):
    """error of the quiet partner over the peak it is held to: its own as a channel, its channel's as a block"""
    w, (x0, x1) = emu_inputs(kind)
    g = 10.0 ** (db / 20.0)
    if same_channel:  # two blocks of ONE channel whose second block is quieter by db
        loud, quiet = x0[:EMU_M], (g * x0[EMU_M:]).astype(np.float32).astype(np.float64)
        peak = max(np.abs(loud).max(), np.abs(quiet).max())
    else:  # two channels
        loud, quiet = x0[:EMU_M], (g * x1[:EMU_M]).astype(np.float32).astype(np.float64)
        peak = np.abs(quiet).max()
    _, got = emulate_pair(loud, quiet, w)
    valid = slice(len(w) - 1, EMU_M)
    return float(np.abs(got[valid] - exact_circular(quiet, w)[valid]).max() / peak)


def test_pairing_emulation(capsys):
    """Recorded, not asserted: a channel paired with a louder CHANNEL takes that channel's rounding error, which grows
    by a factor of ten per 20 dB against its own peak and leaves 1e-6 of it near -60 dB (when this was written: 5e-9 at
    0 dB, 1e-7 at -40 dB, 1e-6 at -60 dB, 1e-5 at -80 dB, 6e-4 at -120 dB for the Morlet-like wavelet; random taps on
    noise 1.5 to 3 times that).  Asserted: two BLOCKS of one channel, held to the channel's peak, stay below a quarter
    of 1e-6 at -120 dB (6e-10 to 5e-9 at every level) -- the pairing the kernels use."""
    lines = []
    for kind in ("morlet", "taps"):
        for db in (0, -40, -60, -80, -120):
            lines.append(f"{kind:6s} {db:5d} dB: channel pair {quiet_error(kind, db, False):.2e} of the quiet channel's "
                         f"peak; block pair {quiet_error(kind, db, True):.2e} of the channel's peak")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for kind in ("morlet", "taps"):
        assert quiet_error(kind, -120, True) <= 0.25 * cc.TOL, kind
