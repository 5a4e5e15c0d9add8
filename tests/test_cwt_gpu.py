"""The continuous wavelet transform on the device against the reference's golden scalograms and against the float64
restatement of tests/test_cwt_host.py: every row within 1e-6 max_t|x_ch| (the wavelets have unit magnitude sum, so
|S| <= max|x|), every size class and both routes (LDS-resident and four-step) by exact wavelet lengths, the resident
route, and the synchrosqueezing kernel.  The bound is per channel and holds for channels of unequal level too -- the
transforms pair two blocks of one channel, never two channels; tests/test_cwt_sweep_gpu.py runs those cases."""

import numpy as np
import pytest
from scipy.signal import oaconvolve

import dsptoolbox_amd as dsp
from cwt_cases import Taps
from dsptoolbox_amd import backend
from dsptoolbox_amd.transforms import MorletWavelet, cwt
from dsptoolbox_amd.transforms._wavelets import _normalised_wavelets
from test_cwt_host import golden, ref_scalogram, ref_squeeze

pytestmark = pytest.mark.gpu
TOL = 1e-6


def row_error(S, ref, td):
    """max over rows and channels of max_t |S - ref| / max_t |x_ch|."""
    peak = np.abs(td).max(axis=0)
    peak[peak == 0] = 1.0
    return float((np.abs(S - ref).max(axis=1) / peak[None, :]).max())


def test_golden_scalograms():
    z = golden()
    x = z["x"]
    sig = dsp.Signal(None, x, 8000)
    worst = 0.0
    i = 0
    while f"cwt_{i}" in z:
        h, step, ch, sq, norm = z[f"cwt_{i}_args"]
        if not sq:
            freqs = z[f"cwt_{i}_freqs"]
            channel = None if ch < 0 else int(ch)
            td = x if ch < 0 else x[:, [int(ch)]]
            for on_dev in (False, True):
                out = cwt(sig, freqs, MorletWavelet(h=h, step=step), channel=channel, on_device=on_dev)
                if on_dev:
                    out = out.to_host()
                assert out.dtype == np.complex128 and out.shape == z[f"cwt_{i}"].shape
                e = row_error(out, z[f"cwt_{i}"], td)
                worst = max(worst, e)
                assert e <= TOL, (i, on_dev, e)
        i += 1
    print(f"golden cwt: worst row error {worst:.2e} of max|x|")


def test_long_signal_all_classes():
    fs, n = 48000, 1 << 18
    rng = np.random.default_rng(3)
    t = np.arange(n) / fs
    x = np.stack([np.sin(2 * np.pi * 1000 * t), rng.standard_normal(n), 0.3 * rng.uniform(-1, 1, n),
                  np.sin(2 * np.pi * (30 + 2000 * t) * t)], axis=1).astype(np.float32).astype(np.float64)
    freqs = np.geomspace(30, 20000, 48)
    w = MorletWavelet(h=3, step=1e-3)
    out = cwt(dsp.Signal(None, x, fs), freqs, w)
    ref = ref_scalogram(x, freqs, w, fs)
    e = row_error(out, ref, x)
    print(f"4 x 2^18, 48 frequencies 30 Hz - 20 kHz: worst row error {e:.2e} of max|x|")
    assert e <= TOL


@pytest.mark.parametrize("n", [1, 2, 1000, 3001, 20000])
def test_exact_lengths(n):
    fs = 8000
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 2)).astype(np.float32).astype(np.float64)
    # class boundaries: M = max(256, 2^ceil(log2(2L))) for the cropped length L; LDS route up to M = 16384
    lens = [1, 2, 3, 4, 127, 128, 129, 130, 255, 256, 257, 511, 512, 513, 4096, 4097, 8192, 8193, 8194, 16385]
    lens = [v for v in lens if v <= 4 * n + 300] + [5 * n + 1, 5 * n + 2]  # and wavelets longer than the signal
    freqs = np.array(lens, dtype=np.float64)
    ref = ref_scalogram(x, freqs, Taps(), fs)
    # (a Signal of one sample cannot be made -- its time data is read as one sample of two channels, as in the
    # reference -- so N = 1 goes through the host entry and a device-resident signal)
    outs = [backend.cwt_host(x, _normalised_wavelets(Taps(), freqs, fs)),
            cwt(dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), fs), freqs, Taps())]
    if n > 1:
        outs.append(cwt(dsp.Signal(None, x, fs), freqs, Taps()))
    for out in outs:
        e = row_error(out, ref, x)
        print(f"N={n}: lengths {lens}: worst {e:.2e}")
        assert e <= TOL


def test_longest_wavelets():
    fs, n = 48000, (1 << 18) + 3
    x = np.random.default_rng(9).standard_normal((n, 1)).astype(np.float32).astype(np.float64)
    freqs = np.array([(1 << 17) + 1, 1 << 18, 40000], dtype=np.float64)  # the four-step route at M = 2^19
    out = cwt(dsp.Signal(None, x, fs), freqs, Taps())
    ref = ref_scalogram(x, freqs, Taps(), fs)
    e = row_error(out, ref, x)
    print(f"L up to 2^18 on 2^18 + 3 samples: worst {e:.2e}")
    assert e <= TOL
    with pytest.raises(NotImplementedError):
        cwt(dsp.Signal(None, x, fs), np.array([(1 << 18) + 1.0]), Taps())


def test_resident_route_equals_host_route():
    fs = 16000
    x32 = np.random.default_rng(5).standard_normal((3, 20000)).astype(np.float32)
    freqs = np.array([4000.0, 80.0, 300.0, 80.0, 1200.0])
    w = MorletWavelet(h=2.5, step=2e-3)
    host_sig = dsp.Signal(None, x32.T.astype(np.float64), fs)
    for channel in (None, [2, 0]):
        host = cwt(host_sig, freqs, w, channel=channel)
        dev_sig = dsp.Signal.from_planar_f32(x32, fs)
        res = cwt(dev_sig, freqs, w, channel=channel, on_device=True)
        assert isinstance(res, backend.DeviceScalogram)
        got = res.to_host()
        assert got.shape == host.shape and got.dtype == np.complex128
        assert np.max(np.abs(got - host)) <= 1e-7 * np.abs(x32).max()
        # a host signal's samples were uploaded into a temporary buffer, not attached to it
        cwt(host_sig, freqs, w, channel=channel, on_device=True)
        assert not host_sig.on_device


def squeeze_signal(n=4000, fs=8000):
    t = np.arange(n) / fs
    rng = np.random.default_rng(11)
    x = np.stack([np.sin(2 * np.pi * 440 * t) + 0.5 * np.sin(2 * np.pi * (200 + 150 * t) * t),
                  0.8 * np.sin(2 * np.pi * 1210 * t) + 0.05 * rng.standard_normal(n)], axis=1)
    return x.astype(np.float32).astype(np.float64), fs


@pytest.mark.parametrize("normalize", [False, True])
def test_squeeze_kernel_against_restatement(normalize):
    x, fs = squeeze_signal()
    freqs = np.array([1210.0, 440.0, 300.0, 445.0, 440.0, 200.0, 1200.0, 2500.0, 230.0, 600.0])
    sig = dsp.Signal.from_planar_f32(np.ascontiguousarray(x.T, dtype=np.float32), fs)
    S = cwt(sig, freqs, MorletWavelet(h=3, step=2e-3), on_device=True)
    S64 = S.to_host()
    got = backend.cwt_squeeze_device(S, freqs, fs, apply_frequency_normalization=normalize).to_host()
    ref, margin = ref_squeeze(S64, freqs, fs, normalize, with_margins=True)
    ok = margin > 1e-9 * freqs.max()
    scale = len(freqs) * np.abs(x).max()
    err = np.abs(got - ref).max(axis=0)[ok].max()
    print(f"squeeze kernel: {ok.mean():.4f} of columns compared, worst {err / scale:.2e}")
    assert ok.mean() > 0.99
    assert err <= 1e-12 * scale


def test_squeeze_end_to_end_golden():
    z = golden()
    x = z["x"]
    sig = dsp.Signal(None, x, 8000)
    i, n_cases = 0, 0
    while f"cwt_{i}" in z:
        h, step, ch, sq, norm = z[f"cwt_{i}_args"]
        if sq:
            freqs = z[f"cwt_{i}_freqs"]
            td = x if ch < 0 else x[:, [int(ch)]]
            w = MorletWavelet(h=h, step=step)
            out = cwt(sig, freqs, w, channel=None if ch < 0 else int(ch), synchrosqueezed=True,
                      apply_synchrosqueezed_normalization=bool(norm))
            _, margin = ref_squeeze(ref_scalogram(td, freqs, w, 8000), freqs, 8000, bool(norm), with_margins=True)
            ok = margin >= 1e-3
            err = np.abs(out - z[f"cwt_{i}"]).max(axis=0)[ok].max()
            print(f"squeeze case {i}: {ok.mean():.4f} of columns compared, worst {err:.2e}")
            assert ok.mean() >= 0.95
            assert err <= 1e-6 * len(freqs) * np.abs(td).max()
            n_cases += 1
        i += 1
    assert n_cases >= 3
