"""CPU-side checks: the C-ABI library builds/loads and exports every symbol the
header declares; host-side logic (framing rules, parameter mapping, API
validation) behaves like the reference.  No compute call is made here."""

import os
import re

import numpy as np
import pytest

import dsptoolbox_amd as dsp
from dsptoolbox_amd import backend
from dsptoolbox_amd._lib import SIGNATURES, load_library
from dsptoolbox_amd.standard.enums import SpectrumScaling, Window
from oracle import dsp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from dsptoolbox_amd._build import build_library
    lib = load_library(build_library())
    header = open(os.path.join(ROOT, "include", "dsptoolbox_amd.h")).read()
    declared = set(re.findall(r"\b(ds_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert declared == set(SIGNATURES), declared ^ set(SIGNATURES)
    assert lib.ds_version() >= 100 and lib.ds_max_fft_len() == 16384


def test_scaling_factors_match_oracle():
    w = np.hanning(64) + 0.1
    for sc in SpectrumScaling:
        for win in (None, w):
            a = np.asarray(sc.get_scaling_factor(64, 48000, win)).ravel()
            b = np.asarray(orc.get_scaling_factor(sc.name, 64, 48000, win)).ravel()
            assert np.allclose(a, b, rtol=1e-15)
        assert sc.fft_norm() == orc.fft_norm(sc.name)
        assert sc.is_amplitude_scaling() == orc.is_amplitude_scaling(sc.name)
        assert sc.has_physical_units() == orc.has_physical_units(sc.name)
        for dst in SpectrumScaling:
            assert np.allclose(sc.conversion_factor(dst, 64, 48000, None),
                               orc.conversion_factor(sc.name, dst.name, 64, 48000, None))


def test_welch_framing_rule():
    win = Window.Hann(256, False)
    hop, f = backend._welch_framing(1000, 256, 50, win)
    assert (hop, f) == (128, orc.compute_number_frames(256, 128, 1000, True)[0])
    with pytest.warns(UserWarning):  # 33 % Hann overlap is not COLA
        hop, f = backend._welch_framing(1024, 256, 33, win)  # overlap truncated: int(84.48) = 84
    assert hop == 256 - 84 and f == int(np.ceil(1024 / hop))


def test_finish_params():
    w = Window.Hann(128, False)
    assert backend._finish_params(SpectrumScaling.FFTBackward, 128, 48000, w) == (1, 1.0, 1.0, 0)
    amp, ns, fac, phys = backend._finish_params(SpectrumScaling.PowerSpectralDensity, 128, 48000, w)
    assert (amp, ns, phys) == (0, 1.0, 1) and np.isclose(fac, 2 / np.sum(w**2) / 48000)
    amp, ns, fac, phys = backend._finish_params(SpectrumScaling.FFTForward, 128, 48000, w)
    assert (amp, phys) == (1, 0) and np.isclose(ns, 1 / 128**2)


def test_signal_container_semantics():
    x = np.arange(12.0).reshape(3, 4)  # more columns than rows -> transposed
    s = dsp.Signal(None, x, 48000)
    assert s.time_data.shape == (4, 3) and s.number_of_channels == 3
    with pytest.raises(AssertionError):
        dsp.Signal(None, x, 48000.0)
    with pytest.warns(UserWarning):
        s2 = dsp.Signal.from_time_data(np.array([0.5, -2.0, 1.0]), 100)
    assert np.isclose(np.max(np.abs(s2.time_data)), 1.0) and np.isclose(s2.amplitude_scale_factor, 0.5)
    ir = dsp.ImpulseResponse(None, np.ones(8), 100)
    assert ir.spectrum_method == dsp.SpectrumMethod.FFT and ir.constrain_amplitude
    c = s.copy_with_new_time_data(np.zeros((10, 2)))
    assert c._spectrum_parameters == s._spectrum_parameters and c.time_data.shape == (10, 2)
    assert s._spectrum_parameters["scaling"] == SpectrumScaling.FFTBackward
    assert s._spectrum_parameters["detrend"] is True and s._spectrogram_parameters["padding"] is True


def test_channel_operations_of_the_containers():
    """MultichannelData (reference classes/_multichannel_data.py:6-118): remove / swap / select / sum on
    Signal and Spectrum; bad channel arguments are AssertionErrors as in the reference."""
    rng = np.random.default_rng(5)
    td = rng.standard_normal((50, 4))
    s = dsp.Signal(None, td.copy(), 8000)
    assert len(s) == 50 and s.number_of_channels == 4
    assert np.array_equal(s.get_channels(2).time_data, td[:, [2]])
    assert np.array_equal(s.get_channels([3, 0]).time_data, td[:, [3, 0]])
    assert np.allclose(s.sum_channels().time_data[:, 0], td.sum(axis=1))
    assert s.swap_channels(np.array([[3, 2, 1, 0]])) is s and np.array_equal(s.time_data, td[:, ::-1])
    for bad in ([0, 1, 2], [0, 0, 1, 2], [0, 1, 2, 4], [-1, 0, 1, 2], [[0, 1], [2, 3]]):
        with pytest.raises(AssertionError):
            s.swap_channels(bad)
    s.remove_channel()
    assert np.array_equal(s.time_data, td[:, [3, 2, 1]])
    s.remove_channel(0)
    assert np.array_equal(s.time_data, td[:, [2, 1]])
    with pytest.raises(AssertionError):
        s.remove_channel(2)
    s.remove_channel(1)
    with pytest.raises(AssertionError):
        s.remove_channel()
    sp = dsp.Spectrum(np.linspace(0, 100, 9), rng.standard_normal((9, 3)) + 1j)
    assert sp.number_of_channels == 3 and len(sp) == 9
    assert sp.get_channels([1]).number_of_channels == 1


def test_filter_and_bank_validation():
    f1 = dsp.Filter.fir_filter(20, 1000.0, dsp.FilterPassType.Lowpass, 48000)
    assert f1.is_fir and f1.order == 20 and len(f1) == 21
    f2 = dsp.Filter.from_ba([2.0, 1.0], [2.0], 48000)
    assert np.allclose(f2.ba[0], [1.0, 0.5]) and np.allclose(f2.ba[1], [1.0])
    with pytest.raises(NotImplementedError):
        dsp.Filter({dsp.FilterCoefficientsType.Sos: np.ones((1, 6))}, 48000)
    fb = dsp.FilterBank([f1, f2])
    s = dsp.Signal(None, np.zeros((100, 2)), 44100)
    with pytest.raises(AssertionError):
        fb.filter_signal(s, dsp.FilterBankMode.Parallel)
    with pytest.raises(AssertionError):
        f1.filter_signal(s)


def test_streaming_fir_classes_host_logic():
    """filterbanks.* (classes/fir_filter_realtime.py): constructor checks and the reference's error
    behaviour, without touching the device (prepare() allocates the device-resident state and is
    covered by the GPU tests)."""
    fb = dsp.filterbanks
    with pytest.raises(AssertionError):
        fb.FIRFilterOverlapSave(np.ones((4, 2)))
    with pytest.raises(AssertionError):
        fb.FIRFilterOverlapSave.from_filter(dsp.Filter.from_ba([1.0], [1.0, 0.5], 48000))
    with pytest.raises(AssertionError):
        fb.FIRUniformPartitioned(np.ones((4, 2)))
    o = fb.FIRFilterOverlapSave(np.ones(700))
    with pytest.raises(NotImplementedError):
        o.process_sample(0.0, 0)
    with pytest.raises(NotImplementedError):
        o.set_n_channels(1)
    m = fb.FIRUniformPartitionedMultichannel(np.array([[4.0, 0.0], [2.0, 1.0], [0.0, -1.0]]))
    assert np.allclose(m.fir, np.array([[1.0, 0.0], [0.5, 0.25], [0.0, -0.25]]))  # peak-normalised


def test_host_marshalling_helpers():
    """ds_host_planar_f32 / ds_host_interleave_f64 (threaded cast + transpose at the boundary, no
    device work) against numpy, incl. the thresholds below which numpy is used."""
    from dsptoolbox_amd import backend
    rng = np.random.default_rng(5)
    for n, c in ((2**20 + 3, 3), (300001, 7), (2**21, 1), (1000, 2)):
        y = rng.standard_normal((n, c))
        a = backend._planar_f32(y)
        assert a.dtype == np.float32 and a.flags.c_contiguous
        assert np.array_equal(a, np.ascontiguousarray(y.T, dtype=np.float32))
        b = backend._interleaved_f64(a)
        assert b.dtype == np.float64 and np.array_equal(b, a.T.astype(np.float64))
    v = rng.standard_normal((2**20 + 1, 4))[:, ::2]          # not C-contiguous: numpy path
    assert np.array_equal(backend._planar_f32(v), np.ascontiguousarray(v.T, dtype=np.float32))
    z = (rng.standard_normal((2**19 + 1, 3)) + 1j * rng.standard_normal((2**19 + 1, 3))).astype(np.complex64)
    assert np.array_equal(backend._widen(z), z.astype(np.complex128))
    f = rng.standard_normal(2**20 + 7).astype(np.float32)
    assert np.array_equal(backend._widen(f), f.astype(np.float64))
    lib = load_library()
    assert lib.ds_host_planar_f32(None, 10, 1, None, 10, 0) != 0   # argument check, no crash


def test_compute_transfer_function_validation():
    a = dsp.Signal(None, np.zeros((100, 2)), 48000)
    b = dsp.Signal(None, np.zeros((100, 3)), 48000)
    with pytest.raises(AssertionError):
        dsp.transfer_functions.compute_transfer_function(a, b, 64)
    c = dsp.Signal(None, np.zeros((90, 1)), 48000)
    with pytest.raises(AssertionError):
        dsp.transfer_functions.compute_transfer_function(a, c, 64)
    with pytest.raises(AssertionError):
        dsp.transfer_functions.spectral_deconvolve(a, c)


def test_precision_routing_rules():
    """Which estimates the host mirror sends through the float64 kernels: short ones (fewer than 128
    frames, frame spectra up to 1.25 GB; matrices 256 MB) for every window the reference allows -- 2^18 samples since round 4 --, small
    transfer-function problems, nothing under "f32"; median averaging up to 4096 frames; "f64" raises where the route ends."""
    assert backend._x64_short("auto", 2, 5, 262144, "mean") and backend._x64_short("auto", 3, 1, 32768, "median")
    assert not backend._x64_short("auto", 2, 5, 524288, "mean")       # beyond the reference's longest window
    assert not backend._x64_short("auto", 64, 127, 262144, "mean")    # 17 GB of frame spectra
    assert backend._x64_short("auto", 10, 13, 262144, "mean")         # 272 MB: the cap is 1.25 GB ...
    assert backend._tf_x64_applies("auto", 1, 64, 8, 262144, "mean")     # ... = 64 + 1 channels x 2^20 samples
    # ... for every window since round 5 (it was 256 MB up to 16384 samples: end to end the float64 route costs no more,
    # tools/x64_cap_time.py): 420 MB of 8192-sample frames, and the 20 + 20 channels x 61 frames of 16384 samples of the sweeps
    assert backend._x64_short("auto", 64, 100, 8192, "mean") and backend._tf_x64_applies("auto", 20, 20, 61, 16384, "mean")
    assert backend._x64_short("auto", 64, 127, 16384, "mean") and not backend._x64_short("auto", 128, 127, 16384, "mean")  # 1.0 / 2.0 GB
    # the matrix keeps 256 MB (its float64 pair sums grow with the square of the channel count)
    assert not backend._x64_short("auto", 64, 100, 8192, "mean", cap=backend._X64_MATRIX_BYTES)
    assert not backend._x64_short("auto", 2, 128, 1024, "mean") and not backend._x64_short("f32", 2, 5, 1024, "mean")
    assert backend._tf_x64_applies("auto", 1, 3, 7, 131072, "mean") and backend._tf_x64_applies("auto", 1, 2, 2000, 256, "mean")
    assert not backend._tf_x64_applies("auto", 1, 64, 511, 4096, "mean")  # the headline shape stays on the fp32 kernels
    assert not backend._tf_x64_applies("f32", 1, 3, 7, 1024, "mean") and not backend._tf_x64_applies(None, 1, 3, 7, 1024, "mean")
    assert backend._tf_x64_applies("f64", 1, 64, 511, 4096, "mean")
    with pytest.raises(NotImplementedError):
        backend._tf_x64_applies("f64", 1, 1, 5000, 16, "median")
    with pytest.raises(NotImplementedError):
        backend._tf_x64_applies("f64", 1, 1, 3, 524288, "mean")


def test_no_gpu_means_loud_failure():
    lib = load_library()
    if lib.ds_device_count() > 0:
        pytest.skip("GPU present")
    from dsptoolbox_amd._lib import DeviceError
    s = dsp.Signal(None, np.random.default_rng(0).standard_normal((1000, 2)), 48000)
    with pytest.raises(DeviceError):
        s.get_spectrum()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "dsptoolbox_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} mentions the oracle"


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_host_marshalling_under_sanitizers(sanitizers, tmp_path):
    """SURVEY section 5 / VERDICT r2 item 9: the device-free host side of the boundary
    (csrc/host_marshal.hpp: threaded float64 <-> planar float32 casts, the double-buffered pinned-chunk
    pipelines with a memcpy transport) built by g++ with sanitizers and run on the CPU."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = os.path.join(ROOT, "tests", "host_san", "host_san.cpp")
    exe = str(tmp_path / "host_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", f"-fsanitize={sanitizers}", "-fno-sanitize-recover=all", "-pthread",
                    "-o", exe, src], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    # g++ 11's ThreadSanitizer cannot place its shadow memory beside a binary mapped by high-entropy ASLR
    # (vm.mmap_rnd_bits = 32: "FATAL: ThreadSanitizer: unexpected memory mapping"); setarch -R runs this one
    # process without address randomisation
    setarch = shutil.which("setarch")
    cmd = [setarch, os.uname().machine, "-R", exe] if setarch else [exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "host_san: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
