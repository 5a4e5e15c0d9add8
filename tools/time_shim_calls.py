"""Dev tool: wall time per call of the host shim (Welch first, then STFT, rFFT and FIR) on SMALL shapes, where the kernels take a few tens of microseconds and the
Python between the caller and the C entry is most of the call (tools/time_api_resident.py and tools/time_misc.py time the
large shapes).  Uses only the reference-shaped API and names the shim has had since device-resident signals exist, so the
same file times an older checkout.
    python tools/time_shim_calls.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dsptoolbox_amd as dsp  # noqa: E402
from dsptoolbox_amd import backend  # noqa: E402
from dsptoolbox_amd._lib import DevicePlanar, get_context  # noqa: E402
from dsptoolbox_amd.standard.enums import SpectrumScaling, Window  # noqa: E402

ctx = get_context()
fs = 48000
rng = np.random.default_rng(0)
x = rng.standard_normal((2**16, 1)) * 0.1
y = rng.standard_normal((2**16, 4)) * 0.1
Xd = dsp.Signal.from_planar_f32(backend._planar_f32(x), fs)
Yd = dsp.Signal.from_planar_f32(backend._planar_f32(y), fs)
for s in (Xd, Yd):
    s.set_spectrum_parameters(window_length_samples=1024, overlap_percent=50, detrend=True)
H1 = dsp.TransferFunctionType.H1


def timed(name, fn, reps=3000, warm=200):
    for _ in range(warm):
        fn()
    ts = np.empty(reps)
    for i in range(reps):
        t0 = time.perf_counter()
        fn()
        ts[i] = time.perf_counter() - t0
    print(f"{name:55s} median {np.median(ts) * 1e6:8.1f} us   min {ts.min() * 1e6:8.1f} us   p10 {np.percentile(ts, 10) * 1e6:8.1f} us", flush=True)


timed("welch_transfer_function_device narrow 4+1 ch x 2^16 W1024", lambda: backend.welch_transfer_function_device(
    Yd.device_samples, Xd.device_samples, fs, 1024, "H1", narrow=True))
timed("compute_transfer_function resident (host x64 route)", lambda: dsp.transfer_functions.compute_transfer_function(Yd, Xd, 1024, H1))
timed("_welch_psd_device 4 ch", lambda: backend._welch_psd_device(Yd.device_samples, fs, Window.Hann, 1024, 50.0, True, "mean",
                                                                  SpectrumScaling.FFTBackward))
timed("Signal.get_spectrum resident", lambda: Yd.get_spectrum(force_computation=True))
Sd = dsp.Signal.from_planar_f32(backend._planar_f32(y[:2**14]), fs)  # 32 frames: a short estimate, float64 kernels, host arrays
Sd.set_spectrum_parameters(window_length_samples=1024, overlap_percent=50, detrend=True)
timed("Signal.get_spectrum resident, short (host x64 route)", lambda: Sd.get_spectrum(force_computation=True), reps=1000, warm=50)
xs, ys = x[:4096], y[:4096]
timed("_welch host 4 ch x 4096 (x64 route)", lambda: backend._welch(ys, None, fs, Window.Hann, 1024, 50.0, True, "mean",
                                                                   SpectrumScaling.FFTBackward), reps=1000, warm=50)
timed("_welch host 4 ch x 2^16 (fp32 route)", lambda: backend._welch(y, None, fs, Window.Hann, 256, 50.0, True, "mean",
                                                                    SpectrumScaling.FFTBackward), reps=1000, warm=50)
timed("_csm_welch host 4 ch x 2^16 (fp32 route)", lambda: backend._csm_welch(y, fs, 256, Window.Hann, 50.0, True, "mean",
                                                                            SpectrumScaling.FFTBackward), reps=1000, warm=50)
timed("welch_transfer_function host f32 4+1 ch x 2^16", lambda: backend.welch_transfer_function(y, x, fs, 256, "H1"), reps=1000, warm=50)

# ---- STFT, rFFT, FIR on the call transcript's small shapes (100 samples x 2 channels, W = 16, 50 % overlap)
bw = SpectrumScaling.FFTBackward
small = rng.standard_normal((100, 2)) * 0.1
small_dev = DevicePlanar.from_planar(ctx, backend._planar_f32(small))
taps = [np.ones(5), np.ones(5) * 0.5, np.ones(5) * 0.25]
timed("_stft_device keep_on_device 2 ch x 100 W16", lambda: backend._stft_device(small_dev, fs, 16, Window.Hann, 50.0, None, True,
                                                                                 True, bw, True))
timed("_stft host planar 2 ch x 100 W16", lambda: backend._stft(small, fs, 16, Window.Hann, 50.0, None, True, True, bw),
      reps=1000, warm=50)
timed("rfft_spectrum host 2 ch x 100 nfft 128", lambda: backend.rfft_spectrum(small, 128), reps=1000, warm=50)
timed("fir_filter_bank host parallel 3 x 5 taps", lambda: backend.fir_filter_bank(small, taps, backend.DS_FB_PARALLEL),
      reps=1000, warm=50)
timed("fir_filter_bank_device parallel 3 x 5 taps", lambda: backend.fir_filter_bank_device(small_dev, taps, backend.DS_FB_PARALLEL),
      reps=1000, warm=50)
Big = dsp.Signal.from_planar_f32(rng.standard_normal((64, 512000), dtype=np.float32) * 0.1, fs)
Big.set_spectrogram_parameters(window_length_samples=1024, overlap_percent=50, detrend=True)
timed("Signal.get_spectrogram(on_device=True) 64 ch x 512000 W1024", lambda: Big.get_spectrogram(on_device=True), reps=200, warm=10)
