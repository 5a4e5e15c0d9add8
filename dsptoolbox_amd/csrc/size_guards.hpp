// Size predicates shared by device code and the host-side sanitizer run (tests/host_san): plain integer
// arithmetic, no HIP types.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define DS_HD __host__ __device__
#else
#define DS_HD
#endif

// k_welch_finish (kernels_finish.hpp) reads the partial slabs of one chunk -- sx floats of input auto spectra,
// sy complex values of cross spectra (and sy floats of output auto spectra) -- through raw-buffer descriptors whose
// size and per-lane offsets are 32-bit byte counts.  A slab of 4 GiB or more (windows of 2^23 / 2^24 samples with
// 128 / 64 output channels on the four-step path) would wrap; such slabs take the kernel's plain 64-bit loads.
DS_HD inline bool welch_finish_wide_slab(int64_t sx, int64_t sy) {
    const int64_t limit = (int64_t)0xfffffff0;  // the hardware range check compares against a 32-bit size
    return sx * 4 >= limit || sy * 8 >= limit;
}

// k_smooth (kernels_smooth.hpp) sums directly: bins x window taps x channels multiply-adds per call, with no
// transform route for long windows.  One call is kept under about a second of device time: the bound is the
// measured rate of the kernel, 1.75e13 multiply-adds per second at 64 channels, rounded down.  Beyond it the entries answer DS_ERR_UNSUP.
constexpr double kSmoothMaxWork = 1e13;
DS_HD inline bool smooth_work_too_large(int64_t n_bins, int64_t n_window, int64_t n_ch) {
    return (double)n_bins * (double)n_window * (double)n_ch > kSmoothMaxWork;
}

// k_dft and k_csmooth (kernels_direct.hpp) sum directly as well.  Their work is counted in the terms really summed:
// frequencies x samples x channels for the plain DFT, the kept sample ranges of every (bin, channel) for the windowed
// one (each term there costs an exp), the clipped band lengths x channels for complex smoothing (each band point costs a
// pow).  One call is kept under about a second of device time; the bounds are the measured rates
// rounded down to one digit: 1.20e12 terms per second for the plain DFT (8 channels x 2^20 samples x 1024 frequencies),
// 2.03e10 kept terms per second for the windowed one (8 x 65536 samples, 5 cycles: the few low bins that keep the whole
// signal set the time; with nothing skipped it sums 6.3e11 per second), 2.53e11 for complex smoothing (8 x 65537 bins,
// 1/3 octave).  Beyond them the entries answer DS_ERR_UNSUP.
constexpr double kDftMaxWork = 1e12;
constexpr double kDftWindowedMaxWork = 2e10;
constexpr double kCsmoothMaxWork = 2e11;
DS_HD inline bool dft_work_too_large(double terms, bool windowed) {
    return terms > (windowed ? kDftWindowedMaxWork : kDftMaxWork);
}
DS_HD inline bool csmooth_work_too_large(double terms) { return terms > kCsmoothMaxWork; }

// The complex128 transforms of kernels_fft64.hpp: powers of two up to 2^22 (four-step, both factors at most 2048 -- one
// workgroup holds up to 8192 points in LDS -- and 64 MB per column and buffer), every other length up to 2^21 (Bluestein's padded
// length M >= 2 n - 1 is then at most 2^22).  Beyond them the entries answer DS_ERR_UNSUP.
constexpr int64_t kFft64MaxPow2 = (int64_t)1 << 22;
constexpr int64_t kFft64MaxAny = (int64_t)1 << 21;
DS_HD inline bool fft64_len_unsupported(int64_t n) {
    const bool pow2 = n > 0 && (n & (n - 1)) == 0;
    return n > (pow2 ? kFft64MaxPow2 : kFft64MaxAny);
}
