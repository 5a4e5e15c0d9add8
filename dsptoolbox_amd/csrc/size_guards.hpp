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

// Latency estimation (kernels_latency.hpp).  The full-mode correlation of Na and Nb samples has L = Na + Nb - 1 rows and
// runs on the power-of-two transform of at least L points: L <= 2^22 (kFft64MaxPow2).  The window around the peaks, M rows,
// takes the transform of any length and its bounds (fft64_len_unsupported).  The columns of both signals are transformed in
// one batch, one grid row per column: at most 65535 together.  polynomial_points <= 16: the fit has degree 2 p - 1, and
// beyond a few points it is ill-conditioned long before the bound.  Beyond any of these the entries answer DS_ERR_UNSUP.
constexpr int kLatencyMaxPoints = 16;
constexpr int kLatencyMaxColumns = 65535;
DS_HD inline bool latency_shape_unsupported(int64_t rows, int64_t columns, int64_t points) {
    return rows > kFft64MaxPow2 || columns > kLatencyMaxColumns || points > kLatencyMaxPoints;
}

// Linear prediction (kernels_lpc.hpp).  One workgroup holds a pair's frame in LDS, of which a workgroup may declare
// 160 KiB = 163840 bytes.  Burg keeps the forward and the backward error row, two coefficient rows of 256 doubles and
// eight partial sums: (2 L + 520) 8 bytes <= 163840 allows L <= 9980.  Yule-Walker keeps the frame, 260 zeros behind it
// and two rows of 256: (L + 772) 8 bytes, L <= 19708.  Both methods take the same bound, the power of two below the
// smaller figure: windows up to 8192 samples (Burg then declares 135232 bytes, Yule-Walker 71712).  Orders up to 255:
// order + 1 coefficients, one per lane of the 256-lane workgroup (Levinson's and Burg's coefficient update, the
// recursion's four states per lane of a wave).  The grid is one workgroup per (frame, channel) pair, fewer than 2^31.
// The work of a call is counted as frames x channels x window x (order + 1) products; one call is kept under about a
// second of device time.  The rate of these kernels has not been measured yet: the bound is
// provisional, a tenth of kDftMaxWork, whose kernel sustains 1.2e12 float64 multiply-adds per second, and is to be
// replaced by the measured rate of tools/time_lpc.py rounded down.  Beyond any of these the entries answer DS_ERR_UNSUP.
constexpr int kLpcMaxWindow = 8192;
constexpr int kLpcMaxOrder = 255;
constexpr int64_t kLpcMaxPairs = ((int64_t)1 << 31) - 1;
constexpr double kLpcMaxWork = 1e11;
DS_HD inline bool lpc_shape_unsupported(int64_t window, int64_t order, int64_t pairs) {
    return window > kLpcMaxWindow || order > kLpcMaxOrder || pairs > kLpcMaxPairs;
}
DS_HD inline bool lpc_work_too_large(int64_t pairs, int64_t window, int64_t order) {
    return (double)pairs * (double)window * (double)(order + 1) > kLpcMaxWork;
}

// The all-pass table of warp and laguerre (kernels_warp.hpp, warp_plan.hpp): n_in x n_out cells, each depending on three
// neighbours, swept tile anti-diagonal by tile anti-diagonal -- ceil((n_in - 1) / 1024) + ceil((n_out - 1) / 256) - 1 launches
// one after the other, whatever the channel count.  The side bound is the ceiling the feature was given, 2^17 samples (the
// longest room responses in practice): a two-channel warp of that length takes 79 ms on the device, far
// inside the two seconds one call may take, so no smaller power of two is needed.  Channels come in groups of 4, each group
// a further workgroup per tile that repeats the table; the work of a call is counted as n_in x n_out x groups table cells.
// With every compute unit busy (64 channels x 32768 samples: 512 workgroups in the widest launch) the kernel sustains
// 6.6e11 cells per second; the bound is that rate times two seconds, rounded down.  grid.y carries the groups: at most
// 65536 channels.  Beyond any of these the entries answer DS_ERR_UNSUP.
constexpr int64_t kWarpMaxSide = (int64_t)1 << 17;
constexpr int kWarpMaxChannels = 65536;
constexpr double kWarpMaxWork = 1e12;
DS_HD inline bool warp_shape_unsupported(int64_t n_in, int64_t n_out, int64_t n_ch) {
    return n_in > kWarpMaxSide || n_out > kWarpMaxSide || n_ch > kWarpMaxChannels;
}
DS_HD inline bool warp_work_too_large(int64_t n_in, int64_t n_out, int64_t groups) {
    return (double)n_in * (double)n_out * (double)groups > kWarpMaxWork;
}

// Shoebox room simulation (kernels_room.hpp).  The image-source entry enumerates (2 LIMIT + 1)^3 cells of eight sources
// twice (count, fill) and keeps a list of 4-byte ids of the kept sources of one slab of l planes, which the sum pass
// sorts and adds per output sample.  Cells per call: at most 2^27 (LIMIT <= 255: T60 = 2 s in a room of 2.6 m a side),
// 1.07e9 sources -- eleven times the largest shape measured (1.17e7 cells, 9.4e7 sources, 1.2 ms of kernels: DESIGN
// section 19), so a call stays far below a second.  List bytes per slab: at most 1 GiB unless the caller asks for less;
// a slab is at least one plane and its ids stay below 2^31 (the sort's padding key is 2^32 - 1; the segment starts are
// 32-bit).  Output samples: at most 2^24 per band (the scan is one workgroup), bands at most 8.  The modal sum costs one
// division per (mode, frequency); it sustains 2.0e11 terms per second (68920 modes x 24000 frequencies in 8.4 ms), and
// the bound is half a second of that.  Beyond any of these the entries answer DS_ERR_UNSUP.
constexpr int64_t kIsmMaxCells = (int64_t)1 << 27;
constexpr int64_t kIsmMaxListBytes = (int64_t)1 << 30;
constexpr int64_t kIsmMaxOut = (int64_t)1 << 24;
constexpr int kIsmMaxBands = 8;
constexpr double kModalMaxWork = 1e11;
DS_HD inline int64_t ism_cells(int64_t limit) { return (2 * limit + 1) * (2 * limit + 1) * (2 * limit + 1); }
DS_HD inline bool ism_shape_unsupported(int64_t limit, int64_t n_out, int64_t n_band) {
    return limit > 1024 || ism_cells(limit) > kIsmMaxCells || n_out > kIsmMaxOut || n_band > kIsmMaxBands;  // (1024: no overflow in ism_cells)
}
// l planes per slab whose ids fit list_bytes (0: not even one plane does)
DS_HD inline int64_t ism_slab_planes(int64_t limit, int64_t list_bytes) {
    const int64_t side = 2 * limit + 1, plane_ids = side * side * 8;
    int64_t ids = list_bytes / 4;
    if (ids > (((int64_t)1 << 31) - 1)) ids = ((int64_t)1 << 31) - 1;
    const int64_t planes = ids / plane_ids;
    return planes > side ? side : planes;
}
DS_HD inline bool modal_work_too_large(int64_t n_modes, int64_t n_freq) {
    return (double)n_modes * (double)n_freq > kModalMaxWork;
}

// Variable-Q transform (kernels_vqt.hpp).  The result, octaves x bins rows of samples x channels complex128, is written
// once by the last interpolation stage: at most 2^34 bytes (the 2 channel x 2^20 sample call at the defaults writes
// 2^32).  The workspace beside it (the decimated samples, the bank's rows and the first interpolation stage) is
// (octaves + 1) / d of that.  The other bounds are what the LDS staging of a workgroup holds, 160 KiB:
//   d <= 48        k_vqt_decimate stages (255 d + 20 d + 1) samples of one channel, or (63 d + 20 d + 1) of four, and
//                  the 20 d + 1 taps: 135208 bytes at d = 48 with four channels;
//   octaves <= 7   the first interpolation stage goes up by 2^o, at most 64: 21 x 64 taps, 10752 bytes;
//   L_i <= 2048    k_vqt_bank stages a kernel's L complex taps and 64 + L - 1 samples of four channels: 100320 bytes.
// grid.z carries octaves x bins and grid.y the channel groups of four: at most 65535 each.  Beyond any of these the
// entries answer DS_ERR_UNSUP.
constexpr int64_t kVqtMaxOutputBytes = (int64_t)1 << 34;
constexpr int kVqtMaxDecimation = 48;
constexpr int kVqtMaxOctaves = 7;
constexpr int kVqtMaxKernel = 2048;
constexpr int kVqtMaxRows = 65535;
DS_HD inline bool vqt_output_too_large(int64_t rows, int64_t n_samples, int64_t n_ch) {
    return (double)rows * (double)n_samples * (double)n_ch * 16.0 > (double)kVqtMaxOutputBytes;
}
DS_HD inline bool vqt_shape_unsupported(int64_t d, int64_t n_oct, int64_t longest_kernel, int64_t rows, int64_t n_ch) {
    return d > kVqtMaxDecimation || n_oct > kVqtMaxOctaves || longest_kernel > kVqtMaxKernel || rows > kVqtMaxRows ||
           (n_ch + 3) / 4 > kVqtMaxRows;
}

// Audio effects (kernels_fx.hpp).  A stream is one channel of one band; grid.y (or grid.x of the one-workgroup-per-stream
// kernels) carries the streams: at most 65535.  A stream's padded length -- the delay's repetitions and the chorus's
// largest delay included -- stays below 2^28 samples (the chorus index table is 32-bit), and streams x padded samples at
// most 2^30: the float64 intermediate between the recursion and the restore stage is then at most 8 GiB.  The follower is
// serial in time per stream, 35 ns a sample, so the longest stream takes under ten seconds.
// Distortion sums at most 8 curves, the chorus at most 64 voices (registers and kernel arguments, not a measured rate).
// Beyond any of these the entries answer DS_ERR_UNSUP.
constexpr int kFxMaxStreams = 65535;
constexpr int64_t kFxMaxSamples = (int64_t)1 << 28;
constexpr int64_t kFxMaxElements = (int64_t)1 << 30;
constexpr int kFxMaxCurves = 8;
constexpr int kFxMaxVoices = 64;
DS_HD inline bool fx_shape_unsupported(int64_t n_streams, int64_t n_padded) {
    return n_streams > kFxMaxStreams || n_padded > kFxMaxSamples || (double)n_streams * (double)n_padded > (double)kFxMaxElements;
}

// Levels and loudness (kernels_level.hpp).  grid.y carries the channels: at most 65535.  A channel stays below 2^31
// samples (grid.x of the sample-parallel kernels, 256 lanes each, and the 32-bit count of the reduction's workgroups) and
// channels x samples at most 2^33: the host's float64 array is then 64 GiB, beyond what a call could stage anyway.  The
// moving window rebuilds a sum of W squares once per tile of 1024 outputs, so its work is counted as samples x channels x
// (2 + W / 1024) squares and kept below 1e12, a provisional bound (no rate of that kernel has been measured) that only
// windows of many thousand samples on the longest signals reach.  Beyond any of these the entries answer DS_ERR_UNSUP.
constexpr int kLevelMaxChannels = 65535;
constexpr int64_t kLevelMaxSamples = ((int64_t)1 << 31) - 1;
constexpr int64_t kLevelMaxElements = (int64_t)1 << 33;
constexpr double kLevelMovingMaxWork = 1e12;
DS_HD inline bool level_shape_unsupported(int64_t n_ch, int64_t n) {
    return n_ch > kLevelMaxChannels || n > kLevelMaxSamples || (double)n_ch * (double)n > (double)kLevelMaxElements;
}
DS_HD inline bool level_moving_work_too_large(int64_t n_ch, int64_t n, int64_t w) {
    return (double)n_ch * (double)n * (2.0 + (double)(w < n ? w : n) / 1024.0) > kLevelMovingMaxWork;
}

// Rational-ratio resampling (kernels_resample.hpp, resample_plan.hpp).  The rate r = max(up, down) of the reduced ratio is
// at most 640 (44100 <-> 192000): its tap table, 110 KB at most, shares the 160 KiB of LDS with the tile's input window.
// The samples of one call -- the longer of input and output, times the channels -- stay at 2^31: a host call stages both
// arrays in float64, 32 GiB together at the bound.  grid.y carries the channel groups: at most 65535 channels.  Beyond
// any of these the entries answer DS_ERR_UNSUP.
constexpr int kResampleMaxRate = 640;
constexpr int64_t kResampleMaxSamples = (int64_t)1 << 31;
constexpr int kResampleMaxChannels = 65535;
DS_HD inline bool resample_shape_unsupported(int64_t up, int64_t down, int64_t n_in, int64_t n_out, int64_t n_ch) {
    const int64_t longer = n_in > n_out ? n_in : n_out;
    return up > kResampleMaxRate || down > kResampleMaxRate || n_ch > kResampleMaxChannels ||
           (double)longer * (double)n_ch > (double)kResampleMaxSamples;
}

// Spectral subtraction (kernels_specsub.hpp).  A window is a power of two from 4 to 2^14 samples: its W / 2 complex
// points, 128 KiB at the bound, and 2 KiB of partial sums share the 160 KiB of LDS of one workgroup (the default block of
// 0.1 s gives 2^14 at 192 kHz).  The step is 1 .. W.  The frame workspace, 8 (W + 2) bytes x frames x streams, stays at
// 2^32 bytes (eight bands of two channels of ten seconds at 48 kHz and 50 % overlap hold 1.2e8).  The overlap-add reads
// samples x streams x ceil(W / step) terms, one lane per sample: at most 2^29, which is what the workspace bound allows
// where the step divides the window (frames x W doubles); a step that does not divide it rounds the covering frames up,
// and such a call is held to the same work.  No measured rate enters either bound yet.  grid.x carries the frames, fewer
// than 2^31; streams and samples as for the other effects (fx_shape_unsupported).  Beyond any of these the entry answers
// DS_ERR_UNSUP.
constexpr int kSpecsubMinWindow = 4;
constexpr int kSpecsubMaxWindow = 16384;
constexpr int64_t kSpecsubMaxWorkspaceBytes = (int64_t)1 << 32;
constexpr int64_t kSpecsubMaxOlaTerms = (int64_t)1 << 29;
DS_HD inline int64_t specsub_frames(int64_t n, int64_t window, int64_t step) { return (n + 2 * window + step - 1) / step; }
DS_HD inline bool specsub_window_unsupported(int64_t window) { return window > kSpecsubMaxWindow; }
DS_HD inline bool specsub_work_too_large(int64_t n_streams, int64_t n, int64_t window, int64_t step) {
    const double frames = (double)specsub_frames(n, window, step);
    return frames > 2147483647.0 || 8.0 * (double)(window + 2) * frames * (double)n_streams > (double)kSpecsubMaxWorkspaceBytes ||
           (double)n * (double)n_streams * (double)((window + step - 1) / step) > (double)kSpecsubMaxOlaTerms;
}
