// Spectral subtraction: the reference's effects.SpectralSubtractor (effects/effects.py:138-550 with
// standard/_framed_signal_representation.py), whose loop runs one irfft per (frame, channel).  Analysis, a per-bin change
// of the magnitudes, synthesis and a weighted overlap-add with the squared window's envelope divided out; float64
// throughout, each kernel in the reference's operation order (no contraction into fused multiply-adds).  gfx950.
//
// A stream is one channel of one band; its samples are read through dsfx::Src<T> (kernels_fx.hpp) where they lie.  The
// signal is padded VIRTUALLY by W zeros at both ends: padded sample i is x[i - W] inside [W, W + n) and 0 elsewhere; frame
// f holds padded samples f step .. f step + W - 1, F = ceil((n + 2 W) / step) frames.  A frame's slot in the workspace is
// W / 2 + 1 complex bins = W + 2 doubles: k_ss_analyze fills it with the spectrum, k_ss_track rewrites the bins, and
// k_ss_synth overwrites them with the frame's W samples.
//
//   k_ss_analyze   grid (frames, streams): the variance of the unwindowed frame in a fixed order and its gate flag, the
//                  window, the real transform of W points as W / 2 complex points in LDS (f64c::radix2_lds) and the split.
//   k_ss_track     one lane per (bin, stream): adaptive mode walks the frames in order with the noise amplitude in a
//                  register, TRACK_TILE frames' bins loaded ahead; static mode has no recursion, so lanes also spread
//                  over tiles of frames and the subtracted term comes from a table.  Exponents 1 and 2 have their own
//                  instantiation (sqrt, no pow).
//   k_ss_synth     grid (frames, streams): the inverse packed transform, 1 / W, times the synthesis window.
//   k_ss_ola       one lane per KEPT output sample: the covering frames in ascending order, the squared window over the
//                  same frames, the envelope's floor, the division.  One writer per sample, no atomics.
//   k_ss_peak      the peaks of input and output per stream, from the partial peaks k_ss_analyze (one per frame: every
//                  sample lies in a frame) and k_ss_ola (one per workgroup) leave; k_fx_scale restores the peak.  The
//                  one-workgroup-per-stream k_fx_stats took 0.29 ms a pass over 480 000 samples, three quarters of a
//                  two-channel call's kernel time (profiles/specsub_timing.txt).
#pragma once
#include <float.h>
#include <stdint.h>

#include "fft64_common.hpp"
#include "kernels_fx.hpp"

namespace dsss {

using dsfx::Src;

constexpr int NT = 256;         // threads of every kernel here (f64c::radix2_lds strides by 256)
constexpr int TRACK_TILE = 8;   // frames whose bins a lane of k_ss_track loads before it walks them
constexpr int OLA_TILE = 256;   // kept output samples of one workgroup of k_ss_ola
constexpr int MIN_WINDOW = 4;   // the packed transform has at least two points

enum Mode { MODE_ADAPTIVE = 0, MODE_STATIC = 1 };
enum Power { POWER_ONE = 1, POWER_TWO = 2, POWER_ANY = 0 };

struct Frames {
    int W, lgW, step, n_frames;
    int64_t n;  // samples of a stream
    __host__ __device__ int bins() const { return W / 2 + 1; }
    __host__ __device__ size_t pitch() const { return (size_t)W + 2; }  // doubles of a frame's slot
};

// dynamic LDS of k_ss_analyze and k_ss_synth: the W / 2 points and NT partial sums behind them
inline size_t frame_lds(int W) { return (size_t)(W / 2) * sizeof(double2) + NT * sizeof(double); }

template <typename T>
struct AnalyzeArgs {
    Src<T> x;
    Frames fr;
    const double* win;  // [W] analysis window
    const double2* tw;  // [W / 2]: exp(-2 pi i k / W)
    double thr_db;
    double2* spec;      // [streams][frames][W / 2 + 1]
    uint8_t* gate;      // [streams][frames]: 1 where 10 log10(max(var, tiny)) < thr_db
    double* peak;       // [streams][frames]: the largest |sample| of the frame
};

template <typename T>
__global__ __launch_bounds__(NT) void k_ss_analyze(AnalyzeArgs<T> a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) double2 buf[];
    const int tid = threadIdx.x, f = blockIdx.x, s = blockIdx.y;
    const int W = a.fr.W, M = W / 2, lg = a.fr.lgW - 1;
    double* red = reinterpret_cast<double*>(buf + M);
    const int64_t first = (int64_t)f * a.fr.step - W;  // the frame's first sample, as an index into x
    auto sample = [&](int64_t i) { return (i >= 0 && i < a.fr.n) ? a.x.at(i, s) : 0.0; };
    double part = 0.0, pk = 0.0;
    for (int m = tid; m < M; m += NT) {
        const double v0 = sample(first + 2 * m), v1 = sample(first + 2 * m + 1);
        part += v0 + v1;
        pk = dsfx::nan_max(pk, dsfx::nan_max(fabs(v0), fabs(v1)));
        buf[__brev((unsigned)m) >> (32 - lg)] = make_double2(v0 * a.win[2 * m], v1 * a.win[2 * m + 1]);  // bit-reversed in
    }
    const double mean = dsfx::block_sum<NT>(part, red) / (double)W;
    part = 0.0;
    for (int m = tid; m < M; m += NT) {
        const double d0 = sample(first + 2 * m) - mean, d1 = sample(first + 2 * m + 1) - mean;
        part += d0 * d0 + d1 * d1;
    }
    const double var = dsfx::block_sum<NT>(part, red) / (double)W;
    pk = dsfx::block_peak<NT>(pk, red);
    if (tid == 0) {
        a.gate[(size_t)s * a.fr.n_frames + f] = 10.0 * log10(var < DBL_MIN ? DBL_MIN : var) < a.thr_db ? 1 : 0;
        a.peak[(size_t)s * a.fr.n_frames + f] = pk;
    }
    __syncthreads();
    f64c::radix2_lds(buf, M, lg, a.tw, 2, tid);
    // X[k] = (Z[k] + conj Z[M-k]) / 2 + W^k (Z[k] - conj Z[M-k]) / (2i), k = 0 .. M
    double2* out = a.spec + ((size_t)s * a.fr.n_frames + f) * (M + 1);
    for (int k = tid; k <= M; k += NT) {
        const double2 zk = buf[k & (M - 1)], zm = buf[(M - k) & (M - 1)];
        const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
        const double2 o = make_double2(0.5 * (zk.y + zm.y), -0.5 * (zk.x - zm.x));
        const double2 w = k < M ? a.tw[k] : make_double2(-1.0, 0.0);
        out[k] = make_double2(e.x + (o.x * w.x - o.y * w.y), e.y + (o.x * w.y + o.y * w.x));
    }
}

struct TrackArgs {
    double2* spec;        // [streams][frames][bins], rewritten in place
    const uint8_t* gate;  // [streams][frames] (adaptive)
    const double* table;  // [streams][bins]: |noise PSD|^(e / 2) (static)
    int bins, n_frames, mode;
    double ff, factor, expo;
};

template <int POWER>
__device__ __forceinline__ double ss_raise(double v, double e) {
    return POWER == POWER_ONE ? v : (POWER == POWER_TWO ? v * v : pow(v, e));
}
template <int POWER>
__device__ __forceinline__ double ss_root(double v, double e) {
    return POWER == POWER_ONE ? v : (POWER == POWER_TWO ? sqrt(v) : pow(v, 1.0 / e));
}

inline int track_bin_blocks(int bins) { return (bins + NT - 1) / NT; }
inline int track_frame_tiles(int n_frames, int mode) { return mode == MODE_ADAPTIVE ? 1 : (n_frames + TRACK_TILE - 1) / TRACK_TILE; }

// grid = (track_bin_blocks x track_frame_tiles, streams), the bin blocks fastest
template <int POWER>
__global__ __launch_bounds__(NT) void k_ss_track(TrackArgs a) {
#pragma clang fp contract(off)
    const int blocks = (a.bins + NT - 1) / NT, tile = (int)(blockIdx.x / (unsigned)blocks);
    const int k = (int)(blockIdx.x % (unsigned)blocks) * NT + threadIdx.x, s = blockIdx.y, F = a.n_frames;
    if (k >= a.bins) return;
    const bool adaptive = a.mode == MODE_ADAPTIVE;
    const int f_begin = adaptive ? 0 : tile * TRACK_TILE;
    const int f_end = adaptive ? F : min(F, f_begin + TRACK_TILE);
    double2* col = a.spec + (size_t)s * F * a.bins + k;
    const uint8_t* gate = a.gate + (size_t)s * F;
    const double keep = 1.0 - a.ff;
    double noise = 0.0;
    double term = adaptive ? 0.0 : a.factor * a.table[(size_t)s * a.bins + k];
    for (int f0 = f_begin; f0 < f_end; f0 += TRACK_TILE) {
        double2 v[TRACK_TILE];
        bool g[TRACK_TILE];
#pragma unroll
        for (int u = 0; u < TRACK_TILE; ++u) {
            const int f = f0 + u;
            v[u] = f < f_end ? col[(size_t)f * a.bins] : make_double2(0.0, 0.0);
            g[u] = adaptive && f < f_end && gate[f] != 0;
        }
#pragma unroll
        for (int u = 0; u < TRACK_TILE; ++u) {
            const int f = f0 + u;
            if (f >= f_end) break;
            const double mag = sqrt(v[u].x * v[u].x + v[u].y * v[u].y);
            if (adaptive) {
                if (g[u]) noise = noise * a.ff + mag * keep;
                term = a.factor * ss_raise<POWER>(noise, a.expo);
            }
            double rest = ss_raise<POWER>(mag, a.expo) - term;
            rest = rest < 0.0 ? 0.0 : rest;  // (a NaN stays one, as numpy's clip keeps it)
            const double now = ss_root<POWER>(rest, a.expo);
            // the phase is kept; exp(1j angle(0)) = 1
            const double scale = now / mag;
            col[(size_t)f * a.bins] = mag > 0.0 ? make_double2(v[u].x * scale, v[u].y * scale) : make_double2(now, 0.0);
        }
    }
}

struct SynthArgs {
    double2* spec;      // [streams][frames][W / 2 + 1]; a frame's W samples overwrite its bins
    Frames fr;
    const double* win;  // [W] synthesis window
    const double2* tw;
};

// grid = (frames, streams); numpy's irfft: the imaginary parts of bin 0 and bin W / 2 do not count
__global__ __launch_bounds__(NT) void k_ss_synth(SynthArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) double2 buf[];
    const int tid = threadIdx.x, f = blockIdx.x, s = blockIdx.y;
    const int W = a.fr.W, M = W / 2, lg = a.fr.lgW - 1;
    double2* slot = a.spec + ((size_t)s * a.fr.n_frames + f) * (M + 1);
    // Z[k] = (X[k] + conj X[M-k]) + i conj(W^k) (X[k] - conj X[M-k]): twice the transform of even + i odd samples
    for (int k = tid; k < M; k += NT) {
        double2 xk = slot[k], xm = slot[M - k];
        if (k == 0) xk.y = 0.0, xm.y = 0.0;
        const double2 e = make_double2(xk.x + xm.x, xk.y - xm.y), d = make_double2(xk.x - xm.x, xk.y + xm.y);
        const double2 w = a.tw[k];
        const double2 o = make_double2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);
        buf[__brev((unsigned)k) >> (32 - lg)] = make_double2(e.x - o.y, e.y + o.x);
    }
    __syncthreads();  // (every bin is read before any sample is stored below: the stages' barriers lie between)
    f64c::radix2_lds<true>(buf, M, lg, a.tw, 2, tid);
    const double scale = 1.0 / (double)W;
    double2* out = slot;  // samples 2 m and 2 m + 1 as one 16-byte store
    for (int m = tid; m < M; m += NT) {
        const double2 z = buf[m];
        out[m] = make_double2(z.x * scale * a.win[2 * m], z.y * scale * a.win[2 * m + 1]);
    }
}

struct OlaArgs {
    const double* frames;  // [streams][frames] slots of W + 2 doubles, the first W the windowed samples
    Frames fr;
    const double* win;     // [W] synthesis window, squared here for the envelope
    double floor;          // the envelope is clipped from below at this; negative: not clipped
    double* yd;            // [streams][n]
    double* peak;          // [streams][gridDim.x]: the largest |output| of the workgroup's samples
};

// grid = (ceil(n / OLA_TILE), streams)
__global__ __launch_bounds__(OLA_TILE) void k_ss_ola(OlaArgs a) {
#pragma clang fp contract(off)
    __shared__ double sh[OLA_TILE];
    const int s = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * OLA_TILE + threadIdx.x;
    const bool live = j < a.fr.n;  // (every lane reaches the reduction's barriers)
    const int W = a.fr.W, step = a.fr.step, F = a.fr.n_frames;
    const int64_t i = j + W;  // the padded sample that is kept as output sample j
    const int64_t f_lo = (j + step) / step;  // ceil((i - W + 1) / step)
    const int64_t f_hi = !live ? f_lo - 1 : (i / step < F ? i / step : (int64_t)F - 1);
    const double* base = a.frames + (size_t)s * F * a.fr.pitch();
    double acc = 0.0, env = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
        const int o = (int)(i - f * step);  // 0 <= o < W by the choice of f_lo and f_hi
        const double w = a.win[o];
        acc += base[(size_t)f * a.fr.pitch() + o];
        env += w * w;
    }
    if (a.floor >= 0.0 && env < a.floor) env = a.floor;
    if (env > DBL_MIN) acc /= env;
    if (live) a.yd[(size_t)s * a.fr.n + j] = acc;
    const double pk = dsfx::block_peak<OLA_TILE>(fabs(acc), sh);  // (a lane past the end holds 0)
    if (threadIdx.x == 0) a.peak[(size_t)s * gridDim.x + blockIdx.x] = pk;
}

struct PeakArgs {
    const double* frame_peak;  // [streams][n_frame] of k_ss_analyze
    const double* block_peak;  // [streams][n_block] of k_ss_ola
    int n_frame, n_block;
    double *st_in, *st_out;    // [streams][dsfx::STAT] as k_fx_stats leaves them, the peak first; the rest 0
};

// grid = (streams, 2): y = 0 the input's peak, y = 1 the output's
__global__ __launch_bounds__(NT) void k_ss_peak(PeakArgs a) {
    __shared__ double sh[NT];
    const int s = blockIdx.x;
    const bool out = blockIdx.y != 0;
    const int n = out ? a.n_block : a.n_frame;
    const double* part = (out ? a.block_peak : a.frame_peak) + (size_t)s * n;
    double pk = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) pk = dsfx::nan_max(pk, part[i]);
    pk = dsfx::block_peak<NT>(pk, sh);
    if (threadIdx.x != 0) return;
    double* st = (out ? a.st_out : a.st_in) + (size_t)s * dsfx::STAT;
    st[0] = pk;
    st[1] = st[2] = st[3] = 0.0;
}

}  // namespace dsss
