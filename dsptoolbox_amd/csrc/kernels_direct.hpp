// Direct sums with no transform behind them, float64, gfx950: the DFT at arbitrary frequencies (transforms.dft,
// transforms/_transforms.py:_dft_backend of the reference), the same sum under a Gaussian window per bin and channel
// (transfer_functions.window_frequency_dependent, _fdw_backend) and the band sums of complex smoothing
// (transfer_functions.complex_smoothing, _complex_smoothing_backend).
//   k_dft          part[chunk][k][c] = sum over the chunk's samples of x[n][c] w_k,c[n] exp(-2 pi i f_k n / fs).
//                  A workgroup owns FT frequencies x CT channels x one sample chunk; the SL lanes of a frequency take
//                  samples a + s, a + s + SL, ... and rotate by exp(-2 pi i f_k SL / fs), re-seeded from an exactly
//                  reduced phase every RESEED steps; the SL lane sums are added in lane order through LDS.
//                  Windowed (alpha given): every (bin, channel) walks only peak_c +- dist_k, the samples whose weight
//                  reaches the caller's floor.
//   k_dft_combine  out[k][c] = the chunk partials added in chunk order
//   k_csmooth      out[i][col] = sum_m W_i[m] v[lo_i + m][col] / sum_m W_i[m] on a real (bins, columns) array -- a
//                  complex spectrum is 2 C such columns.  One wave per bin, lanes stride the band, a fixed lane tree
//                  adds up; the grid runs from the last bin (the longest band) to the first.
//   k_colmap       squares or square roots of the leading columns (the power domains)
// No kernel uses atomics: results are the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsdirect {

constexpr int NT = 256;       // lanes of every kernel here
constexpr int FT = 16;        // k_dft: frequencies per workgroup
constexpr int SL = NT / FT;   // k_dft: sample lanes per frequency
constexpr int CT = 4;         // k_dft: channels per workgroup
constexpr int RESEED = 32;    // k_dft: rotation steps between two exactly reduced phases
constexpr int CHUNK_UNIT = 1024;  // k_dft: sample chunks are multiples of this
constexpr int WAVES = NT / 64;    // k_csmooth: bins per workgroup
constexpr int WCT = 8;            // k_csmooth: columns per wave

struct DftArgs {
    const void* x;       // element (n, c) at x[n ss + c cs], double or float
    int64_t ss, cs;
    int64_t n_samples;
    int n_ch;
    const double* freqs;  // [n_freq] Hz
    int64_t n_freq;
    double fs;
    const double* alpha;   // [n_freq] (windowed form)
    const int64_t* peak;   // [n_ch]
    const int64_t* dist;   // [n_freq]: samples further than this from the peak are skipped
    double half;
    int64_t chunk;
    double2* part;         // [n_chunks][n_freq][n_ch]
};

// exp(-2 pi i (r_hi + r_lo) n) with the product reduced exactly: hi + lo = r_hi n without rounding
__device__ __forceinline__ void unit_phase(double r_hi, double r_lo, double n, double* re, double* im) {
    const double h = r_hi * n, l = fma(r_hi, n, -h) + r_lo * n;
    sincospi(-2.0 * ((h - rint(h)) + l), im, re);
}

// the lane's share of [a, b): samples a + s, a + s + SL, ... for NC channels that share the rotation
template <typename T, bool WIN, int NC>
__device__ __forceinline__ void dft_walk(const DftArgs& p, int64_t a, int64_t b, int s, double r_hi, double r_lo,
                                         double step_re, double step_im, const T* const* col, double al, int64_t pk,
                                         double2* acc) {
    for (int64_t n = a + s; n < b;) {
        double wr, wi;
        unit_phase(r_hi, r_lo, (double)n, &wr, &wi);
        for (int j = 0; j < RESEED && n < b; ++j, n += SL) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                double v = (double)col[q][n * p.ss];
                if (WIN) {
                    const double d = (double)(n - pk) / p.half;
                    v *= exp(al * (-0.5 * (d * d)));
                }
                acc[q].x = fma(v, wr, acc[q].x);
                acc[q].y = fma(v, wi, acc[q].y);
            }
            const double t = wr * step_re - wi * step_im;
            wi = fma(wr, step_im, wi * step_re);
            wr = t;
        }
    }
}

// grid = (frequency tiles, sample chunks, channel tiles)
template <typename T, bool WIN>
__global__ __launch_bounds__(NT) void k_dft(DftArgs p) {
    __shared__ double2 red[NT][CT];
    const int tid = threadIdx.x, fk = tid / SL, s = tid % SL;
    const int64_t k = (int64_t)blockIdx.x * FT + fk;
    const int c0 = blockIdx.z * CT;
    const int64_t n0 = (int64_t)blockIdx.y * p.chunk;
    const int64_t n1 = n0 + p.chunk < p.n_samples ? n0 + p.chunk : p.n_samples;
    double2 acc[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) acc[q] = make_double2(0.0, 0.0);
    if (k < p.n_freq) {
        const double f = p.freqs[k];
        const double r_hi = f / p.fs, r_lo = fma(-r_hi, p.fs, f) / p.fs;  // f / fs to twice the precision
        double step_re, step_im;
        unit_phase(r_hi, r_lo, (double)SL, &step_re, &step_im);
        const T* col[CT];
#pragma unroll
        for (int q = 0; q < CT; ++q) {
            const int c = c0 + q < p.n_ch ? c0 + q : p.n_ch - 1;
            col[q] = (const T*)p.x + c * p.cs;
        }
        if (WIN) {
            const double al = p.alpha[k];
            const int64_t d = p.dist[k];
#pragma unroll
            for (int q = 0; q < CT; ++q) {
                const int64_t pk = p.peak[c0 + q < p.n_ch ? c0 + q : p.n_ch - 1];
                const int64_t a = pk - d > n0 ? pk - d : n0, b = pk + d + 1 < n1 ? pk + d + 1 : n1;
                dft_walk<T, true, 1>(p, a, b, s, r_hi, r_lo, step_re, step_im, col + q, al, pk, acc + q);
            }
        } else {
            dft_walk<T, false, CT>(p, n0, n1, s, r_hi, r_lo, step_re, step_im, col, 0.0, 0, acc);
        }
    }
#pragma unroll
    for (int q = 0; q < CT; ++q) red[tid][q] = acc[q];
    __syncthreads();
    if (tid < FT * CT) {
        const int fo = tid / CT, q = tid % CT;
        double2 sum = red[fo * SL][q];
        for (int l = 1; l < SL; ++l) {
            sum.x += red[fo * SL + l][q].x;
            sum.y += red[fo * SL + l][q].y;
        }
        const int64_t ko = (int64_t)blockIdx.x * FT + fo;
        if (ko < p.n_freq && c0 + q < p.n_ch) p.part[((int64_t)blockIdx.y * p.n_freq + ko) * p.n_ch + c0 + q] = sum;
    }
}

struct CombineArgs {
    const double2* part;  // [n_chunks][n_out]
    int64_t n_out;
    int n_chunks;
    double2* out;
};

__global__ __launch_bounds__(NT) void k_dft_combine(CombineArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_out) return;
    double2 sum = p.part[idx];
    for (int j = 1; j < p.n_chunks; ++j) {
        const double2 t = p.part[(int64_t)j * p.n_out + idx];
        sum.x += t.x;
        sum.y += t.y;
    }
    p.out[idx] = sum;
}

struct CsmoothArgs {
    const double* v;  // (n_bins, ld_in): the columns [0, n_cols) are smoothed
    int64_t ld_in;
    double* out;      // (n_bins, ld_out)
    int64_t ld_out;
    int n_cols;
    int64_t n_bins;
    const int *lo, *hi, *wlen, *pass;  // [n_bins]: the clipped band [lo, hi), the unclipped length, the copy flag
    const double *wx, *wy;             // [n_proto] the window prototype on linspace(-1, 1, n_proto)
    int n_proto;
};

// numpy.interp(10 ** linspace(log10 3, 0, wlen)[m] - 2, wx, wy)
__device__ __forceinline__ double band_weight(const CsmoothArgs& p, int m, int wlen) {
    const double start = 0.47712125471966244;  // log10(3)
    double y = start;
    if (wlen > 1) y = m == wlen - 1 ? 0.0 : (double)m * ((0.0 - start) / (double)(wlen - 1)) + start;
    const double x = pow(10.0, y) - 2.0;
    const int P = p.n_proto;
    if (x <= p.wx[0]) return p.wy[0];
    if (x >= p.wx[P - 1]) return p.wy[P - 1];
    int j = (int)((x + 1.0) * 0.5 * (double)(P - 1));
    j = j < 0 ? 0 : (j > P - 2 ? P - 2 : j);
    while (j < P - 2 && p.wx[j + 1] <= x) ++j;
    while (j > 0 && p.wx[j] > x) --j;
    const double slope = (p.wy[j + 1] - p.wy[j]) / (p.wx[j + 1] - p.wx[j]);
    return slope * (x - p.wx[j]) + p.wy[j];
}

// grid = (ceil(n_bins / WAVES), ceil(n_cols / WCT)); workgroup g holds the bins n_bins - 1 - (g WAVES + wave)
__global__ __launch_bounds__(NT) void k_csmooth(CsmoothArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t i = p.n_bins - 1 - ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (i < 0) return;
    const int c0 = blockIdx.y * WCT;
    if (p.pass[i]) {
        if (lane < WCT && c0 + lane < p.n_cols) p.out[i * p.ld_out + c0 + lane] = p.v[i * p.ld_in + c0 + lane];
        return;
    }
    const int lo = p.lo[i], eff = p.hi[i] - lo, wlen = p.wlen[i];
    double acc[WCT], sw = 0.0;
#pragma unroll
    for (int q = 0; q < WCT; ++q) acc[q] = 0.0;
    for (int m = lane; m < eff; m += 64) {
        const double w = band_weight(p, m, wlen);
        const double* row = p.v + (int64_t)(lo + m) * p.ld_in;
        sw += w;
#pragma unroll
        for (int q = 0; q < WCT; ++q) acc[q] = fma(w, row[c0 + q < p.n_cols ? c0 + q : p.n_cols - 1], acc[q]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        sw += __shfl_down(sw, off);
#pragma unroll
        for (int q = 0; q < WCT; ++q) acc[q] += __shfl_down(acc[q], off);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < WCT; ++q)
            if (c0 + q < p.n_cols) p.out[i * p.ld_out + c0 + q] = acc[q] / sw;
    }
}

struct ColmapArgs {
    double* v;  // (n_bins, ld): the columns [0, n_cols) are replaced
    int64_t n_bins, ld;
    int n_cols;
    int root;   // 0: v * v, 1: sqrt(v)
};

__global__ __launch_bounds__(NT) void k_colmap(ColmapArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_cols) return;
    double* e = p.v + idx / p.n_cols * p.ld + idx % p.n_cols;
    *e = p.root ? sqrt(*e) : *e * *e;
}

}  // namespace dsdirect
