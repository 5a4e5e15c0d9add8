// Latency estimation by cross-correlation (reference: standard.latency, standard/latency_delay.py:15-156; _latency,
// standard/_standard_backend.py:14-34; _fractional_latency, _get_fractional_impulse_peak_index and
// _get_correlation_of_latencies, helpers/latency.py:10-149, 218-265; _remove_ir_latency_from_phase, :152-181).
// float64 throughout, gfx950.  The transforms are those of kernels_fft64.hpp on its planar double2 arrays (column c at
// x + c ld); what is added here:
//   k_xmul         P[k] = B[k] conj(A[k]) over the n_fft bins of every pair, written over A.  Its inverse transform is
//                  the circular correlation r; scipy's full-mode correlate(b, a)[k] is r[(k - (Na - 1)) mod n_fft].
//   k_peak         argmax |x| over a row range per channel, the lowest index winning among equal values: every lane keeps
//                  a (value, index) pair over its rows in ascending order, the pairs are reduced over the wave by lane
//                  swaps and over the workgroup's four waves through LDS; k_peak_final reduces the workgroups' pairs.
//   k_window       rows [lo, lo + M) of the correlation, through the rotation and scaled, as a dense (M, C) real array:
//                  what the Hilbert transform of the window loads.
//   k_near         the 2 p + 2 values imag(h[d - p .. d + p + 1]) / M around each channel's peak; NaN for a row outside
//                  the window.
//   k_lag_partial  per (pair, candidate lag) row the sums over the overlapped span of the two signals, the delayed one
//   k_lag_final    read |lag| samples in: first sum x, sum y (MOMENTS false), then with the means the centred sums
//                  sum x'^2, sum y'^2, sum x'y' and r = sum x'y' / sqrt(sum x'^2 sum y'^2) clipped to [-1, 1].  The
//                  block partials and their tree are those of kernels_dist.hpp.
//   k_lat_phase    wrap(phase + 2 pi f tau) on a dense (bins, C) phase array, numpy's floor modulo.
// No atomics, every element has one writer, every sum a fixed order: a call returns the same bits every time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_dist.hpp"

namespace dslat {

constexpr int NT = 256;
constexpr int PEAK_SPAN = 4096;  // rows per workgroup of the peak search

struct XmulArgs {
    double2* x;     // planar: the columns of a (n_ch of them), then those of b (n_ch_b: n_ch, or 1 for every pair)
    int64_t n, ld;  // bins per column, column stride
    int n_ch, n_ch_b;
};

// grid = ceil(n n_ch / 256)
__global__ __launch_bounds__(NT) void k_xmul(XmulArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n * p.n_ch) return;
    const int64_t c = idx / p.n, k = idx - c * p.n;
    double2* e = p.x + c * p.ld + k;
    const double2 a = *e;
    const double2 b = p.x[(p.n_ch + (p.n_ch_b == 1 ? 0 : c)) * p.ld + k];
    *e = make_double2(fma(b.x, a.x, b.y * a.y), fma(b.y, a.x, -(b.x * a.y)));
}

// Row k of channel c is v[c * col_stride + ((k + rot) mod n_mod) * row_stride], doubles.  The correlation in a planar
// double2 array: col_stride = 2 ld, row_stride = 2 (the real parts), rot = n_fft - (Na - 1), n_mod = n_fft.  A
// sample-major (n, C) array: v + c with col_stride = 1, row_stride = C, rot = 0, n_mod = n.
struct RowView {
    const double* v;
    int64_t col_stride, row_stride, rot, n_mod;
    __device__ __forceinline__ double at(int c, int64_t k) const {
        int64_t j = k + rot;
        if (j >= n_mod) j -= n_mod;  // k < n_mod and rot <= n_mod (Na = 1: rot == n_mod), so j < 2 n_mod: one suffices
        return v[(int64_t)c * col_stride + j * row_stride];
    }
};

struct PeakArgs {
    RowView in;
    int64_t lo, hi;  // rows searched: [lo, hi)
    int n_wg;        // ceil((hi - lo) / PEAK_SPAN)
    double* pv;      // [n_ch][n_wg]: the workgroup's largest |x| (-1: it had no row)
    int64_t* pi;     // [n_ch][n_wg]: its row
    int64_t* peaks;  // [n_ch] (k_peak_final)
};

__device__ __forceinline__ void peak_take(double& v, int64_t& i, double v2, int64_t i2) {
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

// the best pair of the workgroup, valid in lane 0
__device__ inline void peak_block(double& v, int64_t& i, double* sv, int64_t* si) {
    for (int s = 32; s > 0; s >>= 1) {
        const double v2 = __shfl_down(v, s, 64);
        const int lo = __shfl_down((int)(i & 0xffffffff), s, 64), hi = __shfl_down((int)(i >> 32), s, 64);
        peak_take(v, i, v2, ((int64_t)hi << 32) | (uint32_t)lo);
    }
    const int t = threadIdx.x;
    if ((t & 63) == 0) {
        sv[t >> 6] = v;
        si[t >> 6] = i;
    }
    __syncthreads();
    if (t == 0)
        for (int w = 1; w < NT / 64; ++w) peak_take(v, i, sv[w], si[w]);
}

// grid = (n_wg, n_ch)
__global__ __launch_bounds__(NT) void k_peak(PeakArgs p) {
    __shared__ double sv[NT / 64];
    __shared__ int64_t si[NT / 64];
    const int c = blockIdx.y, t = threadIdx.x;
    const int64_t k0 = p.lo + (int64_t)blockIdx.x * PEAK_SPAN;
    double v = -1.0;
    int64_t i = INT64_MAX;
    for (int j = 0; j < PEAK_SPAN / NT; ++j) {
        const int64_t k = k0 + (int64_t)j * NT + t;
        if (k >= p.hi) break;
        const double a = fabs(p.in.at(c, k));
        if (a > v) {  // ascending rows: an equal value later on does not replace
            v = a;
            i = k;
        }
    }
    peak_block(v, i, sv, si);
    if (t == 0) {
        p.pv[(size_t)c * p.n_wg + blockIdx.x] = v;
        p.pi[(size_t)c * p.n_wg + blockIdx.x] = i;
    }
}

// grid = n_ch: peaks[c]
__global__ __launch_bounds__(NT) void k_peak_final(PeakArgs p) {
    __shared__ double sv[NT / 64];
    __shared__ int64_t si[NT / 64];
    const int c = blockIdx.x, t = threadIdx.x;
    double v = -1.0;
    int64_t i = INT64_MAX;
    for (int w = t; w < p.n_wg; w += NT) peak_take(v, i, p.pv[(size_t)c * p.n_wg + w], p.pi[(size_t)c * p.n_wg + w]);
    peak_block(v, i, sv, si);
    if (t == 0) p.peaks[c] = i;
}

struct WindowArgs {
    RowView in;
    int64_t lo, m;  // rows [lo, lo + m)
    int n_ch;
    double scale;
    double* out;    // (m, n_ch)
};

// grid = ceil(m n_ch / 256); neighbouring lanes take neighbouring rows of one channel
__global__ __launch_bounds__(NT) void k_window(WindowArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.m * p.n_ch) return;
    const int64_t c = idx / p.m, k = idx - c * p.m;
    p.out[k * p.n_ch + c] = p.in.at((int)c, p.lo + k) * p.scale;
}

struct NearArgs {
    const double2* h;      // the window's analytic signal times m, planar
    int64_t ld, m, lo;
    const int64_t* peaks;  // [n_ch], rows of the whole array
    int n_ch, p;
    double* out;           // [n_ch][2 p + 2]
};

// grid = ceil(n_ch (2 p + 2) / 256)
__global__ __launch_bounds__(NT) void k_near(NearArgs a) {
    const int idx = blockIdx.x * NT + threadIdx.x, w = 2 * a.p + 2;
    if (idx >= a.n_ch * w) return;
    const int c = idx / w, j = idx - c * w;
    const int64_t row = a.peaks[c] - a.lo - a.p + j;
    a.out[idx] = row >= 0 && row < a.m ? a.h[(int64_t)c * a.ld + row].y / (double)a.m : __builtin_nan("");
}

// ---- Pearson's r of two channels, one of them read |lag| samples in ----------------------------------------------------
// Row j of the table pairs column col_t of t ("time_data" of _get_correlation_of_latencies) with column col_o of o
// ("other_time_data") at the integer lag: lag > 0 delays o, otherwise t; the delayed one loses its first |lag| samples
// and both are cut to n = min(len(delayed) - |lag|, len(undelayed)).  n < 2 gives NaN (the host refuses such a lag).
struct LagArgs {
    const double *t, *o;  // sample-major (n_t, n_ch_t), (n_o, n_ch_o)
    int64_t n_t, n_o;
    int n_ch_t, n_ch_o;
    const int64_t* rows;  // [n_rows][3]: col_t, col_o, lag
    int n_wg;             // workgroups per row: ceil(longest span / SPAN)
    const double* mean;   // [n_rows][2] (MOMENTS)
    double* partial;      // [n_rows][n_wg][NS]
    double* out;          // k_lag_final: the means [n_rows][2], or with MOMENTS r [n_rows]
};

struct LagSpan {
    const double *x, *y;  // the delayed one from its first kept sample, the undelayed one
    int64_t sx, sy, n;
};

__device__ __forceinline__ LagSpan lag_span(const LagArgs& p, int row) {
    const int64_t ct = p.rows[3 * row], co = p.rows[3 * row + 1], lag = p.rows[3 * row + 2];
    const int64_t s = lag < 0 ? -lag : lag;
    LagSpan r;
    const bool o_delayed = lag > 0;
    const int64_t n_del = o_delayed ? p.n_o : p.n_t, n_und = o_delayed ? p.n_t : p.n_o;
    r.n = n_del - s < n_und ? n_del - s : n_und;
    if (r.n < 0) r.n = 0;
    const double* tt = p.t + ct;
    const double* oo = p.o + co;
    r.sx = o_delayed ? p.n_ch_o : p.n_ch_t;
    r.sy = o_delayed ? p.n_ch_t : p.n_ch_o;
    r.x = (o_delayed ? oo : tt) + (r.n > 0 ? s * r.sx : 0);
    r.y = o_delayed ? tt : oo;
    return r;
}

// grid = (n_rows, n_wg)
template <bool MOMENTS>
__global__ __launch_bounds__(NT) void k_lag_partial(LagArgs p) {
    using namespace dsdist;
    __shared__ double red[NS * NT];
    const int row = blockIdx.x, wg = blockIdx.y, t = threadIdx.x;
    const LagSpan s = lag_span(p, row);
    const double mx = MOMENTS ? p.mean[2 * row] : 0.0, my = MOMENTS ? p.mean[2 * row + 1] : 0.0;
    double v[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t n0 = (int64_t)wg * SPAN;
    for (int i = 0; i < PER_LANE; ++i) {
        const int64_t nn = n0 + (int64_t)i * NT + t;
        if (nn >= s.n) break;
        const double x = s.x[nn * s.sx], y = s.y[nn * s.sy];
        if (MOMENTS) {
            const double xc = x - mx, yc = y - my;
            v[0] = fma(xc, xc, v[0]);
            v[1] = fma(yc, yc, v[1]);
            v[2] = fma(xc, yc, v[2]);
        } else {
            v[3] += x;
            v[4] += y;
        }
    }
    tree(v, red);
    if (t == 0)
        for (int k = 0; k < NS; ++k) p.partial[((size_t)row * p.n_wg + wg) * NS + k] = v[k];
}

// grid = n_rows
template <bool MOMENTS>
__global__ __launch_bounds__(NT) void k_lag_final(LagArgs p) {
    using namespace dsdist;
    __shared__ double red[NS * NT];
    const int row = blockIdx.x, t = threadIdx.x;
    double v[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int w = t; w < p.n_wg; w += NT)
        for (int k = 0; k < NS; ++k) v[k] += p.partial[((size_t)row * p.n_wg + w) * NS + k];
    tree(v, red);
    if (t != 0) return;
    const int64_t n = lag_span(p, row).n;
    if (!MOMENTS) {
        p.out[2 * row] = v[3] / (double)n;
        p.out[2 * row + 1] = v[4] / (double)n;
        return;
    }
    double r = v[2] / sqrt(v[0] * v[1]);  // a constant channel: 0 / 0, NaN as pearsonr gives it
    if (n < 2) r = __builtin_nan("");
    if (r > 1.0) r = 1.0;
    if (r < -1.0) r = -1.0;
    p.out[row] = r;
}

// ---- the latency's linear phase, before the unwrap ---------------------------------------------------------------------
struct LatPhaseArgs {
    double* ph;             // (n_bins, n_ch), in place
    int64_t n_bins;
    int n_ch;
    double delta_f, fs;
    const double* latency;  // [n_ch], samples
};

// grid = ceil(n_bins n_ch / 256): (x + pi) % (2 pi) - pi of x = phase + 2 pi f (latency / fs), f = k delta_f
__global__ __launch_bounds__(NT) void k_lat_phase(LatPhaseArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    const int64_t k = idx / p.n_ch, c = idx - k * p.n_ch;
    const double pi = 3.141592653589793, two_pi = 2.0 * pi;
    const double x = p.ph[idx] + two_pi * ((double)k * p.delta_f) * (p.latency[c] / p.fs);
    double m = fmod(x + pi, two_pi);
    if (m < 0.0) m += two_pi;  // numpy's modulo takes the divisor's sign
    p.ph[idx] = m - pi;
}

}  // namespace dslat
