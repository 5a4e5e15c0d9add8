// Per-channel sums over a pair of signals, float64, for distances.snr and distances.si_sdr (the reference's
// _snr and _sisdr, distances/_distances.py:64-101): in fixed order, without atomics, the same bits on every call.
// With the per-channel parameters (alpha, mu_a, mu_b), all zero where none are given, one pass returns
//     sum (a - mu_a)^2,  sum (b - mu_b)^2,  sum a b,  sum a,  sum b,  sum (alpha a - b)^2.
// A first pass without parameters gives the moments (the means, alpha = <a, b> / <a, a>); a second pass with them
// gives the centred sums of the reference's rms (it is numpy's std) and si_sdr's residual TERM BY TERM -- neither is
// formed from the moments, which cancels when b is close to alpha a or a mean is large.  gfx950.
//   k_pair_partial  one workgroup per SPAN samples of one channel: lane t adds samples t, t + NT, ... in order, then a
//                   tree over the lanes.
//   k_pair_final    one workgroup per channel: the workgroups' partial sums, lane t adding partials t, t + NT, ...,
//                   then the same tree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsdist {

constexpr int NT = 256;              // lanes per workgroup
constexpr int PER_LANE = 16;         // samples per lane
constexpr int SPAN = NT * PER_LANE;  // samples per workgroup
constexpr int NS = 6;                // sums per channel

template <typename T>
struct PairArgs {
    const T *a, *b;
    int64_t sac, san, sbc, sbn;  // sample n of channel c at a[c sac + n san] (sac = 0: one channel for all), b likewise
    int64_t n;
    int n_wg;                    // ceil(n / SPAN)
    const double* par;           // [n_ch][3]: alpha, mu_a, mu_b; or null (zeros)
    double* partial;             // [n_ch][n_wg][NS]
};

// the sums over the workgroup's lanes, fixed tree; the result is valid in every lane
__device__ inline void tree(double (&v)[NS], double* red) {
    const int t = threadIdx.x;
    for (int k = 0; k < NS; ++k) red[k * NT + t] = v[k];
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < NS; ++k) red[k * NT + t] += red[k * NT + t + s];
        __syncthreads();
    }
    for (int k = 0; k < NS; ++k) v[k] = red[k * NT];
}

// grid = (n_wg, n_ch), block = NT
template <typename T>
__global__ __launch_bounds__(NT) void k_pair_partial(PairArgs<T> p) {
    __shared__ double red[NS * NT];
    const int c = blockIdx.y, t = threadIdx.x;
    const T* a = p.a + (int64_t)c * p.sac;
    const T* b = p.b + (int64_t)c * p.sbc;
    const double al = p.par ? p.par[3 * c] : 0.0, ma = p.par ? p.par[3 * c + 1] : 0.0, mb = p.par ? p.par[3 * c + 2] : 0.0;
    double v[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t n0 = (int64_t)blockIdx.x * SPAN;
    for (int i = 0; i < PER_LANE; ++i) {
        const int64_t nn = n0 + (int64_t)i * NT + t;
        if (nn >= p.n) break;
        const double x = (double)a[nn * p.san], y = (double)b[nn * p.sbn];
        const double xc = x - ma, yc = y - mb, r = al * x - y;
        v[0] = fma(xc, xc, v[0]);
        v[1] = fma(yc, yc, v[1]);
        v[2] = fma(x, y, v[2]);
        v[3] += x;
        v[4] += y;
        v[5] = fma(r, r, v[5]);
    }
    tree(v, red);
    if (t == 0)
        for (int k = 0; k < NS; ++k) p.partial[((size_t)c * p.n_wg + blockIdx.x) * NS + k] = v[k];
}

// grid = n_ch, block = NT: out[c][NS]
__global__ __launch_bounds__(NT) void k_pair_final(const double* partial, int n_wg, double* out) {
    __shared__ double red[NS * NT];
    const int c = blockIdx.x, t = threadIdx.x;
    double v[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int w = t; w < n_wg; w += NT)
        for (int k = 0; k < NS; ++k) v[k] += partial[((size_t)c * n_wg + w) * NS + k];
    tree(v, red);
    if (t == 0)
        for (int k = 0; k < NS; ++k) out[c * NS + k] = v[k];
}

// ---- frequency-weighted segmental SNR (distances.fw_snr_seg; _fw_snr_seg_per_channel, distances/_distances.py:104-195) ----
// The band signals of x and xhat (real parts of the gammatone bank's outputs) lie in HBM as float64 planar
// (band, channel, sample).  A chunk of frames is worked on at a time; its columns are ordered (frame, band, channel).
//   k_fw_frame   one complex column per (frame, band, channel): x_band w + i xhat_band w, zeros past the signal's end.
//   (the float64 transform of kernels_fft64.hpp, one per column, gives both spectra: X is the conjugate-even part of the
//    result Z, Xhat the conjugate-odd part)
//   k_fw_reduce  one workgroup per (frame, channel), the bands in turn: |X|, |Xhat| on bins 0 .. Lw / 2, their sums
//                (block reductions), W = |X|^gamma, the normalised spectra; every lane adds
//                log10(X^2 / (X - Xhat + 1e-30)^2) W and W for its own bins (k = lane, lane + NT, ...) into two rows of
//                LDS that no other lane touches; then the mean over the bins of 10 snr / weights, clipped.
//   k_fw_mean    one workgroup per channel: the mean over the frames.
// A frame whose normalising sum is zero gives NaN, as in the reference; NaN passes the clip (its comparisons are false).
struct FrameArgs {
    const double *xb, *xhb;  // [n_band][n_ch_x][n], [n_band][n_ch][n]
    const double* win;       // [lw]
    int64_t n, hop, frame0;  // the chunk's first frame
    int lw, n_band, n_ch, n_ch_x;
    int64_t n_cols, ld;
    double2* z;              // column col at z + col ld
};

// grid = (ceil(lw / NT), n_cols)
__global__ __launch_bounds__(NT) void k_fw_frame(FrameArgs p) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= p.lw) return;
    const int64_t col = blockIdx.y;
    const int c = (int)(col % p.n_ch), b = (int)((col / p.n_ch) % p.n_band);
    const int64_t m = p.frame0 + col / ((int64_t)p.n_ch * p.n_band);
    const int64_t nn = m * p.hop + t;
    double2 v = make_double2(0.0, 0.0);
    if (nn < p.n) {
        const double w = p.win[t];
        v.x = p.xb[((int64_t)b * p.n_ch_x + (p.n_ch_x == 1 ? 0 : c)) * p.n + nn] * w;
        v.y = p.xhb[((int64_t)b * p.n_ch + c) * p.n + nn] * w;
    }
    p.z[col * p.ld + t] = v;
}

struct ReduceArgs {
    const double2* z;  // the transformed columns
    int64_t ld;
    int lw, n_band, n_ch;
    double gamma, lo, hi;
    int64_t frame0;
    double* frames;    // [n_frames][n_ch]
};

__device__ inline void tree2(double& a, double& b, double* red) {
    const int t = threadIdx.x;
    __syncthreads();  // (the previous use of red is read)
    red[t] = a;
    red[NT + t] = b;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[t] += red[t + s];
            red[NT + t] += red[NT + t + s];
        }
        __syncthreads();
    }
    a = red[0];
    b = red[NT];
}

// |X[k]| and |Xhat[k]| from Z = FFT(x + i xhat): X = (Z[k] + conj Z[N - k]) / 2, Xhat = (Z[k] - conj Z[N - k]) / 2i
__device__ inline void pair_mags(const double2* col, int k, int lw, double& ax, double& ah) {
    const double2 u = col[k], v = col[k == 0 ? 0 : lw - k];
    ax = 0.5 * hypot(u.x + v.x, u.y - v.y);
    ah = 0.5 * hypot(u.x - v.x, u.y + v.y);
}

__host__ __device__ inline size_t fw_reduce_lds_bytes(int lw) { return sizeof(double) * (2 * (size_t)(lw / 2 + 1) + 2 * NT); }

// grid = (frames of the chunk, n_ch), block = NT; dynamic LDS = fw_reduce_lds_bytes(lw)
__global__ __launch_bounds__(NT) void k_fw_reduce(ReduceArgs p) {
    extern __shared__ double fwlds[];
    const int t = threadIdx.x, nb = p.lw / 2 + 1, c = blockIdx.y;
    double* snr = fwlds;
    double* wts = snr + nb;
    double* red = wts + nb;
    for (int k = t; k < nb; k += NT) snr[k] = wts[k] = 0.0;
    for (int b = 0; b < p.n_band; ++b) {
        const double2* col = p.z + (((int64_t)blockIdx.x * p.n_band + b) * p.n_ch + c) * p.ld;
        double sx = 0.0, sh = 0.0;
        for (int k = t; k < nb; k += NT) {
            double ax, ah;
            pair_mags(col, k, p.lw, ax, ah);
            sx += ax;
            sh += ah;
        }
        tree2(sx, sh, red);
        for (int k = t; k < nb; k += NT) {
            double ax, ah;
            pair_mags(col, k, p.lw, ax, ah);
            const double w = pow(ax, p.gamma);
            const double xn = ax / sx, xh = ah / sh;  // normalise, then subtract
            const double d = xn - xh + 1e-30;
            snr[k] += log10((xn * xn) / (d * d)) * w;
            wts[k] += w;
        }
    }
    double v = 0.0, unused = 0.0;
    for (int k = t; k < nb; k += NT) v += 10.0 * snr[k] / wts[k];
    tree2(v, unused, red);
    if (t == 0) {
        v /= (double)nb;
        if (v < p.lo) v = p.lo;
        if (v > p.hi) v = p.hi;
        p.frames[(p.frame0 + blockIdx.x) * p.n_ch + c] = v;
    }
}

// grid = n_ch, block = NT: out[c] = mean over the frames
__global__ __launch_bounds__(NT) void k_fw_mean(const double* frames, int64_t n_frames, int n_ch, double* out) {
    __shared__ double red[2 * NT];
    const int c = blockIdx.x, t = threadIdx.x;
    double v = 0.0, unused = 0.0;
    for (int64_t m = t; m < n_frames; m += NT) v += frames[m * n_ch + c];
    tree2(v, unused, red);
    if (t == 0) out[c] = v / (double)n_frames;
}

}  // namespace dsdist
