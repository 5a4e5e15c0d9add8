// Continuous wavelet transform (transforms.cwt of the reference) and its synchrosqueezing.
//
// Row f of the scalogram is the "same"-mode convolution of every channel with the complex taps w_f:
//     S[f, n, c] = sum_k w_f[k] x_c[n + h_f - k],   0 <= n < N,
// h_f = (L_f - 1) // 2 for the full wavelet.  The host crops each wavelet to the taps that can meet the signal
// (k in [h - N + 1, h + N - 1]) and lowers h_f by what it cut at the front, so a wavelet longer than the signal
// costs a transform of about 4N points, not 2 L.
//
// Overlap-save in size classes.  The frequencies of one class share one power-of-two block length M >= 2 L_f and
// one segment layout: block b holds x[b V - cc + j], j < M (zeros outside the signal), with cc the class's largest
// L_f - 1 - h_f.  For every frequency of the class the circular product with the tap spectrum is the linear
// convolution at j >= L_f - 1, and output sample n = b V + t sits at j = t + h_f + cc.  V = M - max(h_f) - cc.
//   k_cwt_fwd<M>   one real block pair (blocks 2q, 2q + 1 of ONE channel as real / imaginary part) -> its M-point
//                  spectrum, computed ONCE per class and shared by all the class's wavelets
//   k_cwt_wspec<M> the wavelet's full complex spectrum (taps / M, zero padded), once per frequency
//   k_cwt_inv<M>   per (block, channel, frequency): unpack the block from the pair spectrum, multiply, inverse
//                  M-point transform in LDS, store the V valid samples as complex64 straight into (F, N, C)
// The two halves of a pair are blocks of the same channel, never two channels: the float32 transform's rounding error is
// proportional to the pair's norm, so a channel paired with one 60 dB hotter would leave 1e-6 of its OWN peak (the
// contract of every row), while two blocks of one channel are both held to that channel's peak.  The partner of the last
// block of an odd count is zeros, and a silent channel's rows are exactly zero.
// Blocks beyond one workgroup's LDS (M >= 2^15) take the four-step route (kernels_bigfft.hpp, N1 = 1024): the
// forward spectra through k_big_cols / k_big_rows, the inverse through k_cwt_bcols (the spectral product fused
// into its column load) and k_cwt_brows (the "same" window fused into its transposed store).  The inverse runs
// as conj(fft(conj(V))) with the 1/M folded into the tap spectrum.
//
// k_cwt_squeeze: one lane per (t, c) column of the device scalogram; gradient, |S|^2, phase transform and every
// comparison in float64 from the complex64 values, the frequencies in the caller's order, sums into the lane's own
// column (no atomics, the reference's summation order).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"
#include "kernels_bigfft.hpp"

namespace dscwt {
using namespace dsfft;

constexpr int MIN_M = 256;               // smallest block (shorter wavelets share it)
constexpr int MAX_LDS_M = 16384;         // LDS-resident route up to here, four-step beyond
constexpr int64_t MAX_TAPS = 1 << 18;    // longest wavelet (DS_ERR_UNSUP beyond)
constexpr int BIG_N1 = 1024;

// per-frequency record of a class (int64 so one upload carries it)
struct Freq {
    int64_t row;   // row of the output buffer
    int64_t toff;  // first cropped tap in the class's tap array
    int64_t len;   // cropped taps
    int64_t j0;    // position of output sample b V in block b: h_f + cc
};

// block pairs of a class: blocks 2q and 2q + 1 of one channel share a transform
__host__ __device__ __forceinline__ int n_block_pairs(int n_blocks) { return (n_blocks + 1) / 2; }

// two real segments of one channel -> complex block: z = xc[sa] + i xc[sa + V]; zeros outside the signal and, with
// has_b false (no block 2q + 1), in the imaginary part
__device__ __forceinline__ float2 seg_pair(const float* __restrict__ xc, int64_t n_samples, int64_t sa, int64_t V,
                                           bool has_b) {
    float2 z = make_float2(0.f, 0.f);
    const int64_t sb = sa + V;
    if (sa >= 0 && sa < n_samples) z.x = xc[sa];
    if (has_b && sb >= 0 && sb < n_samples) z.y = xc[sb];
    return z;
}

// the spectrum of block 2q (odd = false) or 2q + 1 (odd) from the pair spectrum Z at bins k and (M - k) mod M
__device__ __forceinline__ float2 unpack(float2 P, float2 Qc, bool odd) {
    return odd ? make_float2(0.5f * (P.y + Qc.y), -0.5f * (P.x - Qc.x))
               : make_float2(0.5f * (P.x + Qc.x), 0.5f * (P.y - Qc.y));
}

struct FwdArgs {
    const float* x;     // planar fp32, channel ch[c] at x + ch[c] * ld
    int64_t ld, n_samples;
    const int* ch;      // [n_ch] device
    int n_ch, n_blocks;
    int64_t V, cc;
    float2* Z;          // [channel][block pair][M]
    const float2* tw;
};

template <int M>
__global__ __launch_bounds__(Plan<M>::NT) void k_cwt_fwd(FwdArgs p) {
    extern __shared__ __align__(16) float2 lds[];
    const int tid = threadIdx.x, q = blockIdx.x, c = blockIdx.y;
    const int64_t s0 = (int64_t)(2 * q) * p.V - p.cc;
    const float* xc = p.x + (int64_t)p.ch[c] * p.ld;
    const bool has_b = 2 * q + 1 < p.n_blocks;
    for (int j = tid; j < M; j += Plan<M>::NT) lds[lidx(j)] = seg_pair(xc, p.n_samples, s0 + j, p.V, has_b);
    __syncthreads();
    float2 v[Plan<M>::VMAX];
    fft<M, false, false, false>(v, lds, p.tw, tid);
    __syncthreads();
    float2* z = p.Z + ((int64_t)c * n_block_pairs(p.n_blocks) + q) * M;
    for (int k = tid; k < M; k += Plan<M>::NT) z[k] = lds[lidx(k)];
}

struct WspecArgs {
    const float2* taps;  // class taps (cropped), complex64
    const Freq* fr;      // [nf]
    float inv_m;         // 1 / M
    float2* W;           // [nf][M]
    const float2* tw;
};

template <int M>
__global__ __launch_bounds__(Plan<M>::NT) void k_cwt_wspec(WspecArgs p) {
    extern __shared__ __align__(16) float2 lds[];
    const int tid = threadIdx.x, fi = blockIdx.x;
    const Freq f = p.fr[fi];
    for (int j = tid; j < M; j += Plan<M>::NT) {
        float2 w = make_float2(0.f, 0.f);
        if (j < f.len) {
            w = p.taps[f.toff + j];
            w.x *= p.inv_m;
            w.y *= p.inv_m;
        }
        lds[lidx(j)] = w;
    }
    __syncthreads();
    float2 v[Plan<M>::VMAX];
    fft<M, false, false, false>(v, lds, p.tw, tid);
    __syncthreads();
    float2* o = p.W + (int64_t)fi * M;
    for (int k = tid; k < M; k += Plan<M>::NT) o[k] = lds[lidx(k)];
}

struct InvArgs {
    const float2* Z;   // [channel][block pair][M]
    const float2* W;   // [nf][M], scaled by 1 / M
    const Freq* fr;
    int n_ch, n_blocks;
    int64_t V, n_samples;
    float2* out;       // (rows, N, C)
    const float2* tw;
};

template <int M>
__global__ __launch_bounds__(Plan<M>::NT) void k_cwt_inv(InvArgs p) {
    extern __shared__ __align__(16) float2 lds[];
    const int tid = threadIdx.x, b = blockIdx.x, c = blockIdx.y, fi = blockIdx.z;
    const Freq f = p.fr[fi];
    const float2* z = p.Z + ((int64_t)c * n_block_pairs(p.n_blocks) + (b >> 1)) * M;
    const float2* w = p.W + (int64_t)fi * M;
    const bool odd = b & 1;
    for (int k = tid; k < M; k += Plan<M>::NT)
        lds[lidx(k)] = cmul(unpack(z[k], z[(M - k) & (M - 1)], odd), w[k]);
    __syncthreads();
    float2 v[Plan<M>::VMAX];
    fft<M, true, false, false>(v, lds, p.tw, tid);
    __syncthreads();
    const int64_t n0 = (int64_t)b * p.V;
    const int64_t nv = p.n_samples - n0 < p.V ? p.n_samples - n0 : p.V;
    float2* o = p.out + (f.row * p.n_samples + n0) * p.n_ch + c;
    for (int t = tid; t < nv; t += Plan<M>::NT) o[(int64_t)t * p.n_ch] = lds[lidx((int)f.j0 + t)];
}

// ---- four-step route (M = 1024 * n2) ----
// complex segments of every (channel, block pair) into zs[channel][block pair][M], for k_big_cols / k_big_rows
struct SegArgs {
    const float* x;
    int64_t ld, n_samples;
    const int* ch;
    int n_ch, n_blocks;
    int64_t V, cc, M;
    float2* zs;
};
__global__ void k_cwt_segments(SegArgs p) {
    const int64_t bt = blockIdx.y;  // channel * block pairs + block pair
    const int nbp = n_block_pairs(p.n_blocks);
    const int c = (int)(bt / nbp), q = (int)(bt % nbp);
    const int64_t s0 = (int64_t)(2 * q) * p.V - p.cc;
    const float* xc = p.x + (int64_t)p.ch[c] * p.ld;
    const bool has_b = 2 * q + 1 < p.n_blocks;
    float2* z = p.zs + bt * p.M;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.M; j += (int64_t)gridDim.x * blockDim.x)
        z[j] = seg_pair(xc, p.n_samples, s0 + j, p.V, has_b);
}

// zero-padded taps / M of every frequency of the class into zw[fi][M]
struct PadArgs {
    const float2* taps;
    const Freq* fr;
    int64_t M;
    float inv_m;
    float2* zw;
};
__global__ void k_cwt_pad(PadArgs p) {
    const int fi = blockIdx.y;
    const Freq f = p.fr[fi];
    float2* z = p.zw + (int64_t)fi * p.M;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.M; j += (int64_t)gridDim.x * blockDim.x) {
        float2 w = make_float2(0.f, 0.f);
        if (j < f.len) {
            w = p.taps[f.toff + j];
            w.x *= p.inv_m;
            w.y *= p.inv_m;
        }
        z[j] = w;
    }
}

// item = (fi * n_blocks + b) * n_ch + c (item0 + blockIdx.y)
struct BigInvArgs {
    const float2* Z;   // [channel][block pair][M] natural order
    const float2* W;   // [nf][M] natural order, scaled by 1 / M
    const Freq* fr;
    int n_ch, n_blocks;
    int64_t item0, M, V, n_samples;
    int n2, ct;
    float2* zt;        // [item - item0][M]: columns stage output
    float2* out;       // (rows, N, C)
    const float2* tw;  // the length-1024 table (cols) or length-n2 table (rows)
};

__device__ __forceinline__ void big_item(const BigInvArgs& p, int64_t item, int& fi, int& b, int& c) {
    c = (int)(item % p.n_ch);
    const int64_t fb = item / p.n_ch;
    b = (int)(fb % p.n_blocks);
    fi = (int)(fb / p.n_blocks);
}

// k_big_cols with the load z[n] = conj(A_c[n] W_f[n]) (the inverse as a forward transform of the conjugate)
template <int N1>
__global__ __launch_bounds__(1024) void k_cwt_bcols(BigInvArgs p) {
    using C = Cfg<N1>;
    constexpr int CHS = dsbig::ch_stride<N1>();
    extern __shared__ __align__(16) float2 lds[];
    const int team = threadIdx.x / C::NT, tid = threadIdx.x % C::NT;
    const int j20 = blockIdx.x * p.ct;
    int fi, b, c;
    big_item(p, p.item0 + blockIdx.y, fi, b, c);
    const int64_t M = p.M;
    const float2* z = p.Z + ((int64_t)c * n_block_pairs(p.n_blocks) + (b >> 1)) * M;
    const float2* w = p.W + (int64_t)fi * M;
    const bool odd = b & 1;
    const int total = N1 * p.ct;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int j = i % p.ct, n1 = i / p.ct;
        const int64_t n = (int64_t)n1 * p.n2 + j20 + j;
        const float2 v = cmul(unpack(z[n], z[(M - n) & (M - 1)], odd), w[n]);
        lds[j * CHS + lidx(n1)] = make_float2(v.x, -v.y);
    }
    __syncthreads();
    float2* buf = lds + team * CHS;
    float2 v[C::VMAX];
    fft<N1, false, false, false>(v, buf, p.tw, tid);
    team_barrier<N1>();
    const int j2 = j20 + team;
    for (int k1 = tid; k1 < N1; k1 += C::NT) {
        double s, co;
        sincospi(-2.0 * (double)((int64_t)j2 * k1) / (double)M, &s, &co);
        buf[lidx(k1)] = cmul(buf[lidx(k1)], make_float2((float)co, (float)s));
    }
    __syncthreads();
    float2* zo = p.zt + (int64_t)blockIdx.y * M;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int j = i % p.ct, k1 = i / p.ct;
        zo[(int64_t)k1 * p.n2 + j20 + j] = lds[j * CHS + lidx(k1)];
    }
}

// k_big_rows whose transposed store keeps only the block's valid window, conjugated, in (rows, N, C)
template <int N2>
__global__ __launch_bounds__(1024) void k_cwt_brows(BigInvArgs p) {
    using C = Cfg<N2>;
    constexpr int CHS = dsbig::ch_stride<N2>();
    extern __shared__ __align__(16) float2 lds[];
    const int team = threadIdx.x / C::NT, tid = threadIdx.x % C::NT;
    const int k10 = blockIdx.x * p.ct;
    int fi, b, c;
    big_item(p, p.item0 + blockIdx.y, fi, b, c);
    const Freq f = p.fr[fi];
    const float2* zi = p.zt + (int64_t)blockIdx.y * p.M + (int64_t)(k10 + team) * N2;
    float2* buf = lds + team * CHS;
    float2 v[C::VMAX];
    for_each_reg<N2, C::R1>(tid, [&](int idx, int n) { v[idx] = zi[n]; });
    fft<N2, false, true, false>(v, buf, p.tw, tid);
    __syncthreads();
    const int64_t n0 = (int64_t)b * p.V;
    const int64_t nv = p.n_samples - n0 < p.V ? p.n_samples - n0 : p.V;
    float2* o = p.out + (f.row * p.n_samples + n0) * p.n_ch + c;
    const int total = N2 * p.ct;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int j = i % p.ct, k2 = i / p.ct;
        const int64_t t = (int64_t)k2 * BIG_N1 + k10 + j - f.j0;  // natural index m = k2 N1 + k1
        if (t >= 0 && t < nv) {
            const float2 r = lds[j * CHS + lidx(k2)];
            o[t * p.n_ch] = make_float2(r.x, -r.y);
        }
    }
}

// ---- synchrosqueezing (transforms/_transforms.py:227-301) ----
struct SqueezeArgs {
    const float2* S;        // (F, N, C) complex64
    int n_freq, n_ch;
    int64_t n_samples;
    const double* freqs;    // [F]
    const double* delta_f;  // [F]  delta_w * freqs
    const double* norm;     // [F]  (1 / (freqs / fs)) ** -1.5, or nullptr
    double fs;
    double2* out;           // (F, N, C) complex128
};

__global__ __launch_bounds__(256) void k_cwt_squeeze(SqueezeArgs p) {
#pragma clang fp contract(off)
    const int64_t cols = p.n_samples * p.n_ch;
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= cols) return;
    const int64_t t = col / p.n_ch, FS = cols;  // row stride
    for (int f = 0; f < p.n_freq; ++f) p.out[f * FS + col] = make_double2(0.0, 0.0);
    const int64_t nx = t + 1 < p.n_samples ? col + p.n_ch : col;  // np.gradient: one-sided at the ends
    const int64_t pv = t > 0 ? col - p.n_ch : col;
    const bool interior = t > 0 && t + 1 < p.n_samples;
    for (int f = 0; f < p.n_freq; ++f) {
        const float2 s32 = p.S[f * FS + col];
        const double sr = s32.x, si = s32.y;
        const float2 a = p.S[f * FS + nx], b = p.S[f * FS + pv];
        double gr = (double)a.x - (double)b.x, gi = (double)a.y - (double)b.y;
        if (interior) {
            gr = gr / 2.0;
            gi = gi / 2.0;
        }
        const double mag = hypot(sr, si);
        double ph = 0.0;
        if (mag * mag > 1e-40) {
            // numpy's complex division (Smith), imaginary part of g / S
            double qi;
            if (fabs(sr) >= fabs(si)) {
                const double rat = si / sr, scl = 1.0 / (sr + si * rat);
                qi = (gi - gr * rat) * scl;
            } else {
                const double rat = sr / si, scl = 1.0 / (si + sr * rat);
                qi = (gi * rat - gr) * scl;
            }
            ph = fabs(qi / 2.0 / 3.141592653589793) * p.fs;
        }
        int ind = 0;
        double best = fabs(p.freqs[0] - ph);
        for (int k = 1; k < p.n_freq; ++k) {
            const double d = fabs(p.freqs[k] - ph);
            if (d < best) {
                best = d;
                ind = k;
            }
        }
        if (best > p.delta_f[f]) continue;
        double2& o = p.out[ind * FS + col];
        if (p.norm) {
            o.x += sr * p.norm[f];
            o.y += si * p.norm[f];
        } else {
            o.x += sr;
            o.y += si;
        }
    }
}

}  // namespace dscwt
