// Variable-Q transform (reference: transforms.vqt, transforms/transforms.py:812-923; _get_kernels_vqt,
// transforms/_transforms.py:327-383) and the integer-ratio polyphase resampler it needs (scipy.signal.resample_poly with
// its default filter, one of `up` and `down` being 1).  float64 throughout, gfx950.  Arrays are sample-major with the
// channels fastest: (samples, C) real, (rows, samples, C) complex128.
//   k_vqt_decimate  out[m] = sum_k h[k] x[m D + half - k], half = (ntaps - 1) / 2: P(x, 1, D) for real samples.  The
//                   samples are read through a sample and a channel stride, float64 interleaved on the host's side or
//                   float32 planar where a device-resident signal lies, and widened as they are staged.
//   k_vqt_bank      z[i][m] = sum_l k_i[l] td[m + (L_i - 1) / 2 - l]: the same-mode convolution of one octave's samples
//                   with every kernel of the bank, all octaves in one launch.
//   k_vqt_interp    out[m] = sum_j h[p + U j] z[a + HW - j] for m = U a + p, j = 0 .. 2 HW: P(z, U, 1).  Of the 20 U + 1
//                   taps only every U-th meets a sample that is not a stuffed zero: 21 terms per output value.  A lane
//                   takes four outputs of one phase p, which share their taps and slide one window of inputs.  A row's
//                   output goes to row row0 + i row_step of its destination and stops at n_out samples, so the last
//                   stage writes the flipped, trimmed (F, N, C) result directly, each value once.
// A rate of 1 is the one-tap filter [1.0] (HW = 0, half = 0): the copy scipy returns early.  Terms outside the input are
// zeros staged in LDS.  No atomics, every element has one writer, every sum a fixed order: a call returns the same bits
// every time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsvqt {

constexpr int NT = 256;
constexpr int INTERP_R = 4;       // outputs of one phase per lane of k_vqt_interp
constexpr int INTERP_PASSES = 4;  // passes of a workgroup's lanes over its tile (interp_span)
constexpr int MAX_OCT = 7;     // octaves of one call: the first interpolation stage goes up to 2^6

// channels a workgroup takes together (they are neighbours in memory): 1, 2 or 4.  The sample tile of k_vqt_decimate and
// k_vqt_bank is NT / ch_group samples.
__host__ __device__ inline int ch_group(int n_ch) { return n_ch == 1 ? 1 : n_ch == 2 ? 2 : 4; }
__host__ __device__ inline int ch_shift(int cg) { return cg == 1 ? 0 : cg == 2 ? 1 : 2; }

template <typename T>
struct DecArgs {
    const T* x;      // sample n of channel c at x[n ss + c cs]
    int64_t ss, cs, n_in;
    int n_ch, cg;
    const double* h;  // [ntaps]
    int ntaps, D;
    double* out;      // (n_out, n_ch)
    int64_t n_out;
};

// doubles of LDS: the taps, then the staged span of (NT / cg - 1) D + ntaps samples of cg channels
__host__ __device__ inline size_t dec_lds_doubles(int ntaps, int D, int cg) {
    return (size_t)ntaps + ((size_t)(NT / cg - 1) * D + ntaps) * cg;
}

// grid = (ceil(n_out / (NT / cg)), ceil(n_ch / cg))
template <typename T>
__global__ __launch_bounds__(NT) void k_vqt_decimate(DecArgs<T> p) {
    extern __shared__ double lds[];
    double* hs = lds;
    double* xs = lds + p.ntaps;
    const int t = threadIdx.x, cg = p.cg, sh = ch_shift(cg), dt = NT >> sh, half = (p.ntaps - 1) / 2;
    const int64_t m0 = (int64_t)blockIdx.x * dt;
    const int c0 = blockIdx.y * cg;
    const int span = (dt - 1) * p.D + p.ntaps;
    const int64_t j0 = m0 * p.D - half;  // the first staged sample
    for (int k = t; k < p.ntaps; k += NT) hs[k] = p.h[k];
    for (int e = t; e < span * cg; e += NT) {
        int s, c;
        if (p.ss == 1) {  // planar: neighbouring lanes take neighbouring samples
            c = e / span;
            s = e - c * span;
        } else {
            s = e >> sh;
            c = e & (cg - 1);
        }
        const int64_t j = j0 + s;
        double v = 0.0;
        if (j >= 0 && j < p.n_in && c0 + c < p.n_ch) v = (double)p.x[j * p.ss + (int64_t)(c0 + c) * p.cs];
        xs[s * cg + c] = v;
    }
    __syncthreads();
    const int ml = t >> sh, cl = t & (cg - 1);
    const int64_t m = m0 + ml;
    if (m >= p.n_out || c0 + cl >= p.n_ch) return;
    const double* xp = xs + (size_t)(ml * p.D + p.ntaps - 1) * cg + cl;  // the sample tap 0 meets
    double acc = 0.0;
    for (int k = 0; k < p.ntaps; ++k) acc = fma(hs[k], xp[-(k * cg)], acc);
    p.out[m * p.n_ch + c0 + cl] = acc;
}

// One octave of the bank: its samples td + td_off (m, C) and its rows z + z_off (bins, m, C).
struct BankOct {
    int64_t td_off, z_off, m;
};

struct BankArgs {
    const double* td;
    const BankOct* oc;     // [n_oct]
    const int64_t* kdesc;  // [bins][2]: first tap, length
    const double2* ktaps;
    double2* z;
    int n_ch, cg, bins;
};

// bytes of LDS: the longest kernel's taps, then NT / cg + lmax - 1 samples of cg channels
__host__ __device__ inline size_t bank_lds_bytes(int lmax, int cg) {
    return (size_t)lmax * 16 + ((size_t)(NT / cg) + lmax - 1) * cg * 8;
}

// grid = (ceil(m_0 / (NT / cg)), ceil(n_ch / cg), n_oct bins)
__global__ __launch_bounds__(NT) void k_vqt_bank(BankArgs p) {
    extern __shared__ double2 lds2[];
    const int r = blockIdx.z, o = r / p.bins, i = r - o * p.bins;
    const BankOct oc = p.oc[o];
    const int t = threadIdx.x, cg = p.cg, sh = ch_shift(cg), bt = NT >> sh;
    const int64_t m0 = (int64_t)blockIdx.x * bt;
    if (m0 >= oc.m) return;  // (the whole workgroup: the lower octaves have fewer tiles)
    const int c0 = blockIdx.y * cg;
    const int64_t toff = p.kdesc[2 * i];
    const int L = (int)p.kdesc[2 * i + 1], h = (L - 1) / 2;
    double2* ks = lds2;
    double* xs = (double*)(lds2 + L);
    for (int l = t; l < L; l += NT) ks[l] = p.ktaps[toff + l];
    const int span = bt + L - 1;
    const int64_t j0 = m0 + h - (L - 1);  // the first staged sample
    const double* td = p.td + oc.td_off;
    for (int e = t; e < span * cg; e += NT) {
        const int s = e >> sh, c = e & (cg - 1);
        const int64_t j = j0 + s;
        xs[e] = (j >= 0 && j < oc.m && c0 + c < p.n_ch) ? td[j * p.n_ch + c0 + c] : 0.0;
    }
    __syncthreads();
    const int ml = t >> sh, cl = t & (cg - 1);
    const int64_t m = m0 + ml;
    if (m >= oc.m || c0 + cl >= p.n_ch) return;
    const double* xp = xs + (size_t)(ml + L - 1) * cg + cl;  // the sample tap 0 meets
    double re = 0.0, im = 0.0;
    for (int l = 0; l < L; ++l) {
        const double2 k = ks[l];
        const double x = xp[-(l * cg)];
        re = fma(k.x, x, re);
        im = fma(k.y, x, im);
    }
    p.z[oc.z_off + ((int64_t)i * oc.m + m) * p.n_ch + c0 + cl] = make_double2(re, im);
}

// One octave of an interpolation launch: row i of the input, n_in samples at in + in_off + i n_in C, goes to row
// row0 + i row_step of the destination at out + out_off, whose rows hold n_out samples (the output is cut there).
struct InterpOct {
    int64_t in_off, n_in, out_off, n_out, row0, row_step, taps_off, U, HW;
};

template <typename V>
struct InterpArgs {
    const V* in;
    V* out;
    const double* taps;  // octave o's 2 HW U + 1 taps at taps + taps_off
    const InterpOct* oc;
    int n_ch, cg, bins;
};

__device__ __forceinline__ void vqt_mad(double h, double z, double& acc) { acc = fma(h, z, acc); }
__device__ __forceinline__ void vqt_mad(double h, double2 z, double2& acc) {
    acc.x = fma(h, z.x, acc.x);
    acc.y = fma(h, z.y, acc.y);
}
__device__ __forceinline__ void vqt_zero(double& v) { v = 0.0; }
__device__ __forceinline__ void vqt_zero(double2& v) { v = make_double2(0.0, 0.0); }

// input samples whose outputs one workgroup takes: INTERP_R per lane and phase, and as many such groups as fill four
// passes of the workgroup's lanes over (group, phase, channel), at most 128.  The tile is interp_span U output samples
// and starts at a multiple of U.
__host__ __device__ inline int interp_span(int U, int cg) {
    const int g = INTERP_PASSES * NT / (U * cg);
    return INTERP_R * (g < 1 ? 1 : g > 128 ? 128 : g);
}
// doubles of LDS ahead of the samples: (2 HW + 1) U taps (those past 2 HW U are zeros), an even count
__host__ __device__ inline size_t interp_tap_doubles(int U, int HW) { return ((size_t)(2 * HW + 1) * U + 1) & ~(size_t)1; }
// staged input samples of one tile: the span and HW on either side
__host__ __device__ inline size_t interp_lds_bytes(int U, int HW, int cg, size_t elem) {
    return interp_tap_doubles(U, HW) * 8 + ((size_t)interp_span(U, cg) + 2 * HW) * cg * elem;
}

// grid = (ceil(longest n_out / (interp_span U)), ceil(n_ch / cg), octaves of the launch x bins).  A lane takes INTERP_R
// outputs of one phase and channel, U apart: they share their 2 HW + 1 taps, and their inputs are one window sliding by
// a sample per tap, so a tap costs one 8-byte and one sample read from LDS for INTERP_R multiply-adds.  HW is 10, or 0
// for the one-tap copy of a rate of 1.
template <typename V, int HW>
__global__ __launch_bounds__(NT) void k_vqt_interp(InterpArgs<V> p) {
    extern __shared__ double lds[];
    constexpr int R = INTERP_R, NJ = 2 * HW + 1;
    const int r_ = blockIdx.z, e = r_ / p.bins, i = r_ - e * p.bins;
    const InterpOct o = p.oc[e];
    const int t = threadIdx.x, cg = p.cg, sh = ch_shift(cg), c0 = blockIdx.y * cg;
    const int U = (int)o.U, A = interp_span(U, cg);
    const int64_t a0 = (int64_t)blockIdx.x * A, m0 = a0 * U;
    if (m0 >= o.n_out) return;  // (the whole workgroup)
    const int ntaps = 2 * HW * U + 1, nh = NJ * U;
    double* hs = lds;
    V* zs = (V*)(lds + interp_tap_doubles(U, HW));
    for (int k = t; k < nh; k += NT) hs[k] = k < ntaps ? p.taps[o.taps_off + k] : 0.0;
    const V* in = p.in + o.in_off + (int64_t)i * o.n_in * p.n_ch;
    const int nq = A + 2 * HW;  // input samples a0 - HW .. a0 + A - 1 + HW
    for (int el = t; el < nq * cg; el += NT) {
        const int s = el >> sh, c = el & (cg - 1);
        const int64_t q = a0 - HW + s;
        V v;
        vqt_zero(v);
        if (q >= 0 && q < o.n_in && c0 + c < p.n_ch) v = in[q * p.n_ch + c0 + c];
        zs[el] = v;
    }
    __syncthreads();
    V* out = p.out + o.out_off + (o.row0 + o.row_step * i) * o.n_out * p.n_ch;
    const int n_items = (A / R * U) << sh;
    for (int el = t; el < n_items; el += NT) {
        const int cl = el & (cg - 1), rest = el >> sh, g = rest / U, ph = rest - g * U;
        if (c0 + cl >= p.n_ch) continue;
        const int la0 = g * R;  // outputs m0 + (la0 + r) U + ph, r = 0 .. R - 1
        const double* hp = hs + ph;
        const V* zp = zs + (size_t)(la0 + 2 * HW) * cg + cl;  // the sample tap ph meets for r = 0
        V acc[R], zw[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            vqt_zero(acc[r]);
            zw[r] = zp[r * cg];
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const double h = hp[j * U];
#pragma unroll
            for (int r = 0; r < R; ++r) vqt_mad(h, zw[r], acc[r]);
            if (j + 1 < NJ) {
#pragma unroll
                for (int r = R - 1; r > 0; --r) zw[r] = zw[r - 1];
                zw[0] = zp[-((j + 1) * cg)];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t m = m0 + (int64_t)(la0 + r) * U + ph;
            if (m < o.n_out) out[m * p.n_ch + c0 + cl] = acc[r];
        }
    }
}

}  // namespace dsvqt
