// Recursive (IIR) filtering of cascades of second-order sections, float64 recursion: what
// scipy.signal.sosfilt / lfilter compute for Filter.filter_signal (classes/filter_helpers.py:207-280, :288-382)
// and, filter by filter, for FilterBank.filter_signal.  gfx950.
//
// A stream is one (filter, channel) pair.  Every section is transposed direct form II:
//     y = b0 x + z1,   z1' = b1 x - a1 y + z2,   z2' = b2 x - a2 y      (a0 = 1: normalised by the host)
// and the cascade of K sections has the state vector S = (z1_0, z2_0, z1_1, z2_1, ...), D = 2K values -- sosfilt's
// zi[k][j] is S[2k + j].  With zero input the state moves as S' = A S; over a block of L samples
//     S_{b+1} = Phi S_b + s_b,     Phi = A^L,
// s_b the final state of block b run from zero state.  The recursion is parallelised over time with that carry, in
// the three passes of block_carry.hpp:
//   k_iir_group    one wave per (group, stream): s_b of every block, then the in-wave scan gives t_g.
//   k_block_carry  one wave per stream: T_{g+1} = Phi^B T_g + t_g from T_0 = zi.
//   k_iir_apply    one wave per (group, channel), every filter in turn: s_b again, the in-wave scan from T_g gives each
//                  block's true entry state, and each lane reruns its block from it and writes the output.
// The output thus differs from the serial recursion only by the rounding of the carried states.
#pragma once
#include "block_carry.hpp"

namespace iir {

using carry::B;
using carry::G;
using carry::L;
using carry::TP;
constexpr int MAX_SEC = 32;  // sections per cascade (D = 64 state values: one per lane in the scans)

template <typename T>
struct Args {
    const T* x;
    int64_t sxc, sxn;  // sample n of channel c at x[c sxc + n sxn]
    T* y;
    int64_t syf, syc, syn;  // output sample n of filter f, channel c at y[f syf + c syc + n syn] (summed: f = 0)
    int64_t n;              // samples per channel
    int n_ch, n_filt, n_sec, summed;
    int64_t n_groups;       // ceil(n / G)
    const double* sos;      // [n_filt][n_sec][5]: b0 b1 b2 a1 a2, normalised by a0
    const double* phi;      // [n_filt][D][D]  A^L
    const double* phig;     // [n_filt][D][D]  A^(L B)
    double* gst;            // [n_filt n_ch][n_groups][D]: t_g (k_iir_group), then T_g (k_block_carry)
    const double* zi;       // [n_filt][n_sec][2][n_ch] or null (zero initial state)
    double* zf;             // [n_filt][n_sec][2][n_ch] or null
};

// dynamic LDS: x tile [B][TP], output tile [B][TP], block states [B][D + 1], Phi or Phi^(LB) [D][D]
__host__ __device__ inline size_t lds_bytes(int n_sec, bool out_tile) {
    const size_t d = 2 * (size_t)n_sec;
    return sizeof(double) * ((out_tile ? 2 : 1) * (size_t)B * TP + (size_t)B * (d + 1) + d * d);
}

// one lane's block through the cascade, section after section, in place in w; only the first nv samples
// (the valid ones of a partial last block) move the state.  st: the lane's D state values in LDS, read as
// the entry state unless from_zero, left holding the final state.
__device__ inline void cascade(double (&w)[L], int nv, const double* __restrict__ sos, int n_sec, double* st,
                               bool from_zero) {
    for (int k = 0; k < n_sec; ++k) {
        const double b0 = sos[5 * k], b1 = sos[5 * k + 1], b2 = sos[5 * k + 2];
        const double a1 = sos[5 * k + 3], a2 = sos[5 * k + 4];
        double z1 = from_zero ? 0.0 : st[2 * k], z2 = from_zero ? 0.0 : st[2 * k + 1];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            if (i < nv) {
                const double xi = w[i];
                const double yi = fma(b0, xi, z1);
                z1 = fma(b1, xi, fma(-a1, yi, z2));
                z2 = fma(b2, xi, -a2 * yi);
                w[i] = yi;
            }
        }
        st[2 * k] = z1;
        st[2 * k + 1] = z2;
    }
}

// grid = (n_groups - 1, n_filt n_ch), block = B: the zero-entry state t_g of every group but the last
template <typename T>
__global__ __launch_bounds__(B) void k_iir_group(Args<T> p) {
    extern __shared__ double lds[];
    const int d = 2 * p.n_sec, lane = threadIdx.x;
    const int stream = blockIdx.y, f = stream / p.n_ch, c = stream % p.n_ch;
    const int64_t g = blockIdx.x;
    double* xt = lds;
    double* sb = xt + B * TP;
    double* pm = sb + B * (d + 1);
    carry::load_matrix(p.phi + (size_t)f * d * d, d * d, pm);
    carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
    __syncthreads();
    double w[L];
#pragma unroll
    for (int i = 0; i < L; ++i) w[i] = xt[lane * TP + i];
    cascade(w, carry::valid_in_block(p.n, g, lane), p.sos + (size_t)f * p.n_sec * 5, p.n_sec, sb + lane * (d + 1), true);
    __syncthreads();
    const double t = carry::scan(sb, pm, d, 0.0, false);
    if (lane < d) p.gst[((size_t)stream * p.n_groups + g) * d + lane] = t;
}

// grid = (n_groups, n_ch), block = B: every filter over one group of one channel -- the x tile is read once
template <typename T>
__global__ __launch_bounds__(B) void k_iir_apply(Args<T> p) {
    extern __shared__ double lds[];
    const int d = 2 * p.n_sec, lane = threadIdx.x, c = blockIdx.y;
    const int64_t g = blockIdx.x;
    double* xt = lds;
    double* ot = xt + B * TP;
    double* sb = ot + B * TP;
    double* pm = sb + B * (d + 1);
    double* st = sb + lane * (d + 1);
    const int nv = carry::valid_in_block(p.n, g, lane);
    const bool last = carry::holds_last(p, g, lane, nv);
    carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
    double acc[L];
#pragma unroll
    for (int i = 0; i < L; ++i) acc[i] = 0.0;
    for (int f = 0; f < p.n_filt; ++f) {
        const double* sos = p.sos + (size_t)f * p.n_sec * 5;
        __syncthreads();  // (pm and sb of the previous filter are done with)
        carry::load_matrix(p.phi + (size_t)f * d * d, d * d, pm);
        double w[L];
#pragma unroll
        for (int i = 0; i < L; ++i) w[i] = xt[lane * TP + i];
        cascade(w, nv, sos, p.n_sec, st, true);
        __syncthreads();
        const size_t stream = (size_t)f * p.n_ch + c;
        const double t0 = lane < d ? p.gst[(stream * p.n_groups + g) * d + lane] : 0.0;
        carry::scan(sb, pm, d, t0, true);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < L; ++i) w[i] = xt[lane * TP + i];
        cascade(w, nv, sos, p.n_sec, st, false);
        if (last)
            for (int i = 0; i < d; ++i) p.zf[((size_t)f * d + i) * p.n_ch + c] = st[i];
        if (p.summed) {
#pragma unroll
            for (int i = 0; i < L; ++i) acc[i] += w[i];
            continue;
        }
#pragma unroll
        for (int i = 0; i < L; ++i) ot[lane * TP + i] = w[i];
        __syncthreads();
        carry::store_tile(ot, p.y + (int64_t)f * p.syf + (int64_t)c * p.syc, p.syn, p.n, g);
    }
    if (!p.summed) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < L; ++i) ot[lane * TP + i] = acc[i];
    __syncthreads();
    carry::store_tile(ot, p.y + (int64_t)c * p.syc, p.syn, p.n, g);
}

}  // namespace iir
