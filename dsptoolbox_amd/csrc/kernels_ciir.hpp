// Recursive filtering of cascades of second-order sections with COMPLEX coefficients, complex float64 recursion:
// what scipy.signal.sosfilt computes for a complex sos array and real samples (the gammatone bank's four cascaded
// complex one-pole sections, filterbanks/filterbanks.py:217-303 of the reference).  gfx950.
//
// The algorithm is that of kernels_iir.hpp with complex states: every section is transposed direct form II with
// complex b0 b1 b2 a1 a2, a cascade of K sections has D = 2K complex state values, and over a block of L samples
//     S_{b+1} = Phi S_b + s_b,     Phi = A^L  (complex),
// carried by the same three passes:
//   k_ciir_group  one lane per block, one wave per group: s_b of every block, then the in-wave scan gives t_g.
//   k_ciir_carry  one wave per stream: T_{g+1} = Phi^(LB) T_g + t_g from T_0 = zi.
//   k_ciir_apply  one wave per (group, channel), every filter in turn: each lane reruns its block from its true
//                 entry state and writes the output's real plane and, where asked for, its imaginary plane.
// The input samples are real; the block (L, B), the padded tile with its load and store and valid_in_block are
// block_carry.hpp's.  Complex values are kept as separate real and imaginary doubles in registers and LDS (two planes),
// and as interleaved (re, im) pairs in global memory.
#pragma once
#include "block_carry.hpp"

namespace ciir {

using carry::B;
using carry::G;
using carry::L;
using carry::TP;
// sections per complex cascade: D = 32 complex state values.  With 32 sections Phi (64 KB), the block states
// (66 KB) and the tiles would not fit the 160 KB of LDS; with 16 the apply kernel takes 82 KB.
constexpr int CIIR_MAX_SEC = 16;

template <typename T>
struct Args {
    const T* x;
    int64_t sxc, sxn;       // real sample n of channel c at x[c sxc + n sxn]
    double *yr, *yi;        // output planes; yi may be null (real part only)
    int64_t syf, syc, syn;  // output sample n of filter f, channel c at y?[f syf + c syc + n syn]
    int64_t n;              // samples per channel
    int n_ch, n_filt, n_sec;
    int64_t n_groups;       // ceil(n / G)
    const double* sos;      // [n_filt][n_sec][5][2]: b0 b1 b2 a1 a2 (re, im), normalised by a0
    const double* phi;      // [n_filt][2][D][D]  A^L, real plane then imaginary plane
    const double* phig;     // [n_filt][2][D][D]  A^(L B)
    double* gst;            // [n_filt n_ch][n_groups][D][2]: t_g (k_ciir_group), then T_g (k_ciir_carry)
    const double* zi;       // [n_filt][n_sec][2][n_ch][2] or null (zero initial state)
    double* zf;             // [n_filt][n_sec][2][n_ch][2] or null
};

// dynamic LDS: x tile [B][TP], output tile [B][TP] (one plane at a time), block states 2 x [B][D + 1],
// Phi or Phi^(LB) 2 x [D][D]
__host__ __device__ inline size_t lds_bytes(int n_sec, bool out_tile) {
    const size_t d = 2 * (size_t)n_sec;
    return sizeof(double) * ((out_tile ? 2 : 1) * (size_t)B * TP + 2 * (size_t)B * (d + 1) + 2 * d * d);
}

// one lane's block through the cascade, in place in (wr, wi); only the first nv samples move the state.
// (sr, si): the lane's D state values in LDS, read as the entry state unless from_zero, left holding the final state.
__device__ inline void cascade(double (&wr)[L], double (&wi)[L], int nv, const double* __restrict__ sos, int n_sec,
                               double* sr, double* si, bool from_zero) {
    for (int k = 0; k < n_sec; ++k) {
        const double* q = sos + 10 * k;
        const double b0r = q[0], b0i = q[1], b1r = q[2], b1i = q[3], b2r = q[4], b2i = q[5];
        const double a1r = q[6], a1i = q[7], a2r = q[8], a2i = q[9];
        double z1r = from_zero ? 0.0 : sr[2 * k], z1i = from_zero ? 0.0 : si[2 * k];
        double z2r = from_zero ? 0.0 : sr[2 * k + 1], z2i = from_zero ? 0.0 : si[2 * k + 1];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            if (i < nv) {
                const double xr = wr[i], xi = wi[i];
                const double yr = fma(b0r, xr, fma(-b0i, xi, z1r));
                const double yi = fma(b0r, xi, fma(b0i, xr, z1i));
                z1r = fma(b1r, xr, fma(-b1i, xi, fma(-a1r, yr, fma(a1i, yi, z2r))));
                z1i = fma(b1r, xi, fma(b1i, xr, fma(-a1r, yi, fma(-a1i, yr, z2i))));
                z2r = fma(b2r, xr, fma(-b2i, xi, fma(-a2r, yr, a2i * yi)));
                z2i = fma(b2r, xi, fma(b2i, xr, fma(-a2r, yi, -a2i * yr)));
                wr[i] = yr;
                wi[i] = yi;
            }
        }
        sr[2 * k] = z1r;
        si[2 * k] = z1i;
        sr[2 * k + 1] = z2r;
        si[2 * k + 1] = z2i;
    }
}

// acc + sum_j P[lane][j] S[j], lane i < D holding S[i] = (sr, si)
__device__ inline void carry_step(const double* rowr, const double* rowi, int d, double sr, double si, double& ar,
                                  double& ai) {
    for (int j = 0; j < d; ++j) {
        const double pr = __shfl(sr, j), pi = __shfl(si, j);
        ar = fma(rowr[j], pr, fma(-rowi[j], pi, ar));
        ai = fma(rowr[j], pi, fma(rowi[j], pr, ai));
    }
}

// serial scan over the B blocks of a group: S <- P S + s_b.  With keep_entry the entry state of block b replaces
// s_b in (sbr, sbi).  Leaves the state after the last block in (sr, si).
__device__ inline void scan(double* sbr, double* sbi, const double* pmr, const double* pmi, int d, double& sr, double& si,
                            bool keep_entry) {
    const int lane = threadIdx.x;
    const double* rowr = pmr + (lane < d ? lane : 0) * d;
    const double* rowi = pmi + (lane < d ? lane : 0) * d;
    for (int b = 0; b < B; ++b) {
        const int o = b * (d + 1) + lane;
        double ar = lane < d ? sbr[o] : 0.0, ai = lane < d ? sbi[o] : 0.0;
        carry_step(rowr, rowi, d, sr, si, ar, ai);
        if (keep_entry && lane < d) {
            sbr[o] = sr;
            sbi[o] = si;
        }
        sr = ar;
        si = ai;
    }
}

// grid = (n_groups - 1, n_filt n_ch), block = B: the zero-entry state t_g of every group but the last
template <typename T>
__global__ __launch_bounds__(B) void k_ciir_group(Args<T> p) {
    extern __shared__ double clds[];
    const int d = 2 * p.n_sec, lane = threadIdx.x;
    const int stream = blockIdx.y, f = stream / p.n_ch, c = stream % p.n_ch;
    const int64_t g = blockIdx.x;
    double* xt = clds;
    double* sbr = xt + B * TP;
    double* sbi = sbr + B * (d + 1);
    double* pmr = sbi + B * (d + 1);
    double* pmi = pmr + d * d;
    carry::load_matrix(p.phi + (size_t)f * 2 * d * d, 2 * d * d, pmr);  // (both planes)
    carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
    __syncthreads();
    double wr[L], wi[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
        wr[i] = xt[lane * TP + i];
        wi[i] = 0.0;
    }
    cascade(wr, wi, carry::valid_in_block(p.n, g, lane), p.sos + (size_t)f * p.n_sec * 10, p.n_sec,
            sbr + lane * (d + 1), sbi + lane * (d + 1), true);
    __syncthreads();
    double sr = 0.0, si = 0.0;
    scan(sbr, sbi, pmr, pmi, d, sr, si, false);
    if (lane < d) {
        double* o = p.gst + (((size_t)stream * p.n_groups + g) * d + lane) * 2;
        o[0] = sr;
        o[1] = si;
    }
}

struct CarryArgs {
    const double* phig;  // [n_filt][2][D][D]
    double* gst;         // [n_filt n_ch][n_groups][D][2]
    const double* zi;    // [n_filt][n_sec][2][n_ch][2] or null
    int64_t n_groups;
    int n_ch, n_sec;
};

// grid = n_filt n_ch, block = B: the entry state T_g of every group, in place of t_g
__global__ __launch_bounds__(B) void k_ciir_carry(CarryArgs p) {
    extern __shared__ double clds[];
    const int d = 2 * p.n_sec, lane = threadIdx.x;
    const int stream = blockIdx.x, f = stream / p.n_ch, c = stream % p.n_ch;
    double* pmr = clds;
    double* pmi = pmr + d * d;
    carry::load_matrix(p.phig + (size_t)f * 2 * d * d, 2 * d * d, pmr);
    __syncthreads();
    const double* rowr = pmr + (lane < d ? lane : 0) * d;
    const double* rowi = pmi + (lane < d ? lane : 0) * d;
    double sr = 0.0, si = 0.0;
    if (p.zi && lane < d) {
        const double* z = p.zi + (((size_t)f * d + lane) * p.n_ch + c) * 2;
        sr = z[0];
        si = z[1];
    }
    double* gs = p.gst + (size_t)stream * p.n_groups * d * 2;
    for (int64_t g = 0; g < p.n_groups; ++g) {
        double* o = gs + (g * d + (lane < d ? lane : 0)) * 2;
        const bool has = lane < d && g + 1 < p.n_groups;
        double ar = has ? o[0] : 0.0, ai = has ? o[1] : 0.0;
        carry_step(rowr, rowi, d, sr, si, ar, ai);
        if (lane < d) {
            o[0] = sr;
            o[1] = si;
        }
        sr = ar;
        si = ai;
    }
}

// grid = (n_groups, n_ch), block = B: every filter over one group of one channel -- the x tile is read once
template <typename T>
__global__ __launch_bounds__(B) void k_ciir_apply(Args<T> p) {
    extern __shared__ double clds[];
    const int d = 2 * p.n_sec, lane = threadIdx.x, c = blockIdx.y;
    const int64_t g = blockIdx.x;
    double* xt = clds;
    double* ot = xt + B * TP;
    double* sbr = ot + B * TP;
    double* sbi = sbr + B * (d + 1);
    double* pmr = sbi + B * (d + 1);
    double* pmi = pmr + d * d;
    double* sr = sbr + lane * (d + 1);
    double* si = sbi + lane * (d + 1);
    const int nv = carry::valid_in_block(p.n, g, lane);
    const bool last = carry::holds_last(p, g, lane, nv);
    // one output plane, from the lanes' registers through the tile to y in coalesced rows
    auto store_plane = [&](const double (&w)[L], double* y) {
        __syncthreads();  // (the tile's previous plane is written out)
#pragma unroll
        for (int i = 0; i < L; ++i) ot[lane * TP + i] = w[i];
        __syncthreads();
        carry::store_tile(ot, y, p.syn, p.n, g);
    };
    carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
    for (int f = 0; f < p.n_filt; ++f) {
        const double* sos = p.sos + (size_t)f * p.n_sec * 10;
        __syncthreads();  // (pm, sb and the tile of the previous filter are done with)
        carry::load_matrix(p.phi + (size_t)f * 2 * d * d, 2 * d * d, pmr);
        double wr[L], wi[L];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            wr[i] = xt[lane * TP + i];
            wi[i] = 0.0;
        }
        cascade(wr, wi, nv, sos, p.n_sec, sr, si, true);
        __syncthreads();
        const size_t stream = (size_t)f * p.n_ch + c;
        double tr = 0.0, ti = 0.0;
        if (lane < d) {
            const double* t0 = p.gst + ((stream * p.n_groups + g) * d + lane) * 2;
            tr = t0[0];
            ti = t0[1];
        }
        scan(sbr, sbi, pmr, pmi, d, tr, ti, true);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < L; ++i) {
            wr[i] = xt[lane * TP + i];
            wi[i] = 0.0;
        }
        cascade(wr, wi, nv, sos, p.n_sec, sr, si, false);
        if (last)
            for (int i = 0; i < d; ++i) {
                double* z = p.zf + (((size_t)f * d + i) * p.n_ch + c) * 2;
                z[0] = sr[i];
                z[1] = si[i];
            }
        const int64_t off = (int64_t)f * p.syf + (int64_t)c * p.syc;
        store_plane(wr, p.yr + off);
        if (p.yi) store_plane(wi, p.yi + off);
    }
}

}  // namespace ciir
