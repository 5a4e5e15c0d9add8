// Structure filters: the reference's sample-by-sample filter classes -- LatticeLadderFilter (FIR lattice, IIR
// lattice-ladder, second-order-section lattice-ladder; classes/lattice_ladder_filter.py), WarpedFIR / WarpedIIR
// (classes/warped_filters.py) and KautzFilter (classes/kautz_filter.py) -- as float64 recursions.  gfx950.
//
// A stream is one channel through one structure.  Every structure is a recursion (y, S') = step(x, S) over D <= 64
// real state values, linear and time-invariant, so with zero input S' = A S and over a block of L samples
//     S_{b+1} = Phi S_b + s_b,     Phi = A^L,
// s_b the final state of block b run from zero state: the block carry of block_carry.hpp (DESIGN sections 9 and 18),
// in its three passes with its L, B, padded tile and in-wave scan:
//   k_sfilt_group  one lane per block, one wave per group: s_b of every block, then the scan gives t_g.
//   k_block_carry  one wave per stream: T_{g+1} = Phi^B T_g + t_g from T_0 = zi, for any D, odd or even.
//   k_sfilt_apply  one wave per (group, channel): s_b again, the scan from T_g gives each block's true entry state,
//                  and each lane reruns its block from it, writes the output and, at the last sample, zf.
// A lane's state lives in its row of the LDS block-state array (stride D + 1 doubles), so one step function per
// structure serves every D without a register array; the steps are __host__ __device__ and the host probes A with
// them (api.hip: sfilt_tables).  Each step performs the reference's operations in the reference's order.
//
// Packed coefficients (float64, one array per call; `aux` is a count the layout needs beside D):
//   FIR_LATTICE  k[D]
//   IIR_LATTICE  k[D], c[D + 1]
//   SOS_LATTICE  per section k0 k1 c0 c1 c2; D = 2 sections, state (section, j) at S[2 section + j]
//   WARPED_FIR   lambda, b[D]
//   WARPED_IIR   lambda, b[D] (zero-padded), sigma[0 .. aux]: aux = len(a) feedback states
//   KAUTZ        aux real poles: p, g, c each; then (D - aux) / 2 pole pairs: q, r, g1, g2, c1, c2 each.  A tap filter
//                and the all-pass of the same denominator share one direct-form-II state: w[n-1] for a real pole,
//                (w[n-1], w[n-2]) for a pair.
#pragma once
#include "block_carry.hpp"

namespace sfilt {

using carry::B;
using carry::G;
using carry::L;
using carry::TP;
constexpr int MAX_D = 64;  // state values of one structure: one per lane in the scans
// The carry gain, the largest magnitude in Phi = A^L and Phi^B, that the host entries accept: set from the conditioning
// sweep of DESIGN section 18 (tools/sweep_sfilt_gain.py).  The warped IIR realisation is far from normal and its carried
// states' rounding grows with the gain; in the other structures a large entry of Phi is a matter of the states' scales.
constexpr double MAX_GAIN_WARPED_IIR = 30.0;
constexpr double MAX_GAIN = 1.0e6;

enum Kind { FIR_LATTICE = 0, IIR_LATTICE = 1, SOS_LATTICE = 2, WARPED_FIR = 3, WARPED_IIR = 4, KAUTZ = 5, N_KINDS = 6 };

inline double max_gain(int kind) { return kind == WARPED_IIR ? MAX_GAIN_WARPED_IIR : MAX_GAIN; }

// doubles in the packed coefficient array of a structure (host side)
inline int coef_count(int kind, int d, int aux) {
    switch (kind) {
        case FIR_LATTICE: return d;
        case IIR_LATTICE: return 2 * d + 1;
        case SOS_LATTICE: return 5 * (d / 2);
        case WARPED_FIR: return 1 + d;
        case WARPED_IIR: return 1 + d + aux + 1;
        default: return 3 * aux + 6 * ((d - aux) / 2);
    }
}

// _lattice_filtering_fir: st[i] is the backward signal of stage i - 1 at the previous sample
__host__ __device__ inline double step_fir_lattice(double x, double* st, const double* k, int d) {
    double xo = x, s0 = x;
    for (int i = 0; i < d; ++i) {
        const double si = st[i];
        const double s1 = -xo * k[i] + si;
        xo -= si * k[i];
        st[i] = s0;
        s0 = s1;
    }
    return xo;
}

// _lattice_ladder_filtering_iir: from the last reflection coefficient down, ladder taps c
__host__ __device__ inline double step_iir_lattice(double x, double* st, const double* k, const double* c, int d) {
    double x_low = 0.0;
    for (int i = d - 1; i >= 0; --i) {
        const double si = st[i];
        x += si * k[i];
        const double s = x * -k[i] + si;
        if (i != d - 1) st[i + 1] = s;
        x_low += s * c[i + 1];
    }
    st[0] = x;
    return x * c[0] + x_low;
}

// _lattice_ladder_filtering_sos: a cascade of two-state lattice-ladder sections
__host__ __device__ inline double step_sos_lattice(double x, double* st, const double* q, int d) {
    for (int sec = 0; sec < d / 2; ++sec, q += 5, st += 2) {
        const double k0 = q[0], k1 = q[1];
        double x_low = 0.0;
        x += st[1] * k1;
        double s = x * -k1 + st[1];
        x_low += s * q[4];
        x += st[0] * k0;
        s = x * -k0 + st[0];
        st[1] = s;
        x_low += s * q[3];
        st[0] = x;
        x = x * q[2] + x_low;
    }
    return x;
}

// WarpedFIR.process_sample: a chain of first-order all-passes; st[d - 1] keeps the last residue
__host__ __device__ inline double step_warped_fir(double x, double* st, double lam, const double* b, int d) {
    double out = x * b[0], residue = x;
    for (int i = 0; i + 1 < d; ++i) {
        const double nr = (st[i + 1] - residue) * lam + st[i];
        st[i] = residue;
        residue = nr;
        out += nr * b[i + 1];
    }
    st[d - 1] = residue;
    return out;
}

// WarpedIIR.process_sample: the sigma feedback over the first m states, then the warped FIR chain
__host__ __device__ inline double step_warped_iir(double x, double* st, const double* q, int d, int m) {
    const double* sig = q + 1 + d;
    double fb = 0.0;
    for (int i = 0; i < m; ++i) fb += sig[i + 1] * st[i];
    x += fb;
    x *= sig[0];
    return step_warped_fir(x, st, q[0], q + 1, d);
}

// KautzFilter: real-pole sections, then pole-pair sections; y = sum of the weighted normalised taps
__host__ __device__ inline double step_kautz(double x, double* st, const double* q, int d, int n_real) {
    double y = 0.0;
    for (int i = 0; i < n_real; ++i, q += 3, ++st) {
        const double p = q[0], w1 = st[0];
        const double w = x + p * w1;
        y += q[1] * w * q[2];
        x = -p * w + w1;
        st[0] = w;
    }
    for (int i = 0; i < (d - n_real) / 2; ++i, q += 6, st += 2) {
        const double qq = q[0], r = q[1], w1 = st[0], w2 = st[1];
        const double w = x - qq * w1 - r * w2;
        y += q[2] * (w - w1) * q[4];
        y += q[3] * (w + w1) * q[5];
        x = r * w + qq * w1 + w2;
        st[1] = w1;
        st[0] = w;
    }
    return y;
}

__host__ __device__ inline double step(int kind, double x, double* st, const double* q, int d, int aux) {
    switch (kind) {
        case FIR_LATTICE: return step_fir_lattice(x, st, q, d);
        case IIR_LATTICE: return step_iir_lattice(x, st, q, q + d, d);
        case SOS_LATTICE: return step_sos_lattice(x, st, q, d);
        case WARPED_FIR: return step_warped_fir(x, st, q[0], q + 1, d);
        case WARPED_IIR: return step_warped_iir(x, st, q, d, aux);
        default: return step_kautz(x, st, q, d, aux);
    }
}

template <typename T>
struct Args {
    const T* x;
    int64_t sxc, sxn;  // sample n of channel c at x[c sxc + n sxn]
    T* y;
    int64_t syc, syn;  // output sample n of channel c at y[c syc + n syn]
    int64_t n;         // samples per channel
    int n_ch, kind, d, aux;
    int64_t n_groups;    // ceil(n / G)
    const double* coef;  // packed, coef_count(kind, d, aux) values
    const double* phi;   // [D][D]  A^L
    const double* phig;  // [D][D]  A^(L B)
    double* gst;         // [n_ch][n_groups][D]: t_g (k_sfilt_group), then T_g (the carry)
    const double* zi;    // [D][n_ch] or null (zero initial state)
    double* zf;          // [D][n_ch] or null
};

// dynamic LDS: x tile [B][TP], output tile [B][TP], block states [B][D + 1], Phi [D][D]
__host__ __device__ inline size_t lds_bytes(int d, bool out_tile) {
    return sizeof(double) * ((out_tile ? 2 : 1) * (size_t)B * TP + (size_t)B * (d + 1) + (size_t)d * d);
}

// one lane's block, sample after sample, from the state in st (LDS), which is left holding the final state; only the
// first nv samples (the valid ones of a partial last block) move it.  out: the lane's output row or null.
template <int KIND>
__device__ inline void block_of(const double* xr, double* out, int nv, const double* __restrict__ q, int d, int aux,
                                double* st) {
    for (int i = 0; i < nv; ++i) {
        const double yi = step(KIND, xr[i], st, q, d, aux);
        if (out) out[i] = yi;
    }
}

__device__ inline void block(int kind, const double* xr, double* out, int nv, const double* q, int d, int aux, double* st) {
    switch (kind) {
        case FIR_LATTICE: return block_of<FIR_LATTICE>(xr, out, nv, q, d, aux, st);
        case IIR_LATTICE: return block_of<IIR_LATTICE>(xr, out, nv, q, d, aux, st);
        case SOS_LATTICE: return block_of<SOS_LATTICE>(xr, out, nv, q, d, aux, st);
        case WARPED_FIR: return block_of<WARPED_FIR>(xr, out, nv, q, d, aux, st);
        case WARPED_IIR: return block_of<WARPED_IIR>(xr, out, nv, q, d, aux, st);
        default: return block_of<KAUTZ>(xr, out, nv, q, d, aux, st);
    }
}

// grid = (n_groups - 1, n_ch), block = B: the zero-entry state t_g of every group but the last
template <typename T>
__global__ __launch_bounds__(B) void k_sfilt_group(Args<T> p) {
    extern __shared__ double slds[];
    const int d = p.d, lane = threadIdx.x, c = blockIdx.y;
    const int64_t g = blockIdx.x;
    double* xt = slds;
    double* sb = xt + B * TP;
    double* pm = sb + B * (d + 1);
    double* st = sb + lane * (d + 1);
    carry::load_matrix(p.phi, d * d, pm);
    carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
    for (int i = 0; i < d; ++i) st[i] = 0.0;
    __syncthreads();
    block(p.kind, xt + lane * TP, nullptr, carry::valid_in_block(p.n, g, lane), p.coef, d, p.aux, st);
    __syncthreads();
    const double t = carry::scan(sb, pm, d, 0.0, false);
    if (lane < d) p.gst[((size_t)c * p.n_groups + g) * d + lane] = t;
}

// grid = (n_groups, n_ch), block = B
template <typename T>
__global__ __launch_bounds__(B) void k_sfilt_apply(Args<T> p) {
    extern __shared__ double slds[];
    const int d = p.d, lane = threadIdx.x, c = blockIdx.y;
    const int64_t g = blockIdx.x;
    double* xt = slds;
    double* ot = xt + B * TP;
    double* sb = ot + B * TP;
    double* pm = sb + B * (d + 1);
    double* st = sb + lane * (d + 1);
    const int nv = carry::valid_in_block(p.n, g, lane);
    const bool last = carry::holds_last(p, g, lane, nv);
    carry::load_matrix(p.phi, d * d, pm);
    carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
    for (int i = 0; i < d; ++i) st[i] = 0.0;
    __syncthreads();
    block(p.kind, xt + lane * TP, nullptr, nv, p.coef, d, p.aux, st);
    __syncthreads();
    const double t0 = lane < d ? p.gst[((size_t)c * p.n_groups + g) * d + lane] : 0.0;
    carry::scan(sb, pm, d, t0, true);
    __syncthreads();
    block(p.kind, xt + lane * TP, ot + lane * TP, nv, p.coef, d, p.aux, st);
    if (last)
        for (int i = 0; i < d; ++i) p.zf[(size_t)i * p.n_ch + c] = st[i];
    __syncthreads();
    carry::store_tile(ot, p.y + (int64_t)c * p.syc, p.syn, p.n, g);
}

}  // namespace sfilt
