// Realtime filters: the reference's sample-by-sample StateVariableFilter (classes/sv_filter.py), IIRFilter
// (classes/iir_filter_realtime.py), ParallelFilter (classes/parallel_filter.py) and StateSpaceFilter
// (classes/state_space_filter.py) as float64 recursions on the block carry, and the direct float64 FIR sum behind FIRFilter
// (classes/fir_filter_realtime.py) and the FIR part of ParallelFilter.  gfx950.
//
// The recursions follow kernels_sfilt.hpp pass for pass (DESIGN sections 9, 18 and 26): a stream is one channel through one
// filter, (y, S') = step(x, S) over D <= 64 real state values, and
//   k_rtfilt_group  one lane per block of L samples, one wave per group: s_b of every block, then the scan gives t_g.
//   k_block_carry   one wave per stream: T_{g+1} = Phi^B T_g + t_g from T_0 = zi.
//   k_rtfilt_apply  one wave per (group, channel): s_b again, the scan from T_g gives each block's entry state, each lane
//                   reruns its block from it, writes the output and, at the last sample, zf.
// A lane's state lives in its row of the LDS block-state array (stride D + 1 doubles); the steps are __host__ __device__
// and the host probes A with them (api.hip: rtfilt_tables).  Each step performs the reference's operations in the
// reference's order.  What is new beside the structure filters:
//   SVF          four outputs a sample (low, high, band, all-pass): the apply pass holds one output tile per band and
//                writes them (band, channel, sample) planar, band b of channel c at y[b syb + c syc + n syn].
//   PARALLEL     aux second-order sections that all read the same input, the signal delayed by `delay` samples with zeros
//                in front (a shifted tile load, not a state); the output is base + y_0 + y_1 + ..., `base` the FIR part's
//                sample (the apply pass loads its tile into the output tile first) or 0.
//   STATE_SPACE  the new state needs the whole old one: a second state row per lane holds it until it is complete.  A's
//                rows are wave-uniform reads from global memory.
//
// Packed coefficients (float64, one array per call; `aux` is a count the layout needs beside D):
//   SVF          g, resonance, 1 / (1 + resonance g + g^2); D = 2
//   TDF2         b[D + 1], a[D + 1] (a[0] = 1, both zero-padded to the order D)
//   PARALLEL     per section b0 b1 b2 a1 a2 (a0 = 1); aux sections, D = 2 aux, state (z1, z2) of section k at S[2 k]
//   STATE_SPACE  A[D][D] row-major, B[D], C[D], D
#pragma once
#include "block_carry.hpp"

namespace rtfilt {

using carry::B;
using carry::G;
using carry::L;
using carry::TP;
constexpr int MAX_D = 64;  // state values of one filter: one per lane in the scans
// The carry gain, the largest magnitude in Phi = A^L and Phi^B, that the host entries accept (DESIGN section 26,
// tools/sweep_rtfilt_gain.py).  The transposed direct form II of a high order and tf2ss's controller-canonical form are
// companion matrices, far from normal, and their carried states' rounding grows with the gain; the 2 x 2 blocks of the
// state-variable and the parallel filter are only stopped when they are not stable.
constexpr double MAX_GAIN_COMPANION = 30.0;
constexpr double MAX_GAIN = 1.0e6;

enum Kind { SVF = 0, TDF2 = 1, PARALLEL = 2, STATE_SPACE = 3, N_KINDS = 4 };

__host__ __device__ inline int n_bands(int kind) { return kind == SVF ? 4 : 1; }
inline double max_gain(int kind) { return (kind == TDF2 || kind == STATE_SPACE) ? MAX_GAIN_COMPANION : MAX_GAIN; }

// doubles in the packed coefficient array of a filter (host side)
inline int coef_count(int kind, int d, int aux) {
    switch (kind) {
        case SVF: return 3;
        case TDF2: return 2 * d + 2;
        case PARALLEL: return 5 * aux;
        default: return d * d + 2 * d + 1;
    }
}

struct Svf {
    double yl, yh, yb, ya;
};

// StateVariableFilter.process_sample
__host__ __device__ inline Svf step_svf(double x, double* st, const double* q) {
    const double g = q[0], r = q[1];
    const double yh = (x - (r + g) * st[0] - st[1]) * q[2];
    const double yb = g * yh + st[0];
    st[0] = g * yh + yb;
    const double yl = g * yb + st[1];
    st[1] = g * yb + yl;
    return Svf{yl, yh, yb, yl - r * yb + yh};
}

// IIRFilter.process_sample: transposed direct form II of order d
__host__ __device__ inline double step_tdf2(double x, double* st, const double* b, const double* a, int d) {
    const double y = b[0] * x + st[0];
    for (int i = 0; i + 1 < d; ++i) st[i] = x * b[i + 1] - y * a[i + 1] + st[i + 1];
    st[d - 1] = x * b[d] - y * a[d];
    return y;
}

// ParallelFilter.filter_signal: sosfilt of every single section over the same input, added to acc in section order
__host__ __device__ inline double step_parallel(double x, double acc, double* st, const double* q, int n_sec) {
    for (int k = 0; k < n_sec; ++k, q += 5, st += 2) {
        const double y = q[0] * x + st[0];
        st[0] = q[1] * x - q[3] * y + st[1];
        st[1] = q[2] * x - q[4] * y;
        acc += y;
    }
    return acc;
}

// StateSpaceFilter.process_sample: y = C s + D x; s' = A s + B x.  nx: d values of room for s' while s is still read
__host__ __device__ inline double step_state_space(double x, double* st, double* nx, const double* q, int d) {
    const double *bv = q + d * d, *cv = bv + d;
    double y = 0.0;
    for (int j = 0; j < d; ++j) y += cv[j] * st[j];
    y += cv[d] * x;
    for (int i = 0; i < d; ++i) {
        const double* row = q + i * d;
        double acc = 0.0;
        for (int j = 0; j < d; ++j) acc += row[j] * st[j];
        nx[i] = acc + bv[i] * x;
    }
    for (int i = 0; i < d; ++i) st[i] = nx[i];
    return y;
}

// one step of any kind for the host's probe of A (the output is not wanted there)
inline void step_state_only(int kind, double x, double* st, double* nx, const double* q, int d, int aux) {
    switch (kind) {
        case SVF: (void)step_svf(x, st, q); return;
        case TDF2: (void)step_tdf2(x, st, q, q + d + 1, d); return;
        case PARALLEL: (void)step_parallel(x, 0.0, st, q, aux); return;
        default: (void)step_state_space(x, st, nx, q, d); return;
    }
}

template <typename T>
struct Args {
    const T* x;
    int64_t sxc, sxn;  // sample n of channel c at x[c sxc + n sxn]
    T* y;
    int64_t syb, syc, syn;  // output sample n of channel c in band b at y[b syb + c syc + n syn]
    int64_t n;              // samples per channel
    int n_ch, kind, d, aux;
    int64_t n_groups;    // ceil(n / G)
    int64_t delay;       // PARALLEL: the sections read x[n - delay], zeros in front
    const double* base;  // PARALLEL: what the sections' outputs are added to, or null (zeros)
    int64_t sbc, sbn;    // base sample n of channel c at base[c sbc + n sbn]
    const double* coef;  // packed, coef_count(kind, d, aux) values
    const double* phi;   // [D][D]  A^L
    const double* phig;  // [D][D]  A^(L B)
    double* gst;         // [n_ch][n_groups][D]: t_g (k_rtfilt_group), then T_g (the carry)
    const double* zi;    // [D][n_ch] or null (zero initial state)
    double* zf;          // [D][n_ch] or null
};

// dynamic LDS: x tile [B][TP], one output tile [B][TP] per band, block states [B][D + 1] (twice for STATE_SPACE: the
// state being built), Phi [D][D]
__host__ __device__ inline size_t lds_bytes(int kind, int d, bool out_tiles) {
    return sizeof(double) * ((size_t)(1 + (out_tiles ? n_bands(kind) : 0)) * B * TP +
                             (size_t)(kind == STATE_SPACE ? 2 : 1) * B * (d + 1) + (size_t)d * d);
}

// group g of one channel's samples, delayed by `delay` samples, into the tile: zeros before the first sample and past
// the end
template <typename T>
__device__ inline void load_tile_delayed(const T* x, int64_t sxn, int64_t n, int64_t g, int64_t delay, double* xt) {
    for (int t = threadIdx.x; t < G; t += B) {
        const int64_t nn = g * G + t, src = nn - delay;
        xt[(t / L) * TP + t % L] = (nn < n && src >= 0) ? (double)x[src * sxn] : 0.0;
    }
}

// one lane's block, sample after sample, from the state in st (LDS), which is left holding the final state; only the
// first nv samples (the valid ones of a partial last block) move it.  out: the lane's row of the first output tile (for
// PARALLEL holding the base samples on entry) or null; nx: the lane's second state row (STATE_SPACE).
template <int KIND>
__device__ inline void block_of(const double* xr, double* out, int nv, const double* __restrict__ q, int d, int aux,
                                double* st, double* nx) {
    for (int i = 0; i < nv; ++i) {
        if (KIND == SVF) {
            const Svf o = step_svf(xr[i], st, q);
            if (out) {
                out[i] = o.yl;
                out[B * TP + i] = o.yh;
                out[2 * B * TP + i] = o.yb;
                out[3 * B * TP + i] = o.ya;
            }
        } else if (KIND == TDF2) {
            const double yi = step_tdf2(xr[i], st, q, q + d + 1, d);
            if (out) out[i] = yi;
        } else if (KIND == PARALLEL) {
            const double yi = step_parallel(xr[i], out ? out[i] : 0.0, st, q, aux);
            if (out) out[i] = yi;
        } else {
            const double yi = step_state_space(xr[i], st, nx, q, d);
            if (out) out[i] = yi;
        }
    }
}

__device__ inline void block(int kind, const double* xr, double* out, int nv, const double* q, int d, int aux, double* st,
                             double* nx) {
    switch (kind) {
        case SVF: return block_of<SVF>(xr, out, nv, q, d, aux, st, nx);
        case TDF2: return block_of<TDF2>(xr, out, nv, q, d, aux, st, nx);
        case PARALLEL: return block_of<PARALLEL>(xr, out, nv, q, d, aux, st, nx);
        default: return block_of<STATE_SPACE>(xr, out, nv, q, d, aux, st, nx);
    }
}

template <typename T>
__device__ inline void load_x(const Args<T>& p, int c, int64_t g, double* xt) {
    if (p.kind == PARALLEL && p.delay > 0)
        load_tile_delayed(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, p.delay, xt);
    else
        carry::load_tile(p.x + (int64_t)c * p.sxc, p.sxn, p.n, g, xt);
}

// grid = (n_groups - 1, n_ch), block = B: the zero-entry state t_g of every group but the last
template <typename T>
__global__ __launch_bounds__(B) void k_rtfilt_group(Args<T> p) {
    extern __shared__ double rlds[];
    const int d = p.d, lane = threadIdx.x, c = blockIdx.y;
    const int64_t g = blockIdx.x;
    double* xt = rlds;
    double* sb = xt + B * TP;
    double* sn = sb + (p.kind == STATE_SPACE ? B * (d + 1) : 0);
    double* pm = sn + B * (d + 1);
    double* st = sb + lane * (d + 1);
    carry::load_matrix(p.phi, d * d, pm);
    load_x(p, c, g, xt);
    for (int i = 0; i < d; ++i) st[i] = 0.0;
    __syncthreads();
    block(p.kind, xt + lane * TP, nullptr, carry::valid_in_block(p.n, g, lane), p.coef, d, p.aux, st, sn + lane * (d + 1));
    __syncthreads();
    const double t = carry::scan(sb, pm, d, 0.0, false);
    if (lane < d) p.gst[((size_t)c * p.n_groups + g) * d + lane] = t;
}

// grid = (n_groups, n_ch), block = B
template <typename T>
__global__ __launch_bounds__(B) void k_rtfilt_apply(Args<T> p) {
    extern __shared__ double rlds[];
    const int d = p.d, lane = threadIdx.x, c = blockIdx.y, nb = n_bands(p.kind);
    const int64_t g = blockIdx.x;
    double* xt = rlds;
    double* ot = xt + B * TP;
    double* sb = ot + nb * B * TP;
    double* sn = sb + (p.kind == STATE_SPACE ? B * (d + 1) : 0);
    double* pm = sn + B * (d + 1);
    double* st = sb + lane * (d + 1);
    const int nv = carry::valid_in_block(p.n, g, lane);
    const bool last = carry::holds_last(p, g, lane, nv);
    carry::load_matrix(p.phi, d * d, pm);
    load_x(p, c, g, xt);
    if (p.kind == PARALLEL) {
        if (p.base)
            carry::load_tile(p.base + (int64_t)c * p.sbc, p.sbn, p.n, g, ot);
        else
            for (int t = lane; t < B * TP; t += B) ot[t] = 0.0;
    }
    for (int i = 0; i < d; ++i) st[i] = 0.0;
    __syncthreads();
    block(p.kind, xt + lane * TP, nullptr, nv, p.coef, d, p.aux, st, sn + lane * (d + 1));
    __syncthreads();
    const double t0 = lane < d ? p.gst[((size_t)c * p.n_groups + g) * d + lane] : 0.0;
    carry::scan(sb, pm, d, t0, true);
    __syncthreads();
    block(p.kind, xt + lane * TP, ot + lane * TP, nv, p.coef, d, p.aux, st, sn + lane * (d + 1));
    if (last)
        for (int i = 0; i < d; ++i) p.zf[(size_t)i * p.n_ch + c] = st[i];
    __syncthreads();
    for (int b = 0; b < nb; ++b)
        carry::store_tile(ot + b * B * TP, p.y + b * p.syb + (int64_t)c * p.syc, p.syn, p.n, g);
}

// ---- the direct FIR sum ---------------------------------------------------------------------------------------------
// y[n] = b[0] x[n] + sum_{i = 0 .. order - 1} b[i + 1] x[n - 1 - i], one fused multiply-add per term in that order, one
// writer per sample: two calls give the same bits.  A workgroup of FIR_NT threads owns FIR_TILE consecutive samples of one
// channel, a thread FIR_R = 4 consecutive ones.  The taps, zero-padded to a multiple of four (nt4 >= order + 1), and the
// window x[n0 - nt4 .. n0 + FIR_TILE) lie in LDS; samples before the signal come from the entry history hist[c][order]
// (x[-order] first) or are zero.  The window is stored in four planes by sample index mod 4, so that the threads of a wave
// read neighbouring addresses: per four taps a thread reads four new samples and four taps for sixteen multiply-adds.
constexpr int FIR_NT = 256, FIR_R = 4, FIR_TILE = FIR_NT * FIR_R, FIR_MAX_TAPS = 4096;

template <typename TI, typename TO>
struct FirArgs {
    const TI* x;
    int64_t sxc, sxn;
    TO* y;
    int64_t syc, syn;
    int64_t n;
    int n_ch, order, nt4;
    const double* taps;  // [nt4], zeros behind b[order]
    const double* hist;  // [n_ch][order] or null (zeros before the first sample)
};

__host__ __device__ inline int fir_nt4(int order) { return (order + 1 + 3) / 4 * 4; }
// doubles in one plane of the window: (nt4 + FIR_TILE) / 4 of them are used; 8 mod 32 spreads the planes over the banks
__host__ __device__ inline int fir_plane(int nt4) { return ((nt4 + FIR_TILE) / 4 + 31) / 32 * 32 + 8; }
__host__ __device__ inline size_t fir_lds_bytes(int nt4) { return sizeof(double) * ((size_t)nt4 + 4 * (size_t)fir_plane(nt4)); }

// grid = (ceil(n / FIR_TILE), n_ch), block = FIR_NT
template <typename TI, typename TO>
__global__ __launch_bounds__(FIR_NT) void k_rtfir(FirArgs<TI, TO> p) {
    extern __shared__ double flds[];
    const int P = p.nt4, U = fir_plane(P), tid = threadIdx.x, c = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * FIR_TILE;
    double* tp = flds;
    double* w = tp + P;
    for (int t = tid; t < P; t += FIR_NT) tp[t] = p.taps[t];
    const TI* xc = p.x + (int64_t)c * p.sxc;
    const double* hc = p.hist ? p.hist + (size_t)c * p.order : nullptr;
    for (int j = tid; j < P + FIR_TILE; j += FIR_NT) {
        const int64_t m = n0 - P + j;
        double v = 0.0;
        if (m >= 0) {
            if (m < p.n) v = (double)xc[m * p.sxn];
        } else if (hc && m >= -(int64_t)p.order) {
            v = hc[p.order + m];
        }
        w[(j & 3) * U + (j >> 2)] = v;
    }
    __syncthreads();
    // c_k = window sample (this thread's first output) - 4 ib + k; m_k the four before them
    int u = P / 4 + tid;
    double c0 = w[u], c1 = w[U + u], c2 = w[2 * U + u], c3 = w[3 * U + u];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int ib = 0; ib < P / 4; ++ib) {
        --u;
        const double m0 = w[u], m1 = w[U + u], m2 = w[2 * U + u], m3 = w[3 * U + u];
        const double b0 = tp[4 * ib], b1 = tp[4 * ib + 1], b2 = tp[4 * ib + 2], b3 = tp[4 * ib + 3];
        a0 = fma(b0, c0, a0); a1 = fma(b0, c1, a1); a2 = fma(b0, c2, a2); a3 = fma(b0, c3, a3);
        a0 = fma(b1, m3, a0); a1 = fma(b1, c0, a1); a2 = fma(b1, c1, a2); a3 = fma(b1, c2, a3);
        a0 = fma(b2, m2, a0); a1 = fma(b2, m3, a1); a2 = fma(b2, c0, a2); a3 = fma(b2, c1, a3);
        a0 = fma(b3, m1, a0); a1 = fma(b3, m2, a1); a2 = fma(b3, m3, a2); a3 = fma(b3, c0, a3);
        c0 = m0; c1 = m1; c2 = m2; c3 = m3;
    }
    const int64_t nn = n0 + 4 * (int64_t)tid;
    TO* yc = p.y + (int64_t)c * p.syc;
    if (nn < p.n) yc[nn * p.syn] = (TO)a0;
    if (nn + 1 < p.n) yc[(nn + 1) * p.syn] = (TO)a1;
    if (nn + 2 < p.n) yc[(nn + 2) * p.syn] = (TO)a2;
    if (nn + 3 < p.n) yc[(nn + 3) * p.syn] = (TO)a3;
}

}  // namespace rtfilt
