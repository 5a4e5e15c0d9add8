// The block carry: the time-parallel form of a linear recursion over D <= 64 state values that the iir, ciir and sfilt
// kernel families share.  gfx950.
//
// With zero input the state moves as S' = A S; over a block of L samples
//     S_{b+1} = Phi S_b + s_b,     Phi = A^L,
// s_b the final state of block b run from zero state.  Three passes carry it:
//   group  one lane per block of L samples, one wave per group of B blocks: s_b for every block, then a serial in-wave
//          scan over the B blocks (lane i holds S[i]) gives the group's state from zero entry, t_g.
//   carry  one wave per stream: T_{g+1} = Phi^B T_g + t_g from T_0 = zi, serially over the groups (k_block_carry for
//          real states).
//   apply  one wave per (group, channel): s_b again, the in-wave scan from T_g gives each block's true entry state, and
//          each lane reruns its block from it and writes the output.
// Here: the block shape, the padded LDS tile and its load and store, the real scan and the real carry kernel.  The
// families keep their recursions, their group and apply kernels and (ciir) the complex scan and carry.  The host builds
// A, Phi and Phi^B with carry_tables.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "carry_tables.hpp"

namespace carry {

constexpr int G = L * B;   // samples per group
constexpr int TP = L + 1;  // LDS tile row: one block, padded against bank conflicts

// group g of one channel's samples (sample n at x[n sxn]) into the tile, zeros past the end
template <typename T>
__device__ inline void load_tile(const T* x, int64_t sxn, int64_t n, int64_t g, double* xt) {
    for (int t = threadIdx.x; t < G; t += B) {
        const int64_t nn = g * G + t;
        xt[(t / L) * TP + t % L] = nn < n ? (double)x[nn * sxn] : 0.0;
    }
}

// the tile to group g of one channel's output (sample n at y[n syn]) in coalesced rows; the caller's barrier lies
// between the lanes' writes to ot and this
template <typename T>
__device__ inline void store_tile(const double* ot, T* y, int64_t syn, int64_t n, int64_t g) {
    for (int t = threadIdx.x; t < G; t += B) {
        const int64_t nn = g * G + t;
        if (nn < n) y[nn * syn] = (T)ot[(t / L) * TP + t % L];
    }
}

__device__ inline void load_matrix(const double* src, int count, double* dst) {
    for (int t = threadIdx.x; t < count; t += B) dst[t] = src[t];
}

__device__ inline int valid_in_block(int64_t n, int64_t g, int lane) {
    const int64_t v = n - (g * G + (int64_t)lane * L);
    return v <= 0 ? 0 : (v >= L ? L : (int)v);
}

// a final state is asked for (p.zf) and this lane's block, nv = valid_in_block of it, holds the last of the p.n samples:
// the lane that writes zf.  p: the family's Args, by reference so that n and zf are read where the test needs them (read
// ahead as plain parameters they change k_ciir_apply's instruction order)
template <typename A>
__device__ inline bool holds_last(const A& p, int64_t g, int lane, int nv) {
    return p.zf && nv > 0 && g * G + (int64_t)lane * L + nv == p.n;
}

// serial scan over the B blocks of a group, lane i < D holding S[i]: S <- P S + s_b.  With keep_entry the entry
// state of block b replaces s_b in sb (what the apply kernels rerun from).  Returns the state after the last block.
__device__ inline double scan(double* sb, const double* pm, int d, double s, bool keep_entry) {
    const int lane = threadIdx.x;
    const double* row = pm + (lane < d ? lane : 0) * d;
    for (int b = 0; b < B; ++b) {
        double* sbb = sb + b * (d + 1);
        double acc = lane < d ? sbb[lane] : 0.0;
        for (int j = 0; j < d; ++j) acc = fma(row[j], __shfl(s, j), acc);
        if (keep_entry && lane < d) sbb[lane] = s;
        s = acc;
    }
    return s;
}

struct CarryArgs {
    const double* phig;  // [n_filt][D][D]
    double* gst;         // [n_filt n_ch][n_groups][D]
    const double* zi;    // [n_filt][D][n_ch] or null
    int64_t n_groups;
    int n_ch, d;
};

// grid = n_filt n_ch, block = B: the entry state T_g of every group, in place of t_g
__global__ __launch_bounds__(B) void k_block_carry(CarryArgs p) {
    extern __shared__ double lds[];
    const int d = p.d, lane = threadIdx.x;
    const int stream = blockIdx.x, f = stream / p.n_ch, c = stream % p.n_ch;
    double* pm = lds;
    load_matrix(p.phig + (size_t)f * d * d, d * d, pm);
    __syncthreads();
    const double* row = pm + (lane < d ? lane : 0) * d;
    double s = (p.zi && lane < d) ? p.zi[((size_t)f * d + lane) * p.n_ch + c] : 0.0;
    double* gs = p.gst + (size_t)stream * p.n_groups * d;
    for (int64_t g = 0; g < p.n_groups; ++g) {
        double acc = (lane < d && g + 1 < p.n_groups) ? gs[g * d + lane] : 0.0;
        for (int j = 0; j < d; ++j) acc = fma(row[j], __shfl(s, j), acc);
        if (lane < d) gs[g * d + lane] = s;
        s = acc;
    }
}

}  // namespace carry
