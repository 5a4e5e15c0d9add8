// The all-pass table of frequency warping and of the discrete Laguerre transform, float64, gfx950 (transforms.warp and
// transforms.laguerre of the reference, transforms/transforms.py:955-1130 with transforms/_transforms.py:386-428):
//   c[i][j] = p c[i-1][j] + c[i-1][j-1] + q c[i][j-1]  (i, j >= 1),   out[j][ch] = sum_i c[i][j] x[i][ch]
// with a given first row c[0][.] and first column c[.][0] (c[0][0] is taken from the column).
//   k_allpass_tile  one workgroup per tile of TI input rows x TJ output columns (warp_plan.hpp) and per group of G
//               channels.  A lane owns an output column: its sum over i stays in its registers, G accumulators.  The
//               lanes of a wave run one row apart -- lane l is at row t - l in step t -- so cell (i, j) finds
//               c[i][j-1] in the left lane's register as that lane left it one step ago (one lane shift, two DPP
//               moves), c[i-1][j-1] in what the shift delivered the step before, and c[i-1][j] in its own register.
//               Wave w + 1 runs STAGGER = 128 steps behind wave w: the last lane of wave w writes its column to LDS,
//               the first lane of wave w + 1 reads it back 65 steps later, and a workgroup barrier every 64 steps
//               separates the two -- no wave ever waits for a value inside a step.  The column left of the tile is
//               staged into the same LDS array (the "column of wave -1"), the last wave's column leaves through it.
//               The tile's rows of x lie in LDS as [row][G]; a lane reads the row it is at, one step ahead of its use.
//               A tile takes rows + 63 + 3 x 128 steps for rows x 256 cells: 70 % of the lane-steps compute at TI = 1024.
//               The tiles I = 0 start their sums with row0[j] x[0]; the tiles J = 0 also add the first column's
//               sum_i col0[i] x[i] to out[0] (a workgroup reduction in a fixed order).  Everything else starts from
//               what the tile above left in out: tiles of one column run in different launches, nothing is atomic
//               and repeats give the same bits.  With p = q = 0 every product is an exact zero or the sample itself.
// No workgroup waits for another: the host launches one grid per tile anti-diagonal (api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "warp_plan.hpp"

namespace dswarp {

constexpr size_t tile_lds_bytes() { return ((size_t)(WAVES + 1) * TI + (size_t)TI * G) * 8; }

struct TileArgs {
    const void* x;       // element (i, ch) at x[i ss + ch cs], double or float
    int64_t ss, cs;
    int n_ch;
    double p, q;
    double* ws;          // the two boundary buffers (warp_plan.hpp)
    double* out;         // (n_out, n_ch)
    Plan plan;
    int64_t d;           // the launch: tiles with I + J = d
};

// the value of the lane to the left (lane 0 keeps its own): wave_shr:1 on both halves
__device__ __forceinline__ double lane_shr1(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// grid = (tiles of the anti-diagonal, channel groups), TJ lanes
template <typename T>
__global__ __launch_bounds__(TJ) void k_allpass_tile(TileArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[WAVES][G];
    double* edge = lds;                        // [WAVES + 1][TI]: row r of the column left of wave w at edge[w TI + r]
    double* xs = lds + (size_t)(WAVES + 1) * TI;  // [TI][G]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Plan& pl = a.plan;
    const Diagonal dg = diagonal(pl, a.d);
    const int64_t I = dg.first_i + blockIdx.x, J = a.d - I;
    const Tile t = tile(pl, I, J);
    const int ch0 = blockIdx.y * G;
    const double* rd = a.ws + read_buffer(a.d) * buffer_doubles(pl);
    double* wr = a.ws + write_buffer(a.d) * buffer_doubles(pl);
    const T* x = (const T*)a.x;

    for (int r = tid; r < t.rows; r += TJ) edge[r] = rd[col_slot(pl, t.i0 + r)];
    for (int k = tid; k < t.rows * G; k += TJ) {
        const int r = k / G, ch = ch0 + k % G;
        xs[k] = ch < a.n_ch ? (double)x[(t.i0 + r) * a.ss + ch * a.cs] : 0.0;
    }
    const int64_t j = t.j0 + tid;
    const bool col_ok = tid < t.cols;
    const double corner = rd[corner_slot(pl, J)];
    double cur = col_ok ? rd[row_slot(pl, j)] : 0.0;                                       // c[i0 - 1][j]
    double diag = tid == 0 ? corner : (tid - 1 < t.cols ? rd[row_slot(pl, j - 1)] : 0.0);  // c[i0 - 1][j - 1]
    double acc[G];  // the tiles I = 0 start from the first row's term, the others from what the tile above left
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int ch = ch0 + g;
        acc[g] = 0.0;
        if (col_ok && ch < a.n_ch) acc[g] = I == 0 ? cur * (double)x[ch * a.cs] : a.out[j * a.n_ch + ch];
    }
    __syncthreads();

    const int steps = t.rows > 0 && t.cols > 0 ? tile_steps(t.rows) : 0;
    const int behind = lane + STAGGER * wave;  // row = step - behind
    const double* in_col = edge + wave * TI;   // the column left of this wave
    double* out_col = edge + (wave + 1) * TI;  // this wave's last column
    for (int t0 = 0; t0 < steps; t0 += WAVE) {
        if (t0 + WAVE > STAGGER * wave && t0 < STAGGER * wave + t.rows + WAVE - 1) {
            // The LDS reads of a step -- the row's samples and, for lane 0, the value left of it -- are issued one step
            // ahead, at a row clamped into the tile, so that no step waits for LDS between its shift and its multiply-adds.
            // Never across a barrier: the first step of a chunk issues its own.
            double xn[G], en;
            {
                const int rn = min(max(t0 - behind, 0), t.rows - 1);
#pragma unroll
                for (int g = 0; g < G; ++g) xn[g] = xs[rn * G + g];
                en = in_col[rn];
            }
            for (int s = 0; s < WAVE; ++s) {
                const int r = t0 + s - behind;
                const bool active = r >= 0 && r < t.rows;
                double left = lane_shr1(cur);  // every lane takes part, whatever row it is at
                if (lane == 0) left = en;
                double xc[G];
#pragma unroll
                for (int g = 0; g < G; ++g) xc[g] = xn[g];
                if (s + 1 < WAVE) {
                    const int rn = min(max(r + 1, 0), t.rows - 1);
#pragma unroll
                    for (int g = 0; g < G; ++g) xn[g] = xs[rn * G + g];
                    en = in_col[rn];
                }
                // lanes outside the tile's rows keep their state and add an exact zero
                const double c = fma(a.q, left, fma(a.p, cur, diag));
                diag = active ? left : diag;
                cur = active ? c : cur;
                const double term = active ? c : 0.0;
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = fma(term, xc[g], acc[g]);
                if (lane == WAVE - 1 && active) out_col[r] = c;
            }
        }
        __syncthreads();
    }

    if (col_ok) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (ch0 + g < a.n_ch) a.out[j * a.n_ch + ch0 + g] = acc[g];
    }
    if (J == 0) {  // the first column's share of out[0]
        double part[G];
#pragma unroll
        for (int g = 0; g < G; ++g) part[g] = 0.0;
        for (int r = tid; r < t.rows; r += TJ) {
#pragma unroll
            for (int g = 0; g < G; ++g) part[g] = fma(edge[r], xs[r * G + g], part[g]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double s = wave_sum(part[g]);
            if (lane == 0) red[wave][g] = s;
        }
        __syncthreads();
        if (tid < G && ch0 + tid < a.n_ch) {
            double s = red[0][tid];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += red[w][tid];
            const double before = I == 0 ? rd[col_slot(pl, 0)] * (double)x[(ch0 + tid) * a.cs] : a.out[ch0 + tid];
            a.out[ch0 + tid] = before + s;
        }
    }
    if (blockIdx.y != 0) return;  // the table does not depend on the channels: group 0 hands it on
    if (I + 1 < pl.tiles_i) {
        if (col_ok) wr[row_slot(pl, j)] = cur;
        if (tid == 0) wr[corner_slot(pl, J)] = t.rows > 0 ? edge[t.rows - 1] : corner;
    }
    if (J + 1 < pl.tiles_j)
        for (int r = tid; r < t.rows; r += TJ) wr[col_slot(pl, t.i0 + r)] = edge[WAVES * TI + r];
}

}  // namespace dswarp
