// Rational-ratio polyphase resampling (reference: standard.resample, standard/resampling.py:9-43, which is
// scipy.signal.resample_poly with its default filter).  float64 arithmetic, gfx950.  For a coprime pair U = up, D = down,
// r = max(U, D), half = 10 r and the taps h = U firwin(20 r + 1, 1 / r, kaiser 5.0):
//     y[m] = sum_n x[n] h[m D + half - n U],   m < ceil(n_in U / D)
// which in polyphase form, t = m D + half, a = t / U, p = t % U, is
//     y[m] = sum_{j = 0 .. (2 half - p) / U} h[p + U j] x[a - j].
//   k_resample_poly  one launch for every ratio but 1 / 1, integer ratios included.  A workgroup takes a tile of output
//                    samples of 1, 2 or 4 neighbouring channels (resample_plan.hpp).  The tap table lies in LDS in
//                    phase-major order, so an output's taps are contiguous; the input window of the tile lies behind it,
//                    zeros where it leaves [0, n_in), widened to float64 as it is staged.  A lane takes up to PASSES
//                    (output, channel) items and sums each with j ascending.  Input and output are addressed through a
//                    sample and a channel stride: float64 interleaved on a host call's side, float32 planar where a
//                    device-resident signal lies.
// No atomics, every output has one writer, every sum a fixed order: a call returns the same bits every time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resample_plan.hpp"

namespace resample {

template <typename TI, typename TO>
struct PolyArgs {
    const TI* x;  // sample n of channel c at x[n xss + c xcs]
    int64_t xss, xcs, n_in;
    const double* hp;  // the phase-major table: table_doubles(pl)
    TO* y;             // sample m of channel c at y[m yss + c ycs]
    int64_t yss, ycs, n_out;
    int n_ch;
    Plan pl;
};

// grid = (ceil(n_out / tile), ceil(n_ch / cg)); LDS: lds_doubles(pl) doubles
template <typename TI, typename TO>
__global__ __launch_bounds__(NT) void k_resample_poly(PolyArgs<TI, TO> q) {
    extern __shared__ double lds[];
    const Plan pl = q.pl;
    const int n_table = table_doubles(pl);
    double* hs = lds;
    double* xs = lds + n_table;
    const int t = threadIdx.x, cg = pl.cg, sh = ch_shift(cg), c0 = blockIdx.y * cg;
    const int64_t m0 = (int64_t)blockIdx.x * pl.tile;
    const Origin o = origin(pl, m0);
    for (int k = t; k < n_table; k += NT) hs[k] = q.hp[k];
    const int n_items = pl.tile << sh, n_staged = pl.span * cg;
    const bool planar_in = q.xss == 1, planar_out = q.yss == 1;  // planar: neighbouring lanes take neighbouring samples
    double acc[PASSES];
#pragma unroll
    for (int it = 0; it < PASSES; ++it) acc[it] = 0.0;
    for (int k = 0; k < pl.chunks; ++k) {
        const int j0 = chunk_first_term(pl, k);
        const int64_t q0 = window_first(pl, o, k);
        if (k) __syncthreads();  // the window of the chunk before has been read
        for (int e = t; e < n_staged; e += NT) {
            int s, c;
            if (planar_in) {
                c = e / pl.span;
                s = e - c * pl.span;
            } else {
                s = e >> sh;
                c = e & (cg - 1);
            }
            const int64_t n = q0 + s;
            double v = 0.0;
            if (n >= 0 && n < q.n_in && c0 + c < q.n_ch) v = (double)q.x[n * q.xss + (int64_t)(c0 + c) * q.xcs];
            xs[s * cg + c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < PASSES; ++it) {
            const int e = t + it * NT;
            if (e >= n_items) continue;
            const int cl = planar_out ? e / pl.tile : e & (cg - 1);
            const int ml = planar_out ? e - cl * pl.tile : e >> sh;
            const Item i = item(pl, o, ml);
            const int last = terms(pl, i.ph), end = last < j0 + pl.jc ? last : j0 + pl.jc;
            const double* hp = hs + i.ph * pl.JS;
            const double* xp = xs + (size_t)window_index(pl, k, i.da, 0) * cg + cl;  // the sample term 0 would meet
            double a = acc[it];
            for (int j = j0; j < end; ++j) a = fma(hp[j], xp[-(j * cg)], a);
            acc[it] = a;
        }
    }
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int e = t + it * NT;
        if (e >= n_items) continue;
        const int cl = planar_out ? e / pl.tile : e & (cg - 1);
        const int ml = planar_out ? e - cl * pl.tile : e >> sh;
        const int64_t m = m0 + ml;
        if (m < q.n_out && c0 + cl < q.n_ch) q.y[m * q.yss + (int64_t)(c0 + cl) * q.ycs] = (TO)acc[it];
    }
}

}  // namespace resample
