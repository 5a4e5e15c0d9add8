// The tile plan of the rational-ratio polyphase resampler (kernels_resample.hpp): plain integer arithmetic, no HIP types,
// shared by the kernel, by api.hip and by the host-side emulation of tests/host_san/resample_plan_san.cpp.
//
// For a coprime pair U = up, D = down: r = max(U, D), half = 10 r, ntaps = 20 r + 1 and
//     y[m] = sum_{j = 0 .. terms(p) - 1} h[p + U j] x[a - j],   t = m D + half, a = t / U, p = t % U,
// terms(p) = (2 half - p) / U + 1 <= J = ceil(ntaps / U).  A workgroup takes `tile` output samples of `cg` neighbouring
// channels.  Its LDS holds the tap table in phase-major order, U rows of JS = J | 1 doubles (row p: h[p + U j], zeros
// behind them; the odd row length keeps neighbouring phases on different banks), and behind it a window of `span` input
// samples of the cg channels.  Across a tile a advances by at most adv = ceil((tile - 1) D / U) samples, and an output
// looks J - 1 samples back.  Where adv + J samples fit, one window serves the whole sum.  Where they do not (decimation
// by hundreds: J is then thousands of samples) the sum runs in `chunks` pieces of jc terms, j ascending, and the window
// is staged again for each: chunk k holds the samples a0 - (k jc + jc - 1) .. a0 - k jc + adv of the tile whose first
// output reads a0, so term j of an output da samples further on reads window sample da + (k jc + jc - 1 - j).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace resample {

constexpr int NT = 256;                       // lanes of a workgroup
constexpr int PASSES = 4;                     // (output, channel) items a lane takes at most: tile cg <= PASSES NT
constexpr int LDS_DOUBLES = 160 * 1024 / 8;   // what a workgroup may declare
// The largest rate r = max(U, D) that is run: 44100 <-> 192000 is 640 / 147.  Its table is at most ntaps + 2 U - 1 <=
// 22 r + 1 = 14081 doubles (110 KB), which leaves every channel of a group of four 1599 samples of window: at least one
// output and one term, whatever the ratio.
constexpr int MAX_RATE = 640;
static_assert((LDS_DOUBLES - (22 * MAX_RATE + 1)) / 4 >= 1, "the table of the largest rate leaves no window");

// channels a workgroup takes together (they are neighbours in memory): 1, 2 or 4
RS_HD inline int ch_group(int n_ch) { return n_ch == 1 ? 1 : n_ch == 2 ? 2 : 4; }
RS_HD inline int ch_shift(int cg) { return cg == 1 ? 0 : cg == 2 ? 1 : 2; }

RS_HD inline int64_t out_len(int64_t n, int U, int D) { return (n * U + D - 1) / D; }

struct Plan {
    int U, D, cg;
    int half, ntaps;  // 10 r, 20 r + 1
    int J, JS;        // terms per output at most; doubles of a table row
    int tile;         // output samples of a workgroup: a power of two, at most PASSES NT / cg
    int adv;          // ceil((tile - 1) D / U)
    int jc, chunks;   // terms per staged window, windows per tile
    int span;         // adv + jc: staged samples per channel
};

RS_HD inline int table_doubles(const Plan& p) { return p.U * p.JS; }
RS_HD inline int lds_doubles(const Plan& p) { return table_doubles(p) + p.span * p.cg; }
RS_HD inline int tile_adv(int tile, int U, int D) { return (int)(((int64_t)(tile - 1) * D + U - 1) / U); }

// U, D coprime, 1 <= U, D <= MAX_RATE
RS_HD inline Plan make_plan(int U, int D, int n_ch) {
    Plan p{};
    p.U = U, p.D = D, p.cg = ch_group(n_ch);
    const int r = U > D ? U : D;
    p.half = 10 * r, p.ntaps = 20 * r + 1;
    p.J = (p.ntaps + U - 1) / U, p.JS = p.J | 1;
    const int w = (LDS_DOUBLES - table_doubles(p)) / p.cg;  // window samples per channel
    // the largest tile whose advance leaves room for the whole sum, or else takes at most half the window
    p.tile = PASSES * NT / p.cg;
    while (p.tile > 1 && tile_adv(p.tile, U, D) + p.J > w && tile_adv(p.tile, U, D) > w / 2) p.tile >>= 1;
    p.adv = tile_adv(p.tile, U, D);
    p.jc = p.J < w - p.adv ? p.J : w - p.adv;
    p.chunks = (p.J + p.jc - 1) / p.jc;
    p.span = p.adv + p.jc;
    return p;
}

// what the first output of a tile reads: t = m0 D + half = a0 U + p0
struct Origin {
    int64_t a0;
    int p0;
};
RS_HD inline Origin origin(const Plan& p, int64_t m0) {
    const int64_t t = m0 * p.D + p.half;
    return Origin{t / p.U, (int)(t % p.U)};
}

// output ml of the tile: it reads from sample a0 + da back, with phase ph
struct Item {
    int da, ph;
};
RS_HD inline Item item(const Plan& p, const Origin& o, int ml) {
    const int local = o.p0 + ml * p.D;  // below (PASSES NT + 1) MAX_RATE
    const int da = local / p.U;
    return Item{da, local - da * p.U};
}
RS_HD inline int terms(const Plan& p, int ph) { return (2 * p.half - ph) / p.U + 1; }

// chunk k of a tile: its terms j0 <= j < j0 + jc, the input sample its window starts at, and where term j of an item
// lies in it
RS_HD inline int chunk_first_term(const Plan& p, int k) { return k * p.jc; }
RS_HD inline int64_t window_first(const Plan& p, const Origin& o, int k) { return o.a0 - (chunk_first_term(p, k) + p.jc - 1); }
RS_HD inline int window_index(const Plan& p, int k, int da, int j) { return da + (chunk_first_term(p, k) + p.jc - 1 - j); }

// the phase-major table the host builds from the taps h[0 .. ntaps): hp has table_doubles(p) elements
inline void phase_major(const Plan& p, const double* h, double* hp) {
    for (int ph = 0; ph < p.U; ++ph)
        for (int j = 0; j < p.JS; ++j) {
            const int64_t k = ph + (int64_t)p.U * j;
            hp[ph * p.JS + j] = k < p.ntaps ? h[k] : 0.0;
        }
}

}  // namespace resample
