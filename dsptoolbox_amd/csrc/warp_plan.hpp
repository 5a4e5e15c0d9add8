// The tile schedule of the all-pass table (kernels_warp.hpp): plain integer arithmetic, no HIP types, shared by the
// kernel, by api.hip and by the host-side emulation of tests/host_san/warp_plan_san.cpp.
//
// The table c[i][j], 0 <= i < n_in, 0 <= j < n_out, has a given first row and first column; the cells i, j >= 1 follow
// c[i][j] = p c[i-1][j] + c[i-1][j-1] + q c[i][j-1].  Tile (I, J) covers the computed cells i = 1 + I TI + r,
// j = 1 + J TJ + l; it needs the row above it, the column left of it and the corner between the two, and hands its last
// row and last column on.  Tiles with I + J = d are independent: launch d runs them all, the stream orders the launches.
//
// Boundary storage: two buffers, read and written alternately.  Launch d reads buffer d & 1 and writes buffer (d + 1) & 1,
// so no slot is read and written inside one launch, whichever workgroup (channel groups repeat the table) gets there
// first.  A buffer holds a row slot per output column, a column slot per input row and a corner slot per tile column:
//   row slot j       c[i0 - 1][j] for the tile (I, J) that owns column j: row0[j] before launch J, later the last row of
//                    tile (I - 1, J), written in launch d - 1;
//   column slot i    c[i][j0 - 1]: col0[i] before launch I, later the last column of tile (I, J - 1);
//   corner slot J    c[i0 - 1][j0 - 1].  It is the last element of the column left of tile (I - 1, J) and the element
//                    before the row above tile (I, J): both of those slots are overwritten in launch d - 1 by the
//                    neighbours, so tile (I - 1, J) carries it along with its last row.  Before launch J it is
//                    row0[J TJ].
// Both buffers start as the same image of row0, col0 and the row-0 corners, built on the host.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define WP_HD __host__ __device__
#else
#define WP_HD
#endif

namespace dswarp {

constexpr int WAVE = 64;
constexpr int WAVES = 4;            // waves of a tile's workgroup
constexpr int TJ = WAVE * WAVES;    // output columns of a tile: a lane each
constexpr int TI = 1024;            // input rows of a tile
constexpr int G = 4;                // channels a workgroup accumulates; further groups are further workgroups
constexpr int STAGGER = 128;        // steps wave w + 1 runs behind wave w (kernels_warp.hpp)

struct Plan {
    int64_t n_in, n_out;
    int64_t tiles_i, tiles_j;  // at least 1 each: the first row and column are folded into the tiles I = 0 and J = 0
    int64_t launches;          // tiles_i + tiles_j - 1
};

struct Diagonal {
    int64_t first_i, count;    // launch d runs the tiles (first_i + b, d - first_i - b), b < count
};

struct Tile {
    int64_t i0, j0;            // first computed row and column
    int rows, cols;            // 0 <= rows <= TI, 0 <= cols <= TJ (0 only where n_in or n_out is 1)
};

WP_HD inline Plan make_plan(int64_t n_in, int64_t n_out) {
    Plan p{n_in, n_out, (n_in - 1 + TI - 1) / TI, (n_out - 1 + TJ - 1) / TJ, 0};
    if (p.tiles_i < 1) p.tiles_i = 1;
    if (p.tiles_j < 1) p.tiles_j = 1;
    p.launches = p.tiles_i + p.tiles_j - 1;
    return p;
}

WP_HD inline Diagonal diagonal(const Plan& p, int64_t d) {
    const int64_t lo = d - (p.tiles_j - 1) > 0 ? d - (p.tiles_j - 1) : 0;
    const int64_t hi = d < p.tiles_i - 1 ? d : p.tiles_i - 1;
    return Diagonal{lo, hi - lo + 1};
}

WP_HD inline Tile tile(const Plan& p, int64_t I, int64_t J) {
    Tile t{1 + I * TI, 1 + J * TJ, 0, 0};
    const int64_t rows = p.n_in - t.i0, cols = p.n_out - t.j0;
    t.rows = (int)(rows > TI ? TI : rows);
    t.cols = (int)(cols > TJ ? TJ : cols);
    return t;
}

// doubles of one boundary buffer, and where its slots lie
WP_HD inline int64_t buffer_doubles(const Plan& p) { return p.n_out + p.n_in + p.tiles_j; }
WP_HD inline int64_t row_slot(const Plan&, int64_t j) { return j; }
WP_HD inline int64_t col_slot(const Plan& p, int64_t i) { return p.n_out + i; }
WP_HD inline int64_t corner_slot(const Plan& p, int64_t J) { return p.n_out + p.n_in + J; }
WP_HD inline int read_buffer(int64_t d) { return (int)(d & 1); }
WP_HD inline int write_buffer(int64_t d) { return (int)((d + 1) & 1); }
WP_HD inline int64_t workspace_doubles(const Plan& p) { return 2 * buffer_doubles(p); }

// the image both buffers start from; init has workspace_doubles(p) elements
inline void initial_image(const Plan& p, const double* row0, const double* col0, double* init) {
    for (int b = 0; b < 2; ++b) {
        double* buf = init + b * buffer_doubles(p);
        for (int64_t j = 0; j < p.n_out; ++j) buf[row_slot(p, j)] = row0[j];
        for (int64_t i = 0; i < p.n_in; ++i) buf[col_slot(p, i)] = col0[i];
        for (int64_t J = 0; J < p.tiles_j; ++J) buf[corner_slot(p, J)] = row0[J * TJ];
    }
}

// steps of a tile's main loop: the last wave's last lane reaches the last row
WP_HD inline int tile_steps(int rows) { return rows + (WAVE - 1) + STAGGER * (WAVES - 1); }

}  // namespace dswarp
