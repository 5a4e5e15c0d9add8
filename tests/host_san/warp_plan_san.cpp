// The tile schedule of the all-pass table (csrc/warp_plan.hpp) and the arrangement of k_allpass_tile
// (csrc/kernels_warp.hpp) emulated in plain C++, built with -fsanitize=address,undefined and run on the CPU
// (tests/test_warp_host.py).  Launch by launch, tile by tile, the emulation does what the kernel does: it stages the
// column left of the tile and the tile's samples, runs the lanes one row apart and the waves STAGGER steps apart in
// chunks of 64 steps between barriers, hands the last lane's column to the next wave through the edge array, folds the
// first row and the first column in, and writes the boundary slots of the other buffer.  Checked:
//   - out agrees with the table computed cell by cell within 1e-13 of each channel's peak;
//   - every boundary slot a tile reads was written by the tile the schedule says (or is still the initial image), so
//     nothing is read before it is written or after it is overwritten, and no launch writes a slot it reads;
//   - every edge value a wave reads was written in an EARLIER chunk (a barrier lies between), whatever order the waves
//     of a chunk run in (here: last wave first);
//   - every index stays inside its array (the sanitizer).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dsptoolbox_amd/csrc/warp_plan.hpp"

using namespace dswarp;

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

static const int64_t INITIAL = -1;

struct Device {
    Plan pl;
    int n_ch;
    double p, q;
    std::vector<double> x;        // (n_in, n_ch)
    std::vector<double> ws;       // two buffers
    std::vector<int64_t> writer;  // per slot: the tile (I tiles_j + J) that wrote it last, or INITIAL
    std::vector<int64_t> read_in, written_in;  // per slot: the last launch that read / wrote it
    std::vector<double> out;      // (n_out, n_ch)
};

static double read_slot(Device& dv, int64_t d, int64_t slot, int64_t expected_writer) {
    const int64_t at = read_buffer(d) * buffer_doubles(dv.pl) + slot;
    REQUIRE(slot >= 0 && slot < buffer_doubles(dv.pl));
    REQUIRE(dv.writer[at] == expected_writer);
    REQUIRE(dv.written_in[at] != d);
    dv.read_in[at] = d;
    return dv.ws[at];
}

static void write_slot(Device& dv, int64_t d, int64_t slot, int64_t tile_id, double v) {
    const int64_t at = write_buffer(d) * buffer_doubles(dv.pl) + slot;
    REQUIRE(slot >= 0 && slot < buffer_doubles(dv.pl));
    REQUIRE(dv.read_in[at] != d);
    dv.ws[at] = v;
    dv.writer[at] = tile_id;
    dv.written_in[at] = d;
}

// one workgroup of k_allpass_tile: tile (I, J) of launch d, channel group `group`
static void run_tile(Device& dv, int64_t d, int64_t I, int64_t J, int group) {
    const Plan& pl = dv.pl;
    const Tile t = tile(pl, I, J);
    REQUIRE(t.rows >= 0 && t.rows <= TI && t.cols >= 0 && t.cols <= TJ);
    const int ch0 = group * G;
    const int64_t id = I * pl.tiles_j + J, above = I > 0 ? id - pl.tiles_j : INITIAL, left_of = J > 0 ? id - 1 : INITIAL;
    std::vector<double> edge((size_t)(WAVES + 1) * TI, 0.0), xs((size_t)TI * G, 0.0);
    std::vector<int> edge_chunk((size_t)(WAVES + 1) * TI, -2);  // -2: never written, -1: staged, else the chunk
    for (int r = 0; r < t.rows; ++r) {
        edge[r] = read_slot(dv, d, col_slot(pl, t.i0 + r), left_of);
        edge_chunk[r] = -1;
    }
    for (int k = 0; k < t.rows * G; ++k) {
        const int r = k / G, ch = ch0 + k % G;
        REQUIRE(t.i0 + r < pl.n_in);
        xs[k] = ch < dv.n_ch ? dv.x[(t.i0 + r) * dv.n_ch + ch] : 0.0;
    }
    const double corner = read_slot(dv, d, corner_slot(pl, J), above);
    std::vector<double> cur(TJ), diag(TJ), acc((size_t)TJ * G, 0.0);
    for (int tid = 0; tid < TJ; ++tid) {
        const int64_t j = t.j0 + tid;
        const bool col_ok = tid < t.cols;
        cur[tid] = col_ok ? read_slot(dv, d, row_slot(pl, j), above) : 0.0;
        diag[tid] = tid == 0 ? corner : (tid - 1 < t.cols ? read_slot(dv, d, row_slot(pl, j - 1), above) : 0.0);
        for (int g = 0; g < G; ++g) {
            const int ch = ch0 + g;
            if (col_ok && ch < dv.n_ch) acc[tid * G + g] = I == 0 ? cur[tid] * dv.x[ch] : dv.out[j * dv.n_ch + ch];
        }
    }
    const int steps = t.rows > 0 && t.cols > 0 ? tile_steps(t.rows) : 0;
    for (int t0 = 0, chunk = 0; t0 < steps; t0 += WAVE, ++chunk) {
        for (int wave = WAVES - 1; wave >= 0; --wave) {
            if (!(t0 + WAVE > STAGGER * wave && t0 < STAGGER * wave + t.rows + WAVE - 1)) continue;
            // lane 0's value from the column left of the wave is read one step ahead of its use, at a row clamped into
            // the tile, never across a barrier: the first step of a chunk reads its own
            double en = 0.0;
            int en_chunk = -2;
            auto fetch = [&](int r) {
                const int rn = r < 0 ? 0 : (r > t.rows - 1 ? t.rows - 1 : r);
                en = edge[wave * TI + rn];
                en_chunk = edge_chunk[wave * TI + rn];
            };
            fetch(t0 - STAGGER * wave);
            for (int s = 0; s < WAVE; ++s) {
                double shifted[WAVE];  // the lane shift: every lane's value before any lane's update
                for (int lane = 0; lane < WAVE; ++lane) shifted[lane] = cur[wave * WAVE + (lane > 0 ? lane - 1 : 0)];
                const double left0 = en;
                const int left0_chunk = en_chunk;
                if (s + 1 < WAVE) fetch(t0 + s - STAGGER * wave + 1);
                for (int lane = 0; lane < WAVE; ++lane) {
                    const int tid = wave * WAVE + lane, r = t0 + s - (lane + STAGGER * wave);
                    if (r < 0 || r >= t.rows) continue;  // (the kernel: state kept, an exact zero added)
                    double left = shifted[lane];
                    if (lane == 0) {
                        REQUIRE(left0_chunk != -2 && left0_chunk < chunk);
                        left = left0;
                    }
                    const double c = std::fma(dv.q, left, std::fma(dv.p, cur[tid], diag[tid]));
                    diag[tid] = left;
                    cur[tid] = c;
                    for (int g = 0; g < G; ++g) acc[tid * G + g] = std::fma(c, xs[r * G + g], acc[tid * G + g]);
                    if (lane == WAVE - 1) {
                        edge[(wave + 1) * TI + r] = c;
                        edge_chunk[(wave + 1) * TI + r] = chunk;
                    }
                }
            }
        }
    }
    // every wave ran through its rows
    if (steps)
        for (int w = 1; w <= WAVES; ++w) REQUIRE(edge_chunk[w * TI + t.rows - 1] >= 0);
    for (int tid = 0; tid < t.cols; ++tid)
        for (int g = 0; g < G; ++g)
            if (ch0 + g < dv.n_ch) dv.out[(t.j0 + tid) * dv.n_ch + ch0 + g] = acc[tid * G + g];
    if (J == 0) {
        for (int g = 0; g < G && ch0 + g < dv.n_ch; ++g) {
            double red[WAVES] = {};
            for (int tid = 0; tid < TJ; ++tid) {  // (the kernel adds a wave's lanes by a butterfly; any order is within the bound)
                double part = 0.0;
                for (int r = tid; r < t.rows; r += TJ) part = std::fma(edge[r], xs[r * G + g], part);
                red[tid / WAVE] += part;
            }
            double s = red[0];
            for (int w = 1; w < WAVES; ++w) s += red[w];
            const double before = I == 0 ? read_slot(dv, d, col_slot(pl, 0), INITIAL) * dv.x[ch0 + g] : dv.out[ch0 + g];
            dv.out[ch0 + g] = before + s;
        }
    }
    if (group != 0) return;
    if (I + 1 < pl.tiles_i) {
        for (int tid = 0; tid < t.cols; ++tid) write_slot(dv, d, row_slot(pl, t.j0 + tid), id, cur[tid]);
        write_slot(dv, d, corner_slot(pl, J), id, t.rows > 0 ? edge[t.rows - 1] : corner);
    }
    if (J + 1 < pl.tiles_j) {
        REQUIRE(t.cols == TJ);
        for (int r = 0; r < t.rows; ++r) {
            REQUIRE(edge_chunk[WAVES * TI + r] >= 0);
            write_slot(dv, d, col_slot(pl, t.i0 + r), id, edge[WAVES * TI + r]);
        }
    }
}

static double check_shape(int64_t n_in, int64_t n_out, int n_ch, double lam, bool laguerre) {
    Device dv;
    dv.pl = make_plan(n_in, n_out);
    dv.n_ch = n_ch;
    dv.p = -lam;
    dv.q = lam;
    std::vector<double> row0(n_out), col0(n_in);
    const double s = laguerre ? std::sqrt(1.0 - lam * lam) : 1.0;
    for (int64_t j = 0; j < n_out; ++j) row0[j] = laguerre ? (j ? row0[j - 1] * lam : s) : (j == 0);
    for (int64_t i = 0; i < n_in; ++i) col0[i] = i ? col0[i - 1] * -lam : s;
    dv.x.resize((size_t)n_in * n_ch);
    uint64_t state = 88172645463325252ull + (uint64_t)n_in * 1315423911u + (uint64_t)n_out;
    for (double& v : dv.x) {  // xorshift noise in [-1, 1) under a decaying envelope
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        const size_t at = (size_t)(&v - dv.x.data()) / n_ch;
        v = ((double)(state >> 11) / 4503599627370496.0 - 1.0) * std::exp(-6.9 * (double)at / (double)n_in);
    }
    const Plan& pl = dv.pl;
    REQUIRE(pl.tiles_i >= 1 && pl.tiles_j >= 1 && pl.launches == pl.tiles_i + pl.tiles_j - 1);
    dv.ws.assign((size_t)workspace_doubles(pl), 0.0);
    initial_image(pl, row0.data(), col0.data(), dv.ws.data());
    dv.writer.assign(dv.ws.size(), INITIAL);
    dv.read_in.assign(dv.ws.size(), -1);
    dv.written_in.assign(dv.ws.size(), -1);
    dv.out.assign((size_t)n_out * n_ch, std::nan(""));  // every element must be written before it is read
    std::vector<int> ran((size_t)(pl.tiles_i * pl.tiles_j), 0);
    const int groups = (n_ch + G - 1) / G;
    for (int64_t d = 0; d < pl.launches; ++d) {
        const Diagonal dg = diagonal(pl, d);
        REQUIRE(dg.count >= 1);
        for (int group = groups - 1; group >= 0; --group)  // (group 0, which writes the boundaries, last)
            for (int64_t b = dg.count - 1; b >= 0; --b) {
                const int64_t I = dg.first_i + b, J = d - I;
                REQUIRE(I >= 0 && I < pl.tiles_i && J >= 0 && J < pl.tiles_j);
                run_tile(dv, d, I, J, group);
                if (group == 0) ++ran[I * pl.tiles_j + J];
            }
    }
    for (int v : ran) REQUIRE(v == 1);

    // the table cell by cell
    std::vector<double> prev(n_out), row(n_out), want((size_t)n_out * n_ch, 0.0);
    for (int64_t i = 0; i < n_in; ++i) {
        for (int64_t j = 0; j < n_out; ++j) {
            if (j == 0) row[j] = col0[i];
            else if (i == 0) row[j] = row0[j];
            else row[j] = dv.p * prev[j] + prev[j - 1] + dv.q * row[j - 1];
            for (int ch = 0; ch < n_ch; ++ch) want[j * n_ch + ch] += row[j] * dv.x[i * n_ch + ch];
        }
        prev.swap(row);
    }
    double worst = 0.0;
    for (int ch = 0; ch < n_ch; ++ch) {
        double peak = 0.0, err = 0.0;
        for (int64_t j = 0; j < n_out; ++j) {
            REQUIRE(std::isfinite(dv.out[j * n_ch + ch]));
            peak = std::fmax(peak, std::fabs(want[j * n_ch + ch]));
            err = std::fmax(err, std::fabs(want[j * n_ch + ch] - dv.out[j * n_ch + ch]));
        }
        REQUIRE(peak > 0.0);
        worst = std::fmax(worst, err / peak);
    }
    if (lam == 0.0 && !laguerre)  // the identity, bit for bit
        for (int64_t j = 0; j < n_out && j < n_in; ++j)
            for (int ch = 0; ch < n_ch; ++ch) REQUIRE(dv.out[j * n_ch + ch] == dv.x[j * n_ch + ch]);
    std::printf("n_in %lld n_out %lld channels %d lambda %g %s: %lld launches, error %.2e\n", (long long)n_in, (long long)n_out,
                n_ch, lam, laguerre ? "laguerre" : "warp", (long long)pl.launches, worst);
    REQUIRE(worst <= 1e-13);
    return worst;
}

int main() {
    const int64_t shapes[][2] = {{1, 1}, {TI + 1, 5}, {5, TJ + 1}, {2 * TI + 1, 2 * TJ + 1}, {3 * TI, TJ - 1},
                                 {TI + 2, 1}, {1, TJ + 2}, {2, 2}, {TI + 2, TJ + 2}};
    for (const auto& sh : shapes) {
        check_shape(sh[0], sh[1], G + 1, -0.876, false);
        check_shape(sh[0], sh[1], 1, 0.99, true);
    }
    check_shape(2 * TI + 1, 2 * TJ + 1, 2, 0.0, false);
    std::printf("warp_plan_san: ok\n");
    return 0;
}
