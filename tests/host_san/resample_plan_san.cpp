// The tile plan of the polyphase resampler (csrc/resample_plan.hpp) and the index arithmetic of k_resample_poly
// (csrc/kernels_resample.hpp) emulated in plain C++, built with -fsanitize=address,undefined and run on the CPU
// (tests/test_resample_host.py).  The cases come from the file named on the command line, one "up down channels n" per
// line.  Workgroup by workgroup, chunk by chunk, the emulation does what the kernel does: it stages the phase-major tap
// table and the chunk's input window into an LDS image of exactly the size the plan declares, then runs every lane's
// items.  Checked:
//   - every window sample an item reads lies inside the staged span and was staged in this chunk;
//   - every tap an item reads lies inside its phase's row of the padded table;
//   - every global read of the input lies inside [0, n) of a channel below n_ch;
//   - every output (m, channel) is written exactly once, and none outside (n_out, n_ch);
//   - the sums equal the definition y[m] = sum_n x[n] h[m D + half - n U] within 2 (J + 2) 2^-53 of the absolute sum;
//   - every index stays inside its array (the sanitizer).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dsptoolbox_amd/csrc/resample_plan.hpp"

using namespace resample;

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

static double tap_value(int k, int ntaps) { return std::cos(0.37 * k) / (1.0 + std::fabs(k - 0.5 * (ntaps - 1)) / 64.0); }
static double sample_value(int64_t n, int c) { return std::sin(0.11 * (double)n + 0.7 * c) + 0.1; }

// interleaved: the host entry's layout (sample stride n_ch); otherwise planar, the resident entry's
static void run_case(int U, int D, int n_ch, int64_t n, bool interleaved) {
    const Plan pl = make_plan(U, D, n_ch);
    REQUIRE(pl.tile >= 1 && (pl.tile & (pl.tile - 1)) == 0 && pl.tile * pl.cg <= PASSES * NT);
    REQUIRE(pl.jc >= 1 && pl.chunks * pl.jc >= pl.J && (pl.chunks - 1) * pl.jc < pl.J);
    REQUIRE(pl.J <= pl.JS && lds_doubles(pl) <= LDS_DOUBLES);
    const int64_t n_out = out_len(n, U, D);
    const int64_t xss = interleaved ? n_ch : 1, xcs = interleaved ? 1 : n;
    std::vector<double> h((size_t)pl.ntaps), x((size_t)n * n_ch), hp((size_t)table_doubles(pl));
    for (int k = 0; k < pl.ntaps; ++k) h[k] = tap_value(k, pl.ntaps);
    for (int64_t i = 0; i < n; ++i)
        for (int c = 0; c < n_ch; ++c) x[(size_t)(i * xss + c * xcs)] = sample_value(i, c);
    phase_major(pl, h.data(), hp.data());
    std::vector<double> y((size_t)n_out * n_ch, 0.0);
    std::vector<int> writes((size_t)n_out * n_ch, 0);
    const int cg = pl.cg, sh = ch_shift(cg), n_items = pl.tile << sh, n_staged = pl.span * cg;
    const int64_t tiles = (n_out + pl.tile - 1) / pl.tile;
    const int groups = (n_ch + cg - 1) / cg;
    for (int64_t bx = 0; bx < tiles; ++bx)
        for (int by = 0; by < groups; ++by) {
            std::vector<double> lds((size_t)lds_doubles(pl));  // exactly what the launch declares
            std::vector<int> staged_in((size_t)n_staged);      // the chunk that staged a window element last
            double* hs = lds.data();
            double* xs = lds.data() + table_doubles(pl);
            const int c0 = by * cg;
            const int64_t m0 = bx * pl.tile;
            const Origin o = origin(pl, m0);
            for (int k = 0; k < table_doubles(pl); ++k) hs[k] = hp[(size_t)k];
            std::vector<double> acc((size_t)PASSES * NT, 0.0);
            for (int k = 0; k < pl.chunks; ++k) {
                const int j0 = chunk_first_term(pl, k);
                const int64_t q0 = window_first(pl, o, k);
                for (int e = 0; e < n_staged; ++e) {  // (the lanes' strided loop visits every e once)
                    int s, c;
                    if (!interleaved) {
                        c = e / pl.span;
                        s = e - c * pl.span;
                    } else {
                        s = e >> sh;
                        c = e & (cg - 1);
                    }
                    REQUIRE(s >= 0 && s < pl.span && c >= 0 && c < cg);
                    const int64_t i = q0 + s;
                    double v = 0.0;
                    if (i >= 0 && i < n && c0 + c < n_ch) {
                        const int64_t at = i * xss + (int64_t)(c0 + c) * xcs;
                        REQUIRE(at >= 0 && at < (int64_t)x.size());
                        v = x[(size_t)at];
                    }
                    REQUIRE(s * cg + c < n_staged);
                    xs[s * cg + c] = v;
                    staged_in[(size_t)(s * cg + c)] = k + 1;
                }
                for (int t = 0; t < NT; ++t)
                    for (int it = 0; it < PASSES; ++it) {
                        const int e = t + it * NT;
                        if (e >= n_items) continue;
                        const int cl = !interleaved ? e / pl.tile : e & (cg - 1);
                        const int ml = !interleaved ? e - cl * pl.tile : e >> sh;
                        REQUIRE(cl >= 0 && cl < cg && ml >= 0 && ml < pl.tile);
                        const Item i = item(pl, o, ml);
                        REQUIRE(i.ph >= 0 && i.ph < U && i.da >= 0 && i.da <= pl.adv);
                        REQUIRE(o.a0 + i.da == ((m0 + ml) * D + pl.half) / U && i.ph == (int)(((m0 + ml) * D + pl.half) % U));
                        const int last = terms(pl, i.ph), end = last < j0 + pl.jc ? last : j0 + pl.jc;
                        REQUIRE(last >= 1 && last <= pl.J);
                        double a = acc[(size_t)e];
                        for (int j = j0; j < end; ++j) {
                            const int tap = i.ph * pl.JS + j, s = window_index(pl, k, i.da, j);
                            REQUIRE(j < pl.JS && tap >= 0 && tap < table_doubles(pl));
                            REQUIRE(s >= 0 && s < pl.span && staged_in[(size_t)(s * cg + cl)] == k + 1);
                            REQUIRE(q0 + s == o.a0 + i.da - j);  // the sample the formula names
                            a = std::fma(hs[tap], xs[s * cg + cl], a);
                        }
                        acc[(size_t)e] = a;
                    }
            }
            for (int e = 0; e < n_items; ++e) {
                const int cl = !interleaved ? e / pl.tile : e & (cg - 1);
                const int ml = !interleaved ? e - cl * pl.tile : e >> sh;
                const int64_t m = m0 + ml;
                if (m < n_out && c0 + cl < n_ch) {
                    const int64_t at = m * n_ch + c0 + cl;
                    REQUIRE(at >= 0 && at < (int64_t)y.size());
                    y[(size_t)at] = acc[(size_t)e];
                    writes[(size_t)at] += 1;
                }
            }
        }
    double worst = 0.0;
    for (int64_t m = 0; m < n_out; ++m)
        for (int c = 0; c < n_ch; ++c) {
            REQUIRE(writes[(size_t)(m * n_ch + c)] == 1);
            long double want = 0.0L, mag = 0.0L;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t k = m * D + pl.half - i * U;
                if (k < 0 || k >= pl.ntaps) continue;
                const long double term = (long double)h[(size_t)k] * (long double)x[(size_t)(i * xss + c * xcs)];
                want += term;
                mag += fabsl(term);
            }
            const double err = (double)fabsl((long double)y[(size_t)(m * n_ch + c)] - want);
            REQUIRE(err <= 2.0 * (pl.J + 2) * 0x1p-53 * (double)mag);
            if (mag > 0 && err / (double)mag > worst) worst = err / (double)mag;
        }
    std::printf("up %d down %d ch %d n %lld %s: tile %d chunks %d span %d lds %d bytes, n_out %lld, worst %.2e\n", U, D, n_ch,
                (long long)n, interleaved ? "interleaved" : "planar", pl.tile, pl.chunks, pl.span, lds_doubles(pl) * 8,
                (long long)n_out, worst);
}

int main(int argc, char** argv) {
    REQUIRE(argc == 2);
    std::FILE* f = std::fopen(argv[1], "r");
    REQUIRE(f != nullptr);
    int U, D, n_ch, cases = 0;
    long long n;
    while (std::fscanf(f, "%d %d %d %lld", &U, &D, &n_ch, &n) == 4) {
        REQUIRE(U >= 1 && D >= 1 && U <= MAX_RATE && D <= MAX_RATE && n_ch >= 1 && n >= 1);
        run_case(U, D, n_ch, n, true);
        run_case(U, D, n_ch, n, false);
        cases += 1;
    }
    std::fclose(f);
    REQUIRE(cases > 0);
    std::printf("resample_plan_san: ok (%d cases, both layouts)\n", cases);
    return 0;
}
