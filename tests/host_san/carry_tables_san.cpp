// The host tables of the block carry (csrc/carry_tables.hpp) -- the transition A of a cascade and its powers
// Phi = A^32 and Phi^64 = A^2048 by repeated squaring -- built with -fsanitize=address,undefined and run on the CPU
// (tests/test_iir_host.py).  For real cascades of 1, 3 and 32 sections, complex cascades of 1 and 16 sections and a
// plain matrix of the odd size D = 63, with poles of radius 0.9 to 0.999 (one of them at 0.999) drawn from a fixed seed:
//   - A from sos_transition agrees with one zero-input step of the cascade from every unit state, taken in long double;
//   - Phi and Phi^64 from carry_powers agree with the same powers of the same A formed in long double by 31, then 2047,
//     plain multiplications by A, within BOUND of the reference's largest magnitude;
//   - a wrong table misses that bound: Phi squared one time too few, and the powers of the transposed A;
//   - every index stays inside its array (the sanitizer).
// The error is max |table - reference| / max |reference| over the matrix.  Measured (x86-64, 80-bit long double):
//
//   case               D  trials   Phi          Phi^64
//   real, 1 section    2    16     1.34e-13     2.01e-11
//   real, 3 sections   6    16     1.57e-14     6.38e-13
//   real, 32 sections 64     1     1.99e-15     4.23e-12
//   complex, 1         2    16     6.88e-14     9.26e-12
//   complex, 16       32     1     7.55e-14     4.80e-13
//   plain matrix      63     1     1.07e-15     4.93e-14
//
// The largest values come from the two-state cascades, drawn sixteen times each.  BOUND is four times the largest value
// seen (the margin of the project's other oracle bounds).  The wrong tables are off by 0.09 and more.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dsptoolbox_amd/csrc/carry_tables.hpp"

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

static const double BOUND = 4 * 2.01e-11;
static const double R_MIN = 0.9, R_MAX = 0.999;

typedef std::complex<double> cplx;
template <typename S> struct Wide { typedef long double type; };
template <> struct Wide<cplx> { typedef std::complex<long double> type; };

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // splitmix64: the same numbers with every standard library
static double uniform() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (double)((z ^ (z >> 31)) >> 11) * 0x1.0p-53;
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * uniform(); }
static cplx pole(double r) { return std::polar(r, uniform(0.0, 2 * M_PI)); }
static double radius(int k) { return k == 0 ? R_MAX : uniform(R_MIN, R_MAX); }

// cf [n_sec][5] = b0 b1 b2 a1 a2 of a stable cascade
static void draw_sections(int n_sec, std::vector<double>& cf) {
    cf.resize((size_t)5 * n_sec);
    for (int k = 0; k < n_sec; ++k) {
        const double r = radius(k), th = uniform(0.0, M_PI);
        for (int i = 0; i < 3; ++i) cf[5 * k + i] = uniform(-1.0, 1.0);
        cf[5 * k + 3] = -2 * r * std::cos(th);
        cf[5 * k + 4] = r * r;
    }
}
static void draw_sections(int n_sec, std::vector<cplx>& cf) {
    cf.resize((size_t)5 * n_sec);
    for (int k = 0; k < n_sec; ++k) {
        const cplx p1 = pole(radius(k)), p2 = pole(uniform(R_MIN, R_MAX));
        for (int i = 0; i < 3; ++i) cf[5 * k + i] = cplx(uniform(-1.0, 1.0), uniform(-1.0, 1.0));
        cf[5 * k + 3] = -(p1 + p2);
        cf[5 * k + 4] = p1 * p2;
    }
}

// an odd-sized matrix that is no cascade's: 2 x 2 rotation blocks and one real pole on the diagonal, coupled above it
static void draw_matrix(int d, std::vector<double>& a) {
    a.assign((size_t)d * d, 0.0);
    for (int i = 0; i + 1 < d; i += 2) {
        const cplx p = pole(radius(i));
        a[(size_t)i * d + i] = a[(size_t)(i + 1) * d + i + 1] = p.real();
        a[(size_t)i * d + i + 1] = -p.imag();
        a[(size_t)(i + 1) * d + i] = p.imag();
    }
    a[(size_t)d * d - 1] = uniform(R_MIN, R_MAX);
    for (int i = 0; i < d; ++i)
        for (int j = (i | 1) + 1; j < d; ++j) a[(size_t)i * d + j] = uniform(-0.05, 0.05);
}

// one zero-input step of the cascade (transposed direct form II, as the kernels run it) from the unit state e_j
template <typename S>
static void check_transition(const std::vector<S>& cf, int n_sec, const std::vector<S>& a) {
    typedef typename Wide<S>::type W;
    const int d = 2 * n_sec;
    REQUIRE(a.size() == (size_t)d * d);
    for (int j = 0; j < d; ++j) {
        std::vector<W> z((size_t)d, W(0.0L));
        z[j] = W(1.0L);
        W x(0.0L);
        for (int k = 0; k < n_sec; ++k) {
            const W y = W(cf[5 * k]) * x + z[2 * k];
            z[2 * k] = W(cf[5 * k + 1]) * x - W(cf[5 * k + 3]) * y + z[2 * k + 1];
            z[2 * k + 1] = W(cf[5 * k + 2]) * x - W(cf[5 * k + 4]) * y;
            x = y;
        }
        for (int i = 0; i < d; ++i) REQUIRE(std::abs(W(a[(size_t)i * d + j]) - z[i]) <= 1e-14L * (1.0L + std::abs(z[i])));
    }
}

// p <- p a, every product formed and summed in long double
template <typename W>
static void times(std::vector<W>& p, const std::vector<W>& a, int d) {
    std::vector<W> r((size_t)d * d, W(0.0L));
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < d; ++k) {
            const W v = p[(size_t)i * d + k];
            const W* ak = &a[(size_t)k * d];
            W* ri = &r[(size_t)i * d];
            for (int j = 0; j < d; ++j) ri[j] += v * ak[j];
        }
    p.swap(r);
}

template <typename S, typename W>
static double error_of(const std::vector<S>& m, const std::vector<W>& ref) {
    REQUIRE(m.size() == ref.size());
    long double err = 0.0L, top = 0.0L;
    for (size_t i = 0; i < m.size(); ++i) {
        err = std::fmax(err, std::abs(W(m[i]) - ref[i]));
        top = std::fmax(top, std::abs(ref[i]));
    }
    REQUIRE(top > 0.0L && std::isfinite(top));
    return (double)(err / top);
}

struct Worst {
    double phi = 0.0, phig = 0.0;
};

// the tables of one A against the long-double products, and the two wrong tables against the bound
template <typename S>
static void check_powers(const std::vector<S>& a, int d, Worst& w) {
    typedef typename Wide<S>::type W;
    std::vector<W> aw(a.begin(), a.end()), ref_phi, ref = aw;
    for (int i = 1; i <= 2047; ++i) {
        times(ref, aw, d);
        if (i == 31) ref_phi = ref;
    }
    std::vector<S> m = a, phi, phig;
    carry::carry_powers(m, d, phi, phig);
    const double e_phi = error_of(phi, ref_phi), e_phig = error_of(phig, ref);
    w.phi = std::fmax(w.phi, e_phi);
    w.phig = std::fmax(w.phig, e_phig);
    REQUIRE(e_phi <= BOUND && e_phig <= BOUND);

    m = a;
    carry::mat_pow2(m, d, 4);  // squared one time too few
    const double e_short = error_of(m, ref_phi);
    REQUIRE(e_short > BOUND);
    std::vector<S> t((size_t)d * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) t[(size_t)i * d + j] = a[(size_t)j * d + i];
    carry::carry_powers(t, d, phi, phig);
    const double e_tr = error_of(phi, ref_phi), e_trg = error_of(phig, ref);
    REQUIRE(e_tr > BOUND && e_trg > BOUND);
    std::printf("    phi %.2e  phi^64 %.2e   wrong tables: one squaring short %.2e, transposed %.2e / %.2e\n", e_phi,
                e_phig, e_short, e_tr, e_trg);
}

template <typename S>
static void cascade_case(const char* what, int n_sec, int trials) {
    Worst w;
    std::printf("%s, %d sections (D = %d), %d trials\n", what, n_sec, 2 * n_sec, trials);
    for (int t = 0; t < trials; ++t) {
        std::vector<S> cf, a;
        draw_sections(n_sec, cf);
        carry::sos_transition(cf.data(), n_sec, a);
        check_transition(cf, n_sec, a);
        check_powers(a, 2 * n_sec, w);
    }
    std::printf("  worst: phi %.2e  phi^64 %.2e  (bound %.2e)\n", w.phi, w.phig, BOUND);
}

int main() {
    cascade_case<double>("real", 1, 16);
    cascade_case<double>("real", 3, 16);
    cascade_case<double>("real", 32, 1);
    cascade_case<cplx>("complex", 1, 16);
    cascade_case<cplx>("complex", 16, 1);
    Worst w;
    std::printf("plain matrix, D = 63, 1 trial\n");
    std::vector<double> a;
    draw_matrix(63, a);
    check_powers(a, 63, w);
    std::printf("  worst: phi %.2e  phi^64 %.2e  (bound %.2e)\n", w.phi, w.phig, BOUND);
    std::printf("carry_tables_san: ok\n");
    return 0;
}
