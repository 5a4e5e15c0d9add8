// Host tables of the block carry S_{b+1} = Phi S_b + s_b (block_carry.hpp): the zero-input state transition A of a
// recursion and its powers Phi = A^L and Phi^B, in float64 or complex float64.  Plain C++17, no HIP types, shared by
// api.hip and by tests/host_san/carry_tables_san.cpp.  Matrices are d x d, row-major.
#pragma once
#include <stddef.h>

#include <vector>

namespace carry {

constexpr int L = 32;  // samples per block (one lane's recursion)
constexpr int B = 64;  // blocks per group (one wave)

template <typename S>
inline void mat_mul(const std::vector<S>& a, const std::vector<S>& b, int d, std::vector<S>& out) {
    std::vector<S> r((size_t)d * d, S(0.0));
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < d; ++k) {
            const S v = a[(size_t)i * d + k];
            if (v == S(0.0)) continue;
            for (int j = 0; j < d; ++j) r[(size_t)i * d + j] += v * b[(size_t)k * d + j];
        }
    out.swap(r);
}

template <typename S>
inline void mat_pow2(std::vector<S>& m, int d, int log2_exp) {  // m <- m^(2^log2_exp)
    for (int i = 0; i < log2_exp; ++i) mat_mul(m, m, d, m);
}

// A of a cascade of n_sec transposed direct-form-II sections, cf [n_sec][5] = b0 b1 b2 a1 a2 (a0 = 1), D = 2 n_sec:
// column j is one zero-input step of the cascade from the unit state e_j
template <typename S>
inline void sos_transition(const S* cf, int n_sec, std::vector<S>& a) {
    const int d = 2 * n_sec;
    a.assign((size_t)d * d, S(0.0));
    for (int j = 0; j < d; ++j) {
        S in(0.0);
        for (int k = 0; k < n_sec; ++k) {
            const S z1 = (j == 2 * k) ? 1.0 : 0.0, z2 = (j == 2 * k + 1) ? 1.0 : 0.0;
            const S y = cf[5 * k] * in + z1;
            a[(size_t)(2 * k) * d + j] = cf[5 * k + 1] * in - cf[5 * k + 3] * y + z2;
            a[(size_t)(2 * k + 1) * d + j] = cf[5 * k + 2] * in - cf[5 * k + 4] * y;
            in = y;
        }
    }
}

// phi = A^L, phig = A^(L B); a is left holding phig
template <typename S>
inline void carry_powers(std::vector<S>& a, int d, std::vector<S>& phi, std::vector<S>& phig) {
    static_assert(L == 32 && B == 64, "the squarings below assume L = 2^5, B = 2^6");
    mat_pow2(a, d, 5);
    phi = a;
    mat_pow2(a, d, 6);
    phig = a;
}

}  // namespace carry
