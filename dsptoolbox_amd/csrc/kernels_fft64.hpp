// Complex128 transforms of any length along axis 0 of an (n, C) array, and the point-wise steps that turn them into the
// analytic signal, the cepstra, the minimum-phase equivalent and the group delay (reference: transforms.hilbert /
// cepstrum / from_complex_cepstrum, transforms/transforms.py:59-110, 763-809; helpers/minimum_phase.py:8-79;
// _group_delay_direct, standard/_standard_backend.py:37-63).  float64 throughout, gfx950.
//
// On the device a call's data is PLANAR: column c of the array is the contiguous run x[c * ld .. c * ld + n) of double2,
// ld >= n (ld = M, the padded power of two, when the length takes Bluestein's route).  k_load brings the host's
// sample-major array into that form (the channel stride is read, nothing is copied on the host), k_store takes
// it back; everything between stays in HBM.
//
//   n = 2^lg <= 8192     k_fft_lds: one workgroup per column, radix-2 in LDS on double2 (8192 x 16 B = 128 KB of 160 KB)
//   n = 2^lg  > 8192     four-step, n = n1 n2, lg n1 = floor(lg / 2): both <= 2048. k_transpose, k_fft_lds over the n2 columns of length n1 with
//                        the twiddle w_n^(j2 k1) on the way out, k_transpose, k_fft_lds over the n1 rows, k_transpose:
//                        natural order.  The twiddle's phase is (j2 k1) mod n in 64-bit integers, then sincospi.
//   any other n          Bluestein on the power-of-two transform of M >= 2 n - 1 points: k_blue (chirp in, spectrum
//                        product, chirp out); the chirp exp(-i pi k^2 / n) takes k^2 mod 2 n in 64-bit integers first
//                        (k_chirp) -- at n = 384000 k^2 reaches 1.5e11 and a phase formed in floating point is lost.
// No atomics, no scratch, every element has one writer: a call returns the same bits every time.
//
// LDS: a double2 is four banks wide, so the 64 lanes of a wave read 16 B each in four passes whatever the stride -- a
// radix-2 stage with stride 2^s >= 16 elements lands the passes on the same 16 banks (4-way on top of the width); at
// 8192 points the thirteen stages are 13 x 2 x 128 KB of LDS traffic per column against one 256 KB round trip to HBM, and
// one workgroup per CU (128 KB) leaves no second column to hide it.  The route is for a handful of columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft64_common.hpp"

namespace fft64 {

using f64c::cmul;

constexpr int NT = 256;
constexpr int LDS_MAX = 8192, LDS_MAX_LG = 13;  // the longest transform one workgroup holds; the table is tw[k] = exp(-2 pi i k / 8192)

struct LdsArgs {
    double2* x;            // column c, batch b at x[c * col_stride + b * n]; transformed in place
    int64_t col_stride;
    int n, lg;
    const double2* tw;     // [LDS_MAX / 2]
    int64_t twid_n;        // > 0: the result k of batch b is multiplied by exp(-+2 pi i (b k mod twid_n) / twid_n)
};

// grid = (batches, C); dynamic LDS = n * 16 bytes.  The whole column is in LDS before the first store, so in place is safe.
template <bool INV>
__global__ __launch_bounds__(NT) void k_fft_lds(LdsArgs p) {
    extern __shared__ __align__(16) double2 buf[];
    const int tid = threadIdx.x, n = p.n, lg = p.lg;
    double2* col = p.x + (int64_t)blockIdx.y * p.col_stride + (int64_t)blockIdx.x * n;
    for (int k = tid; k < n; k += NT) buf[lg ? __brev((unsigned)k) >> (32 - lg) : 0] = col[k];
    __syncthreads();
    f64c::radix2_lds<INV>(buf, n, lg, p.tw, LDS_MAX >> lg, tid);
    if (p.twid_n > 0) {
        const int64_t b = blockIdx.x;
        for (int k = tid; k < n; k += NT) {
            const int64_t r = (b * k) % p.twid_n;  // b, k < 8192: no overflow; the reduction is exact
            double s, c;
            sincospi(2.0 * (double)r / (double)p.twid_n, &s, &c);
            col[k] = cmul(buf[k], make_double2(c, INV ? s : -s));
        }
    } else {
        for (int k = tid; k < n; k += NT) col[k] = buf[k];
    }
}

struct TransposeArgs {
    const double2* in;  // column c: (rows, cols) row-major at in + c * col_stride
    double2* out;       // column c: (cols, rows)
    int rows, cols;     // multiples of 32
    int64_t col_stride;
};

// grid = (cols / 32, rows / 32, C): a 32 x 32 tile through LDS, reads and writes both along the fast axis
__global__ __launch_bounds__(NT) void k_transpose(TransposeArgs p) {
    __shared__ double2 tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const double2* in = p.in + (int64_t)blockIdx.z * p.col_stride;
    double2* out = p.out + (int64_t)blockIdx.z * p.col_stride;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[ty + 8 * j][tx] = in[(int64_t)(r0 + ty + 8 * j) * p.cols + c0 + tx];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(int64_t)(c0 + ty + 8 * j) * p.rows + r0 + tx] = tile[tx][ty + 8 * j];
}

// ---- Bluestein ---------------------------------------------------------------------------------------------------
// w[k] = exp(-i pi k^2 / n), k < n; b[k] = conj w[|k|] laid out circularly over M points (b[M - k] = b[k]), zero between.
struct ChirpArgs {
    double2 *w, *b;
    int64_t n, M;
};

// grid = ceil(M / 256)
__global__ __launch_bounds__(NT) void k_chirp(ChirpArgs p) {
    double2 *w = p.w, *b = p.b;
    const int64_t n = p.n, M = p.M;
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (k >= M) return;
    const int64_t j = k < n ? k : (M - k < n ? M - k : -1);  // M >= 2 n - 1: at most one of the two holds
    if (j < 0) {
        b[k] = make_double2(0.0, 0.0);
        return;
    }
    const int64_t r = (j * j) % (2 * n);  // j < 2^21: j^2 < 2^42
    double s, c;
    sincospi((double)r / (double)n, &s, &c);
    b[k] = make_double2(c, s);
    if (k < n) w[k] = make_double2(c, -s);
}

enum { BLUE_PRE = 0, BLUE_MUL = 1, BLUE_POST = 2 };
struct BlueArgs {
    double2* x;          // planar, column stride ld = M
    const double2* tab;  // w [n] (PRE, POST) or the chirp filter's spectrum [M] (MUL)
    int64_t n, ld;
    int n_ch, mode, inv;  // inv: the conjugate tables
    double scale;         // MUL: 1 / M of the inverse transform that follows
};

// grid = ceil(C rows / 256), rows = ld (PRE: zero past n; MUL) or n (POST)
__global__ __launch_bounds__(NT) void k_blue(BlueArgs p) {
    const int64_t rows = p.mode == BLUE_POST ? p.n : p.ld;
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= rows * p.n_ch) return;
    const int64_t c = idx / rows, k = idx - c * rows;
    double2* e = p.x + c * p.ld + k;
    if (p.mode == BLUE_PRE && k >= p.n) {
        *e = make_double2(0.0, 0.0);
        return;
    }
    double2 t = p.tab[k];
    if (p.inv) t.y = -t.y;
    const double2 v = cmul(*e, t);
    *e = p.mode == BLUE_MUL ? make_double2(v.x * p.scale, v.y * p.scale) : v;
}

// ---- in and out --------------------------------------------------------------------------------------------------
struct LoadArgs {
    const double* in;  // (n_in, C) float64, or complex128 as interleaved doubles
    int in_complex;
    int64_t n_in, n, ld;  // rows kept: min(n_in, n); zero up to ld
    int n_ch;
    double2* x;
};

// grid = ceil(ld C / 256); neighbouring lanes read neighbouring channels of one sample
__global__ __launch_bounds__(NT) void k_load(LoadArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.ld * p.n_ch) return;
    const int64_t k = idx / p.n_ch, c = idx - k * p.n_ch;
    double2 v = make_double2(0.0, 0.0);
    if (k < p.n && k < p.n_in) {
        if (p.in_complex)
            v = reinterpret_cast<const double2*>(p.in)[k * p.n_ch + c];
        else
            v.x = p.in[k * p.n_ch + c];
    }
    p.x[c * p.ld + k] = v;
}

enum { STORE_COMPLEX = 0, STORE_REAL = 1, STORE_ANGLE = 2 };
struct StoreArgs {
    const double2* x;
    int64_t ld, n_rows;
    int n_ch, mode;
    double scale;
    double* out;  // (n_rows, C) complex128 or float64
};

// grid = ceil(n_rows C / 256)
__global__ __launch_bounds__(NT) void k_store(StoreArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_rows * p.n_ch) return;
    const int64_t k = idx / p.n_ch, c = idx - k * p.n_ch;
    const double2 v = p.x[c * p.ld + k];
    if (p.mode == STORE_COMPLEX)
        reinterpret_cast<double2*>(p.out)[idx] = make_double2(v.x * p.scale, v.y * p.scale);
    else if (p.mode == STORE_REAL)
        p.out[idx] = v.x * p.scale;
    else
        p.out[idx] = atan2(v.y, v.x);
}

// ---- point-wise steps on the planar array, in place ----------------------------------------------------------------
// POINT_MASK   the analytic-signal mask: bin 0 (and n / 2 of an even n) kept, 1 .. ceil(n / 2) - 1 doubled, the rest 0
// POINT_FOLD   the same weights on the REAL part (the cepstral fold, helpers/minimum_phase.py:38-46), imaginary part 0
// POINT_LOGABS log |z| + 0 i;   POINT_LOG  the principal log |z| + i arg z of a real signal's spectrum;   POINT_EXP  exp z
// every mode scales z first (the 1 / n of the inverse transform before it)
enum { POINT_MASK = 0, POINT_FOLD = 1, POINT_LOGABS = 2, POINT_LOG = 3, POINT_EXP = 4 };
struct PointArgs {
    double2* x;
    int64_t n, ld;
    int n_ch, mode;
    double scale;
};

__device__ __forceinline__ double fold_weight(int64_t k, int64_t n) {
    if (k == 0 || (2 * k == n)) return 1.0;
    return k < (n + 1) / 2 ? 2.0 : 0.0;
}

// grid = ceil(n C / 256)
__global__ __launch_bounds__(NT) void k_point(PointArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n * p.n_ch) return;
    const int64_t c = idx / p.n, k = idx - c * p.n;
    double2* e = p.x + c * p.ld + k;
    double2 z = *e;
    z.x *= p.scale;
    z.y *= p.scale;
    switch (p.mode) {
    case POINT_MASK: {
        const double w = fold_weight(k, p.n);
        z = make_double2(z.x * w, z.y * w);
    } break;
    case POINT_FOLD:
        z = make_double2(z.x * fold_weight(k, p.n), 0.0);
        break;
    case POINT_LOGABS:
        z = make_double2(log(hypot(z.x, z.y)), 0.0);
        break;
    case POINT_LOG:
        // the spectrum of the REAL signal this mode is used on is real at bin 0 and at n / 2: its rounding-level
        // imaginary part there would pick +pi or -pi for a negative bin at random; +0 gives numpy's +pi
        if (k == 0 || 2 * k == p.n) z.y = 0.0;
        z = make_double2(log(hypot(z.x, z.y)), atan2(z.y, z.x));
        break;
    default: {
        double s, co;
        sincos(z.y, &s, &co);
        const double m = exp(z.x);
        z = make_double2(m * co, m * s);
    }
    }
    *e = z;
}

// -np.gradient(ph, delta_f, axis=0) / pi / 2 of a dense (n_bins, C) array, n_bins >= 2: centred differences, one-sided
// at the two ends, in numpy's own order of operations
struct GradArgs {
    const double* ph;
    int64_t n_bins;
    int n_ch;
    double delta_f;
    double* out;
};

// grid = ceil(n_bins C / 256)
__global__ __launch_bounds__(NT) void k_gradient(GradArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    const int64_t k = idx / p.n_ch, C = p.n_ch;
    double g;
    if (k == 0)
        g = (p.ph[idx + C] - p.ph[idx]) / p.delta_f;
    else if (k == p.n_bins - 1)
        g = (p.ph[idx] - p.ph[idx - C]) / p.delta_f;
    else
        g = (p.ph[idx + C] - p.ph[idx - C]) / (2.0 * p.delta_f);
    p.out[idx] = -g / 3.141592653589793 / 2.0;
}

}  // namespace fft64
