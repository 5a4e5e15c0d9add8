// Linear prediction per (frame, channel) pair, float64, gfx950 (transforms.lpc of the reference,
// transforms/transforms.py:1199-1283 with helpers/ar_estimation.py and standard/_framed_signal_representation.py).
//   k_lpc_yw    one workgroup per pair: the windowed frame goes to LDS once (framed and windowed on the fly, zeros past
//               the signal's end and behind the frame), every wave takes groups of KB consecutive lags and its lanes
//               stride the samples, so a lane reads x[n] once for KB products; the lane sums are added by a fixed
//               butterfly.  Wave 0 then runs the Levinson-Durbin recursion on r[0 .. order] in the statement order of
//               _levison_durbin_recursion (reflection value, k = -value / E, E *= 1 - k^2, the check E <= 0, the
//               symmetric update of a), a lane per coefficient, with a[] in LDS.
//   k_levinson  the same recursion on a host-given (order + 1, columns) autocorrelation, one wave per column.
//   k_lpc_burg  one workgroup per pair: forward and backward errors in LDS (EF[j + i], EB[j] hold pass i's element j,
//               so a pass updates in place and the shift of the reference's slices costs nothing), per pass one
//               workgroup reduction of sum(b f), the reflection coefficient by every lane, the coefficient update on
//               two alternating LDS rows as the reference swaps its two arrays, and den = q den - b'[-1]^2 - f'[0]^2.
//   k_lpc_filter  lfilter([1], a, source) from zero state, one wave per pair, in scipy's transposed direct form II:
//               lane l keeps the states z[4 l .. 4 l + 3] and their coefficients in registers, y = z[0] + x is broadcast
//               from lane 0 and z[k] = z[k + 1] - a[k + 1] y needs one lane shift per sample.
//   k_lpc_ola   _reconstruct_framed_signal: per output sample the covering frames times the window, added in frame
//               order, over the envelope sum w^2 clipped below at 1e-4; samples no frame covers are 0.
// Divisions are IEEE divisions and nothing is atomic: a silent frame gives the reference's NaN (Yule-Walker) or zeros
// (Burg), and results are the same bits from run to run.  The singular flag is a plain store of 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dslpc {

constexpr int NT = 256;          // lanes of k_lpc_yw and k_lpc_burg
constexpr int WAVES = NT / 64;
constexpr int KB = 4;            // k_lpc_yw: lags per wave and sweep over the frame
constexpr int MAX_LAGS = 256;    // order + 1 <= MAX_LAGS: a lane of the workgroup per coefficient (size_guards.hpp)
constexpr int YW_PAD = MAX_LAGS + KB;  // zeros behind the frame: x[n + k] needs no bound check
constexpr int FILT_WAVES = 4;    // k_lpc_filter: pairs per workgroup
constexpr int TAPS = 4;          // k_lpc_filter: states per lane (64 * TAPS >= the largest order)

__host__ __device__ inline size_t yw_lds_bytes(int L) { return ((size_t)L + YW_PAD + 2 * MAX_LAGS) * 8; }
__host__ __device__ inline size_t burg_lds_bytes(int L) { return (2 * (size_t)L + 2 * MAX_LAGS + 2 * WAVES) * 8; }

struct LpcArgs {
    const void* x;       // element (n, c) at x[n ss + c cs], double or float
    int64_t ss, cs;
    int64_t n_samples;
    int n_ch;
    int64_t n_frames;
    const double* window;  // [L]
    int L;
    int64_t hop;
    int order;
    double* a;           // (order + 1, n_frames, n_ch)
    double* var;         // (n_frames, n_ch)
    int* singular;
};

struct LevinsonArgs {
    const double* r;     // (order + 1, n_cols)
    int order;
    int64_t n_cols;
    double* a;           // (order + 1, n_cols)
    double* var;         // (n_cols)
    int* singular;
};

// the sum over the 64 lanes of a wave, the same bits in every lane (a + b = b + a at every level)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// value of lane 0 in every lane, through scalar registers
__device__ __forceinline__ double from_lane0(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// LDS traffic between the lanes of ONE wave: the wave's LDS operations complete in order; the fence keeps the
// compiler from moving accesses across it
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// _levison_durbin_recursion (helpers/ar_estimation.py:28-60) by one whole wave.  r[0 .. order] and a[0 .. order) are
// LDS rows; a[] receives the reference's ar_parameters (a[m] = coefficient m + 1).  Returns the prediction error in
// every lane; *bad is set when it was <= 0 after any order (NaN is not).
__device__ __forceinline__ double levinson_wave(const double* r, double* a, int order, int lane, bool* bad) {
    double E = r[0];
    const double* c = r + 1;  // autocorr_coefficients
    *bad = false;
    for (int m = 0; m < order; ++m) {
        double part = 0.0;
        for (int lag = lane; lag < m; lag += 64) part = fma(a[lag], c[m - lag - 1], part);
        const double value = c[m] + wave_sum(part);
        const double k = -value / E;
        E *= 1.0 - k * k;
        if (E <= 0.0) *bad = true;
        // a[lag] <- a[lag] + k a[m - 1 - lag] for every lag < m at once: what the reference's pairwise in-place
        // update computes; then a[m] = k
        double upd[MAX_LAGS / 64];
#pragma unroll
        for (int q = 0; q < MAX_LAGS / 64; ++q) {
            const int lag = lane + 64 * q;
            upd[q] = lag < m ? a[lag] + k * a[m - 1 - lag] : 0.0;
        }
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < MAX_LAGS / 64; ++q) {
            const int lag = lane + 64 * q;
            if (lag < m) a[lag] = upd[q];
        }
        if (lane == 0) a[m] = k;
        wave_lds_sync();
    }
    return E;
}

// grid = pairs (channel fastest: the workgroups in flight together share the cache lines of interleaved samples)
template <typename T>
__global__ __launch_bounds__(NT) void k_lpc_yw(LpcArgs p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* x = lds;                      // [L + YW_PAD]
    double* r = x + p.L + YW_PAD;         // [MAX_LAGS]
    double* a = r + MAX_LAGS;             // [MAX_LAGS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pair = blockIdx.x;
    const int c = (int)(pair % p.n_ch);
    const int64_t f = pair / p.n_ch;
    const T* col = (const T*)p.x + c * p.cs;
    const int64_t s0 = f * p.hop;
    for (int n = tid; n < p.L + YW_PAD; n += NT) {
        double v = 0.0;
        if (n < p.L && s0 + n < p.n_samples) v = (double)col[(s0 + n) * p.ss] * p.window[n];
        x[n] = v;
    }
    a[tid] = 0.0;
    __syncthreads();
    const int n_lags = p.order + 1;
    const double len = (double)p.L;
    for (int k0 = wave * KB; k0 < n_lags; k0 += WAVES * KB) {
        double acc[KB];
#pragma unroll
        for (int q = 0; q < KB; ++q) acc[q] = 0.0;
        for (int n = lane; n < p.L; n += 64) {
            const double v = x[n];
#pragma unroll
            for (int q = 0; q < KB; ++q) acc[q] = fma(v, x[n + k0 + q], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            const double s = wave_sum(acc[q]);
            if (lane == 0 && k0 + q < n_lags) r[k0 + q] = s / len;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    bool bad;
    const double E = levinson_wave(r, a, p.order, lane, &bad);
    const int64_t plane = p.n_frames * p.n_ch;
    for (int j = lane; j <= p.order; j += 64) p.a[(int64_t)j * plane + pair] = j == 0 ? 1.0 : a[j - 1];
    if (lane == 0) {
        p.var[pair] = E;
        if (bad) *p.singular = 1;
    }
}

// grid = columns, 64 lanes
__global__ __launch_bounds__(64) void k_levinson(LevinsonArgs p) {
    __shared__ double r[MAX_LAGS], a[MAX_LAGS];
    const int lane = threadIdx.x;
    const int64_t col = blockIdx.x;
    for (int j = lane; j < MAX_LAGS; j += 64) {
        r[j] = j <= p.order ? p.r[(int64_t)j * p.n_cols + col] : 0.0;
        a[j] = 0.0;
    }
    wave_lds_sync();
    bool bad;
    const double E = levinson_wave(r, a, p.order, lane, &bad);
    for (int j = lane; j <= p.order; j += 64) p.a[(int64_t)j * p.n_cols + col] = j == 0 ? 1.0 : a[j - 1];
    if (lane == 0) {
        p.var[col] = E;
        if (bad) *p.singular = 1;
    }
}

// the sum over the workgroup of one value per lane, in a fixed order, the same bits in every lane; red: [WAVES]
__device__ __forceinline__ double group_sum(double v, double* red, int lane, int wave) {
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    return s;
}

// _burg_ar_estimation (helpers/ar_estimation.py:162-205).  grid = pairs, channel fastest.
template <typename T>
__global__ __launch_bounds__(NT) void k_lpc_burg(LpcArgs p) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* EF = lds;                   // [L]: pass i's forward error j at EF[j + i]
    double* EB = EF + p.L;              // [L]: its backward error j at EB[j]
    double* a0 = EB + p.L;              // [MAX_LAGS] ar_coeffs / ar_coeffs_prev, swapped every pass
    double* a1 = a0 + MAX_LAGS;
    double* red = a1 + MAX_LAGS;        // [2][WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pair = blockIdx.x;
    const int c = (int)(pair % p.n_ch);
    const int64_t f = pair / p.n_ch;
    const T* col = (const T*)p.x + c * p.cs;
    const int64_t s0 = f * p.hop;
    // EB[j] = x[j], EF[j] = x[j + 1]: the frame is read once, both rows are written from it
    const int M = p.L - 1;
    for (int n = tid; n < p.L; n += NT) {
        double v = 0.0;
        if (s0 + n < p.n_samples) v = (double)col[(s0 + n) * p.ss] * p.window[n];
        EB[n] = v;
        if (n > 0) EF[n - 1] = v;
    }
    a0[tid] = tid == 0 ? 1.0 : 0.0;
    a1[tid] = tid == 0 ? 1.0 : 0.0;
    __syncthreads();
    double part = 0.0;
    for (int j = tid; j < M; j += NT) part += EF[j] * EF[j] + EB[j] * EB[j];
    double den = group_sum(part, red + WAVES, lane, wave);  // (the odd half: pass 0 writes the even one)
    const double epsilon = 2.220446049250313e-16;  // np.finfo(np.float64).eps
    double* cur = a0;   // the reference's ar_coeffs
    double* prev = a1;  // ar_coeffs_prev
    for (int i = 0; i < p.order; ++i) {
        const int len = M - i;
        part = 0.0;
        for (int j = tid; j < len; j += NT) part = fma(EB[j], EF[j + i], part);
        // the halves of red alternate: a wave may write this pass's sum while another still reads the last one's
        const double num = group_sum(part, red + (i & 1) * WAVES, lane, wave);
        const double rc = (-2.0 * num) / (den + epsilon);
        double* t = cur;
        cur = prev;
        prev = t;
        if (tid >= 1 && tid <= i + 1) cur[tid] = prev[tid] + rc * prev[i - tid + 1];
        for (int j = tid; j < len; j += NT) {
            const double fe = EF[j + i], be = EB[j];
            EF[j + i] = fe + rc * be;
            EB[j] = be + rc * fe;
        }
        __syncthreads();
        const double bl = EB[len - 1], f0 = EF[i];
        den = (1.0 - rc * rc) * den - bl * bl - f0 * f0;
    }
    const int64_t plane = p.n_frames * p.n_ch;
    if (tid <= p.order) p.a[(int64_t)tid * plane + pair] = cur[tid];
    if (tid == 0) p.var[pair] = den;
}

struct FilterArgs {
    const double* a;     // (order + 1, n_frames, n_ch)
    const double* src;   // (L, n_frames, n_ch)
    int L;
    int64_t n_pairs;     // n_frames n_ch
    int order;
    double* y;           // (L, n_frames, n_ch)
};

// grid = ceil(pairs / FILT_WAVES), 64 FILT_WAVES lanes
__global__ __launch_bounds__(64 * FILT_WAVES) void k_lpc_filter(FilterArgs p) {
    __shared__ double xs[FILT_WAVES][64], ys[FILT_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * FILT_WAVES + wave;
    if (pair >= p.n_pairs) return;  // (no workgroup barrier below)
    const double a0 = p.a[pair];
    double ak[TAPS], z[TAPS];
    bool live[TAPS];
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        const int k = TAPS * lane + q;  // state z[k] is fed by coefficient a[k + 1]
        live[q] = k < p.order;
        ak[q] = live[q] ? p.a[(int64_t)(k + 1) * p.n_pairs + pair] / a0 : 0.0;
        z[q] = 0.0;
    }
    for (int n0 = 0; n0 < p.L; n0 += 64) {
        const int cnt = p.L - n0 < 64 ? p.L - n0 : 64;
        if (lane < cnt) xs[wave][lane] = p.src[(int64_t)(n0 + lane) * p.n_pairs + pair] / a0;
        wave_lds_sync();
        for (int j = 0; j < cnt; ++j) {
            const double y = from_lane0(z[0] + xs[wave][j]);
            const double up = __shfl_down(z[0], 1, 64);  // z[4 (l + 1)]; the last lane's is dropped below
#pragma unroll
            for (int q = 0; q < TAPS; ++q) {
                const double next = q + 1 < TAPS ? z[q + 1] : (lane < 63 ? up : 0.0);
                z[q] = live[q] ? next - ak[q] * y : 0.0;
            }
            if (lane == 0) ys[wave][j] = y;
        }
        wave_lds_sync();
        if (lane < cnt) p.y[(int64_t)(n0 + lane) * p.n_pairs + pair] = ys[wave][lane];
        wave_lds_sync();
    }
}

struct OlaArgs {
    const double* yf;    // (L, n_frames, n_ch) filtered frames
    const double* window;
    int L;
    int64_t n_frames;
    int n_ch;
    int64_t hop;
    int64_t n_out;
    double* y;           // (n_out, n_ch)
};

// one lane per output value, channel fastest
__global__ __launch_bounds__(NT) void k_lpc_ola(OlaArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_out * p.n_ch) return;
    const int c = (int)(idx % p.n_ch);
    const int64_t n = idx / p.n_ch;
    const int64_t f_lo = n >= p.L ? (n - p.L) / p.hop + 1 : 0;
    int64_t f_hi = n / p.hop;
    if (f_hi > p.n_frames - 1) f_hi = p.n_frames - 1;
    double sum = 0.0, env = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {  // (empty where hop > L leaves the sample between two frames)
        const int64_t m = n - f * p.hop;
        const double w = p.window[m];
        sum += p.yf[(m * p.n_frames + f) * p.n_ch + c] * w;
        env += w * w;
    }
    p.y[idx] = sum / (env < 1e-4 ? 1e-4 : env);
}

}  // namespace dslpc
