// Fractional-octave smoothing (helpers/smoothing.py:_fractional_octave_smoothing of the reference), float64.
//
// Arrays are the reference's (bins, channels), channel fastest.  A complex spectrum is
// smoothed as one (bins, 2 C) array: columns [0, C) hold |z|, columns [C, 2 C) the unwrapped phase, so both take one
// pass through the three real kernels.
//   k_to_log      linear bins 1 .. N -> the logarithmic axis k_log (uploaded by the host, numpy's values): one output
//                 point per lane; scipy's PchipInterpolator on unit-spaced knots (interior derivative: harmonic mean of
//                 the neighbouring slopes, 0 when they differ in sign or one is 0; three-point end rule; N = 2: the
//                 straight line) and its power-sum evaluation of the Hermite cubic
//   k_smooth      out[i] = sum_m wr[m] v[clamp(i - pf + m, 0, N - 1)], wr the unit-sum window reversed by the host,
//                 pf = L / 2: the reference's edge padding (L / 2 in front, L / 2 - (1 - L % 2) behind) and valid-mode
//                 convolution without a padded copy.  A workgroup owns TB bins x tc channels, stages TB + chunk - 1
//                 clamped rows in LDS per window chunk and keeps R consecutive bins per lane in registers (a sliding
//                 window: one LDS read per R multiply-adds); wr is read through the scalar cache.
//   k_to_lin      scipy's interp1d(kind="linear") from k_log back to bins 1 .. N, the bracket found from
//                 floor((N - 1) log l / log N) by comparison against k_log; clip for the first clip_ch columns
//   k_polar       z -> |z| (hypot) and atan2 in the (bins, 2 C) layout
//   k_unwrap      numpy.unwrap along bins (period 2 pi, a step of exactly -pi from a rising difference kept at +pi):
//                 one workgroup per channel scans the 2 pi corrections tile by tile
//   k_recombine   mag (cos ph, sin ph)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dssmooth {

constexpr int NT = 256;          // lanes of every kernel here
constexpr int R = 8;             // consecutive output bins per lane of k_smooth
constexpr int MAX_TC = 16;       // channels per k_smooth workgroup (a power of two)
constexpr int LDS_DOUBLES = 4096;  // one staged image: (TB + chunk - 1) rows x tc channels, 32 KB

// k_smooth's tile for a channel-group width tc: TB = (NT / tc) R output bins, window chunks of TB + 1 taps
inline int smooth_tile_bins(int tc) { return NT / tc * R; }
inline int smooth_chunk(int tc) { return LDS_DOUBLES / tc - smooth_tile_bins(tc) + 1; }

__device__ __forceinline__ double sgn(double x) { return (double)((x > 0.0) - (x < 0.0)); }

// scipy.interpolate.PchipInterpolator._edge_case with h0 = h1 = 1
__device__ __forceinline__ double pchip_edge(double m0, double m1) {
    double d = (3.0 * m0 - m1) / 2.0;
    if (sgn(d) != sgn(m0))
        d = 0.0;
    else if (sgn(m0) != sgn(m1) && fabs(d) > 3.0 * fabs(m0))
        d = 3.0 * m0;
    return d;
}
// the interior derivative between slopes ma (left) and mb (right), unit spacing: w1 = w2 = 3
__device__ __forceinline__ double pchip_mid(double ma, double mb) {
    if (sgn(ma) != sgn(mb) || ma == 0.0 || mb == 0.0) return 0.0;
    return 1.0 / ((3.0 / ma + 3.0 / mb) / 6.0);
}

struct LogArgs {
    const double* v;     // (N, n_ch) dense
    const double* klog;  // [N]
    int64_t n_bins;
    int n_ch;
    double* out;         // (N, n_ch) dense
};

__global__ __launch_bounds__(NT) void k_to_log(LogArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    const int64_t j = idx / p.n_ch, N = p.n_bins;
    const int c = (int)(idx - j * p.n_ch);
    const double xq = p.klog[j];
    int64_t i = (int64_t)floor(xq) - 1;  // knots 1 .. N: interval i is [i + 1, i + 2)
    i = i < 0 ? 0 : (i > N - 2 ? N - 2 : i);
    const double s = xq - (double)(i + 1);
    const double* col = p.v + c;
    const double ym = col[(i > 0 ? i - 1 : 0) * p.n_ch], y0 = col[i * p.n_ch], y1 = col[(i + 1) * p.n_ch],
                 yp = col[(i + 2 < N ? i + 2 : N - 1) * p.n_ch];
    const double m_prev = y0 - ym, m = y1 - y0, m_next = yp - y1;
    double d0 = m, d1 = m;
    if (N > 2) {
        d0 = i == 0 ? pchip_edge(m, m_next) : pchip_mid(m_prev, m);
        d1 = i + 2 == N ? pchip_edge(m, m_prev) : pchip_mid(m, m_next);
    }
    // CubicHermiteSpline's coefficients (dx = 1) and PPoly's evaluation order
    const double t = d0 + d1 - 2.0 * m;
    const double c1 = (m - d0) - t;
    double res = y0, z = s;
    res += d0 * z;
    z *= s;
    res += c1 * z;
    z *= s;
    res += t * z;
    p.out[idx] = res;
}

struct SmoothArgs {
    const double* v;   // (N, n_ch) dense
    const double* wr;  // [L] reversed unit-sum window
    int64_t n_bins, n_window;
    int n_ch, tc, lg_tc;
    double* out;       // (N, n_ch) dense
};

__global__ __launch_bounds__(NT) void k_smooth(SmoothArgs p) {
    __shared__ double lds[LDS_DOUBLES];
    const int tid = threadIdx.x, tc = p.tc;
    const int cl = tid & (tc - 1), base = (tid >> p.lg_tc) * R;
    const int TB = (NT >> p.lg_tc) * R, CH = LDS_DOUBLES / tc - TB + 1;
    const int64_t N = p.n_bins, b0 = (int64_t)blockIdx.x * TB, pf = p.n_window / 2;
    const int c0 = blockIdx.y * tc;
    const double* t = lds + cl;
    double acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.0;
    for (int64_t m0 = 0; m0 < p.n_window; m0 += CH) {
        const int ch = (int)(p.n_window - m0 < CH ? p.n_window - m0 : CH);
        const int rows = TB + ch - 1;
        __syncthreads();  // the previous chunk's reads
        for (int e = tid; e < rows * tc; e += NT) {
            int64_t src = b0 - pf + m0 + (e >> p.lg_tc);
            src = src < 0 ? 0 : (src > N - 1 ? N - 1 : src);
            const int cc = c0 + (e & (tc - 1));
            lds[e] = p.v[src * p.n_ch + (cc < p.n_ch ? cc : p.n_ch - 1)];
        }
        __syncthreads();
        const double* w = p.wr + m0;
        double x[R];  // slot j % R holds row base + j of the image
#pragma unroll
        for (int q = 0; q < R - 1; ++q) x[q] = t[(base + q) * tc];
        int m = 0;
        for (; m + R <= ch; m += R) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                x[(u + R - 1) % R] = t[(base + m + u + R - 1) * tc];
                const double wk = w[m + u];
#pragma unroll
                for (int q = 0; q < R; ++q) acc[q] = fma(wk, x[(u + q) % R], acc[q]);
            }
        }
        for (; m < ch; ++m) {
            const double wk = w[m];
#pragma unroll
            for (int q = 0; q < R; ++q) acc[q] = fma(wk, t[(base + m + q) * tc], acc[q]);
        }
    }
    const int c = c0 + cl;
    if (c >= p.n_ch) return;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int64_t b = b0 + base + q;
        if (b < N) p.out[b * p.n_ch + c] = acc[q];
    }
}

struct LinArgs {
    const double* v;     // (N, n_ch) dense, on the k_log axis
    const double* klog;  // [N] strictly ascending, klog[0] <= 1, klog[N - 1] >= N
    int64_t n_bins;
    int n_ch, clip_ch;   // columns [0, clip_ch): negative results become 0
    double scale;        // (N - 1) / log N
    double* out;         // (N, n_ch) dense
};

__global__ __launch_bounds__(NT) void k_to_lin(LinArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    const int64_t li = idx / p.n_ch, N = p.n_bins;
    const int c = (int)(idx - li * p.n_ch);
    const double l = (double)(li + 1);
    // lo = the last index with klog[lo] < l, within [0, N - 2] (searchsorted "left", clipped, minus one)
    int64_t lo = (int64_t)(p.scale * log(l));
    lo = lo < 0 ? 0 : (lo > N - 2 ? N - 2 : lo);
    while (lo < N - 2 && p.klog[lo + 1] < l) ++lo;
    while (lo > 0 && p.klog[lo] >= l) --lo;
    const double x_lo = p.klog[lo], x_hi = p.klog[lo + 1];
    const double y_lo = p.v[lo * p.n_ch + c], y_hi = p.v[(lo + 1) * p.n_ch + c];
    const double slope = (y_hi - y_lo) / (x_hi - x_lo);
    double r = slope * (l - x_lo) + y_lo;
    if (c < p.clip_ch && r < 0.0) r = 0.0;
    p.out[idx] = r;
}

// (the logarithmic-bins route has no k_to_lin: its clip runs on the smoothed array in place)
struct ClipArgs {
    double* v;  // (N, n_ch) dense
    int64_t n_bins;
    int n_ch, clip_ch;
};
__global__ __launch_bounds__(NT) void k_clip(ClipArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    if ((int)(idx % p.n_ch) < p.clip_ch && p.v[idx] < 0.0) p.v[idx] = 0.0;
}

struct PolarArgs {
    const double2* z;  // (N, n_ch)
    int64_t n_bins;
    int n_ch;
    double* mag;       // (N, 2 n_ch): |z| into columns [0, n_ch)
    double* ph;        // (N, 2 n_ch): atan2 into columns [n_ch, 2 n_ch)
};

__global__ __launch_bounds__(NT) void k_polar(PolarArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    const int64_t b = idx / p.n_ch;
    const int c = (int)(idx - b * p.n_ch);
    const double2 z = p.z[idx];
    const int64_t o = b * 2 * p.n_ch + c;
    p.mag[o] = hypot(z.x, z.y);
    p.ph[o + p.n_ch] = atan2(z.y, z.x);
}

// numpy.unwrap's correction of the step d = p[b] - p[b - 1]
__device__ __forceinline__ double unwrap_step(double d) {
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    double r = fmod(d + pi, two_pi);  // numpy.mod: the result takes the divisor's sign
    if (r != 0.0 && r < 0.0) r += two_pi;
    double dm = r - pi;
    if (dm == -pi && d > 0.0) dm = pi;
    return fabs(d) < pi ? 0.0 : dm - d;
}

struct UnwrapArgs {
    const double* ph;  // column c of channel c, row stride ld
    int64_t n_bins, ld;
    double* out;       // same layout
};

__global__ __launch_bounds__(NT) void k_unwrap(UnwrapArgs p) {
    constexpr int E = 8;  // consecutive bins per lane and tile
    __shared__ double part[NT];
    const int tid = threadIdx.x;
    const double* col = p.ph + blockIdx.x;
    double* oc = p.out + blockIdx.x;
    double carry = 0.0;  // sum of the corrections of every bin before this tile
    for (int64_t t0 = 0; t0 < p.n_bins; t0 += (int64_t)NT * E) {
        const int64_t b0 = t0 + (int64_t)tid * E;
        double v[E + 1], corr[E];
        v[0] = b0 > 0 && b0 - 1 < p.n_bins ? col[(b0 - 1) * p.ld] : 0.0;
#pragma unroll
        for (int k = 0; k < E; ++k) v[k + 1] = b0 + k < p.n_bins ? col[(b0 + k) * p.ld] : 0.0;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            sum += (b0 + k > 0 && b0 + k < p.n_bins) ? unwrap_step(v[k + 1] - v[k]) : 0.0;
            corr[k] = sum;
        }
        // inclusive scan of the lanes' sums
        part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < NT; off <<= 1) {
            const double add = tid >= off ? part[tid - off] : 0.0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const double before = carry + (tid > 0 ? part[tid - 1] : 0.0);
        const double total = part[NT - 1];
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (b0 + k < p.n_bins) oc[(b0 + k) * p.ld] = v[k + 1] + (before + corr[k]);
        carry += total;
        __syncthreads();  // part[] is rewritten by the next tile
    }
}

struct RecombineArgs {
    const double* mp;  // (N, 2 n_ch): magnitude, phase
    int64_t n_bins;
    int n_ch;
    double2* out;      // (N, n_ch)
};

__global__ __launch_bounds__(NT) void k_recombine(RecombineArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n_bins * p.n_ch) return;
    const int64_t b = idx / p.n_ch;
    const int c = (int)(idx - b * p.n_ch);
    const double* i = p.mp + b * 2 * p.n_ch + c;
    double s, co;
    sincos(i[p.n_ch], &s, &co);
    p.out[idx] = make_double2(i[0] * co, i[0] * s);
}

}  // namespace dssmooth
