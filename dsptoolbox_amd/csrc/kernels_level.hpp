// Levels and loudness: the reference's normalize, rms, crest_factor, fade, apply_gain (standard/gain_and_level.py,
// helpers/gain_and_level.py), detrend and envelope (standard/other.py, standard/_standard_backend.py:382-405) and the
// block energies of lufs_integrated.  float64 arithmetic throughout; every sum runs in a fixed order without atomics,
// so a call gives the same bits every time.  gfx950.
//
// A polynomial trend is handled in the basis P_0 .. P_order of the discrete Chebyshev (Gram) polynomials, orthonormal
// on the grid n = 0 .. N - 1.  With t = n - (N - 1) / 2 they obey
//     P_0 = 1 / sqrt(N),   P_1 = a_0 t P_0,   P_{k+1} = a_k t P_k - b_k P_{k-1}
// with a_k = 1 / beta_{k+1}, b_k = beta_k / beta_{k+1}, beta_k^2 = k^2 (N^2 - k^2) / (4 (4 k^2 - 1)): the host forms a_k
// and b_k in long double and the kernels take them by value.  The least-squares polynomial of order d is then
// p(n) = sum_k c_k P_k(n) with c_k = sum_n x[n] P_k(n) -- no normal equations and no power moments sum n^k x, whose
// cancellation grows with N^k.  Order 0 is the mean.
//
//   k_level_project        one workgroup per SPAN samples of one channel: c_k partial sums and max |x|; lane t adds samples
//                          t, t + NT, ... in order, then a tree over the lanes (the max joins it).
//   k_level_final          one workgroup per channel: the workgroups' partials added the same way.
//   k_level_stats          the shape of the projection: sum (x - p(n))^2 term by term, max |x - p(n)| and max |x|.
//   k_level_common         the channels' c_0 replaced by their mean (numpy's std of the flattened signal).
//   k_level_gain           the gain of a normalisation from the stats: factor / peak or factor / rms, per channel or common.
//   k_level_apply*         y[n] = (x[n] - p_c(n)) g_c fade[n] fade[N - 1 - n], every factor optional and skipped when
//                          absent, in this order; 16 bytes per lane (float4 on planar float32, double2 on the host's
//                          interleaved float64), scalar head, tail and misaligned rows.
//   k_level_moving         sqrt(max(0, mean of the last W squares of x - p_1(n))): a workgroup owns TILE outputs, rebuilds
//                          the window sum before its tile from scratch in a fixed order and moves inside the tile by an
//                          LDS scan of d^2[n] - d^2[n - W]; no error is carried from tile to tile.
//   k_level_blocks         one workgroup per (block, channel): the mean of Tg squares of the K-weighted samples.
//   k_level_mag            |z| scale of the analytic signal, into the host's (samples, channels) order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dslevel {

constexpr int NT = 256;              // lanes per workgroup
constexpr int PER_LANE = 16;         // samples per lane of a reduction
constexpr int SPAN = NT * PER_LANE;  // samples per workgroup of a reduction
constexpr int MAX_ORDER = 8;         // polynomial order of a trend
constexpr int NC = MAX_ORDER + 2;    // doubles per channel of a projection record: c_0 .. c_8, max |x|
constexpr int NST = 3;               // doubles per channel of a stats record: sum r^2, max |r|, max |x|
constexpr int TILE_PER_LANE = 4;
constexpr int TILE = NT * TILE_PER_LANE;  // outputs per workgroup of the moving window
constexpr int VEC_BYTES = 16;        // bytes a lane of the apply kernels loads and stores at once

enum Norm { NORM_NONE = 0, NORM_PEAK_EACH = 1, NORM_PEAK_ALL = 2, NORM_RMS_EACH = 3, NORM_RMS_ALL = 4 };

template <typename T>
struct Src {  // sample n of channel c
    using type = T;
    const T* p;
    int64_t ss, cs;
    __device__ double at(int64_t n, int c) const { return (double)p[n * ss + (int64_t)c * cs]; }
};
template <typename T>
struct Dst {
    using type = T;
    T* p;
    int64_t ss, cs;
    __device__ void put(int64_t n, int c, double v) const { p[n * ss + (int64_t)c * cs] = (T)v; }
};

struct Basis {  // order < 0: no polynomial
    int order;
    double half, p0;  // (N - 1) / 2, 1 / sqrt(N)
    double a[MAX_ORDER], b[MAX_ORDER];
};

// numpy's max propagates a NaN; fmax would drop it
__device__ inline double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// P_0 .. P_order at sample n (entries past the order are left alone)
__device__ inline void basis_at(const Basis& bs, int64_t n, double (&P)[MAX_ORDER + 1]) {
    const double t = (double)n - bs.half;
    P[0] = bs.p0;
#pragma unroll
    for (int k = 0; k < MAX_ORDER; ++k) {
        if (k >= bs.order) break;
        P[k + 1] = k == 0 ? bs.a[0] * t * P[0] : bs.a[k] * t * P[k] - bs.b[k] * P[k - 1];
    }
}

// p(n) = sum_k coef[k] P_k(n), the terms added from the highest order down (the small ones first)
__device__ inline double trend_at(const Basis& bs, const double* __restrict__ coef, int64_t n) {
    double P[MAX_ORDER + 1];
    basis_at(bs, n, P);
    double p = 0.0;
#pragma unroll
    for (int k = MAX_ORDER; k >= 0; --k)
        if (k <= bs.order) p = fma(coef[k], P[k], p);
    return p;
}

// NS sums and NM maxima over the workgroup's lanes, fixed tree; the results are valid in every lane
template <int NS, int NM>
__device__ inline void tree(double (&s)[NS], double (&m)[NM], double* red) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k * NT + t] = s[k];
#pragma unroll
    for (int k = 0; k < NM; ++k) red[(NS + k) * NT + t] = m[k];
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k * NT + t] += red[k * NT + t + h];
#pragma unroll
            for (int k = 0; k < NM; ++k) red[(NS + k) * NT + t] = nan_max(red[(NS + k) * NT + t], red[(NS + k) * NT + t + h]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = red[k * NT];
#pragma unroll
    for (int k = 0; k < NM; ++k) m[k] = red[(NS + k) * NT];
}

// grid = n_ch, block = NT: the workgroups' partial records [n_ch][n_wg][NS + NM] -> out[c][NS + NM]
struct FinalArgs {
    const double* partial;
    int n_wg;
    double* out;
};
template <int NS, int NM>
__global__ __launch_bounds__(NT) void k_level_final(FinalArgs p) {
    const double* partial = p.partial;
    const int n_wg = p.n_wg;
    double* out = p.out;
    __shared__ double red[(NS + NM) * NT];
    const int c = blockIdx.x, t = threadIdx.x;
    double s[NS], m[NM];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NM; ++k) m[k] = 0.0;
    for (int w = t; w < n_wg; w += NT) {
        const double* r = partial + ((size_t)c * n_wg + w) * (NS + NM);
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += r[k];
#pragma unroll
        for (int k = 0; k < NM; ++k) m[k] = nan_max(m[k], r[NS + k]);
    }
    tree<NS, NM>(s, m, red);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) out[c * (NS + NM) + k] = s[k];
#pragma unroll
        for (int k = 0; k < NM; ++k) out[c * (NS + NM) + NS + k] = m[k];
    }
}

// ---- projection -----------------------------------------------------------------------------------------------------
template <typename T>
struct ProjectArgs {
    Src<T> x;
    int64_t n;
    int n_wg;         // ceil(n / SPAN)
    Basis bs;         // order >= 0
    double* partial;  // [n_ch][n_wg][NC]
};

// grid = (n_wg, n_ch), block = NT
template <typename T>
__global__ __launch_bounds__(NT) void k_level_project(ProjectArgs<T> p) {
    __shared__ double red[NC * NT];
    const int c = blockIdx.y, t = threadIdx.x;
    double s[MAX_ORDER + 1], m[1] = {0.0};
#pragma unroll
    for (int k = 0; k <= MAX_ORDER; ++k) s[k] = 0.0;
    const int64_t n0 = (int64_t)blockIdx.x * SPAN;
    for (int i = 0; i < PER_LANE; ++i) {
        const int64_t nn = n0 + (int64_t)i * NT + t;
        if (nn >= p.n) break;
        const double x = p.x.at(nn, c);
        double P[MAX_ORDER + 1];
        basis_at(p.bs, nn, P);
#pragma unroll
        for (int k = 0; k <= MAX_ORDER; ++k)
            if (k <= p.bs.order) s[k] = fma(x, P[k], s[k]);
        m[0] = nan_max(m[0], fabs(x));
    }
    tree<MAX_ORDER + 1, 1>(s, m, red);
    if (t == 0) {
        double* r = p.partial + ((size_t)c * p.n_wg + blockIdx.x) * NC;
#pragma unroll
        for (int k = 0; k <= MAX_ORDER; ++k) r[k] = s[k];
        r[MAX_ORDER + 1] = m[0];
    }
}

// grid = 1, block = 64: c_0 of every channel <- the channels' mean c_0 (one common mean), added in channel order
struct CommonArgs {
    double* coef;  // [n_ch][NC]
    int n_ch;
};
__global__ void k_level_common(CommonArgs p) {
    double* coef = p.coef;
    const int n_ch = p.n_ch;
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int c = 0; c < n_ch; ++c) s += coef[(size_t)c * NC];
    s /= (double)n_ch;
    for (int c = 0; c < n_ch; ++c) coef[(size_t)c * NC] = s;
}

// ---- residual statistics --------------------------------------------------------------------------------------------
template <typename T>
struct StatsArgs {
    Src<T> x;
    int64_t n;
    int n_wg;
    Basis bs;
    const double* coef;  // [n_ch][NC]
    double* partial;     // [n_ch][n_wg][NST]
};

// grid = (n_wg, n_ch), block = NT
template <typename T>
__global__ __launch_bounds__(NT) void k_level_stats(StatsArgs<T> p) {
    __shared__ double red[NST * NT];
    const int c = blockIdx.y, t = threadIdx.x;
    const double* coef = p.coef + (size_t)c * NC;
    double s[1] = {0.0}, m[2] = {0.0, 0.0};
    const int64_t n0 = (int64_t)blockIdx.x * SPAN;
    for (int i = 0; i < PER_LANE; ++i) {
        const int64_t nn = n0 + (int64_t)i * NT + t;
        if (nn >= p.n) break;
        const double x = p.x.at(nn, c);
        const double r = x - trend_at(p.bs, coef, nn);
        s[0] = fma(r, r, s[0]);
        m[0] = nan_max(m[0], fabs(r));
        m[1] = nan_max(m[1], fabs(x));
    }
    tree<1, 2>(s, m, red);
    if (t == 0) {
        double* r = p.partial + ((size_t)c * p.n_wg + blockIdx.x) * NST;
        r[0] = s[0], r[1] = m[0], r[2] = m[1];
    }
}

// grid = 1, block = 64: gain[c] of a normalisation.  proj: [n_ch][NC] (its max |x|), stats: [n_ch][NST] (its sum r^2)
struct GainArgs {
    int mode, n_ch;
    int64_t n;
    double factor;
    const double *proj, *stats;
    double* gain;  // [n_ch]
};
__global__ void k_level_gain(GainArgs p) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    double all = 0.0;
    for (int c = 0; c < p.n_ch; ++c) {
        if (p.mode == NORM_PEAK_ALL) all = nan_max(all, p.proj[(size_t)c * NC + MAX_ORDER + 1]);
        if (p.mode == NORM_RMS_ALL) all += p.stats[(size_t)c * NST];
    }
    for (int c = 0; c < p.n_ch; ++c) {
        double d;
        switch (p.mode) {
        case NORM_PEAK_EACH: d = p.proj[(size_t)c * NC + MAX_ORDER + 1]; break;
        case NORM_PEAK_ALL: d = all; break;
        case NORM_RMS_EACH: d = sqrt(p.stats[(size_t)c * NST] / (double)p.n); break;
        default: d = sqrt(all / ((double)p.n * (double)p.n_ch)); break;
        }
        p.gain[c] = p.factor / d;
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------
struct ApplyArgs {
    int64_t n;
    int n_ch;
    Basis bs;            // order < 0: nothing is subtracted
    const double* coef;  // [n_ch][NC]
    const double* gain;  // [n_ch] or null
    const double* fade;  // [l_fade] or null
    int64_t l_fade;
    int at_start, at_end;
};

// the reference's order of operations, one rounding each: subtract, gain, fade in, fade out
__device__ inline double apply_one(const ApplyArgs& a, double x, int64_t n, int c) {
#pragma clang fp contract(off)
    double v = x;
    if (a.bs.order >= 0) v = v - trend_at(a.bs, a.coef + (size_t)c * NC, n);
    if (a.gain) v = v * a.gain[c];
    if (a.fade) {
        if (a.at_start && n < a.l_fade) v = v * a.fade[n];
        if (a.at_end && a.n - 1 - n < a.l_fade) v = v * a.fade[a.n - 1 - n];
    }
    return v;
}

// any layout, one sample per lane: grid = (ceil(n / NT), n_ch)
template <typename TI, typename TO>
struct ApplyAny {
    Src<TI> x;
    Dst<TO> y;
    ApplyArgs a;
};
template <typename TI, typename TO>
__global__ __launch_bounds__(NT) void k_level_apply(ApplyAny<TI, TO> p) {
    const Src<TI>& x = p.x;
    const Dst<TO>& y = p.y;
    const ApplyArgs& a = p.a;
    const int64_t n = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int c = blockIdx.y;
    if (n >= a.n) return;
    y.put(n, c, apply_one(a, x.at(n, c), n, c));
}

// planar float32 rows, four samples per lane: grid = (ceil((n / 4 + 2) / NT), n_ch).  Lane 0 of a row takes the samples
// before the first 16-byte boundary, lane i >= 1 the four from head + 4 (i - 1) on, as a float4 when all four exist; a row
// whose input and output sit differently against the boundary goes sample by sample.
struct ApplyF4 {
    const float* x;
    int64_t ldx;
    float* y;
    int64_t ld_y;
    ApplyArgs a;
};
__global__ __launch_bounds__(NT) void k_level_apply_f4(ApplyF4 p) {
    const ApplyArgs& a = p.a;
    const float* x = p.x;
    float* y = p.y;
    const int64_t ldx = p.ldx, ld_y = p.ld_y;
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    const float* xr = x + (int64_t)c * ldx;
    float* yr = y + (int64_t)c * ld_y;
    const unsigned mx = (unsigned)((uintptr_t)xr & 15), my = (unsigned)((uintptr_t)yr & 15);
    const bool vec = mx == my;
    const int64_t head = vec ? (int64_t)(((16 - mx) & 15) / 4) : 0;
    int64_t s, e;
    if (i == 0) {
        s = 0, e = head < a.n ? head : a.n;
    } else {
        s = head + 4 * (i - 1), e = s + 4 < a.n ? s + 4 : a.n;
    }
    if (s >= e) return;
    if (vec && i > 0 && e - s == 4) {
        const float4 v = *reinterpret_cast<const float4*>(xr + s);
        float4 o;
        o.x = (float)apply_one(a, (double)v.x, s, c);
        o.y = (float)apply_one(a, (double)v.y, s + 1, c);
        o.z = (float)apply_one(a, (double)v.z, s + 2, c);
        o.w = (float)apply_one(a, (double)v.w, s + 3, c);
        *reinterpret_cast<float4*>(yr + s) = o;
        return;
    }
    for (int64_t n = s; n < e; ++n) yr[n] = (float)apply_one(a, (double)xr[n], n, c);
}

// the host's (samples, channels) float64 array taken flat, two values per lane: grid = ceil(ceil(n n_ch / 2) / NT).  Both
// arrays start on a 16-byte boundary (pieces of the staging buffer); an odd last value goes alone.
struct ApplyD2 {
    const double* x;
    double* y;
    ApplyArgs a;
};
__global__ __launch_bounds__(NT) void k_level_apply_d2(ApplyD2 p) {
    const ApplyArgs& a = p.a;
    const double* x = p.x;
    double* y = p.y;
    const int64_t total = a.n * a.n_ch;
    const int64_t f = 2 * ((int64_t)blockIdx.x * NT + threadIdx.x);
    if (f >= total) return;
    const int64_t n0 = f / a.n_ch;
    const int c0 = (int)(f - n0 * a.n_ch);
    if (f + 1 < total) {
        const int c1 = c0 + 1 == a.n_ch ? 0 : c0 + 1;
        const int64_t n1 = c1 == 0 ? n0 + 1 : n0;
        const double2 v = *reinterpret_cast<const double2*>(x + f);
        double2 o;
        o.x = apply_one(a, v.x, n0, c0);
        o.y = apply_one(a, v.y, n1, c1);
        *reinterpret_cast<double2*>(y + f) = o;
    } else {
        y[f] = apply_one(a, x[f], n0, c0);
    }
}

// ---- moving mean square ---------------------------------------------------------------------------------------------
template <typename T>
struct MovingArgs {
    Src<T> x;
    int64_t n, w;        // w >= 1, may exceed n
    int n_ch;
    Basis bs;            // order 1
    const double* coef;  // [n_ch][NC]
    double* out;         // (n, n_ch)
};

// grid = (ceil(n / TILE), n_ch), block = NT.  out[n] = sqrt(max(0, sum_{j = n - w + 1 .. n, j >= 0} d[j]^2 / w))
template <typename T>
__global__ __launch_bounds__(NT) void k_level_moving(MovingArgs<T> p) {
    __shared__ double red[NT];
    __shared__ double scan[NT];
    const int c = blockIdx.y, t = threadIdx.x;
    const double* coef = p.coef + (size_t)c * NC;
    const int64_t n0 = (int64_t)blockIdx.x * TILE;
    auto sq = [&](int64_t j) {
        const double d = p.x.at(j, c) - trend_at(p.bs, coef, j);
        return d * d;
    };
    // the window that ends just before the tile, from scratch: samples max(0, n0 - w) .. n0 - 1
    const int64_t j0 = n0 > p.w ? n0 - p.w : 0;
    double base = 0.0;
    for (int64_t j = j0 + t; j < n0; j += NT) base += sq(j);
    red[t] = base;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    base = red[0];
    // the lane's TILE_PER_LANE consecutive differences d^2[n] - d^2[n - w], running sums inside the lane
    double run[TILE_PER_LANE];
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < TILE_PER_LANE; ++i) {
        const int64_t nn = n0 + (int64_t)t * TILE_PER_LANE + i;
        double d = 0.0;
        if (nn < p.n) {
            d = sq(nn);
            if (nn >= p.w) d -= sq(nn - p.w);
        }
        acc += d;
        run[i] = acc;
    }
    // exclusive scan of the lanes' totals (Hillis-Steele in LDS, fixed order)
    scan[t] = acc;
    __syncthreads();
    for (int h = 1; h < NT; h <<= 1) {
        const double v = t >= h ? scan[t - h] : 0.0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const double before = base + (t > 0 ? scan[t - 1] : 0.0);
#pragma unroll
    for (int i = 0; i < TILE_PER_LANE; ++i) {
        const int64_t nn = n0 + (int64_t)t * TILE_PER_LANE + i;
        if (nn < p.n) {
            const double ms = (before + run[i]) / (double)p.w;
            p.out[nn * p.n_ch + c] = sqrt(ms > 0.0 ? ms : (ms != ms ? ms : 0.0));
        }
    }
}

// ---- block mean squares ---------------------------------------------------------------------------------------------
struct BlockArgs {
    const double* y;  // planar [n_ch][n]
    int64_t n, tg, step;
    int n_ch;
    double* z;        // [n_blocks][n_ch]
};

// grid = (n_blocks, n_ch), block = NT: z = mean of y[b step .. b step + tg)^2
__global__ __launch_bounds__(NT) void k_level_blocks(BlockArgs p) {
    __shared__ double red[NT];
    const int c = blockIdx.y, t = threadIdx.x;
    const double* y = p.y + (int64_t)c * p.n + (int64_t)blockIdx.x * p.step;
    double s = 0.0;
    for (int64_t j = t; j < p.tg; j += NT) s = fma(y[j], y[j], s);
    red[t] = s;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) p.z[(int64_t)blockIdx.x * p.n_ch + c] = red[0] / (double)p.tg;
}

// ---- magnitude of the analytic signal -------------------------------------------------------------------------------
struct MagArgs {
    const double2* z;  // column c at z + c ld
    int64_t ld, n;
    int n_ch;
    double scale;
    double* out;       // (n, n_ch)
};

// grid = ceil(n n_ch / NT)
__global__ __launch_bounds__(NT) void k_level_mag(MagArgs p) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= p.n * p.n_ch) return;
    const int64_t k = idx / p.n_ch;
    const int c = (int)(idx - k * p.n_ch);
    const double2 v = p.z[(int64_t)c * p.ld + k];
    p.out[idx] = hypot(v.x * p.scale, v.y * p.scale);
}

}  // namespace dslevel
