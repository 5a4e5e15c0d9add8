// Weighted sums of fractionally delayed channels, float64 arithmetic: what the reference's fractional_delay
// (standard/latency_delay.py:159-285, filter from standard/_standard_backend.py:259-321 and :430-492) computes
// for one channel, and what MonopoleSource.get_signals_on_array, mix_sources_on_array and
// BeamformerDASTime.get_beamformer_output (beamforming/beamforming.py:1317-1512) add up.  gfx950.
//
//     y[g, t] = sum_{j < J} w[g,j] sum_{k <= order} h(frac[g,j])[k] x_{src[g,j]}[t - shift[g,j] - k],  0 <= t < out_len
//
// x_c[n] = 0 outside [0, len_c).  A term with frac < 0 is a pass-through (the reference's sig.copy() for a delay
// of exactly 0): a single unit tap.
//
//   k_delay_taps  one thread per (term, tap): the Kaiser-windowed sinc of _fractional_delay_filter, in float64,
//                 stored reversed and zero-padded in front to NTP taps, a multiple of R (slot q holds h[NTP-1-q]).
//   k_delay_sum   one wave per output row g, 64 lanes x R consecutive outputs per wave, four rows per workgroup.
//                 For each term j the workgroup stages the source span its four rows read -- once from memory
//                 when the rows share the source and their shifts lie close together, else wave by wave -- into
//                 one LDS window per wave, and each lane slides an R + R register window over it across the taps:
//                 every LDS read feeds R FMAs.  Optionally the row's peak |y| (atomicMax on the bits of a
//                 non-negative double) instead of, or beside, the samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dly {

constexpr int R = 8;                     // consecutive outputs per lane (and taps per register block)
constexpr int WAVES = 4;                 // rows per workgroup
constexpr int THREADS = 64 * WAVES;
constexpr int TT = 64 * R;               // outputs per row and workgroup
constexpr int MAX_ORDER = 255;
constexpr int NTP_MAX = MAX_ORDER + 1;   // padded taps, a multiple of R
constexpr int WL_MAX = TT + NTP_MAX;     // window of one wave: TT + NTP samples
// window sample v sits at v + v / R: consecutive lanes start 9 doubles apart, and the 32 lanes of a ds_read_b64
// group cover all 64 banks
__host__ __device__ constexpr int padded(int v) { return v + v / R; }
constexpr int WIN_LD = padded(WL_MAX);
constexpr int SHARED_SPAN_MAX = 4 * WL_MAX;  // widest span of one source the workgroup stages in one pass

struct TapArgs {
    const double* frac;  // [n_terms]; < 0: pass-through
    int n_terms, order, ntp;
    double beta;         // Kaiser shape parameter (_kaiser_window_beta, on the host)
    double* taps;        // [n_terms][ntp], reversed
};

// I0 of a real argument (sign = +1) or J0 (sign = -1: I0 of the imaginary argument i z) by the power series
__device__ inline double bessel0_series(double z, double sign) {
    const double q = 0.25 * z * z;
    double term = 1.0, sum = 1.0;
    for (int m = 1; m < 400; ++m) {
        term *= sign * q / ((double)m * (double)m);
        sum += term;
        if (fabs(term) <= 1e-17 * fabs(sum)) break;
    }
    return sum;
}

__global__ __launch_bounds__(256) void k_delay_taps(TapArgs p) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)p.n_terms * p.ntp) return;
    const int term = (int)(id / p.ntp), q = (int)(id % p.ntp);
    const int k = p.ntp - 1 - q;  // the tap this slot holds
    double h = 0.0;
    const double frac = p.frac[term];
    if (k <= p.order) {
        if (frac < 0.0) {
            h = k == 0 ? 1.0 : 0.0;
        } else {
            const int order = p.order;
            const bool odd = order % 2 != 0;
            // M_opt: int(frac) - (order - 1) / 2 (odd) or round-half-even(frac) - order / 2 (even); frac < 1
            const double m_opt = odd ? -(double)(order - 1) / 2.0 : (frac > 0.5 ? 1.0 : 0.0) - (double)order / 2.0;
            const double n = ((double)k + m_opt) - frac;
            double sinc = 1.0;
            if (n != 0.0) {
                const double y = 3.141592653589793 * n;  // np.sinc: sin(pi x) / (pi x)
                sinc = sin(y) / y;
            }
            const double alpha = (double)order / 2.0;
            double l = (double)k - frac;
            if (odd) l += 0.5;
            else if (frac > 0.5) l += 1.0;
            const double r = (l - alpha) / alpha;
            const double arg = 1.0 - r * r;
            const double w = (arg >= 0.0 ? bessel0_series(p.beta * sqrt(arg), 1.0)
                                         : bessel0_series(p.beta * sqrt(-arg), -1.0)) /
                             bessel0_series(p.beta, 1.0);
            h = sinc * w;
        }
    }
    p.taps[id] = h;
}

template <typename T>
struct Args {
    const T* x;
    int64_t sxc, sxn;       // sample n of source c at x[c sxc + n sxn]
    const int64_t* len;     // [n_src] valid samples of each source
    T* y;                   // null: peaks only
    int64_t syg, syt;       // output sample t of row g at y[g syg + t syt]
    int64_t out_len;
    int n_rows, n_terms, ntp;
    const int* src;         // [n_rows][n_terms]
    const int64_t* shift;   // [n_rows][n_terms]
    const double* weight;   // [n_rows][n_terms]
    const double* taps;     // [n_rows][n_terms][ntp], reversed (k_delay_taps)
    unsigned long long* peak;  // [n_rows] bits of max |y| (zeroed by the host) or null
};

template <typename T>
__device__ inline double sample(const Args<T>& p, int c, int64_t n) {
    return (n >= 0 && n < p.len[c]) ? (double)p.x[(int64_t)c * p.sxc + n * p.sxn] : 0.0;
}

// grid = (ceil(out_len / TT), ceil(n_rows / WAVES)), block = THREADS
template <typename T>
__global__ __launch_bounds__(THREADS) void k_delay_sum(Args<T> p) {
    __shared__ double win[WAVES][WIN_LD];
    __shared__ double hs[WAVES][NTP_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g0 = blockIdx.y * WAVES, g = g0 + wv;
    const bool row_ok = g < p.n_rows;
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    const int ntp = p.ntp, wl = TT + ntp;
    double out[R];
#pragma unroll
    for (int i = 0; i < R; ++i) out[i] = 0.0;

    for (int j = 0; j < p.n_terms; ++j) {
        // the four rows' sources and window starts (every lane reads the same values)
        int c[WAVES];
        int64_t b[WAVES];
        bool same = true;
        int64_t bmin = INT64_MAX, bmax = INT64_MIN;
        int first = -1;
#pragma unroll
        for (int r = 0; r < WAVES; ++r) {
            const int gr = g0 + r;
            c[r] = -1;
            b[r] = 0;
            if (gr < p.n_rows) {
                const int64_t e = (int64_t)gr * p.n_terms + j;
                c[r] = p.src[e];
                // output t reads x[t - shift - k] with tap slot q = ntp - 1 - k: the window starts at
                // t0 - shift - (ntp - 1)
                b[r] = t0 - p.shift[e] - (ntp - 1);
                if (first < 0) first = c[r];
                same = same && c[r] == first;
                bmin = b[r] < bmin ? b[r] : bmin;
                bmax = b[r] > bmax ? b[r] : bmax;
            }
        }
        if (same && bmax - bmin + wl <= SHARED_SPAN_MAX) {
            // one pass over the span of the shared source; each sample goes to every window that holds it
            const int span = (int)(bmax - bmin) + wl;
            for (int u = threadIdx.x; u < span; u += THREADS) {
                const double v = sample(p, first, bmin + u);
#pragma unroll
                for (int r = 0; r < WAVES; ++r) {
                    const int64_t o = bmin + u - b[r];
                    if (c[r] >= 0 && o >= 0 && o < wl) win[r][padded((int)o)] = v;
                }
            }
        } else if (row_ok) {
            for (int u = lane; u < wl; u += 64) win[wv][padded(u)] = sample(p, c[wv], b[wv] + u);
        }
        if (row_ok) {
            const double* tp = p.taps + ((int64_t)g * p.n_terms + j) * ntp;
            for (int q = lane; q < ntp; q += 64) hs[wv][q] = tp[q];
        }
        __syncthreads();
        if (row_ok) {
            // acc[i] = sum_q taps[q] window[lane R + i + q]
            const double* wp = &win[wv][padded(lane * R)];
            const double* hp = hs[wv];
            double acc[R], v[2 * R];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                acc[i] = 0.0;
                v[i] = wp[padded(i)];
            }
            for (int q0 = 0; q0 < ntp; q0 += R) {
                const double* w8 = wp + padded(q0);
                double h[R];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    v[R + i] = w8[padded(R + i)];
                    h[i] = hp[q0 + i];
                }
#pragma unroll
                for (int qq = 0; qq < R; ++qq)
#pragma unroll
                    for (int i = 0; i < R; ++i) acc[i] = fma(h[qq], v[i + qq], acc[i]);
#pragma unroll
                for (int i = 0; i < R; ++i) v[i] = v[R + i];
            }
            const double wt = p.weight[(int64_t)g * p.n_terms + j];
#pragma unroll
            for (int i = 0; i < R; ++i) out[i] = fma(wt, acc[i], out[i]);
        }
        __syncthreads();
    }
    if (!row_ok) return;
    const int64_t tl = t0 + (int64_t)lane * R;
    double pk = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (tl + i < p.out_len) {
            if (p.y) p.y[(int64_t)g * p.syg + (tl + i) * p.syt] = (T)out[i];
            pk = fmax(pk, fabs(out[i]));
        }
    }
    if (p.peak) {
        for (int o = 32; o > 0; o >>= 1) pk = fmax(pk, __shfl_xor(pk, o));
        if (lane == 0) atomicMax(p.peak + g, (unsigned long long)__double_as_longlong(pk));
    }
}

}  // namespace dly
