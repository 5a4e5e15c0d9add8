// Audio effects: the reference's effects module (effects/effects.py, effects/_effects.py) and the gate of
// standard.activity_detector (standard/_standard_backend.py), whose sample loops are not linear and so cannot go through
// the block carry of block_carry.hpp.  float64 arithmetic throughout, each kernel in the reference's operation order
// (no contraction into fused multiply-adds).  gfx950.
//
// A stream is one channel of one band.  The samples of stream s are read through Src<T>: T = double for a host array
// staged as it is, (samples, streams) interleaved; T = float for planar samples that live on the device.  Results go
// out through Dst<T> in the same layout.
//
//   k_fx_stats     one workgroup per stream: peak |v|, mean and the root of the mean squared deviation of v = x gain,
//                  in two passes and a fixed summation order (numpy's std is two-pass as well).
//   k_fx_follow    one workgroup per stream: the switched one-pole recursion g <- c f + (1 - c) g of the compressor and of
//                  the activity detector.  Tile by tile (FOLLOW_TILE samples) three waves load the samples and put the
//                  level, the knee curve, the power and both products c f into LDS; lane 0 of the fourth wave runs the
//                  recursion over the tile staged the round before, out of LDS -- per sample two multiply-adds that do not
//                  depend on each other, one compare and one select -- and the three waves apply the gains of the tile
//                  before that (or take the detector's threshold) and store.  The serial lane touches neither global
//                  memory nor a transcendental, and waits for neither: the rounds overlap.
//   k_fx_comb      DigitalDelay's y[i] = x[i] + fb sat(y[i - D]): D independent chains per stream, one lane per chain.
//   k_fx_voices    Chorus: out[i] = td[i] + sum_v td[i + m[i, v]] over the zero-padded samples, negative indices wrapping
//                  from the end, mixed with the clean samples.
//   k_fx_curve_peak, k_fx_shape   Distortion: the peak of every selected curve's output, then the sum of the
//                  peak-restored curves and the gain stage.
//   k_fx_tremolo   the samples times a per-sample modulator.
//   k_fx_scale     the last stage of compressor, delay and chorus: the RMS or peak restore (the factor is formed on the
//                  device from two k_fx_stats results) and the gain stage, into the caller's layout.
#pragma once
#include <stdint.h>

namespace dsfx {

constexpr int NT = 256;             // threads of the sample-parallel kernels and of the reductions
constexpr int WAVE = 64;
constexpr int FOLLOW_TILE = 512;    // samples of one follower round: four LDS arrays of two tiles each, 32 KiB
constexpr int FOLLOW_NT = 256;      // the follower's workgroup: wave 0 runs the recursion, waves 1 to 3 work around it
constexpr int FOLLOW_WORKERS = FOLLOW_NT - WAVE;
constexpr int MAX_CURVES = 8;       // distortion curves of one call
constexpr int MAX_VOICES = 64;      // chorus voices of one call
constexpr int STATS_NT = 1024;      // threads of k_fx_stats
constexpr int STATS_UNROLL = 16;    // independent loads a lane of k_fx_stats keeps in flight
constexpr int STAT = 4;             // doubles per stream of a stats record: peak, mean, rms, (unused)

enum Curve { CURVE_ARCTAN = 0, CURVE_HARD = 1, CURVE_SOFT = 2, CURVE_CLEAN = 3, N_CURVES = 4 };
enum Restore { RESTORE_NONE = 0, RESTORE_RMS = 1, RESTORE_PEAK = 2 };
enum Saturation { SAT_DIGITAL = 0, SAT_ARCTAN = 1 };
enum FollowMode { MODE_COMPRESS = 0, MODE_DETECT = 1 };

template <typename T>
struct Src {  // sample n of stream s
    using type = T;
    const T* p;
    int64_t ss, cs;
    __device__ double at(int64_t n, int s) const { return (double)p[n * ss + (int64_t)s * cs]; }
};
template <typename T>
struct Dst {
    T* p;
    int64_t ss, cs;
    __device__ void put(int64_t n, int s, double v) const { p[n * ss + (int64_t)s * cs] = (T)v; }
};

// numpy's max propagates a NaN; fmax would drop it
__device__ inline double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// ---- peak, mean, rms ------------------------------------------------------------------------------------------------
template <typename T>
struct StatsArgs {
    Src<T> x;
    int64_t n;
    double gain;  // v = x gain
    double* st;   // [streams][STAT]
};

template <int N>
__device__ inline double block_sum(double v, double* sh) {  // every thread of the N gets the sum; fixed tree
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int h = N / 2; h > 0; h >>= 1) {
        if (t < h) sh[t] = sh[t] + sh[t + h];
        __syncthreads();
    }
    return sh[0];
}
template <int N>
__device__ inline double block_peak(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int h = N / 2; h > 0; h >>= 1) {
        if (t < h) sh[t] = nan_max(sh[t], sh[t + h]);
        __syncthreads();
    }
    return sh[0];
}

template <typename T>
__global__ __launch_bounds__(STATS_NT) void k_fx_stats(StatsArgs<T> a) {
#pragma clang fp contract(off)
    __shared__ double sh[STATS_NT];
    const int s = blockIdx.x;
    double pk = 0.0, sum = 0.0;
    // one workgroup walks the whole stream, so what it keeps in flight sets its rate: 1024 lanes, STATS_UNROLL loads each
    // (256 lanes with one load a round read 480 000 samples twice in 1.0 ms, a stream)
    for (int64_t n0 = threadIdx.x; n0 < a.n; n0 += (int64_t)STATS_NT * STATS_UNROLL) {
        double v[STATS_UNROLL];
#pragma unroll
        for (int u = 0; u < STATS_UNROLL; ++u) {
            const int64_t n = n0 + (int64_t)u * STATS_NT;
            v[u] = n < a.n ? a.x.at(n, s) * a.gain : 0.0;
        }
#pragma unroll
        for (int u = 0; u < STATS_UNROLL; ++u) {
            pk = nan_max(pk, fabs(v[u]));
            sum += v[u];
        }
    }
    pk = block_peak<STATS_NT>(pk, sh);
    const double mean = block_sum<STATS_NT>(sum, sh) / (double)a.n;
    double m2 = 0.0;
    for (int64_t n0 = threadIdx.x; n0 < a.n; n0 += (int64_t)STATS_NT * STATS_UNROLL) {
        double v[STATS_UNROLL];
#pragma unroll
        for (int u = 0; u < STATS_UNROLL; ++u) {
            const int64_t n = n0 + (int64_t)u * STATS_NT;
            v[u] = n < a.n ? a.x.at(n, s) * a.gain - mean : 0.0;
        }
#pragma unroll
        for (int u = 0; u < STATS_UNROLL; ++u) m2 += v[u] * v[u];
    }
    m2 = block_sum<STATS_NT>(m2, sh);
    if (threadIdx.x == 0) {
        double* st = a.st + (int64_t)s * STAT;
        st[0] = pk;
        st[1] = mean;
        st[2] = sqrt(m2 / (double)a.n);
        st[3] = 0.0;
    }
}

// ---- follower -------------------------------------------------------------------------------------------------------
struct FollowPar {
    double gain;      // compressor: the pre-compression gain
    double thr;       // compressor: threshold of the knee curve, dB; detector: threshold of the mask, dB
    double ratio, knee;
    double c_att, c_rel;
    double min_pow;   // compressor: floor of the squared sample
    int downward, relative;
};
template <typename T>
struct FollowArgs {
    Src<T> x;
    int64_t n;
    FollowPar p;
    const double* st;  // k_fx_stats of x gain: the peaks
    double* yd;        // compressor: [streams][n]
    uint8_t* mask;     // detector: [streams][n]
};

// the array branch of the reference's knee function (the one its sample loop reaches), x a level in dB
__device__ inline double knee_curve(double x, const FollowPar& p) {
#pragma clang fp contract(off)
    const double T = p.thr, R = p.ratio, W = p.knee;
    double y = 0.0;
    if (p.downward) {
        if (x - T < -W / 2) y = x;
        if (fabs(x - T) <= W / 2) {
            const double u = x - T + W / 2;
            y = x + (1 / R - 1) * (u * u) / 2 / W;
        }
        if (x - T > W / 2) y = T + (x - T) / R;
    } else {
        if (x - T < -W / 2) y = T + (x - T) / R;
        if (fabs(x - T) <= W / 2) {
            const double u = x - T - W / 2;
            y = x - (1 / R - 1) * (u * u) / 2 / W;
        }
        if (x - T > W / 2) y = x;
    }
    return y;
}

// One workgroup of four waves per stream.  In round t lane 0 of wave 0 runs the recursion over tile t - 1 while the three
// other waves finish tile t - 2 (gain times sample, or the threshold; the store) and stage tile t (the load, the level, the
// knee curve, the power, both products c f) in the other half of the LDS arrays; a worker lane finishes and stages the
// same indices, so it has read a slot before it overwrites it.  The recursion replaces f by g in place.
template <typename T, int MODE>
__global__ __launch_bounds__(FOLLOW_NT) void k_fx_follow(FollowArgs<T> a) {
#pragma clang fp contract(off)
    __shared__ double s_fg[2][FOLLOW_TILE], s_hi[2][FOLLOW_TILE], s_lo[2][FOLLOW_TILE], s_td[2][FOLLOW_TILE];
    const int s = blockIdx.x, tid = threadIdx.x;
    const FollowPar p = a.p;
    const double peak = a.st[(int64_t)s * STAT];
    const double om_att = 1 - p.c_att, om_rel = 1 - p.c_rel;
    const int64_t tiles = (a.n + FOLLOW_TILE - 1) / FOLLOW_TILE;
    double g = MODE == MODE_COMPRESS ? 1.0 : 0.0;  // carried from tile to tile by lane 0
    for (int64_t t = 0; t < tiles + 2; ++t) {
        const int b = (int)(t & 1);
        if (tid < WAVE) {
            if (tid == 0 && t >= 1 && t - 1 < tiles) {
                const int64_t base = (t - 1) * FOLLOW_TILE;
                const int cnt = (int)(a.n - base < FOLLOW_TILE ? a.n - base : FOLLOW_TILE);
                double* fg = s_fg[b ^ 1];
                const double *hi = s_hi[b ^ 1], *lo = s_lo[b ^ 1];
                if (MODE == MODE_COMPRESS) {
#pragma unroll 8
                    for (int i = 0; i < cnt; ++i) {
                        const double up = hi[i] + om_att * g, down = lo[i] + om_rel * g;
                        g = fg[i] > g ? up : down;
                        fg[i] = g;
                    }
                } else {
#pragma unroll 8
                    for (int i = 0; i < cnt; ++i) {
                        g = hi[i] + lo[i] * g;
                        fg[i] = g;
                    }
                }
            }
        } else {
            if (t >= 2) {  // finish tile t - 2
                const int64_t base = (t - 2) * FOLLOW_TILE;
                const int cnt = (int)(a.n - base < FOLLOW_TILE ? a.n - base : FOLLOW_TILE);
                for (int i = tid - WAVE; i < cnt; i += FOLLOW_WORKERS) {
                    const int64_t n = base + i;
                    if (MODE == MODE_COMPRESS) {
                        double o = s_td[b][i] * s_fg[b][i];
                        if (p.relative) o = o * peak;
                        a.yd[(int64_t)s * a.n + n] = o;
                    } else {
                        a.mask[(int64_t)s * a.n + n] = 10.0 * log10(s_fg[b][i]) > p.thr ? 1 : 0;
                    }
                }
            }
            if (t < tiles) {  // stage tile t
                const int64_t base = t * FOLLOW_TILE;
                const int cnt = (int)(a.n - base < FOLLOW_TILE ? a.n - base : FOLLOW_TILE);
                for (int i = tid - WAVE; i < cnt; i += FOLLOW_WORKERS) {
                    const int64_t n = base + i;
                    if (MODE == MODE_COMPRESS) {
                        double v = a.x.at(n, s) * p.gain;
                        if (p.relative) v = v / peak;
                        const double samp = v * v;
                        const double d = 10.0 * log10(p.min_pow > samp ? p.min_pow : samp);
                        const double f = pow(10.0, (knee_curve(d, p) - d) / 20.0);
                        s_td[b][i] = v;
                        s_fg[b][i] = f;
                        s_hi[b][i] = p.c_att * f;
                        s_lo[b][i] = p.c_rel * f;
                    } else {
                        double v = a.x.at(n, s), q = n > 0 ? a.x.at(n - 1, s) : 0.0;
                        if (p.relative) v = v / peak, q = q / peak;
                        // the reference reads its gain array before writing it: the coefficient is the release one after a
                        // sample with power, 0 after a silent one, and sample 0 keeps the gain 0
                        const double c = (n > 0 && q * q > 0.0) ? p.c_rel : 0.0;
                        s_hi[b][i] = n > 0 ? c * (v * v) : 0.0;
                        s_lo[b][i] = n > 0 ? 1 - c : 0.0;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- comb -----------------------------------------------------------------------------------------------------------
template <typename T>
struct CombArgs {
    Src<T> x;
    int64_t n, n_out, delay;  // n_out = n + padding
    double fb;
    int sat;
    double* yd;  // [streams][n_out]
};

__device__ inline double saturate(double v, int sat) { return sat == SAT_ARCTAN ? 0.5 * atan(2 * v) : v; }  // (one product each: nothing to fuse)

// grid.x covers the chains (delay of them; the n samples themselves when delay == 0), grid.y the streams
template <typename T>
__global__ __launch_bounds__(NT) void k_fx_comb(CombArgs<T> a) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    double* y = a.yd + (int64_t)s * a.n_out;
    if (a.delay == 0) {  // the reference's in-place loop reads the sample it is about to overwrite
        if (k < a.n_out) {
            const double v = k < a.n ? a.x.at(k, s) : 0.0;
            y[k] = v + a.fb * saturate(v, a.sat);
        }
        return;
    }
    if (k >= a.delay) return;
    double prev = 0.0;
    for (int64_t i = k; i < a.n_out; i += a.delay) {
        double v = i < a.n ? a.x.at(i, s) : 0.0;
        if (i >= a.delay) v = v + a.fb * saturate(prev, a.sat);
        y[i] = v;
        prev = v;
    }
}

// ---- voices ---------------------------------------------------------------------------------------------------------
template <typename T>
struct VoicesArgs {
    Src<T> x;
    int64_t n, n_pad;  // n_pad = n + the largest |delay|: the length the indices wrap at
    const int32_t* m;  // [n][voices]
    int voices;
    double mix, one_minus_mix;
    double* yd;  // [streams][n]
};

template <typename T>
__global__ __launch_bounds__(NT) void k_fx_voices(VoicesArgs<T> a) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.n) return;
    const double clean = a.x.at(i, s);
    double acc = clean;
    for (int v = 0; v < a.voices; ++v) {
        int64_t j = i + a.m[i * a.voices + v];
        if (j < 0) j += a.n_pad;
        acc += (j >= 0 && j < a.n) ? a.x.at(j, s) : 0.0;  // (beyond n: the padding)
    }
    a.yd[(int64_t)s * a.n + i] = acc * a.mix + clean * a.one_minus_mix;
}

// ---- shape ----------------------------------------------------------------------------------------------------------
struct CurvePar {
    int kind[MAX_CURVES];
    double level[MAX_CURVES], offset[MAX_CURVES], mix[MAX_CURVES];  // linear level and offset
    int count;
};
template <typename T>
struct ShapeArgs {
    Src<T> x;
    Dst<T> y;
    int64_t n;
    CurvePar cv;
    double gain;       // the post gain
    const double* st;  // k_fx_stats of x: the peaks
    double* cpk;       // [streams][MAX_CURVES]: the peak of every curve's output
};

__device__ inline double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }  // keeps a NaN

__device__ inline double curve(int kind, double x, double peak, double level, double offset) {
#pragma clang fp contract(off)
    switch (kind) {
        case CURVE_ARCTAN: return atan(x / peak * level + offset) * (2 / 3.141592653589793);
        case CURVE_HARD: return clip(x / peak * level + offset, -1.0, 1.0);
        case CURVE_SOFT: {
            double u = x / peak * (2.0 / 3.0);
            u = u + offset;
            u = u * level;
            u = u - u * u * u / 3;
            return clip(u, -(2.0 / 3.0), 2.0 / 3.0);
        }
        default: return x;
    }
}

// grid (streams, curves)
template <typename T>
__global__ __launch_bounds__(NT) void k_fx_curve_peak(ShapeArgs<T> a) {
#pragma clang fp contract(off)
    __shared__ double sh[NT];
    const int s = blockIdx.x, k = blockIdx.y;
    const double peak = a.st[(int64_t)s * STAT];
    const int kind = a.cv.kind[k];
    const double level = a.cv.level[k], offset = a.cv.offset[k], mix = a.cv.mix[k];
    double pk = 0.0;
    for (int64_t n = threadIdx.x; n < a.n; n += NT) pk = nan_max(pk, fabs(curve(kind, a.x.at(n, s), peak, level, offset) * mix));
    pk = block_peak<NT>(pk, sh);
    if (threadIdx.x == 0) a.cpk[(int64_t)s * MAX_CURVES + k] = pk;
}

template <typename T>
__global__ __launch_bounds__(NT) void k_fx_shape(ShapeArgs<T> a) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (n >= a.n) return;
    const double peak = a.st[(int64_t)s * STAT], x = a.x.at(n, s);
    double acc = 0.0;
    for (int k = 0; k < a.cv.count; ++k)
        acc += curve(a.cv.kind[k], x, peak, a.cv.level[k], a.cv.offset[k]) * a.cv.mix[k] * (peak / a.cpk[(int64_t)s * MAX_CURVES + k]);
    a.y.put(n, s, acc * a.gain);
}

// ---- tremolo --------------------------------------------------------------------------------------------------------
template <typename T>
struct TremoloArgs {
    Src<T> x;
    Dst<T> y;
    int64_t n;
    const double* mod;  // [n]
};
template <typename T>
__global__ __launch_bounds__(NT) void k_fx_tremolo(TremoloArgs<T> a) {
    const int s = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (n < a.n) a.y.put(n, s, a.x.at(n, s) * a.mod[n]);
}

// ---- restore and gain -------------------------------------------------------------------------------------------------
template <typename T>
struct ScaleArgs {
    const double* yd;  // [streams][n]
    Dst<T> y;
    int64_t n;
    int restore;
    const double *st_in, *st_out;
    double gain;
};
template <typename T>
__global__ __launch_bounds__(NT) void k_fx_scale(ScaleArgs<T> a) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (n >= a.n) return;
    double v = a.yd[(int64_t)s * a.n + n];
    if (a.restore != RESTORE_NONE) {
        const int f = a.restore == RESTORE_RMS ? 2 : 0;
        v = v * (a.st_in[(int64_t)s * STAT + f] / a.st_out[(int64_t)s * STAT + f]);
    }
    a.y.put(n, s, v * a.gain);
}

}  // namespace dsfx
