// Shoebox room simulation, float64, gfx950: the image-source sum of room_acoustics._generate_rir
// (room_acoustics/_room_acoustics.py:162-269) and the modal sum of ShoeboxRoom.get_analytical_transfer_function
// (:554-685) of the reference.
//
// Image sources.  The reference visits the cells (l, m, n) of a (2 LIMIT + 1)^3 lattice in row-major order; a cell has
// eight sources u = (ux, uy, uz) in the order of U below.  Source (cell, u) lies at pos = (1 - 2u) s + 2 l dim - r, falls
// into bin int(d / c sr + 0.5) and adds damping / (4 pi d) there.  Inside one cell, sources that share a bin do not add:
// the last one in U's order replaces the others (a fancy-index +=).  Across cells they add.  A store pass and a
// per-bin sum pass reproduce that with the same bits on every call:
//   k_ism_count   a lane per cell of the slab of l planes: the eight bins, minus those replaced inside the cell and those
//                 at or beyond n_out, counted per bin with integer atomics.
//   k_ism_scan    exclusive scan of the counts by one workgroup (the counts become the segment starts, a second copy
//                 the fill cursors).
//   k_ism_fill    the same enumeration; every kept source writes its id -- its number ((l m n) u) in the reference's loop
//                 order, counted from the slab's first plane -- at the slot an integer atomic hands out.  The order
//                 inside a segment is therefore arbitrary, and nothing that is summed depends on it:
//   k_ism_sum     a workgroup per bin sorts the segment by id in LDS (bitonic, SORT_CAP ids at a time; a longer segment
//                 is walked in id ranges that hold at most SORT_CAP of its ids, found by halving), recomputes distance
//                 and damping of every id, TILE at a time, and lane b adds band b's terms one after the other in id
//                 order onto what the earlier slabs left in out[b][bin].  That is the reference's own order of additions.
// All bands share the enumeration (the reference derives LIMIT and every distance from the room's T60); only the
// damping differs, read from a host-made table pw[band][wall][k] = beta^k (numpy's **), walls in the order
// south, west, floor, north, east, ceiling, so the device multiplies the reference's factors in the reference's order.
// Contraction is off wherever the reference's statements are evaluated: a fused multiply-add would move a source that
// lies within a rounding error of a bin's edge.
//
// Modal sum.  k_modal_tf: a lane per frequency adds weight_n / (omega_n^2 + 2j eta_n omega_n - omega_f^2) over the
// table of modes in table order -- one writer per bin, nothing atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsroom {

constexpr int NT = 256;         // lanes of every image-source kernel
constexpr int SCAN_NT = 1024;   // k_ism_scan: one workgroup
constexpr int SCAN_PER = 4;     // counts per lane and sweep
constexpr int SORT_CAP = 1024;  // ids sorted in LDS at a time: four per lane (the crowded test case has 1327 in a bin)
constexpr int TILE = NT;        // sorted ids whose terms are evaluated together
constexpr int MAX_BANDS = 8;    // the reference's octave bands (125 Hz ... 16 kHz)
constexpr int MODAL_NT = 64;
constexpr uint32_t ID_PAD = 0xFFFFFFFFu;  // sorts behind every id (ids stay below 2^31: size_guards.hpp)

struct IsmArgs {
    double dim[3], s[3], r[3];
    double c, sr;
    int limit;            // LIMIT: cells -limit .. limit per axis
    int l0, l1;           // this slab: planes l0 <= l + limit < l1
    int64_t n_out;
    int n_band;
    const double* pw;     // [n_band][6][limit + 2]
    uint32_t* count;      // [n_out + 1]: counts, then segment starts
    uint32_t* cursor;     // [n_out + 1]
    uint32_t* list;       // ids of the slab's kept sources
    double* out;          // [n_band][n_out]
};

// the reference's u_vectors, (ux, uy, uz) per row
__constant__ const int U[8][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {1, 1, 1}};

// distance of source u of cell (l, m, n) in the reference's statement order
__device__ __forceinline__ double ism_distance(const IsmArgs& p, int l, int m, int n, int u) {
#pragma clang fp contract(off)
    const int lv[3] = {l, m, n};
    double sq[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double pos = (double)(1 - 2 * U[u][a]) * p.s[a] + (double)(2 * lv[a]) * p.dim[a] - p.r[a];
        sq[a] = pos * pos;
    }
    return sqrt((sq[0] + sq[1]) + sq[2]);
}

// int(d / c * sr + 0.5); the host has checked that it stays below the reference's buffer length (< 2^31)
__device__ __forceinline__ int64_t ism_bin(const IsmArgs& p, double d) {
#pragma clang fp contract(off)
    return (int64_t)(d / p.c * p.sr + 0.5);
}

// the bins of a cell's eight sources; -1 for one that a later source of the cell replaces or that lies beyond n_out
__device__ __forceinline__ void ism_cell_bins(const IsmArgs& p, int l, int m, int n, int64_t* bin) {
#pragma unroll
    for (int u = 0; u < 8; ++u) bin[u] = ism_bin(p, ism_distance(p, l, m, n, u));
    // ascending u: a source is compared with the later ones only, whose bins are still intact when it is
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        bool kept = bin[u] < p.n_out;
#pragma unroll
        for (int v = u + 1; v < 8; ++v) kept = kept && bin[v] != bin[u];
        if (!kept) bin[u] = -1;
    }
}

// cell number -> (l, m, n); false beyond the slab
__device__ __forceinline__ bool ism_cell(const IsmArgs& p, int64_t cell, int* l, int* m, int* n) {
    const int S = 2 * p.limit + 1;
    if (cell >= (int64_t)(p.l1 - p.l0) * S * S) return false;
    *n = (int)(cell % S) - p.limit;
    *m = (int)(cell / S % S) - p.limit;
    *l = (int)(cell / ((int64_t)S * S)) + p.l0 - p.limit;
    return true;
}

__global__ __launch_bounds__(NT) void k_ism_count(IsmArgs p) {
    const int64_t cell = (int64_t)blockIdx.x * NT + threadIdx.x;
    int l, m, n;
    if (!ism_cell(p, cell, &l, &m, &n)) return;
    int64_t bin[8];
    ism_cell_bins(p, l, m, n, bin);
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if (bin[u] >= 0) atomicAdd(&p.count[bin[u]], 1u);
}

__global__ __launch_bounds__(NT) void k_ism_fill(IsmArgs p) {
    const int64_t cell = (int64_t)blockIdx.x * NT + threadIdx.x;
    int l, m, n;
    if (!ism_cell(p, cell, &l, &m, &n)) return;
    int64_t bin[8];
    ism_cell_bins(p, l, m, n, bin);
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if (bin[u] >= 0) p.list[atomicAdd(&p.cursor[bin[u]], 1u)] = (uint32_t)(cell * 8 + u);
}

// count[0 .. n] (n = n_out; count[n] is spare) -> exclusive prefix sums in count and cursor, by one workgroup
__global__ __launch_bounds__(SCAN_NT) void k_ism_scan(IsmArgs p) {
    uint32_t* count = p.count;
    uint32_t* cursor = p.cursor;
    const int64_t n = p.n_out;
    __shared__ uint32_t wave_total[SCAN_NT / 64];
    __shared__ uint32_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base <= n; base += (int64_t)SCAN_NT * SCAN_PER) {
        const int64_t i0 = base + (int64_t)tid * SCAN_PER;
        uint32_t v[SCAN_PER], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_PER; ++k) {
            v[k] = i0 + k < n ? count[i0 + k] : 0u;  // count[n] itself is not a bin: it receives the total
            sum += v[k];
        }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        uint32_t run = before + incl - sum;
#pragma unroll
        for (int k = 0; k < SCAN_PER; ++k) {
            if (i0 + k <= n) {
                count[i0 + k] = run;
                cursor[i0 + k] = run;
            }
            run += v[k];
        }
        __syncthreads();
        if (tid == SCAN_NT - 1) carry_s = run;
        __syncthreads();
    }
}

// ascending bitonic sort of key[0 .. n), n a power of two, by the whole workgroup
__device__ __forceinline__ void ism_sort(uint32_t* key, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += NT) {
                const int q = i ^ j;
                if (q > i) {
                    const uint32_t a = key[i], b = key[q];
                    if ((a > b) == ((i & k) == 0)) {
                        key[i] = b;
                        key[q] = a;
                    }
                }
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void k_ism_sum(IsmArgs p) {
    __shared__ uint32_t key[SORT_CAP];
    __shared__ double term[MAX_BANDS][TILE];
    __shared__ int n_in;
    const int tid = threadIdx.x;
    const int64_t bin = blockIdx.x;
    const uint32_t seg0 = p.count[bin], seg1 = p.count[bin + 1];
    const int64_t count = (int64_t)seg1 - seg0;
    if (count == 0) return;
    const int S = 2 * p.limit + 1, T = p.limit + 2;
    const int64_t span = (int64_t)(p.l1 - p.l0) * S * S * 8;  // ids of the slab: 0 .. span
    double acc = tid < p.n_band ? p.out[(int64_t)tid * p.n_out + bin] : 0.0;
    int64_t lo = 0, width = span;
    while (lo < span) {
        const int64_t hi = lo + width < span ? lo + width : span;
        // the segment's ids in [lo, hi) go to LDS, if there are at most SORT_CAP of them
        if (tid == 0) n_in = 0;
        __syncthreads();
        if (count > SORT_CAP) {
            int mine = 0;
            for (int64_t i = tid; i < count; i += NT) {
                const uint32_t id = p.list[seg0 + i];
                mine += id >= lo && id < hi;
            }
            if (mine) atomicAdd(&n_in, mine);
            __syncthreads();
            const int total = n_in;
            __syncthreads();
            if (total > SORT_CAP) {  // ids are distinct, so a range of one id always fits
                width = (width + 1) / 2;
                continue;
            }
            if (tid == 0) n_in = 0;
            __syncthreads();
        }
        for (int64_t i = tid; i < count; i += NT) {
            const uint32_t id = p.list[seg0 + i];
            if (id >= lo && id < hi) key[atomicAdd(&n_in, 1)] = id;
        }
        __syncthreads();
        const int m_in = n_in;
        int pow2 = 1;
        while (pow2 < m_in) pow2 <<= 1;
        for (int i = m_in + tid; i < pow2; i += NT) key[i] = ID_PAD;
        ism_sort(key, pow2);  // begins and ends with a barrier
        for (int t0 = 0; t0 < m_in; t0 += TILE) {
            const int here = m_in - t0 < TILE ? m_in - t0 : TILE;
            if (tid < here) {
#pragma clang fp contract(off)
                const uint32_t id = key[t0 + tid];
                const int u = id & 7;
                int l, m, n;
                ism_cell(p, id >> 3, &l, &m, &n);
                const double d = ism_distance(p, l, m, n, u);
                const double spread = 4.0 * 3.141592653589793 * d;
                const int k1[3] = {abs(l - U[u][0]), abs(m - U[u][1]), abs(n - U[u][2])};
                const int k2[3] = {abs(l), abs(m), abs(n)};
                for (int b = 0; b < p.n_band; ++b) {
                    const double* w = p.pw + (int64_t)b * 6 * T;
                    const double d1 = (w[k1[0]] * w[T + k1[1]]) * w[2 * T + k1[2]];
                    const double d2 = (w[3 * T + k2[0]] * w[4 * T + k2[1]]) * w[5 * T + k2[2]];
                    term[b][tid] = d1 * d2 / spread;
                }
            }
            __syncthreads();
            if (tid < p.n_band)
                for (int i = 0; i < here; ++i) acc += term[tid][i];
            __syncthreads();
        }
        lo = hi;
    }
    if (tid < p.n_band) p.out[(int64_t)tid * p.n_out + bin] = acc;
}

struct ModalArgs {
    const double* omega_n;  // [n_modes], the reference's loop order
    const double* eta;      // [n_modes]
    const double* weight;   // [n_modes]: prod(cos(k s) cos(k r)) / cn
    int64_t n_modes;
    const double* omega2;   // [n_freq]: omega_f^2
    int64_t n_freq;
    double2* p;             // [n_freq]
};

__global__ __launch_bounds__(MODAL_NT) void k_modal_tf(ModalArgs q) {
    const int64_t f = (int64_t)blockIdx.x * MODAL_NT + threadIdx.x;
    if (f >= q.n_freq) return;
    const double w2 = q.omega2[f];
    double re = 0.0, im = 0.0;
    for (int64_t n = 0; n < q.n_modes; ++n) {
        // the table's entries are the same for every lane: scalar loads
        const double on = q.omega_n[n], a = fma(on, on, -w2), b = 2.0 * q.eta[n] * on;
        const double g = q.weight[n] / fma(a, a, b * b);  // w / (a + jb) = w (a - jb) / (a^2 + b^2)
        re += g * a;
        im -= g * b;
    }
    q.p[f] = make_double2(re, im);
}

}  // namespace dsroom
