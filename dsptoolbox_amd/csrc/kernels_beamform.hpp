// Gridded frequency-domain beamformers beyond delay-and-sum (beamforming/beamforming.py:883-1314 of the
// reference), float64 throughout.  Three kernels, one bin per workgroup where a bin's matrix must be whole:
//
//   k_bf_eigh      Hermitian eigendecomposition of every bin's CSM (C <= 64): cyclic complex Jacobi in the
//                  parallel (round-robin) ordering, matrix and eigenvectors in LDS.  Eigenvalues ascending, as
//                  numpy's eigh; the lower triangle is what is read, as eigh does.
//   k_bf_project   P[g][k] = |v_k^H h_g|^2 for every grid point, reduced on the spot to the MVDR
//                  (1 / sum_k P / lambda_k) or Functional (sum_k P sign(lambda_k)|lambda_k|^(1/gamma), then
//                  (q / n)^gamma n) map, or stored for the leading n_eig eigenvectors (Orthogonal).
//   k_bf_orth_pick Orthogonal's per-bin argmax-and-assign, in eigenvalue order (a later pick overwrites).
//   k_bf_cleansc   CLEAN-SC's whole deconvolution loop for one bin (_beamforming.py:194-297): D in LDS, the
//                  steering vectors streamed from HBM, the residual map in a workspace row owned thread by thread.
//
// Layouts: csm [bin][i][j] complex128, h [bin][i][g] complex128, map [g][bin] float64.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>

namespace bf {

constexpr int MAX_CH = 64;        // one bin's C x C complex128 matrix (64 KiB) lives in LDS
constexpr int THREADS = 256;
constexpr int LD = MAX_CH + 1;    // LDS row stride of the Jacobi matrices
constexpr int VLD = MAX_CH + 16;  // k_bf_project: 16-column chunks may run past C (zero columns)
constexpr int MAX_SWEEPS = 40;    // Jacobi: 6-8 sweeps at C = 64 on random matrices
constexpr int FIXED_POINT_STEPS = 20;  // CLEAN-SC's h_ iteration (the reference follows acoular)

enum Method { MVDR = 0, FUNCTIONAL = 1, ORTHOGONAL = 2 };

__device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline double2 cmulc(double2 a, double2 b) {  // conj(a) * b
    return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}
__device__ inline double2 conjd(double2 a) { return make_double2(a.x, -a.y); }
__device__ inline double abs2(double2 a) { return a.x * a.x + a.y * a.y; }

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// numpy's argmax order: the first NaN wins, then the largest value, then the lowest index
__device__ inline bool better(double va, int ia, double vb, int ib) {
    const bool na = isnan(va), nb = isnan(vb);
    if (na != nb) return na;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}
// block-wide (value, index) argmax; every thread gets the winner.  red_v / red_i: THREADS / 64 slots.
__device__ inline void block_argmax(double& v, int& idx, double* red_v, int* red_i) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(idx, o);
        if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();  // the slots may still be read from the previous call
    if ((threadIdx.x & 63) == 0) { red_v[w] = v; red_i[w] = idx; }
    __syncthreads();
    v = red_v[0];
    idx = red_i[0];
    for (int k = 1; k < THREADS / 64; ++k)
        if (better(red_v[k], red_i[k], v, idx)) { v = red_v[k]; idx = red_i[k]; }
}
__device__ inline double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < THREADS / 64; ++k) s += red[k];
    return s;
}
__device__ inline double block_max(double v, double* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = red[0];
    for (int k = 1; k < THREADS / 64; ++k) m = fmax(m, red[k]);
    return m;
}

// ---- eigendecomposition ------------------------------------------------------------------
struct EighArgs {
    const double2* a;  // [bin][n][n]
    int n;
    double* w;    // [bin][n] ascending
    double2* v;   // [bin][n][n], column k = eigenvector of w[k]
};

// round-robin schedule on m (even) indices: index 0 stays, the others rotate; round r, pair k
__device__ inline void rr_pair(int r, int k, int m, int& p, int& q) {
    auto pos = [&](int j) { return j == 0 ? 0 : 1 + (j - 1 + r) % (m - 1); };
    p = pos(k);
    q = pos(m - 1 - k);
}

__global__ __launch_bounds__(THREADS) void k_bf_eigh(EighArgs p) {
    __shared__ double2 A[MAX_CH * LD];
    __shared__ double2 V[MAX_CH * LD];
    __shared__ double rc[MAX_CH / 2];
    __shared__ double2 rs[MAX_CH / 2];
    __shared__ int rp[MAX_CH / 2], rq[MAX_CH / 2];
    __shared__ double red[THREADS / 64];
    __shared__ int rank[MAX_CH];
    const int n = p.n, t = threadIdx.x, b = blockIdx.x;
    const double2* a = p.a + (size_t)b * n * n;
    double amax = 0.0;
    for (int e = t; e < n * n; e += THREADS) {
        const int i = e / n, j = e - i * n;
        double2 x = i >= j ? a[e] : conjd(a[j * n + i]);  // the lower triangle, as eigh (UPLO='L')
        if (i == j) x.y = 0.0;
        amax = fmax(amax, fmax(fabs(x.x), fabs(x.y)));
        A[i * LD + j] = x;
        V[i * LD + j] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    }
    // scale by 2^-ex so that the largest |entry| is in [0.5, 1): exact, and the sums of squares below neither
    // overflow nor go subnormal (as LAPACK scales before eigh); the eigenvalues are scaled back on output
    int ex = 0;
    amax = block_max(amax, red);
    if (amax > 0.0 && amax <= DBL_MAX) frexp(amax, &ex);
    if (ex != 0)
        for (int e = t; e < n * n; e += THREADS) {
            double2& x = A[(e / n) * LD + e % n];
            x = make_double2(ldexp(x.x, -ex), ldexp(x.y, -ex));
        }
    __syncthreads();
    double fro2 = 0.0;
    for (int e = t; e < n * n; e += THREADS) fro2 += abs2(A[(e / n) * LD + e % n]);
    const double skip = 1e-18 * sqrt(block_sum(fro2, red));  // rotations below this change nothing
    const int m = n + (n & 1), np = m / 2;  // odd n: one dummy index, its pairs rest
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        double off = 0.0, tot = 0.0;
        for (int e = t; e < n * n; e += THREADS) {
            const int i = e / n, j = e - i * n;
            const double x = abs2(A[i * LD + j]);
            tot += x;
            if (i != j) off += x;
        }
        off = block_sum(off, red);
        tot = block_sum(tot, red);
        if (!(off > 4.9e-32 * tot)) break;  // (2^-52)^2: the off-diagonal part is below rounding
        for (int r = 0; r < m - 1; ++r) {
            if (t < np) {
                int pp, qq;
                rr_pair(r, t, m, pp, qq);
                double c = 1.0;
                double2 s = make_double2(0.0, 0.0);
                if (pp < n && qq < n) {
                    const double ap = A[pp * LD + pp].x, aq = A[qq * LD + qq].x;
                    const double2 bpq = A[pp * LD + qq];
                    const double ab = sqrt(abs2(bpq));
                    if (ab > skip) {
                        // J = [[c, s e^{i phi}], [-s e^{-i phi}, c]] zeroes the (p, q) entry of J^H A J
                        const double th = (aq - ap) / (2.0 * ab);
                        const double tt = fabs(th) < 1e100 ? (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0))
                                                           : 0.5 / th;
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        const double sn = tt * c;
                        s = make_double2(sn * bpq.x / ab, sn * bpq.y / ab);
                    }
                } else {
                    pp = qq = -1;
                }
                rc[t] = c;
                rs[t] = s;
                rp[t] = pp;
                rq[t] = qq;
            }
            __syncthreads();
            // A <- A J (columns p, q of every pair)
            for (int e = t; e < n * np; e += THREADS) {
                const int k = e / n, i = e - k * n;
                const int pp = rp[k], qq = rq[k];
                if (pp < 0) continue;
                const double c = rc[k];
                const double2 s = rs[k];
                const double2 xp = A[i * LD + pp], xq = A[i * LD + qq];
                const double2 sq = cmulc(s, xq);  // conj(s) xq
                const double2 ps = cmul(xp, s);
                A[i * LD + pp] = make_double2(c * xp.x - sq.x, c * xp.y - sq.y);
                A[i * LD + qq] = make_double2(ps.x + c * xq.x, ps.y + c * xq.y);
            }
            __syncthreads();
            // A <- J^H A (rows p, q), V <- V J
            for (int e = t; e < n * np; e += THREADS) {
                const int k = e / n, j = e - k * n;
                const int pp = rp[k], qq = rq[k];
                if (pp < 0) continue;
                const double c = rc[k];
                const double2 s = rs[k];
                const double2 xp = A[pp * LD + j], xq = A[qq * LD + j];
                const double2 sq = cmul(s, xq);
                const double2 sp = cmulc(s, xp);  // conj(s) xp
                A[pp * LD + j] = j == qq ? make_double2(0.0, 0.0) : make_double2(c * xp.x - sq.x, c * xp.y - sq.y);
                A[qq * LD + j] = j == pp ? make_double2(0.0, 0.0) : make_double2(sp.x + c * xq.x, sp.y + c * xq.y);
                const double2 vp = V[j * LD + pp], vq = V[j * LD + qq];
                const double2 vs = cmulc(s, vq);
                const double2 ps = cmul(vp, s);
                V[j * LD + pp] = make_double2(c * vp.x - vs.x, c * vp.y - vs.y);
                V[j * LD + qq] = make_double2(ps.x + c * vq.x, ps.y + c * vq.y);
            }
            __syncthreads();
        }
    }
    // ascending order (stable on ties, as argsort would place equal values)
    if (t < n) {
        const double lt = A[t * LD + t].x;
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const double lj = A[j * LD + j].x;
            r += (lj < lt) || (lj == lt && j < t);
        }
        rank[t] = r;
        p.w[(size_t)b * n + r] = ldexp(lt, ex);
    }
    __syncthreads();
    double2* vo = p.v + (size_t)b * n * n;
    for (int e = t; e < n * n; e += THREADS) {
        const int i = e / n, k = e - i * n;
        vo[i * n + rank[k]] = V[i * LD + k];
    }
}

// ---- projection |V^H h|^2 and the per-method reduction --------------------------------------
struct ProjArgs {
    const double* w;    // [bin][n]
    const double2* v;   // [bin][n][n]
    const double2* h;   // [bin][n][G]
    int n, n_grid, n_bins, method, n_eig;
    double gamma;
    double* map;        // MVDR / Functional: [G][bins]
    double* proj;       // Orthogonal: [bin][e][G], e = 0 the largest eigenvalue
};

__global__ __launch_bounds__(THREADS) void k_bf_project(ProjArgs p) {
    __shared__ double2 Vs[MAX_CH * VLD];
    __shared__ double coef[VLD];
    const int n = p.n, G = p.n_grid, b = blockIdx.y, t = threadIdx.x;
    const double2* v = p.v + (size_t)b * n * n;
    for (int e = t; e < MAX_CH * VLD; e += THREADS) {
        const int i = e / VLD, k = e - i * VLD;
        Vs[e] = (i < n && k < n) ? v[i * n + k] : make_double2(0.0, 0.0);
    }
    for (int k = t; k < VLD; k += THREADS) {
        double cf = 0.0;
        if (k < n) {
            const double lam = p.w[(size_t)b * n + k];
            if (p.method == MVDR) cf = 1.0 / lam;
            else if (p.method == FUNCTIONAL) cf = (lam < 0.0 ? -1.0 : 1.0) * pow(fabs(lam), 1.0 / p.gamma);
        }
        coef[k] = cf;
    }
    __syncthreads();
    const int g = blockIdx.x * THREADS + t;
    if (g >= G) return;
    const double2* hg = p.h + (size_t)b * n * G + g;
    const int k0 = p.method == ORTHOGONAL ? n - p.n_eig : 0;
    double acc_map = 0.0, hn = 0.0;
    for (int kc = k0; kc < n; kc += 16) {
        double2 acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = make_double2(0.0, 0.0);
        for (int i = 0; i < n; ++i) {
            const double2 hv = hg[(size_t)i * G];
            if (kc == k0) hn += abs2(hv);
            const double2* vr = Vs + i * VLD + kc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double2 x = cmulc(hv, vr[r]);  // conj(h_i) v_ik
                acc[r].x += x.x;
                acc[r].y += x.y;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = kc + r;
            const double P = abs2(acc[r]);
            if (k < n && p.method == ORTHOGONAL) p.proj[((size_t)b * p.n_eig + (n - 1 - k)) * G + g] = P;
            else acc_map += P * coef[k];  // coef is 0 past n
        }
    }
    if (p.method == MVDR) p.map[(size_t)g * p.n_bins + b] = 1.0 / acc_map;
    else if (p.method == FUNCTIONAL) p.map[(size_t)g * p.n_bins + b] = pow(acc_map / hn, p.gamma) * hn;
}

// Orthogonal: for e = 0 .. n_eig - 1, i = argmax_g P[e][g], map[i] = P[e][i] * lambda_(n-1-e) -- an assignment
__global__ __launch_bounds__(THREADS) void k_bf_orth_pick(ProjArgs p) {
    __shared__ double red_v[THREADS / 64];
    __shared__ int red_i[THREADS / 64];
    const int G = p.n_grid, b = blockIdx.x, t = threadIdx.x;
    for (int g = t; g < G; g += THREADS) p.map[(size_t)g * p.n_bins + b] = 0.0;
    __syncthreads();
    for (int e = 0; e < p.n_eig; ++e) {
        const double* row = p.proj + ((size_t)b * p.n_eig + e) * G;
        double v = -INFINITY;
        int idx = INT_MAX;
        for (int g = t; g < G; g += THREADS)
            if (better(row[g], g, v, idx)) { v = row[g]; idx = g; }
        block_argmax(v, idx, red_v, red_i);
        if (t == 0) p.map[(size_t)idx * p.n_bins + b] = v * p.w[(size_t)b * p.n + p.n - 1 - e];
    }
}

// ---- CLEAN-SC ------------------------------------------------------------------------------
struct CleanArgs {
    const double2* csm;  // [bin][n][n]
    const double2* h;    // [bin][n][G]
    int n, n_grid, n_bins, max_iter, remove_diag;
    double safety;
    double* resid;       // workspace [bin][G]: the dirty map being cleaned
    double* map;         // [G][bins]: the clean map
};

__device__ inline double l1_norm(const double2* D, int n, double* red) {  // largest column sum of |D|
    double cs = 0.0;
    if (threadIdx.x < n)
        for (int i = 0; i < n; ++i) cs += sqrt(abs2(D[i * LD + threadIdx.x]));
    if (threadIdx.x < 64) {
        cs = wave_max(cs);
        if (threadIdx.x == 0) red[0] = cs;
    }
    __syncthreads();
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(THREADS) void k_bf_cleansc(CleanArgs p) {
    __shared__ double2 D[MAX_CH * LD];
    __shared__ double2 wmax[MAX_CH], dw[MAX_CH], hc[MAX_CH];
    __shared__ double red_v[THREADS / 64];
    __shared__ int red_i[THREADS / 64];
    const int n = p.n, G = p.n_grid, nb = p.n_bins, b = blockIdx.x, t = threadIdx.x;
    const double s = p.safety;
    const double2* a = p.csm + (size_t)b * n * n;
    for (int e = t; e < MAX_CH * MAX_CH; e += THREADS) {
        const int i = e / MAX_CH, j = e - i * MAX_CH;
        double2 x = make_double2(0.0, 0.0);
        if (i < n && j < n && !(p.remove_diag && i == j)) x = a[i * n + j];
        D[i * LD + j] = x;
    }
    const double2* hb = p.h + (size_t)b * n * G;
    double* r = p.resid + (size_t)b * G;
    __syncthreads();
    // the dirty map Re(h^H D h), D h in 16-row chunks (rows past n are zero)
    for (int g = t; g < G; g += THREADS) {
        p.map[(size_t)g * nb + b] = 0.0;
        double q = 0.0;
        for (int ic = 0; ic < n; ic += 16) {
            double2 acc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = make_double2(0.0, 0.0);
            for (int j = 0; j < n; ++j) {
                const double2 hv = hb[(size_t)j * G + g];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const double2 x = cmul(D[(ic + k) * LD + j], hv);
                    acc[k].x += x.x;
                    acc[k].y += x.y;
                }
            }
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (ic + k < n) q += cmulc(hb[(size_t)(ic + k) * G + g], acc[k]).x;
        }
        r[g] = q;
    }
    double norm_cur = l1_norm(D, n, red_v);  // l1_norm ends on a barrier: the map zeros are visible too
    double norm_prev = 2.0 * norm_cur;      // the reference's D[0] = 2 CSM
    for (int it = 0; it < p.max_iter; ++it) {
        double pw = -INFINITY;
        int idx = INT_MAX;
        for (int g = t; g < G; g += THREADS)
            if (better(r[g], g, pw, idx)) { pw = r[g]; idx = g; }
        block_argmax(pw, idx, red_v, red_i);
        if (t == 0) p.map[(size_t)idx * nb + b] += pw * s;
        if (norm_cur >= norm_prev) break;
        if (t < n) wmax[t] = hb[(size_t)t * G + idx];
        __syncthreads();
        if (t < n) {
            double2 acc = make_double2(0.0, 0.0);
            for (int j = 0; j < n; ++j) {
                const double2 x = cmul(D[t * LD + j], wmax[j]);
                acc.x += x.x;
                acc.y += x.y;
            }
            dw[t] = make_double2(acc.x / pw, acc.y / pw);
        }
        __syncthreads();
        if (t < 64) {  // the fixed point for h_, one lane per microphone
            const bool on = t < n;
            const double2 wv = on ? wmax[t] : make_double2(0.0, 0.0);
            const double2 dv = on ? dw[t] : make_double2(0.0, 0.0);
            const double w2 = abs2(wv);
            double2 hv = wv;
            for (int k = 0; k < FIXED_POINT_STEPS; ++k) {
                const double H = abs2(hv);
                const double den = sqrt(1.0 + wave_sum(on ? H * w2 : 0.0));
                hv = make_double2((dv.x + H * wv.x) / den, (dv.y + H * wv.y) / den);
            }
            if (on) hc[t] = hv;
        }
        __syncthreads();
        // dirty map -= s Re(h^H G h), G = pw h_ h_^H (diagonal zeroed if asked)
        for (int g = t; g < G; g += THREADS) {
            double2 y = make_double2(0.0, 0.0);
            double dg = 0.0;
            for (int i = 0; i < n; ++i) {
                const double2 hv = hb[(size_t)i * G + g];
                const double2 x = cmulc(hv, hc[i]);
                y.x += x.x;
                y.y += x.y;
                if (p.remove_diag) dg += abs2(hv) * abs2(hc[i]);
            }
            r[g] -= (pw * abs2(y) - pw * dg) * s;
        }
        // D -= s G
        for (int e = t; e < n * n; e += THREADS) {
            const int i = e / n, j = e - i * n;
            if (p.remove_diag && i == j) continue;
            const double2 gij = cmulc(hc[j], hc[i]);  // h_i conj(h_j)
            D[i * LD + j].x -= s * (gij.x * pw);
            D[i * LD + j].y -= s * (gij.y * pw);
        }
        __syncthreads();
        norm_prev = norm_cur;
        norm_cur = l1_norm(D, n, red_v);
    }
}

}  // namespace bf
