// What the Welch kernel families (1024, 2048h, 4096, 8192, 16384, long) share: small device helpers, one definition
// each.  The families pull them in with `using`; their kernels, Args types and launch geometry stay their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_lds.hpp"

namespace welchc {

using dsfft::cmul;   // (fma form: a.x b.x - a.y b.y, a.x b.y + a.y b.x)
using dsfft::pos16;  // register of output k of a 16-point DFT
// (dft16 is NOT shared: dsfft::dft16<INV> multiplies by W16^2 as two fmas, welch4096::dft16 as add then multiply)

// order the LDS traffic of ONE wave (hardware executes it in program order; this keeps the
// compiler from moving a read above the write of another lane it cannot see)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the last pair of an odd frame count when frame F would still overlap the signal: its second frame is dropped
template <typename A>
__device__ __forceinline__ bool needs_drop(const A& p, int pr) {
    return pr == p.n_pairs - 1 && (p.n_frames & 1) && (int64_t)p.n_frames * p.hop < p.n_samples;
}

// padded position of bin k in a fold image (stride-16 bins of neighbouring lanes -> 17)
__device__ __forceinline__ int fold_pos(int k) { return k + (k >> 4); }

// Windows of R x 4096 samples split into R classes (bin R k' + r is bin k' of class r): the fold partner N - k of that
// bin lies in class (R - r) mod R, at index
__device__ __forceinline__ int fold_index(int r, int kp) { return r == 0 ? ((4096 - kp) & 4095) : (4095 - kp); }

// psx[q][cx][k] = sum over the pairs [p0, p1) of chunk q of px[cx][pair][k] (fp64), k < NB.  One workgroup of 256.
template <int NB, typename A>
__device__ __forceinline__ void px_sum(const A& p, int q, int cx, int p0, int p1) {
    const float* __restrict__ px = p.px + (int64_t)cx * p.n_pairs * NB;
    for (int k = threadIdx.x; k < NB; k += 256) {
        double sum = 0.0;
        for (int pr = p0; pr < p1; ++pr) sum += (double)px[(int64_t)pr * NB + k];
        p.psx[((int64_t)q * p.n_cx + cx) * NB + k] = (float)sum;
    }
}

// The same sum over unfolded class images pxu[cx][pair][r][k'] of R = 1 << lgR classes, folded on the way:
// psx[cq][cx][k] = sum of (|W[k]|^2 + |W[N - k]|^2) / 2, one thread per bin.  grid = (ceil(nb / 256), n_chunks, n_cx)
template <typename A>
__device__ __forceinline__ void px_sum_folded(const A& p, int R, int lgR) {
    constexpr int M = 4096;
    const int nb = R * (M / 2) + 1, N = R * M;
    const int k = blockIdx.x * 256 + threadIdx.x, cq = blockIdx.y, cx = blockIdx.z;
    if (k >= nb) return;
    const int p0 = (int)((int64_t)cq * p.n_pairs / p.n_chunks), p1 = (int)((int64_t)(cq + 1) * p.n_pairs / p.n_chunks);
    const float* __restrict__ pxu = p.pxu + (int64_t)cx * p.n_pairs * N;
    const int r = k & (R - 1), kp = (k >> lgR) & (M - 1), rm = (R - r) & (R - 1);
    const int ia = r * M + kp, ib = rm * M + fold_index(r, kp);
    double sum = 0.0;
    for (int pr = p0; pr < p1; ++pr) sum += (double)pxu[(int64_t)pr * N + ia] + (double)pxu[(int64_t)pr * N + ib];
    p.psx[((int64_t)cq * p.n_cx + cx) * nb + k] = (float)(0.5 * sum);
}

}  // namespace welchc
