// What the float64 transforms share (kernels_welch_f64.hpp, kernels_fft64.hpp): the twiddle table and the radix-2
// stages that run on double2 values in LDS.  gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace f64c {

// tw[k] = exp(-2 pi i k / W), k < half = W / 2.  grid = ceil(half / 256)
__global__ __launch_bounds__(256) void k_twiddles(double2* tw, int half) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= half) return;
    double s, c;
    sincospi(-(double)k / (double)half, &s, &c);
    tw[k] = make_double2(c, s);
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// Radix-2 decimation in time over buf[0 .. M), M = 2^lg, bit-reversed order in, natural order out, 256 lanes.
// exp(-2 pi i k / M) = tw[k * tstep]; INV takes the conjugate twiddles (the unnormalised inverse).  Every stage ends
// with a barrier; the caller places one between its own writes to buf and this.
template <bool INV = false>
__device__ __forceinline__ void radix2_lds(double2* buf, int M, int lg, const double2* __restrict__ tw, int tstep, int tid) {
    for (int s = 0; s < lg; ++s) {
        const int half = 1 << s;
        for (int i = tid; i < M / 2; i += 256) {
            const int j = i & (half - 1), a = ((i >> s) << (s + 1)) + j, b = a + half;
            double2 w = tw[(size_t)(j << (lg - 1 - s)) * tstep];
            if (INV) w.y = -w.y;
            const double2 u = buf[a], v = buf[b];
            const double2 t = make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            buf[a] = make_double2(u.x + t.x, u.y + t.y);
            buf[b] = make_double2(u.x - t.x, u.y - t.y);
        }
        __syncthreads();
    }
}

}  // namespace f64c
