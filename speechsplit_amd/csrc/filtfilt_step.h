// scipy.signal.filtfilt for a 6-coefficient filter as an exact sequence of IEEE double operations (internal; filtfilt.hip).  The
// reference's 5th-order 30 Hz Butterworth high-pass has its poles at |z| = 0.988 .. 0.996 and scipy runs it in direct form, which is
// ill-conditioned there: ANY other arrangement of the arithmetic (sections, a scan, a fused multiply-add) lands ~3e-7 of max |y| away
// from scipy, and the mel spectrogram moves by more than the project's 1e-6.  So every product and every sum below is
// rounded on its own, in scipy's order (lfilter's transposed direct form II loop), and the result is scipy's to the bit.  Every
// function switches contraction off for its own body; they are __host__ __device__ so that a host program can hold them against scipy without a GPU.
#pragma once
#include "common.h"
#include "kernels.h"

namespace ss {

// sample j of the odd extension of x [n] by FILT_PAD at both ends, j in [0, n + 2 FILT_PAD); needs n > FILT_PAD
__host__ __device__ inline double filt_ext(const double* __restrict__ x, int n, int j) {
#pragma clang fp contract(off)
    const int i = j - FILT_PAD;
    if (i < 0) return 2.0 * x[0] - x[-i];
    if (i < n) return x[i];
    return 2.0 * x[n - 1] - x[2 * (n - 1) - i];
}

// one step from the six products p_i = b_i u: y = p0 + z0; z_i = (p_{i+1} + z_{i+1}) - a_{i+1} y; z4 = p5 - a5 y.  This is the DEFINITION of a
// step (and what a host program runs); the kernel makes the same operations with one state a lane (filtfilt.hip, filt_step_lanes).
__host__ __device__ inline double filt_step_products(const double* __restrict__ p, const double* __restrict__ a, double* __restrict__ z) {
#pragma clang fp contract(off)
    const double y = p[0] + z[0];
#pragma unroll
    for (int i = 0; i < FILT_NCOEF - 2; ++i) {
        const double t = p[i + 1] + z[i + 1];
        const double m = a[i + 1] * y;
        z[i] = t - m;
    }
    z[FILT_NCOEF - 2] = p[FILT_NCOEF - 1] - a[FILT_NCOEF - 1] * y;
    return y;
}

__host__ __device__ inline void filt_products(const FiltCoef& c, double u, double* __restrict__ p) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < FILT_NCOEF; ++i) p[i] = c.b[i] * u;
}

__host__ __device__ inline void filt_start(const FiltCoef& c, double u0, double* __restrict__ z) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < FILT_NCOEF - 1; ++i) z[i] = c.zi[i] * u0;
}

// make_spect_f0.py:54-55: y * gain + (r - 0.5) * dither_scale, r the host's prng.rand value (nullptr: no dither)
__host__ __device__ inline double filt_epilogue(double y, double gain, const double* __restrict__ r, double dither_scale) {
#pragma clang fp contract(off)
    const double g = y * gain;
    if (!r) return g;
    const double d = *r - 0.5;
    const double e = d * dither_scale;
    return g + e;
}

}  // namespace ss
