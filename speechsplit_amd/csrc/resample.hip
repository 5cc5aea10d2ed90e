// ss_resample: scipy.signal.resample_poly(x, up, down) with a caller-supplied FIR h, on ragged batches.  include/speechsplit_amd.h states
// the definition: y[m] = 0.0 + sum_k x[k] h[m down + half - k up], k ascending, every product and every sum rounded to double on its own.
// That is scipy's polyphase loop written out, and the result equals scipy's to the bit; any other order of the sum does not.
//
// One workgroup per (tile of RS_TILE outputs, row); one thread per output, which runs its own taps in order.  Nothing crosses threads, so a
// row is what it would be alone whatever else is in the batch.  The work is bound by memory traffic (8 bytes read a sample, 8 written an
// output), so the row's input span for the tile is staged once in LDS: a tile at 1/3 reads 826 samples, 3.2 for each output, where its 256
// threads would otherwise fetch 61 each.  The taps stay where they are: at iteration j the lanes of a wavefront read h[j up + phase], phase
// < up, i.e. one stretch of at most `up` doubles -- h as given is already the layout that coalesces across lanes, and it lives in L2
// (8821 doubles at 160/441, 12801 at 640/441: too big to sit in LDS beside the span at full occupancy).  No image of h is built and no scratch
// is needed.  Ratios whose span outgrows the LDS array (down / up above ~7: a tile at 1/16 spans 4400 samples) read x from global memory.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ss {

namespace {

constexpr int RS_TILE = 256;     // outputs a workgroup, one a thread
constexpr int RS_SPAN = 2048;    // doubles of x a tile may stage (16 KB of LDS)

// input samples a tile of RS_TILE outputs can touch, at most: (t_last - (t_first - (n_taps - 1))) / up + 2
long resample_span(int up, int down, int n_taps) { return ((long)(RS_TILE - 1) * down + (n_taps - 1)) / up + 2; }

// grid = (ceil(M / RS_TILE), B), block = RS_TILE.  x [B][max_n], h [n_taps], y [B][M].
template <bool STAGED>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const double* __restrict__ x, const int* __restrict__ n, int max_n, long M, int up,
                                                           int down, const double* __restrict__ h, int n_taps, double* __restrict__ y) {
    __shared__ double xs[STAGED ? RS_SPAN : 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nraw = n ? n[b] : max_n;
    const long nb = nraw < 1 ? 1 : (nraw > max_n ? max_n : nraw);
    const long mb = (nb * up + down - 1) / down;                       // the row's own outputs
    const long m0 = (long)blockIdx.x * RS_TILE, m = m0 + tid;
    const long half = (n_taps - 1) / 2;
    const double* __restrict__ xr = x + (long)b * max_n;
    double* __restrict__ yr = y + (long)b * M;
    if (m0 >= mb) {                                                    // a tile behind the row: zeros only
        if (m < M) yr[m] = 0.0;
        return;
    }
    // the tile's input span [k0, k1]: the first tap of its first output to the last tap of its last, inside [0, nb)
    const long m1 = (m0 + RS_TILE < mb ? m0 + RS_TILE : mb) - 1;
    const long lo = m0 * down + half - (n_taps - 1);
    const long k0 = lo <= 0 ? 0 : (lo + up - 1) / up;
    const long k1t = (m1 * down + half) / up, k1 = k1t < nb - 1 ? k1t : nb - 1;
    if (STAGED) {
        for (long k = k0 + tid; k <= k1; k += RS_TILE) xs[k - k0] = xr[k];
        __syncthreads();
    }
    if (m >= M) return;
    double acc = 0.0;
    if (m < mb) {
        // tap index t - k up for input k; q is the last input that reaches tap >= 0, p its tap.  j = q - k counts the taps p, p + up, ..
        const long t = m * down + half, q = t / up, p = t % up;
        const long jn = p < n_taps ? (n_taps - 1 - p) / up + 1 : 0;     // taps of this phase
        long j = (q < jn - 1 ? q : jn - 1);                            // k >= 0 and tap < n_taps
        const long jlo = q - (nb - 1) > 0 ? q - (nb - 1) : 0;          // k < nb: a bound of the loop, never a zero tap multiplied in
        // j descending: k ascending.  Unrolled so that the loads of several taps are in flight together; the sum stays one chain, in order.
#pragma unroll 4
        for (; j >= jlo; --j) {
            const long k = q - j;
            const double xv = STAGED ? xs[k - k0] : xr[k];
            const double prod = xv * h[p + j * up];
            acc = acc + prod;
        }
    }
    yr[m] = acc;
}

}  // namespace

long resample_len(long n, int up, int down) { return (n * up + down - 1) / down; }

long resample_scratch_bytes(int up, int n_taps) { return 0; }

hipError_t resample(const double* x, const int* n, int B, int max_n, int up, int down, const double* h, int n_taps, double* y, hipStream_t s) {
    if (B < 1 || B > FEAT_MAX_ROWS || max_n < 1 || up < 1 || up > RESAMPLE_MAX_RATE || down < 1 || down > RESAMPLE_MAX_RATE || n_taps < 1 ||
        n_taps % 2 == 0)
        return hipErrorInvalidValue;
    const long M = resample_len(max_n, up, down);
    const dim3 grid((unsigned)((M + RS_TILE - 1) / RS_TILE), B);
    if (resample_span(up, down, n_taps) <= RS_SPAN)
        hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_TILE), 0, s, x, n, max_n, M, up, down, h, n_taps, y);
    else
        hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_TILE), 0, s, x, n, max_n, M, up, down, h, n_taps, y);
    return hipGetLastError();
}

}  // namespace ss
