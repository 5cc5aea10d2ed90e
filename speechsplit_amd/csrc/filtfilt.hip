// ss_filtfilt: scipy.signal.filtfilt(b, a, x) for the reference's 5th-order Butterworth high-pass (make_spect_f0.py:54, utils.py:10-14) and
// the scaling and dither of :55, on ragged batches.  include/speechsplit_amd.h states the algorithm; filtfilt_step.h holds its arithmetic and
// says why it is fixed to the bit.
//
// One workgroup of two wavefronts per row, one launch for both passes, no wait across workgroups.  The recurrence is serial: the loop-carried
// chain is three dependent double operations a sample (the add into y, the product with a1, the subtraction into z0) over 2 (n + 36)
// samples, and nothing on it may be reassociated.  What is not on it is taken off it, 256 samples at a time through LDS:
//   * wavefront 1 builds the extension (pass 1) or reads the first pass's output backwards (pass 2), forms the six products b_i u, and
//     stores finished blocks -- with the gain and dither applied on the way out in pass 2 -- while wavefront 0 runs the block before;
//   * wavefront 0 runs the 256 steps with the five states spread over lanes 0 .. 4 (lane i holds z_i and a_{i+1}): a step is one add
//     (t = b_{i+1} u + z_{i+1}, the neighbour's state through a DPP row shift, before y is known), y = b0 u + z0 on lane 0 handed to the row's
//     lanes by a DPP row broadcast, one product a_{i+1} y and one subtraction -- four double operations issued a step instead of sixteen, each the
//     very operation filtfilt_step.h's filt_step_products makes; its LDS reads do not depend on the chain and are issued a group ahead.
// Time is ~2 (n + 36) steps whatever B is, while every row has its wavefront slots (estimate and measurement).
#include "common.h"
#include "filtfilt_step.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ss {

namespace {

constexpr int FT = 128, WL = 64, CH = 256;       // threads a row (two wavefronts), lanes a wavefront, steps in a block

// z of lane + 1 (within a row of 16 lanes; lanes 0 .. 4 are all that count)
__device__ __forceinline__ double from_next_lane(double z) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(z), 0x101 /* row_shl:1 */, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(z), 0x101, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// y of the first lane of the row of 16 lanes (row_newbcast: a lane-to-lane move, no detour through scalar registers)
__device__ __forceinline__ double from_lane_0(double y) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(y), 0x150 /* row_newbcast:0 */, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(y), 0x150, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// one step with every lane of the wavefront in step: lane i < 5 of each row of 16 holds z_i in z and a_{i+1} in a_own, pn is its product
// b_{i+1} u and p0 the product b0 u; lanes 5 .. 15 compute along on zeros, and the four rows of a wavefront compute the same thing.
// filt_step_products' operations, one state a lane.  Returns y, the same on every lane.
__device__ __forceinline__ double filt_step_lanes(double p0, double pn, bool top, double a_own, double& z) {
    const double y = from_lane_0(p0 + z);                            // the chain: this add, the product, the subtraction
    const double up = from_next_lane(z);
    const double t = top ? pn : pn + up;                             // z4 = b5 u - a5 y: nothing above it
    const double m = a_own * y;
    z = t - m;
    return y;
}

// len steps from the products in P (CH + FG rows, so that the read-ahead stays inside it).  The products of the next FG steps are read while
// the current FG run: an LDS read's latency is off the chain.  Every lane writes the same y to Y[k].
constexpr int FG = 8;
__device__ __forceinline__ void filt_run_lanes(const double (*__restrict__ P)[FILT_NCOEF], double* __restrict__ Y, int len, int tid, int col,
                                               double a_own, double& z) {
    const bool top = tid == FILT_NCOEF - 2;
    double q0[FG], qn[FG], r0[FG], rn[FG];
#pragma unroll
    for (int j = 0; j < FG; ++j) {
        q0[j] = P[j][0];
        qn[j] = P[j][col];
    }
    int k = 0;
    for (; k + FG <= len; k += FG) {
#pragma unroll
        for (int j = 0; j < FG; ++j) {
            r0[j] = P[k + FG + j][0];
            rn[j] = P[k + FG + j][col];
        }
#pragma unroll
        for (int j = 0; j < FG; ++j) Y[k + j] = filt_step_lanes(q0[j], qn[j], top, a_own, z);
#pragma unroll
        for (int j = 0; j < FG; ++j) {
            q0[j] = r0[j];
            qn[j] = rn[j];
        }
    }
    for (; k < len; ++k) Y[k] = filt_step_lanes(P[k][0], P[k][col], top, a_own, z);
}

// The two passes share everything but where a sample comes from and where a result goes.  j counts the steps of a pass from 0.
struct FiltRow {
    const double* x;        // [n]
    const double* dither;   // [n] or nullptr
    double* y;              // [n]
    double* v;              // [n + 36]: the first pass's output
    int n, N;               // the row's own samples; N = n + 36 steps a pass
    double gain, dither_scale;
};

template <int PASS>
__device__ __forceinline__ void filt_stage(const FiltRow& r, const FiltCoef& c, double (*__restrict__ P)[FILT_NCOEF], int j0, int len, int lane) {
    for (int k = lane; k < len; k += WL) filt_products(c, PASS == 1 ? filt_ext(r.x, r.n, j0 + k) : r.v[r.N - 1 - (j0 + k)], P[k]);
}

template <int PASS>
__device__ __forceinline__ void filt_store(const FiltRow& r, const double* __restrict__ Y, int j0, int len, int lane) {
    for (int k = lane; k < len; k += WL) {
        if (PASS == 1) {
            r.v[j0 + k] = Y[k];
        } else {
            const int i = r.N - 1 - (j0 + k) - FILT_PAD;
            if (i >= 0 && i < r.n) r.y[i] = filt_epilogue(Y[k], r.gain, r.dither ? r.dither + i : nullptr, r.dither_scale);
        }
    }
}

// One pass, CH steps a block, two LDS buffers: wavefront 0 runs block c from buffer c & 1 while wavefront 1 stores block c - 1 and stages block
// c + 1 in the other buffer; one workgroup barrier a block hands the buffers over.
template <int PASS>
__device__ __forceinline__ void filt_pass(const FiltRow& r, const FiltCoef& c, double (*__restrict__ P)[CH + FG][FILT_NCOEF],
                                          double (*__restrict__ Y)[CH], int wave, int lane, int li, int col, double a_own, double& z) {
    const int nch = (r.N + CH - 1) / CH;
    if (wave == 1) filt_stage<PASS>(r, c, P[0], 0, r.N < CH ? r.N : CH, lane);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int j0 = ch * CH, len = r.N - j0 < CH ? r.N - j0 : CH;
        if (wave == 0) {
            filt_run_lanes(P[ch & 1], Y[ch & 1], len, li, col, a_own, z);
        } else {
            if (ch > 0) filt_store<PASS>(r, Y[(ch - 1) & 1], j0 - CH, CH, lane);
            if (ch + 1 < nch) filt_stage<PASS>(r, c, P[(ch + 1) & 1], j0 + CH, r.N - j0 - CH < CH ? r.N - j0 - CH : CH, lane);
        }
        __syncthreads();
    }
    if (wave == 1) filt_store<PASS>(r, Y[(nch - 1) & 1], (nch - 1) * CH, r.N - (nch - 1) * CH, lane);
    __syncthreads();                             // pass 1: the row's v is written by this workgroup and read back by it
}

// grid = (B), block = 128: wavefront 0 the recurrence, wavefront 1 everything else.  x, dither, y [B][max_n]; v [B][max_n + 36] (scratch)
__global__ __launch_bounds__(FT) void filtfilt_kernel(const double* __restrict__ x, const int* __restrict__ n, int max_n, FiltCoef c,
                                                      double gain, const double* __restrict__ dither, double dither_scale,
                                                      double* __restrict__ y, double* __restrict__ v) {
    __shared__ __attribute__((aligned(16))) double P[2][CH + FG][FILT_NCOEF];   // the last FG rows of each: read ahead, never used
    __shared__ double Y[2][CH];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / WL, lane = tid % WL, li = lane % 16;   // li: the lane within its row of 16
    const int nraw = n ? n[b] : max_n;
    const int nb = nraw < 513 ? 513 : (nraw > max_n ? max_n : nraw);
    FiltRow r;
    r.x = x + (long)b * max_n;
    r.dither = dither ? dither + (long)b * max_n : nullptr;
    r.y = y + (long)b * max_n;
    r.v = v + (long)b * (max_n + 2 * FILT_PAD);
    r.n = nb;
    r.N = nb + 2 * FILT_PAD;
    r.gain = gain;
    r.dither_scale = dither_scale;
    double a_own = 0.0, zi_own = 0.0;                 // lane i < 5 of a row: a_{i+1} and zi_i
#pragma unroll
    for (int i = 0; i < FILT_NCOEF - 1; ++i)
        if (li == i) {
            a_own = c.a[i + 1];
            zi_own = c.zi[i];
        }
    const int col = li < FILT_NCOEF - 1 ? li + 1 : 0;

    // pass 1: v[j] = step(ext[j]), j ascending, from z = zi ext[0]
    double z = zi_own * filt_ext(r.x, nb, 0);
    filt_pass<1>(r, c, P, Y, wave, lane, li, col, a_own, z);
    // pass 2: w[j] = step(v[j]), j descending, from z = zi v[N - 1]; out[j - 18] = w[j] gain + dither
    z = zi_own * r.v[r.N - 1];
    filt_pass<2>(r, c, P, Y, wave, lane, li, col, a_own, z);
    for (int i = nb + tid; i < max_n; i += FT) r.y[i] = 0.0;
}

}  // namespace

long filtfilt_scratch_bytes(int B, int max_n) { return (((long)B * (max_n + 2 * FILT_PAD) * 8) + 255) & ~255L; }

hipError_t filtfilt(const double* x, const int* n, int B, int max_n, const FiltCoef& c, double gain, const double* dither,
                    double dither_scale, double* y, double* scratch, hipStream_t s) {
    if (B < 1 || B > FEAT_MAX_ROWS || max_n < 513) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filtfilt_kernel, dim3(B), dim3(FT), 0, s, x, n, max_n, c, gain, dither, dither_scale, y, scratch);
    return hipGetLastError();
}

}  // namespace ss
