// Gradients with respect to the network's INPUTS (ss_g3_backward_inputs / ss_g6_backward_inputs): the two pieces the parameter
// backward does not need -- the layer-0 convolutions' input-gradient weights and the speaker-embedding contraction.
#include "kernels.h"

namespace ss {

// wb[ci][k][co] = w[co][ci][4 - k]: the flipped taps the input-gradient GEMM of a conv block reads (conv_pack's wb, for the layer-0
// blocks, whose forward has no use for it).  Any Ci / Co.
__global__ __launch_bounds__(256) void conv_pack_dx_kernel(const float* __restrict__ w, int Co, int Ci, float* __restrict__ wb) {
    const long n = (long)Ci * 5 * Co;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int co = (int)(i % Co);
        const int k = (int)((i / Co) % 5);
        const int ci = (int)(i / (5L * Co));
        wb[i] = w[((long)co * Ci + ci) * 5 + (4 - k)];
    }
}

hipError_t conv_pack_dx(const float* w, int Co, int Ci, float* wb, hipStream_t s) {
    int g = cdiv((long)Ci * 5 * Co, 256);
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(conv_pack_dx_kernel, dim3(g), dim3(256), 0, s, w, Co, Ci, wb);
    return hipGetLastError();
}

// One workgroup per utterance b:
//   phase 1  S[g] = sum over the utterance's `rows` rows of dg[., g]           (g < 8H, rows in order, one column per thread)
//   phase 2  out[b][j] = sum_g S[g] * W(g, col0 + j),  W = [w_f ; w_r]       (PARTS slices of g per output column, then the
//            slices added in slice order by one thread per column)
// Every sum runs in a fixed order: the result does not depend on scheduling.
constexpr int SPK_THREADS = 1024;
__global__ __launch_bounds__(SPK_THREADS) void spk_grad_kernel(const float* __restrict__ dg, long ld, long b_stride, int rows,
                                                               const float* __restrict__ w_f, const float* __restrict__ w_r, long w_ld, int col0,
                                                               int H4, int E, float* __restrict__ out) {
    extern __shared__ float lds[];            // [2 * H4] time sums, then [parts][E] slice partials
    const int G = 2 * H4;
    const float* src = dg + (long)blockIdx.x * b_stride;
    for (int g = threadIdx.x; g < G; g += SPK_THREADS) {
        float acc = 0.f;
#pragma unroll 4
        for (int r = 0; r < rows; ++r) acc += src[(long)r * ld + g];
        lds[g] = acc;
    }
    __syncthreads();
    float* part = lds + G;
    const int parts = SPK_THREADS / E;
    const int j = threadIdx.x % E, p = threadIdx.x / E;
    if (p < parts) {
        const int per = (G + parts - 1) / parts;
        const int g0 = p * per, g1 = min(G, g0 + per);
        float acc = 0.f;
#pragma unroll 8
        for (int g = g0; g < g1; ++g) {
            const float* wr = g < H4 ? w_f + (long)g * w_ld : w_r + (long)(g - H4) * w_ld;
            acc = fmaf(lds[g], wr[col0 + j], acc);
        }
        part[p * E + j] = acc;
    }
    __syncthreads();
    if (threadIdx.x < E) {
        float acc = 0.f;
        for (int q = 0; q < parts; ++q) acc += part[q * E + threadIdx.x];
        out[(long)blockIdx.x * E + threadIdx.x] = acc;
    }
}

hipError_t spk_grad(const float* dg, long ld, long b_stride, int rows, const float* w_f, const float* w_r, long w_ld, int col0, int H4, int E,
                    float* out, int B, hipStream_t s) {
    if (E < 1 || E > SPK_THREADS || H4 < 1 || rows < 1 || B < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)(2 * H4 + (SPK_THREADS / E) * E) * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spk_grad_kernel, dim3(B), dim3(SPK_THREADS), lds, s, dg, ld, b_stride, rows, w_f, w_r, w_ld, col0, H4, E, out);
    return hipGetLastError();
}

}  // namespace ss
