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

// ---- gradients of the CODES a decode ran on (ss_g3_decode_backward / ss_g6_decode_backward) ----
// The decoder input repeats each code row over its block of freq frames (dec_in_from_codes), so a code element's gradient is the sum of the
// decoder-input gradient over the block's frames: dst[b][blk][c] = sum_u d_in[row(b, blk * k + u)][col + c], u = 0 .. k - 1 ascending, one
// thread per element (float4 of elements where the code's columns are whole aligned float4s: CodeGradPack::vec), no atomics -- the same bits
// on every run.  k = freq rows of the slab [B, TP, ld] (row0 = HALO, rows_b = TP), or k = 1 row of the compact form [B, T / f, ld], which
// holds the block sums already (row0 = 0, rows_b = T / f).  grid = (x, B, codes), block 256; memory-bound, every input element read once.
struct CodeGradPack {
    CodeGrad s[3];
    int vec[3];
    int n;
};

__global__ __launch_bounds__(256) void dec_in_codes_grad_kernel(CodeGradPack p, const float* __restrict__ d_in, int ld, int T, long rows_b, int row0,
                                                                int compact) {
    const CodeGrad c = p.s[blockIdx.z];
    const int b = blockIdx.y;
    const int W = 2 * c.H, nb = T / c.freq, k = compact ? 1 : c.freq;
    const float* src = d_in + ((long)b * rows_b + row0) * ld + c.col;
    float* dst = c.dst + (long)b * nb * W;
    if (p.vec[blockIdx.z]) {
        const int Q = W / 4, n = nb * Q;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
            const int blk = i / Q, cc = (i - blk * Q) * 4;
            const float* r = src + (long)blk * k * ld + cc;
            float4 acc = *reinterpret_cast<const float4*>(r);
            for (int u = 1; u < k; ++u) {
                const float4 v = *reinterpret_cast<const float4*>(r + (long)u * ld);
                acc.x += v.x;
                acc.y += v.y;
                acc.z += v.z;
                acc.w += v.w;
            }
            *reinterpret_cast<float4*>(dst + (long)blk * W + cc) = acc;
        }
        return;
    }
    const int n = nb * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int blk = i / W, cc = i - blk * W;
        const float* r = src + (long)blk * k * ld + cc;
        float acc = r[0];
        for (int u = 1; u < k; ++u) acc += r[(long)u * ld];
        dst[i] = acc;
    }
}

hipError_t dec_in_codes_grad(const CodeGrad* g, int n, const float* d_in, int ld, int B, int T, int f, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (n < 0 || n > 3 || !d_in || B < 1 || T < 1 || ld < 1 || f < 0 || (f && T % f)) return hipErrorInvalidValue;
    CodeGradPack p{};
    p.n = n;
    int most = 1;
    for (int i = 0; i < n; ++i) {
        const CodeGrad& c = g[i];
        if (!c.dst || c.H < 1 || c.freq < 1 || T % c.freq || c.col < 0 || (long)c.col + 2L * c.H > ld || (f && c.freq != f)) return hipErrorInvalidValue;
        p.s[i] = c;
        p.vec[i] = c.H % 2 == 0 && c.col % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(c.dst) | reinterpret_cast<uintptr_t>(d_in)) % 16 == 0;
        const int elems = (T / c.freq) * 2 * c.H / (p.vec[i] ? 4 : 1);
        most = elems > most ? elems : most;
    }
    int gx = cdiv(most, 256);
    if (gx > 64) gx = 64;
    const long TP = T + 2 * HALO;
    hipLaunchKernelGGL(dec_in_codes_grad_kernel, dim3(gx, B, n), dim3(256), 0, s, p, d_in, ld, T, f ? (long)(T / f) : TP, f ? 0 : HALO, f ? 1 : 0);
    return hipGetLastError();
}

}  // namespace ss
