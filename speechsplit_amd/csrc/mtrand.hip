// ss_mt19937_rand: numpy.random.RandomState.rand on the device -- MT19937 continued from a caller-supplied state, two tempered words a
// double, bit for bit -- and ss_dither_rows, which gathers the contiguous stream into the [B][max_n] layout ss_filtfilt takes.
// include/speechsplit_amd.h states both definitions.
//
// The generator is a recurrence: word n + 624 needs words n, n + 1 and n + 397, so 227 consecutive words are independent and no more, and
// a call of `count` draws is a chain of 2 count / 227 dependent steps whatever else the device could do beside it.  One workgroup walks it:
//   * the last 1024 words live in an LDS ring indexed by (n & 1023).  A step reads [n, n + 227] and [n + 397, n + 623] and writes
//     [n + 624, n + 850], i.e. the slots of [n - 400, n - 174): nothing a step reads, and nothing younger than 400 words;
//   * wavefronts 0 .. 3 (227 lanes of them) run the step: three LDS reads, five integer operations, one LDS write, one barrier;
//   * wavefronts 4 .. 7 run one step behind on words that are final: tempering, the conversion to double and the coalesced stores are off
//     the chain.  A draw whose two words straddle a step waits for the second; the ring keeps the first far longer than that.
// The conversion is exact in double (a 27-bit integer times 2^26, plus a 26-bit integer, over 2^53), so neither rounding nor contraction
// can change it; contraction is off all the same.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ss {

namespace {

constexpr int MT_N = 624, MT_M = 397, MT_STEP = MT_N - MT_M;       // 227 independent words a step
constexpr int MT_RING = 1024, MT_GEN = 256, MT_THREADS = 512;      // ring words; threads that generate (4 wavefronts); all threads
constexpr unsigned MT_A = 0x9908b0dfu, MT_UPPER = 0x80000000u, MT_LOWER = 0x7fffffffu;

__device__ __forceinline__ unsigned mt_temper(unsigned y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// grid = 1, block = 512.  state [625] in/out: key, then pos.  out [count].  count >= 1.
// Words are numbered from the key: x[0 .. 623] = key, stream word j = temper(x[pos + j]), draw i takes words 2i and 2i + 1.
__global__ __launch_bounds__(MT_THREADS) void mt19937_rand_kernel(unsigned* __restrict__ state, long count, double* __restrict__ out) {
    __shared__ unsigned x[MT_RING];
    const int tid = threadIdx.x;
    for (int j = tid; j < MT_N; j += MT_THREADS) x[j] = state[j];
    const unsigned praw = state[MT_N];
    const long pos = praw > (unsigned)MT_N ? MT_N : (long)praw;
    const long tot = pos + 2 * count;
    const long K = (tot - 1) / MT_N;                   // regenerations: the end state is x[624 K .. 624 K + 623]
    const long fresh = K * MT_N;                       // words to generate: x[624 .. 624 + fresh)
    const long steps = (fresh + MT_STEP - 1) / MT_STEP;
    __syncthreads();

    long n = tid;                                      // a generating lane's word of the current step (it writes x[n + 624])
    int r = tid;                                       // n & 1023
    long done = 0;                                     // draws stored before this phase
    for (long k = 0; k <= steps; ++k) {
        if (tid < MT_GEN) {
            if (tid < MT_STEP && n < fresh) {
                const unsigned y = (x[r] & MT_UPPER) | (x[(r + 1) & (MT_RING - 1)] & MT_LOWER);
                x[(r + MT_N) & (MT_RING - 1)] = x[(r + MT_M) & (MT_RING - 1)] ^ (y >> 1) ^ ((y & 1u) ? MT_A : 0u);
            }
            n += MT_STEP;
            r = (r + MT_STEP) & (MT_RING - 1);
        } else {
            // words below 624 + 227 k were final at the last barrier; this phase's step writes at and above that
            const long have = MT_N + k * MT_STEP < MT_N + fresh ? MT_N + k * MT_STEP : MT_N + fresh;
            const long can = (have - pos) / 2, upto = can < count ? can : count;
            for (long i = done + (tid - MT_GEN); i < upto; i += MT_THREADS - MT_GEN) {
                const long a = pos + 2 * i;
                const unsigned w0 = mt_temper(x[a & (MT_RING - 1)]), w1 = mt_temper(x[(a + 1) & (MT_RING - 1)]);
                out[i] = ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0;
            }
            done = upto;
        }
        __syncthreads();
    }
    // numpy's state after the same draws: the whole last block, however little of it is consumed
    if (K > 0)
        for (int j = tid; j < MT_N; j += MT_THREADS) state[j] = x[(fresh + j) & (MT_RING - 1)];
    if (tid == 0) state[MT_N] = (unsigned)(tot - fresh);
}

constexpr int DR_THREADS = 256, DR_TILE = 1024;        // columns a workgroup: four a thread, 256 apart

// grid = (ceil(max_n / DR_TILE), B), block = 256.  draws [count], first i64[B], n i32[B], out [B][max_n].
__global__ __launch_bounds__(DR_THREADS) void dither_rows_kernel(const double* __restrict__ draws, long count, const long* __restrict__ first,
                                                                 const int* __restrict__ n, int max_n, double* __restrict__ out) {
    const int b = blockIdx.y;
    const int nraw = n[b];
    const long nb = nraw < 0 ? 0 : (nraw > max_n ? max_n : nraw);
    const long last = count - nb > 0 ? count - nb : 0;                 // the last start that keeps the row inside draws
    const long fraw = first[b];
    const long f = fraw < 0 ? 0 : (fraw > last ? last : fraw);
    double* __restrict__ row = out + (long)b * max_n;
    const long i0 = (long)blockIdx.x * DR_TILE + threadIdx.x;
#pragma unroll
    for (int u = 0; u < DR_TILE / DR_THREADS; ++u) {
        const long i = i0 + u * DR_THREADS;
        if (i < max_n) row[i] = (i < nb && f + i < count) ? draws[f + i] : 0.0;
    }
}

}  // namespace

hipError_t mt19937_rand(unsigned* state, long count, double* out, hipStream_t s) {
    if (!state || count < 0 || count > MT_MAX_COUNT || (count > 0 && !out)) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;                 // the state is unchanged and nothing is written
    hipLaunchKernelGGL(mt19937_rand_kernel, dim3(1), dim3(MT_THREADS), 0, s, state, count, out);
    return hipGetLastError();
}

hipError_t dither_rows(const double* draws, long count, const long* first, const int* n, int B, int max_n, double* out, hipStream_t s) {
    if (!draws || !first || !n || !out || count < 0 || count > MT_MAX_COUNT || B < 1 || B > FEAT_MAX_ROWS || max_n < 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((long)max_n + DR_TILE - 1) / DR_TILE), B);
    hipLaunchKernelGGL(dither_rows_kernel, grid, dim3(DR_THREADS), 0, s, draws, count, first, n, max_n, out);
    return hipGetLastError();
}

}  // namespace ss
