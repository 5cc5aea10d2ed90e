// ss_remove_silence: trim the ends of a recording and cap its pauses, on ragged batches.  include/speechsplit_amd.h states the definition in
// full: levels of 256-sample blocks (the energy of the 512-sample window centred on each, from in-order sums of 128-sample quarters), a strict
// relative threshold, a hangover, the run rules, and the gather with a 128-sample cross-fade at every join.  Every operation is an IEEE double
// add, multiply, compare or copy in a fixed order, so the result is the definition to the bit; the pragma below keeps hipcc from contracting a
// product and a sum into a fused multiply-add.
//
// Three kernels, bound by memory traffic (x read once for the levels and at most once more for the gather, y written once):
//   levels  one workgroup per (tile of SIL_TILE blocks, row).  The tile's 2 SIL_TILE + 2 quarters (one of halo on either side) are loaded
//           coalesced into LDS, one padded row a quarter; one thread a quarter then adds its 128 squares in order out of LDS (the padding
//           spreads the 32 threads over the banks), and one thread a block adds its four quarters.  The halo costs 2 / 30 more reads of x.
//   mask    one wavefront per row over at most 8191 blocks: the maximum, then 64-block chunks with ballots and a carried state -- the
//           activity bits and their prefix count, the dilation (a difference of prefix counts) with the last dilated block at or before each
//           block, the next dilated block in a pass backwards with the run rules, and the prefix count of the kept blocks that writes inv.
//   gather  one thread per output sample.  inv and K are read back with every index clamped into the row's own blocks and samples.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace ss {

namespace {

constexpr int SIL_TILE = 15;                      // blocks a workgroup of the level kernel
constexpr int SIL_QUARTERS = 2 * SIL_TILE + 2;    // their quarters, with one of halo on either side: 32
constexpr int SIL_QLEN = 128, SIL_QPAD = SIL_QLEN + 1;
constexpr int SIL_THREADS = 256;
constexpr int SIL_CHUNKS = (SIL_MAX_BLOCKS + 63) / 64;

__device__ __forceinline__ int clamp_len(const int* n, int b, int hi) {
    const int raw = n ? n[b] : hi;
    return raw < 1 ? 1 : (raw > hi ? hi : raw);
}

// grid = (ceil(Jmax / SIL_TILE), B), block = SIL_THREADS.  x [B][max_n] -> e [B][Jmax], zeros behind the row's own J_b blocks.
__global__ __launch_bounds__(SIL_THREADS) void silence_levels_kernel(const double* __restrict__ x, const int* __restrict__ n, int max_n, int Jmax,
                                                                     double* __restrict__ e) {
    __shared__ double xs[SIL_QUARTERS * SIL_QPAD];
    __shared__ double qs[SIL_QUARTERS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nb = clamp_len(n, b, max_n);
    const int J = (nb + 255) / 256, NQ = (nb + SIL_QLEN - 1) / SIL_QLEN;
    const int j0 = blockIdx.x * SIL_TILE;
    double* __restrict__ er = e + (long)b * Jmax;
    if (j0 >= J) {                                                     // a tile behind the row: zeros only
        if (tid < SIL_TILE && j0 + tid < Jmax) er[j0 + tid] = 0.0;
        return;
    }
    const double* __restrict__ xr = x + (long)b * max_n;
    const int q0 = 2 * j0 - 1;                                         // the tile's first quarter (-1 in the first tile: it does not exist)
    const long s0 = (long)q0 * SIL_QLEN;
    for (int i = tid; i < SIL_QUARTERS * SIL_QLEN; i += SIL_THREADS) {
        const long s = s0 + i;
        if (s >= 0 && s < nb) xs[(i / SIL_QLEN) * SIL_QPAD + i % SIL_QLEN] = xr[s];       // nothing at or beyond n_b is read
    }
    __syncthreads();
    if (tid < SIL_QUARTERS) {
        const int q = q0 + tid;
        double acc = 0.0;
        if (q >= 0 && q < NQ) {
            const int len = nb - q * SIL_QLEN < SIL_QLEN ? nb - q * SIL_QLEN : SIL_QLEN;
            const double* row = xs + tid * SIL_QPAD;
            const double v0 = row[0];
            acc = v0 * v0;
#pragma unroll 8
            for (int i = 1; i < len; ++i) {
                const double v = row[i];
                const double sq = v * v;
                acc = acc + sq;
            }
        }
        qs[tid] = acc;
    }
    __syncthreads();
    if (tid < SIL_TILE && j0 + tid < Jmax) {
        const int j = j0 + tid;
        double lvl = 0.0;
        if (j < J) {
            bool first = true;
            for (int k = 0; k < 4; ++k) {                              // Q_{2j-1}, Q_{2j}, Q_{2j+1}, Q_{2j+2}: those that exist, in that order
                const int q = 2 * j - 1 + k;
                if (q < 0 || q >= NQ) continue;
                const double v = qs[q - q0];
                lvl = first ? v : lvl + v;
                first = false;
            }
        }
        er[j] = lvl;
    }
}

// grid = B, block = 64 (one wavefront).  e [B][Jmax]; cnt (nullable) holds samples (cnt_is_samples) or blocks a row -> inv [B][Jmax], k [B].
__global__ __launch_bounds__(64) void silence_mask_kernel(const double* __restrict__ e, const int* __restrict__ cnt, int cnt_is_samples, int max_n,
                                                          int Jmax, double ratio, int hang, int edge, int pause, int* __restrict__ inv,
                                                          int* __restrict__ kout) {
    __shared__ unsigned short pre[SIL_MAX_BLOCKS + 1];                 // active blocks in [0, j)
    __shared__ unsigned short lastd[SIL_MAX_BLOCKS];                   // 1 + the last dilated block at or before j (0: none)
    __shared__ unsigned long long dbits[SIL_CHUNKS], kbits[SIL_CHUNKS];
    const int b = blockIdx.x, lane = threadIdx.x;
    int J;
    if (cnt_is_samples) J = (clamp_len(cnt, b, max_n) + 255) / 256;
    else J = clamp_len(cnt, b, Jmax);
    const double* __restrict__ er = e + (long)b * Jmax;
    int* __restrict__ ir = inv + (long)b * Jmax;
    const int chunks = (J + 63) / 64;
    const unsigned long long below = (1ull << lane) - 1ull;            // the lanes under this one

    // E_max: order-free and exact; a NaN level makes it NaN (nothing is active then)
    double mx = er[0];
    bool nan = false;
    for (int j = lane; j < J; j += 64) {
        const double v = er[j];
        nan |= v != v;
        if (v > mx) mx = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(mx, o);
        if (other > mx) mx = other;
    }
    const bool any_nan = __ballot(nan) != 0ull;
    const double thr = ratio * mx;

    // activity and its prefix count
    int carry = 0;
    for (int c = 0; c < chunks; ++c) {
        const int j = 64 * c + lane;
        const bool a = j < J && !any_nan && er[j] > thr;               // strictly
        const unsigned long long m = __ballot(a);
        if (j < J) pre[j] = (unsigned short)(carry + __popcll(m & below));
        carry += __popcll(m);
    }
    if (lane == 0) pre[J] = (unsigned short)carry;
    const bool none = carry == 0;                                      // E_max is 0 or not finite: every block is kept
    __syncthreads();

    // dilation: d_j = an active block in [j - hang, j + hang]; and the last dilated block at or before j
    const int h = hang < J ? hang : J;
    int last = 0;
    for (int c = 0; c < chunks; ++c) {
        const int j = 64 * c + lane;
        bool d = false;
        if (j < J) {
            const int lo = j - h < 0 ? 0 : j - h, hi = j + h + 1 > J ? J : j + h + 1;
            d = pre[hi] > pre[lo];
        }
        const unsigned long long m = __ballot(d);
        const unsigned long long upto = m & (below | (1ull << lane));
        if (j < J) lastd[j] = (unsigned short)(upto ? 64 * c + 64 - __clzll(upto) : last);
        if (m) last = 64 * c + 64 - __clzll(m);
        if (lane == 0) dbits[c] = m;
    }
    __syncthreads();

    // backwards: the next dilated block at or after j, and with both ends of a silent run the rule of that run
    int next = J;
    for (int c = chunks - 1; c >= 0; --c) {
        const int j = 64 * c + lane;
        const unsigned long long m = dbits[c];
        const unsigned long long from = m & ~below;
        bool keep = false;
        if (j < J) {
            if (none || ((m >> lane) & 1ull)) keep = true;
            else {
                const int s = lastd[j], t = (from ? 64 * c + __ffsll((long long)from) - 1 : next) - 1;      // the run is blocks s .. t
                const int R = t - s + 1;
                if (s == 0) keep = j > t - (R < edge ? R : edge);                                           // leading: its last blocks
                else if (t == J - 1) keep = j < s + (R < edge ? R : edge);                                  // trailing: its first blocks
                else if (pause < 0 || R <= pause) keep = true;
                else keep = j < s + (pause + 1) / 2 || j > t - pause / 2;
            }
        }
        const unsigned long long km = __ballot(keep);
        if (lane == 0) kbits[c] = km;
        if (m) next = 64 * c + __ffsll((long long)m) - 1;
    }
    __syncthreads();

    // inv: the kept blocks, ascending; -1 behind them
    int K = 0;
    for (int c = 0; c < chunks; ++c) {
        const unsigned long long km = kbits[c];
        if ((km >> lane) & 1ull) ir[K + __popcll(km & below)] = 64 * c + lane;
        K += __popcll(km);
    }
    for (int j = K + lane; j < Jmax; j += 64) ir[j] = -1;
    if (lane == 0) kout[b] = K;
}

struct SilFade {
    double g[SIL_QLEN];
};

// grid = (ceil(max_n / 256), B), block = 256: output block c of row b.  x [B][max_n], inv [B][Jmax], k [B] -> y [B][max_n], m [B].
__global__ __launch_bounds__(256) void silence_gather_kernel(const double* __restrict__ x, const int* __restrict__ n, int max_n, int Jmax,
                                                             const int* __restrict__ inv, const int* __restrict__ k, SilFade f,
                                                             double* __restrict__ y, int* __restrict__ mout) {
    const int b = blockIdx.y, c = blockIdx.x, r = threadIdx.x;
    const int nb = clamp_len(n, b, max_n);
    const int J = (nb + 255) / 256;
    const int* __restrict__ ir = inv + (long)b * Jmax;
    // whatever inv and k hold, every index below lies inside the row's own blocks and samples
    const int kraw = k[b], K = kraw < 1 ? 1 : (kraw > J ? J : kraw);
    const int lraw = ir[K - 1], lastb = lraw < 0 ? 0 : (lraw > J - 1 ? J - 1 : lraw);
    const int lastlen = nb - 256 * lastb < 256 ? nb - 256 * lastb : 256;
    const int mb = 256 * (K - 1) + lastlen;                            // <= 256 (J - 1) + 256, and <= n_b when the map is what the mask wrote
    const int mclamped = mb > nb ? nb : mb;
    if (c == 0 && r == 0) mout[b] = mclamped;
    const long i = 256L * c + r;
    if (i >= max_n) return;
    double* __restrict__ yr = y + (long)b * max_n;
    if (i >= mclamped) {
        yr[i] = 0.0;
        return;
    }
    const double* __restrict__ xr = x + (long)b * max_n;
    const int sraw = ir[c], s = sraw < 0 ? 0 : (sraw > J - 1 ? J - 1 : sraw);
    const int slen = nb - 256 * s < 256 ? nb - 256 * s : 256;
    long src = 256L * s + r;
    if (src > nb - 1) src = nb - 1;                                    // a corrupt map only
    double v = xr[src];
    if (c > 0) {
        const int araw = ir[c - 1], a = araw < 0 ? 0 : (araw > J - 1 ? J - 1 : araw);
        if (a + 1 != s && r < (slen < SIL_QLEN ? slen : SIL_QLEN)) {   // a join: fade from the signal that followed the last kept block
            long tail = 256L * (a + 1) + r;
            if (tail > nb - 1) tail = nb - 1;                          // a corrupt map only: block a + 1 is a full block otherwise
            const double g = f.g[r];
            const double og = 1.0 - g;
            const double p = xr[tail] * og;
            const double q = v * g;
            v = p + q;
        }
    }
    yr[i] = v;
}

bool silence_shape_ok(int B, int max_n) { return B >= 1 && B <= FEAT_MAX_ROWS && max_n >= 1 && max_n <= 256 * SIL_MAX_BLOCKS; }

}  // namespace

int silence_blocks(int max_n) { return (max_n + 255) / 256; }

static long up256(long v) { return (v + 255) / 256 * 256; }

long silence_scratch_bytes(int B, int max_n) {
    const long J = silence_blocks(max_n);
    return up256((long)B * J * 8) + up256((long)B * J * 4) + up256((long)B * 4);
}

SilenceScratch silence_scratch(void* base, int B, int max_n) {
    const long J = silence_blocks(max_n);
    char* p = (char*)base;
    SilenceScratch sc;
    sc.e = (double*)p;
    p += up256((long)B * J * 8);
    sc.inv = (int*)p;
    p += up256((long)B * J * 4);
    sc.k = (int*)p;
    return sc;
}

hipError_t silence_levels(const double* x, const int* n, int B, int max_n, double* e, hipStream_t s) {
    if (!silence_shape_ok(B, max_n)) return hipErrorInvalidValue;
    const int Jmax = silence_blocks(max_n);
    hipLaunchKernelGGL(silence_levels_kernel, dim3((Jmax + SIL_TILE - 1) / SIL_TILE, B), dim3(SIL_THREADS), 0, s, x, n, max_n, Jmax, e);
    return hipGetLastError();
}

hipError_t silence_mask(const double* e, const int* cnt, bool cnt_is_samples, int B, int max_n, double ratio, int hang, int edge, int pause,
                        int* inv, int* k, hipStream_t s) {
    if (!silence_shape_ok(B, max_n) || hang < 0 || edge < 0 || pause < -1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(silence_mask_kernel, dim3(B), dim3(64), 0, s, e, cnt, cnt_is_samples ? 1 : 0, max_n, silence_blocks(max_n), ratio, hang,
                       edge, pause, inv, k);
    return hipGetLastError();
}

hipError_t silence_gather(const double* x, const int* n, int B, int max_n, const int* inv, const int* k, const double* g, double* y, int* m,
                          hipStream_t s) {
    if (!silence_shape_ok(B, max_n)) return hipErrorInvalidValue;
    SilFade f;
    for (int i = 0; i < SIL_QLEN; ++i) f.g[i] = g[i];
    hipLaunchKernelGGL(silence_gather_kernel, dim3((max_n + 255) / 256, B), dim3(256), 0, s, x, n, max_n, silence_blocks(max_n), inv, k, f, y, m);
    return hipGetLastError();
}

}  // namespace ss
