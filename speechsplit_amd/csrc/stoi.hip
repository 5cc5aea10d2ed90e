// Waveform scores: the short-time objective intelligibility measure (STOI; Taal, Hendriks, Heusdens, Jensen 2011) and its extended form
// (ESTOI; Jensen, Taal 2016) of a degraded waveform y against a time-aligned clean one x, both at 10 kHz.  include/speechsplit_amd.h states
// the definition completely, every sum's order included; tests/stoi_ref.py restates it in numpy.  In short:
//
//   frames     f = 0 .. F-1 start at 128 f, F = floor((n - 256) / 128) + 1; window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i < 256 (the host
//              computes it: the kernels take the table by value, so it is the C library's cosine, not a device approximation of it).
//   energies   e_f = 20 log10(sqrt(sum_i (w[i] x[128 f + i])^2) + eps), i in order; frame f is kept when e_f > max_f e_f - 40.
//   compaction the K kept frames, in order, overlap-added at hop 128: x'[s] = w[r + 128] x[128 inv[c - 1] + r + 128] + w[r] x[128 inv[c] + r],
//              c = s / 128, r = s % 128, the earlier frame first, a frame outside 0 .. K-1 absent; y' the same through x's map.
//   envelopes  frames of x' / y' at 128 m, m < M = K - 1, windowed by w, zero-padded to 512 points; X[j][m] = sqrt(sum_{k in [lo_j, hi_j)}
//              (re^2 + im^2)), k ascending.
//   segments   s < S = M - 29, frames s .. s + 29; d_s by the STOI or the ESTOI rule (the header has both), score = (sum_s d_s) / S with s
//              ascending; S < 1: NaN.
//
// Float64 throughout, no atomics, every sum in a fixed order, multiply-adds not fused (contraction is off for this file): the same bits on
// every run, and a row inside a ragged batch gives what it gives alone.
//
// Six kernels, one stage each:
//
//   energy_kernel   one thread per (frame, row): 256 multiply-square-adds in index order, then the level in dB.
//   mask_kernel     one workgroup per row: the maximum (a tree; a maximum has no order), then the keep mask in chunks of 256 frames with a
//                   ballot / popcount exclusive count -- integers, so exact in any order -- that gives each kept frame its slot; the
//                   inverse map inv[slot] = frame is what the next stage reads, -1 behind the K kept frames.
//   compact_kernel  one thread per output sample, a gather of at most two frames through inv.  Every index read back from memory (K, inv)
//                   is clamped into the row's own frames: a corrupt scratch changes numbers, never addresses.
//   bands_kernel    one workgroup per (transform frame, row, signal).  The 512-point transform of the zero-padded frame is taken as the even
//                   bins of fft_lds.h's 1024-point transform of the same frame padded further: X1024[2k] = X512[k] exactly in exact
//                   arithmetic, and the code is the transform the vocoder and the mel spectrogram already test.  It costs 2.2 times the
//                   butterflies of a 512-point transform (5120 against 2304); a frame is 256 samples in, 15 numbers out, and the whole
//                   stage is tens of microseconds at the sizes this project scores (tools/stoi_bench.py), so a second transform was not
//                   worth its tests.  Thread j < n_bands then sums its band's bins in ascending order.
//   segment_kernel  one wavefront per (segment, row): the 30-frame block of both envelopes in LDS, thread j owns band j's row (norms,
//                   scale, clip, mean, centred norm, dot product: each a loop over the 30 frames in order); for ESTOI thread t then owns
//                   column t.  Thread 0 adds the per-band (per-column) terms in order.
//   final_kernel    one thread per row: the ordered sum of d_s, the division, the NaN for S < 1, and S and K as doubles.
#include "common.h"
#include "fft_lds.h"
#include "kernels.h"

#include <math.h>

// no fused multiply-adds anywhere below: see the note on arithmetic above
#pragma clang fp contract(off)

namespace ss {

using namespace fftlds;

namespace {

constexpr double EPS = 2.220446049250313080847263336181640625e-16;      // 2^-52
constexpr int FRAME = STOI_FRAME, SHIFT = STOI_HOP, NSEG = STOI_SEG, MAXJ = STOI_MAX_BANDS;

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline int row_n(const int* n, int b, int max_n) { return clampi(n ? n[b] : max_n, 1, max_n); }

// grid = (ceil(Fs / 256), B), block = 256.  x [B][max_n]; e [B][Fs]: the level of every frame of the row, -inf behind its own F frames.
__global__ __launch_bounds__(256) void energy_kernel(const double* __restrict__ x, const int* __restrict__ n, int max_n, StoiTables tb,
                                                     double* __restrict__ e, int Fs) {
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= Fs) return;
    double v = -INFINITY;
    if (f < stoi_frames(row_n(n, b, max_n))) {
        const double* xr = x + (long)b * max_n + (long)SHIFT * f;
        double acc = 0.0;
        for (int i = 0; i < FRAME; ++i) {
            const double t = tb.w[i] * xr[i];
            acc += t * t;
        }
        v = 20.0 * log10(sqrt(acc) + EPS);
    }
    e[(long)b * Fs + f] = v;
}

// grid = B, block = 256.  e [B][Fs] -> inv [B][Fs] (inv[slot] = frame for slot < K, -1 behind), K [B].
__global__ __launch_bounds__(256) void mask_kernel(const double* __restrict__ e, const int* __restrict__ n, int max_n, int Fs,
                                                   int* __restrict__ inv, int* __restrict__ Kd) {
    __shared__ double red[256];
    __shared__ int wtot[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = stoi_frames(row_n(n, b, max_n));
    e += (long)b * Fs;
    inv += (long)b * Fs;
    double mx = -INFINITY;
    for (int f = tid; f < F; f += 256) mx = e[f] > mx ? e[f] : mx;
    red[tid] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid + h] > red[tid] ? red[tid + h] : red[tid];
        __syncthreads();
    }
    const double thr = red[0] - STOI_RANGE_DB;
    int base = 0;
    for (int f0 = 0; f0 < F; f0 += 256) {
        const int f = f0 + tid;
        const bool keep = f < F && e[f] > thr;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            off += w < wave ? wtot[w] : 0;
            total += wtot[w];
        }
        if (keep) inv[base + off + __popcll(bal & ((1ull << lane) - 1ull))] = f;
        base += total;
        __syncthreads();
    }
    for (int k = base + tid; k < Fs; k += 256) inv[k] = -1;
    if (tid == 0) Kd[b] = base;
}

// grid = (ceil(Ls / 256), B), block = 256.  x, y [B][max_n] -> xp, yp [B][Ls], zeros behind the row's own 128 (K - 1) + 256 samples.
__global__ __launch_bounds__(256) void compact_kernel(const double* __restrict__ x, const double* __restrict__ y, const int* __restrict__ n,
                                                      int max_n, StoiTables tb, const int* __restrict__ inv, const int* __restrict__ Kd,
                                                      int Fs, double* __restrict__ xp, double* __restrict__ yp, int Ls) {
    const int b = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= Ls) return;
    const int F = stoi_frames(row_n(n, b, max_n));
    const int K = clampi(Kd[b], 0, F);
    const int len = K > 0 ? SHIFT * (K - 1) + FRAME : 0;
    double vx = 0.0, vy = 0.0;
    if (s < len) {
        const int c = s / SHIFT, r = s - c * SHIFT;
        const double* xr = x + (long)b * max_n;
        const double* yr = y + (long)b * max_n;
        inv += (long)b * Fs;
        if (c >= 1) {                                            // the earlier frame first: its second half
            const long at = (long)SHIFT * clampi(inv[c - 1], 0, F - 1) + r + SHIFT;
            vx = tb.w[r + SHIFT] * xr[at];
            vy = tb.w[r + SHIFT] * yr[at];
        }
        if (c < K) {
            const long at = (long)SHIFT * clampi(inv[c], 0, F - 1) + r;
            const double qx = tb.w[r] * xr[at], qy = tb.w[r] * yr[at];
            vx = c >= 1 ? vx + qx : qx;
            vy = c >= 1 ? vy + qy : qy;
        }
    }
    xp[(long)b * Ls + s] = vx;
    yp[(long)b * Ls + s] = vy;
}

// transform frames of a signal of len samples: the starts 128 m strictly below len - 256
__host__ __device__ inline int frames_below(int len) { return len > FRAME ? (len - FRAME + SHIFT - 1) / SHIFT : 0; }

// grid = (Ms, B, signals), block = 256.  sig [B][ld] -> env [B][n_bands][Ms], zeros at and behind the row's own M frames.  The row's length
// is 128 (K - 1) + 256 with K = Kd[b] clamped into 0 .. Ms + 1 (the call), or len[b] clamped into 1 .. ld (the test hook, Kd == nullptr).
__global__ __launch_bounds__(NT) void bands_kernel(const double* __restrict__ sig0, const double* __restrict__ sig1, int ld,
                                                   const int* __restrict__ Kd, const int* __restrict__ len, StoiTables tb,
                                                   double* __restrict__ env0, double* __restrict__ env1, int Ms) {
    __shared__ FftLds L;
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, J = tb.n_bands;
    const double* sig = (blockIdx.z ? sig1 : sig0) + (long)b * ld;
    double* env = (blockIdx.z ? env1 : env0) + (long)b * J * Ms;
    int M;
    if (Kd) {
        const int K = clampi(Kd[b], 0, Ms + 1);
        M = K > 0 ? K - 1 : 0;
    } else {
        M = frames_below(clampi(len ? len[b] : ld, 1, ld));
    }
    if (m >= M) {                                                // uniform over the workgroup: nobody reaches a barrier
        if (tid < J) env[(long)tid * Ms + m] = 0.0;
        return;
    }
    for (int i = tid; i < NFFT; i += NT) {
        L.re[i] = i < FRAME ? tb.w[i] * sig[(long)SHIFT * m + i] : 0.0;
        L.im[i] = 0.0;
    }
    fft_twiddles(L, tid);
    __syncthreads();
    for (int s = 0; s < LOGN; ++s) {
        fft_stage(L, tid, s, false);
        __syncthreads();
    }
    if (tid < J) {
        double acc = 0.0;
        for (int k = tb.lo[tid]; k < tb.hi[tid]; ++k) {           // bin k of the 512-point transform is bin 2 k of this one
            const int p = brev10(2 * k);
            const double re = L.re[p], im = L.im[p];
            const double q = re * re + im * im;
            acc += q;
        }
        env[(long)tid * Ms + m] = sqrt(acc);
    }
}

// mean, centre, divide by (norm + eps) over cnt elements stride apart, in place; every loop in index order
__device__ inline void normalise(double* v, int cnt, int stride) {
    double sum = 0.0;
    for (int i = 0; i < cnt; ++i) sum += v[i * stride];
    const double mean = sum / (double)cnt;
    double q = 0.0;
    for (int i = 0; i < cnt; ++i) {
        const double c = v[i * stride] - mean;
        v[i * stride] = c;
        q += c * c;
    }
    const double den = sqrt(q) + EPS;
    for (int i = 0; i < cnt; ++i) v[i * stride] = v[i * stride] / den;
}

// grid = (Ss, B), block = 64.  ex, ey [B][n_bands][Ms] -> d [B][Ss], zeros at and behind the row's own S segments.
__global__ __launch_bounds__(64) void segment_kernel(const double* __restrict__ ex, const double* __restrict__ ey, const int* __restrict__ Kd,
                                                     int J, int extended, double clip, int Ms, double* __restrict__ d, int Ss) {
    __shared__ double X[MAXJ * NSEG], Y[MAXJ * NSEG], part[MAXJ];
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = clampi(Kd[b], 0, Ms + 1);
    const int S = (K > 0 ? K - 1 : 0) - NSEG + 1;
    if (s >= S) {                                                // uniform over the workgroup
        if (tid == 0) d[(long)b * Ss + s] = 0.0;
        return;
    }
    ex += (long)b * J * Ms + s;
    ey += (long)b * J * Ms + s;
    for (int e = tid; e < J * NSEG; e += 64) {
        const int j = e / NSEG, t = e - j * NSEG;
        X[e] = ex[(long)j * Ms + t];
        Y[e] = ey[(long)j * Ms + t];
    }
    __syncthreads();
    if (!extended) {
        if (tid < J) {
            double* xr = X + tid * NSEG;
            double* yr = Y + tid * NSEG;
            double nx = 0.0, ny = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                nx += xr[t] * xr[t];
                ny += yr[t] * yr[t];
            }
            const double alpha = sqrt(nx) / (sqrt(ny) + EPS);
            for (int t = 0; t < NSEG; ++t) {
                const double a = alpha * yr[t], c = xr[t] * clip;
                yr[t] = a < c ? a : c;
            }
            normalise(xr, NSEG, 1);
            normalise(yr, NSEG, 1);
            double acc = 0.0;
            for (int t = 0; t < NSEG; ++t) acc += xr[t] * yr[t];
            part[tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int j = 0; j < J; ++j) sum += part[j];
            d[(long)b * Ss + s] = sum / (double)J;
        }
    } else {
        if (tid < J) {
            normalise(X + tid * NSEG, NSEG, 1);
            normalise(Y + tid * NSEG, NSEG, 1);
        }
        __syncthreads();
        if (tid < NSEG) {
            normalise(X + tid, J, NSEG);
            normalise(Y + tid, J, NSEG);
            double acc = 0.0;
            for (int j = 0; j < J; ++j) acc += X[j * NSEG + tid] * Y[j * NSEG + tid];
            part[tid] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int t = 0; t < NSEG; ++t) sum += part[t];
            d[(long)b * Ss + s] = sum / (double)NSEG;
        }
    }
}

// grid = ceil(B / 64), block = 64.  d [B][Ss] -> out [B][3] = score, S, K.  Ms == 0 (no row can have a segment): d is not read.
__global__ __launch_bounds__(64) void final_kernel(const double* __restrict__ d, const int* __restrict__ Kd, int B, int Fs, int Ss,
                                                   double* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int K = clampi(Kd[b], 0, Fs);
    int S = (K > 0 ? K - 1 : 0) - NSEG + 1;
    S = S < 0 ? 0 : (S > Ss ? Ss : S);
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += d[(long)b * Ss + s];
    out[3 * b] = S >= 1 ? sum / (double)S : NAN;
    out[3 * b + 1] = (double)S;
    out[3 * b + 2] = (double)K;
}

constexpr long align256(long n) { return (n + 255) & ~255L; }

}  // namespace

StoiShape stoi_shape(int max_n) {
    StoiShape g;
    g.F = stoi_frames(max_n);
    g.L = g.F > 0 ? SHIFT * (g.F - 1) + FRAME : 0;
    g.M = g.F > 0 ? g.F - 1 : 0;
    g.S = g.M >= NSEG ? g.M - NSEG + 1 : 0;
    return g;
}

int stoi_bands_frames(int max_len) { return frames_below(max_len); }

// e, inv, K, x', y', the two envelopes at the most bands a call may ask for, d: each part rounded up to 256 bytes
long stoi_scratch_bytes(int B, int max_n) {
    const StoiShape g = stoi_shape(max_n);
    return align256(8L * B * g.F) + align256(4L * B * g.F) + align256(4L * B) + 2 * align256(8L * B * g.L) +
           2 * align256(8L * B * MAXJ * g.M) + align256(8L * B * g.S);
}

StoiScratch stoi_scratch(void* base, int B, int max_n) {
    const StoiShape g = stoi_shape(max_n);
    StoiScratch sc;
    char* p = (char*)base;
    sc.e = (double*)p;
    p += align256(8L * B * g.F);
    sc.inv = (int*)p;
    p += align256(4L * B * g.F);
    sc.K = (int*)p;
    p += align256(4L * B);
    sc.xp = (double*)p;
    p += align256(8L * B * g.L);
    sc.yp = (double*)p;
    p += align256(8L * B * g.L);
    sc.ex = (double*)p;
    p += align256(8L * B * MAXJ * g.M);
    sc.ey = (double*)p;
    p += align256(8L * B * MAXJ * g.M);
    sc.d = (double*)p;
    return sc;
}

void stoi_tables(const int* band_lo, const int* band_hi, int n_bands, StoiTables* tb) {
    for (int i = 0; i < FRAME; ++i) tb->w[i] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)(i + 1) / 257.0);
    for (int j = 0; j < MAXJ; ++j) {
        tb->lo[j] = j < n_bands ? band_lo[j] : 0;
        tb->hi[j] = j < n_bands ? band_hi[j] : 0;
    }
    tb->n_bands = n_bands;
}

static bool stoi_args_ok(int B, int max_n) { return B >= 1 && B <= STOI_MAX_ROWS && max_n >= FRAME; }

hipError_t stoi_compact(const double* x, const double* y, const int* n, int B, int max_n, const StoiTables& tb, bool from_map, double* e,
                        int* inv, int* K, double* xp, double* yp, hipStream_t s) {
    if (!stoi_args_ok(B, max_n)) return hipErrorInvalidValue;
    const StoiShape g = stoi_shape(max_n);
    if (!from_map) {
        hipLaunchKernelGGL(energy_kernel, dim3((g.F + 255) / 256, B), dim3(256), 0, s, x, n, max_n, tb, e, g.F);
        hipLaunchKernelGGL(mask_kernel, dim3(B), dim3(256), 0, s, e, n, max_n, g.F, inv, K);
    }
    hipLaunchKernelGGL(compact_kernel, dim3((g.L + 255) / 256, B), dim3(256), 0, s, x, y, n, max_n, tb, inv, K, g.F, xp, yp, g.L);
    return hipGetLastError();
}

hipError_t stoi_bands(const double* sig, const int* len, int B, int max_len, const StoiTables& tb, double* env, hipStream_t s) {
    const int Ms = frames_below(max_len);
    if (B < 1 || B > STOI_MAX_ROWS || Ms < 1 || tb.n_bands < 1 || tb.n_bands > MAXJ) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bands_kernel, dim3(Ms, B, 1), dim3(NT), 0, s, sig, sig, max_len, (const int*)nullptr, len, tb, env, env, Ms);
    return hipGetLastError();
}

hipError_t stoi(const double* x, const double* y, const int* n, int B, int max_n, const StoiTables& tb, int extended, double* out,
                const StoiScratch& sc, hipStream_t s) {
    if (!stoi_args_ok(B, max_n) || tb.n_bands < 1 || tb.n_bands > MAXJ) return hipErrorInvalidValue;
    const StoiShape g = stoi_shape(max_n);
    hipError_t err = stoi_compact(x, y, n, B, max_n, tb, false, sc.e, sc.inv, sc.K, sc.xp, sc.yp, s);
    if (err != hipSuccess) return err;
    if (g.M > 0)
        hipLaunchKernelGGL(bands_kernel, dim3(g.M, B, 2), dim3(NT), 0, s, sc.xp, sc.yp, g.L, sc.K, (const int*)nullptr, tb, sc.ex, sc.ey, g.M);
    if (g.S > 0)
        hipLaunchKernelGGL(segment_kernel, dim3(g.S, B), dim3(64), 0, s, sc.ex, sc.ey, sc.K, tb.n_bands, extended,
                           1.0 + pow(10.0, -STOI_BETA_DB / 20.0), g.M, sc.d, g.S);
    hipLaunchKernelGGL(final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, sc.d, sc.K, B, g.F, g.S, out);
    return hipGetLastError();
}

}  // namespace ss
