// Pitch tracker: waveform -> F0 track, the stand-in for the reference's `pysptk.sptk.rapt` call (make_spect_f0.py:64).  It is the published
// core of RAPT (Talkin 1995, "A robust algorithm for pitch tracking"): normalised cross-correlation (NCCF) candidates per frame, then dynamic
// programming over the frames, with Talkin's published constants.  It is NOT a port of SPTK's rapt and claims no parity with it: RAPT's
// two-rate search (a decimated first pass) is left out, and its spectral-stationarity term (an LPC analysis per frame) is optional and
// off by default (ss_pitch_track_stat: stat_kernel and dp_kernel<true> below).  The output follows RAPT's
// otype=2 convention -- ln(F0 in Hz), -1e10 for unvoiced frames, one value per 256-sample hop -- so f0_normalize takes it unchanged.
// include/speechsplit_amd.h states the algorithm completely; tests/pitch_ref.py restates it in numpy.
//
// Three launches, float64 throughout, no atomics, every sum in a fixed order -- the same bits on every run:
//
//   nccf_kernel   one workgroup per (frame, utterance).  The segment (S = 120 + Lmax <= 520 samples, zero outside the utterance) is staged in
//                 LDS; its mean and its sum of squares are each a per-thread partial (j = tid, tid + 256, tid + 512, in that order) followed
//                 by a 256-leaf pairwise tree; then one thread per lag k (threads loop: K reaches 385) runs j = 0 .. 119 in order over the
//                 three sums it needs: sum y_j y_{j+k}, e_k = sum y_{j+k}^2 and e_0 = sum y_j^2.  e_k is summed directly and not carried as a
//                 running sum e_{k+1} = e_k - y_k^2 + y_{k+120}^2: the running form saves a third of the multiply-adds, which is nothing
//                 here, and its cancellation error -- up to 2.3e-13 in phi on the tests' speech inputs, measured in numpy -- is at or past
//                 the parity bounds the tests hold phi to (1.9e-13 .. 4.6e-13 there); the direct form stays within 1.7e-15.  Bound: K x 120 x 3 multiply-adds from LDS per frame, ~0.14 M for K = 385.
//   cand_kernel   one workgroup per (frame, utterance): phi's maximum (a tree; a maximum has no rounding), the five-condition peak test and
//                 the parabolic refinement per lag, then each candidate counts the candidates that precede it (larger v, or equal v and a
//                 smaller lag) and, if fewer than 19 do, writes itself into that slot: selection by rank, no sort, no atomics.
//   dp_kernel     one wavefront per utterance, sequential over its frames.  Lane a owns destination state a and runs b = 0 .. (states of
//                 the previous frame) - 1 in order with a strict <, so the lowest b wins a tie; the previous frame's costs sit in LDS (20 doubles,
//                 double-buffered: one barrier a frame; reading them from the other lanes' registers by shuffle instead measured 12 % slower).  The
//                 frequency term uses ln L_a - ln L_b with ln L stored per candidate (20 logarithms a frame instead of 400).  Backpointers
//                 go to scratch; the backtrack reads one row of them per frame across the lanes and selects by shuffle, so its loads do not
//                 depend on the path.  Bound: F sequential steps -- latency, not throughput: about one
//                 global-load round trip per frame (the one-frame prefetch is shorter than that latency, and the barrier waits for it).
//                 dp_kernel<true> also fetches S_i one step ahead, beside rms, and adds VTR_S_C S_i to the two voicing transitions;
//                 dp_kernel<false> is the arithmetic above and nothing else.
//   stat_kernel   (ss_pitch_track_stat only, between nccf and cand) one workgroup per (frame, utterance).  The 801 samples that the frame's
//                 two 30 ms windows cover together are staged in LDS once; both pre-emphasised, windowed signals (2 x 480) are formed there
//                 (the staging buffer then holds the partial sums).
//                 The 38 (window, lag) autocorrelation sums are cut into 24 chunks of 20 terms (y_j = 0 for j >= 480): thread t < 240
//                 takes chunk t / 10 of four consecutive lags of one window (t % 10: window, lag group) in index order, sliding
//                 y_{j+k} through registers -- two LDS reads for four multiply-adds, where one lag a thread pays two for one -- and
//                 thread t < 38 adds its sum's 24 partials in chunk order.  The two Levinson recursions (18 dependent steps: 171
//                 multiply-adds in the inner products, as many in the updates, a division per step) run side by side in lanes 0 and 1
//                 of one wavefront, each serially with a in registers (fully unrolled; rho sits in LDS, where 38 threads put
//                 ff r_k / r_0, and is read at constant offsets off the dependent chain): the header fixes index order for the
//                 recursion's inner products, so spreading a step over lanes would leave the products serial and pay a shuffle per term
//                 for the update alone; two lanes of ONE wavefront, because a serial lane costs its wavefront's whole issue slot
//                 whatever the number of lanes in use.  Then 19 threads form c_k, one thread the distortion and S.  Bound: 38 x 480
//                 multiply-adds from LDS per frame, 18 k, a fifth of the NCCF's at K = 257, plus ~0.8 k dependent double operations of
//                 one wavefront per frame -- the latter is what the time is.
//
// Batches: row b has n_b = min(max(n[b], 513), max_n) samples and F_b = n_b / 256 + 1 frames; every kernel computes row b as if it were alone
// and never reads a sample at or beyond n_b; phi / rms beyond F_b are exact zeros, f0 beyond F_b is -1e10.
#include "common.h"
#include "kernels.h"

#include <math.h>

namespace ss {

namespace {

constexpr int HOP = 256, W = 120, NT = 256, NST = PITCH_STATES, BPLD = 32;
constexpr int MAXS = W + PITCH_MAX_LAG;                        // 520
constexpr int MAXK = PITCH_MAX_LAG - PITCH_MIN_LAG + 1;        // 385
constexpr double FS = 16000.0, CAND_TR = 0.3, LAG_WT = 0.3, FREQ_WT = 0.02, DOUBL_C = 0.35, VTRAN_C = 0.005, VTR_A_C = 0.5, VO_BIAS = 0.0,
                 A_FACT = 10000.0, UNVOICED = -1e10, LN2 = 0.69314718055994530942;
// the spectral-stationarity term: 30 ms windows whose centres are 20 ms apart, LPC order 2 + fs / 1000
constexpr int STAT_W = 480, STAT_GAP = 320, LPC_ORD = 18, STAT_SPAN = STAT_W + STAT_GAP + 1, STAT_SUMS = 2 * (LPC_ORD + 1);
// the autocorrelation sums: a thread takes 4 consecutive lags of one window over one chunk of 20 terms; 5 lag groups x 2 windows x 24 chunks
constexpr int STAT_CHUNK = 20, STAT_CHUNKS = STAT_W / STAT_CHUNK, STAT_LAGS = 4, STAT_GROUPS = (LPC_ORD + STAT_LAGS) / STAT_LAGS,
              STAT_PAD = 24, STAT_LD = STAT_W + STAT_PAD + 24;   // a window's row: 480 values, zeros behind them; 528 = 16 mod 32 apart in LDS banks
constexpr double PREEMP = 0.4, STAT_FF = 1.0 / (1.0 + 1e-3), VTR_S_C = 0.5, TWO_PI = 6.28318530717958647693;
static_assert(2 * STAT_GROUPS * STAT_CHUNKS <= NT && STAT_CHUNKS * STAT_CHUNK == STAT_W, "one thread per (window, lag group, chunk)");
static_assert(STAT_GROUPS * STAT_LAGS - 1 <= STAT_PAD && STAT_PAD <= NT, "the last chunk's reads stay inside the zeros");

__device__ inline int row_samples(const int* n, int b, int max_n) {
    const int v = n ? n[b] : max_n;
    return v < 513 ? 513 : (v > max_n ? max_n : v);
}

// 256 leaves, pairwise: red[t] += red[t + s] for s = 128, 64, .. 1.  Every thread gets the result.
__device__ inline double block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ inline double block_max(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid = (max_frames, B), block = 256.  wav [B][max_n]; phi [B][max_frames][K]; rms [B][max_frames].
__global__ __launch_bounds__(NT) void nccf_kernel(const double* __restrict__ wav, const int* __restrict__ n, int max_n, int max_frames,
                                                  double scale, PitchLags g, double* __restrict__ phi, double* __restrict__ rms) {
    __shared__ double y[MAXS];
    __shared__ double red[NT];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nb = row_samples(n, b, max_n), F = nb / HOP + 1, K = g.lmax - g.lmin + 1, S = W + g.lmax;
    const long fr = (long)b * max_frames + f;
    phi += fr * K;
    if (f >= F) {
        for (int kk = tid; kk < K; kk += NT) phi[kk] = 0.0;
        if (tid == 0) rms[fr] = 0.0;
        return;
    }
    const double* x = wav + (long)b * max_n;
    const int start = HOP * f - S / 2;
    double part = 0.0;
    for (int j = tid; j < S; j += NT) {
        const int i = start + j;
        const double z = (i >= 0 && i < nb) ? scale * x[i] : 0.0;
        y[j] = z;
        part += z;
    }
    const double mu = block_sum(part, red, tid) / (double)S;
    part = 0.0;
    for (int j = tid; j < S; j += NT) {
        const double v = y[j] - mu;
        y[j] = v;
        part += v * v;
    }
    const double sq = block_sum(part, red, tid);                  // its barriers also publish y
    if (tid == 0) rms[fr] = sqrt(sq / (double)S + 1.0);
    for (int kk = tid; kk < K; kk += NT) {
        const int k = g.lmin + kk;                                // j + k <= 119 + Lmax = S - 1
        double num = 0.0, ek = 0.0, e0 = 0.0;
        for (int j = 0; j < W; ++j) {
            const double a = y[j], c = y[j + k];
            num += a * c;
            ek += c * c;
            e0 += a * a;
        }
        phi[kk] = num / sqrt(e0 * ek + A_FACT);
    }
}

// grid = (max_frames, B), block = 256.  Per frame < F_b: cost / lag / lnlag [NST] (state 0 = unvoiced, then the kept candidates by
// decreasing v, the smaller lag first on equal v) and cnt = the number of states.  Slots at or beyond cnt are not written.
__global__ __launch_bounds__(NT) void cand_kernel(const double* __restrict__ phi, const int* __restrict__ n, int max_n, int max_frames,
                                                  PitchLags g, double* __restrict__ cost, double* __restrict__ lag,
                                                  double* __restrict__ lnlag, int* __restrict__ cnt) {
    __shared__ double p[MAXK];
    __shared__ double vv[MAXK];       // the refined peak value of a candidate, -1 for every other lag (a candidate's v is >= phi_k > 0)
    __shared__ double red[NT];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nb = row_samples(n, b, max_n), K = g.lmax - g.lmin + 1;
    if (f >= nb / HOP + 1) return;
    const long fr = (long)b * max_frames + f;
    phi += fr * K;
    double m = -INFINITY;
    for (int kk = tid; kk < K; kk += NT) {
        p[kk] = phi[kk];
        m = fmax(m, p[kk]);
    }
    const double phimax = block_max(m, red, tid);                 // its barriers also publish p
    double L[2], v[2];                                            // K <= 385: at most two lags per thread
    for (int kk = tid, u = 0; kk < K; kk += NT, ++u) {
        v[u] = -1.0;
        L[u] = 1.0;
        if (kk >= 1 && kk < K - 1) {
            const double lo = p[kk - 1], c = p[kk], hi = p[kk + 1];
            if (c > lo && c >= hi && c > 0.0 && c >= CAND_TR * phimax) {
                const double den = lo - 2.0 * c + hi;
                const double delta = den < 0.0 ? 0.5 * (lo - hi) / den : 0.0;
                L[u] = (double)(g.lmin + kk) + delta;
                v[u] = c - 0.25 * (lo - hi) * delta;
            }
        }
        vv[kk] = v[u];
    }
    __syncthreads();
    cost += fr * NST;
    lag += fr * NST;
    lnlag += fr * NST;
    for (int kk = tid, u = 0; kk < K; kk += NT, ++u) {
        if (v[u] < 0.0 && kk != 0) continue;
        int before = 0, total = 0;
        for (int j = 0; j < K; ++j) {
            const double o = vv[j];
            total += o >= 0.0;
            before += o > v[u] || (o == v[u] && j < kk);
        }
        if (kk == 0) {                                            // lag Lmin is never a candidate: this thread writes state 0 and the count
            cost[0] = VO_BIAS + fmax(phimax, 0.0);
            lag[0] = 1.0;
            lnlag[0] = 0.0;
            cnt[fr] = 1 + (total < NST - 1 ? total : NST - 1);
        } else if (before < NST - 1) {
            cost[1 + before] = 1.0 - v[u] * (1.0 - LAG_WT * L[u] / (double)g.lmax);
            lag[1 + before] = L[u];
            lnlag[1 + before] = log(L[u]);
        }
    }
}

// grid = B, block = 64 (one wavefront).  f0 [B][max_frames]; bp [B][max_frames][BPLD] bytes.  STAT: stat [B][max_frames], read at frames
// 1 .. F_b - 1 only; without it stat is not touched.
template <bool STAT>
__global__ __launch_bounds__(64) void dp_kernel(const double* __restrict__ rms, const double* __restrict__ stat,
                                                const double* __restrict__ cost,
                                                const double* __restrict__ lag, const double* __restrict__ lnlag,
                                                const int* __restrict__ cnt, const int* __restrict__ n, int max_n, int max_frames,
                                                unsigned char* __restrict__ bp, double* __restrict__ f0) {
    __shared__ double Dl[2][NST], lnl[2][NST];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int F = row_samples(n, b, max_n) / HOP + 1;                 // >= 3
    const long base = (long)b * max_frames;
    const int sl = lane < NST ? lane : 0;
    int cprev = cnt[base];
    if (lane < cprev) {
        Dl[0][lane] = cost[base * NST + lane];
        lnl[0][lane] = lnlag[base * NST + lane];
    }
    __syncthreads();
    // frame i's operands are fetched one step ahead: they do not depend on the recurrence
    int c_n = cnt[base + 1];
    double d_n = cost[(base + 1) * NST + sl], ln_n = lnlag[(base + 1) * NST + sl], r_n = rms[base + 1] / rms[base], s_n = 0.0;
    if constexpr (STAT) s_n = stat[base + 1];
    for (int i = 1; i < F; ++i) {
        const int ci = c_n, cur = i & 1, prv = cur ^ 1;
        const double d = d_n, ln_a = ln_n, rr = r_n, sp = s_n;
        if (i + 1 < F) {
            c_n = cnt[base + i + 1];
            d_n = cost[(base + i + 1) * NST + sl];
            ln_n = lnlag[(base + i + 1) * NST + sl];
            r_n = rms[base + i + 1] / rms[base + i];
            if constexpr (STAT) s_n = stat[base + i + 1];
        }
        if (lane < ci) {
            double up = VTRAN_C + VTR_A_C / rr, down = VTRAN_C + VTR_A_C * rr;         // unvoiced -> voiced, voiced -> unvoiced
            if constexpr (STAT) {
                up += VTR_S_C * sp;
                down += VTR_S_C * sp;
            }
            double best = Dl[prv][0] + (lane == 0 ? 0.0 : up);
            int arg = 0;
            for (int q = 1; q < cprev; ++q) {
                double t;
                if (lane == 0) {
                    t = down;
                } else {
                    const double xi = ln_a - lnl[prv][q];
                    t = FREQ_WT * fmin(fabs(xi), fmin(DOUBL_C + fabs(xi - LN2), DOUBL_C + fabs(xi + LN2)));
                }
                const double tot = Dl[prv][q] + t;
                if (tot < best) {
                    best = tot;
                    arg = q;
                }
            }
            Dl[cur][lane] = d + best;
            lnl[cur][lane] = ln_a;
            bp[(base + i) * BPLD + lane] = (unsigned char)arg;        // read back below by the lane that wrote it
        }
        cprev = ci;
        __syncthreads();                                              // publishes Dl[cur] and lnl[cur]
    }
    const int last = (F - 1) & 1;
    int state = 0;
    double best = Dl[last][0];
    for (int q = 1; q < cprev; ++q)
        if (Dl[last][q] < best) {
            best = Dl[last][q];
            state = q;
        }
    for (int i = F - 1; i >= 0; --i) {
        const double Lv = lag[(base + i) * NST + sl];
        const int back = i > 0 ? (int)bp[(base + i) * BPLD + sl] : 0;
        const double Ls = __shfl(Lv, state);
        if (lane == 0) f0[base + i] = state ? log(FS / Ls) : UNVOICED;
        state = __shfl(back, state);
    }
    for (int i = F + lane; i < max_frames; i += 64) f0[base + i] = UNVOICED;
}

// Levinson-Durbin on rho [LPC_ORD + 1] (LDS, read at constant offsets: the reads do not depend on the recursion), serially in the calling
// lane with a in registers (every loop unrolls).  Per step the inner product starts from rho_m and adds a_q rho_{m-q} for q = 1 .. m - 1 in
// order; a_q and a_{m-q} are updated together from their old values.  rho = (1, 0, ..) leaves a = (1, 0, ..) and E = 1.
__device__ inline void levinson(const double* rho, double (&a)[LPC_ORD + 1], double& E) {
    a[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= LPC_ORD; ++k) a[k] = 0.0;
    E = 1.0;
#pragma unroll
    for (int m = 1; m <= LPC_ORD; ++m) {
        double acc = rho[m];
#pragma unroll
        for (int q = 1; q < m; ++q) acc += a[q] * rho[m - q];
        const double kappa = -acc / E;
#pragma unroll
        for (int q = 1; 2 * q <= m; ++q) {
            const double lo = a[q], hi = a[m - q];
            a[q] = lo + kappa * hi;
            if (2 * q < m) a[m - q] = hi + kappa * lo;
        }
        a[m] = kappa;
        E = E * (1.0 - kappa * kappa);
    }
}

// grid = (max_frames, B), block = 256.  wav [B][max_n]; stat [B][max_frames]: S_i for 1 <= i < F_b, exact zeros at frame 0 and beyond F_b.
__global__ __launch_bounds__(NT) void stat_kernel(const double* __restrict__ wav, const int* __restrict__ n, int max_n, int max_frames,
                                                  double scale, double* __restrict__ stat) {
    __shared__ double buf[STAT_CHUNKS * STAT_SUMS];               // u: samples 256 f - 400 .. 256 f + 400; once y is formed, the partial sums
    __shared__ double y[2][STAT_LD];                              // window A (centred 160 samples before the frame), window B (160 after)
    __shared__ double r[STAT_SUMS], rho[STAT_SUMS];               // r^A_0 .. r^A_18, r^B_0 .. r^B_18, and rho likewise
    __shared__ double a_b[LPC_ORD + 1], c[LPC_ORD + 1], e_a;
    static_assert(STAT_SPAN <= STAT_CHUNKS * STAT_SUMS, "u fits where the partial sums go");
    double* u = buf;
    double(*part)[STAT_SUMS] = reinterpret_cast<double(*)[STAT_SUMS]>(buf);
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nb = row_samples(n, b, max_n), F = nb / HOP + 1;
    const long fr = (long)b * max_frames + f;
    if (f == 0 || f >= F) {
        if (tid == 0) stat[fr] = 0.0;
        return;
    }
    const double* x = wav + (long)b * max_n;
    const int start = HOP * f - (STAT_GAP + STAT_W) / 2;
    for (int j = tid; j < STAT_SPAN; j += NT) {
        const int i = start + j;
        u[j] = (i >= 0 && i < nb) ? scale * x[i] : 0.0;
    }
    __syncthreads();
    for (int j = tid; j < STAT_W; j += NT) {
        const double w = 0.5 - 0.5 * cos(TWO_PI * ((double)j + 0.5) / (double)STAT_W);
        y[0][j] = w * (u[j + 1] - PREEMP * u[j]);
        y[1][j] = w * (u[STAT_GAP + j + 1] - PREEMP * u[STAT_GAP + j]);
    }
    if (tid < STAT_PAD) y[0][STAT_W + tid] = y[1][STAT_W + tid] = 0.0;               // y_j = 0 for j >= 480: every chunk has 20 terms
    __syncthreads();
    if (tid < 2 * STAT_GROUPS * STAT_CHUNKS) {
        // lags k0 .. k0 + 3 of one window over j = j0 .. j0 + 19: y_{j+k0} .. y_{j+k0+3} slide through registers, so a step reads two values
        // for four multiply-adds.  (The fifth group's fourth lag would be 19: computed, not stored.)
        const int ch = tid / (2 * STAT_GROUPS), g = tid % (2 * STAT_GROUPS), w = g / STAT_GROUPS, k0 = STAT_LAGS * (g % STAT_GROUPS);
        const double* v = y[w];
        const int j0 = STAT_CHUNK * ch;                           // j + k0 + 3 <= 479 + 19: inside the zeros
        double v0 = v[j0 + k0], v1 = v[j0 + k0 + 1], v2 = v[j0 + k0 + 2], a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int j = j0; j < j0 + STAT_CHUNK; ++j) {
            const double h = v[j], v3 = v[j + k0 + 3];
            a0 += h * v0;
            a1 += h * v1;
            a2 += h * v2;
            a3 += h * v3;
            v0 = v1;
            v1 = v2;
            v2 = v3;
        }
        double* out = part[ch] + w * (LPC_ORD + 1) + k0;
        out[0] = a0;
        out[1] = a1;
        out[2] = a2;
        if (k0 + 3 <= LPC_ORD) out[3] = a3;
    }
    __syncthreads();
    if (tid < STAT_SUMS) {
        double acc = part[0][tid];
#pragma unroll
        for (int ch = 1; ch < STAT_CHUNKS; ++ch) acc += part[ch][tid];
        r[tid] = acc;
    }
    __syncthreads();
    if (tid < STAT_SUMS) {                                        // rho_0 = 1, rho_k = ff r_k / r_0; all zeros behind rho_0 when r_0 == 0
        const int k = tid % (LPC_ORD + 1);
        const double r0 = r[tid - k];
        rho[tid] = k == 0 ? 1.0 : (r0 == 0.0 ? 0.0 : STAT_FF * r[tid] / r0);
    }
    __syncthreads();
    if (tid < 2) {                                                // lanes 0 and 1 of one wavefront: window A, window B, one instruction stream
        double a[LPC_ORD + 1], E;
        levinson(rho + (tid ? LPC_ORD + 1 : 0), a, E);
        if (tid == 0) {
            e_a = E;
        } else {
#pragma unroll
            for (int k = 0; k <= LPC_ORD; ++k) a_b[k] = a[k];
        }
    }
    __syncthreads();
    if (tid <= LPC_ORD) {                                         // c_0 = sum a_q^2, c_k = 2 sum_{q <= 18 - k} a_q a_{q+k}, q in order
        double acc = 0.0;
        for (int q = 0; q + tid <= LPC_ORD; ++q) acc += a_b[q] * a_b[q + tid];
        c[tid] = tid ? 2.0 * acc : acc;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = c[0];
        for (int k = 1; k <= LPC_ORD; ++k) acc += c[k] * rho[k];
        const double d = acc / e_a;
        stat[fr] = fmin(0.2 / (fmax(d, 1.0) - 0.8), 1.0);
    }
}

constexpr long align256(long n) { return (n + 255) & ~255L; }

}  // namespace

bool pitch_lags(double lo_hz, double hi_hz, PitchLags* g) {
    if (!(lo_hz > 0.0) || !(hi_hz > 0.0) || !(lo_hz < hi_hz)) return false;
    const double lmin = floor(FS / hi_hz), lmax = ceil(FS / lo_hz);
    if (!(lmin >= PITCH_MIN_LAG) || !(lmax <= PITCH_MAX_LAG) || lmax - lmin + 1 < 3) return false;
    g->lmin = (int)lmin;
    g->lmax = (int)lmax;
    return true;
}

long pitch_scratch_bytes(int B, int max_frames, int K) {
    const long fr = (long)B * max_frames;
    return align256(fr * K * 8) + align256(fr * 8) + 3 * align256(fr * NST * 8) + align256(fr * 4) + align256(fr * BPLD);
}

long pitch_stat_scratch_bytes(int B, int max_frames, int K) { return pitch_scratch_bytes(B, max_frames, K) + align256((long)B * max_frames * 8); }

double* pitch_stat_track(void* base, int B, int max_frames, int K) { return (double*)((char*)base + pitch_scratch_bytes(B, max_frames, K)); }

PitchScratch pitch_scratch(void* base, int B, int max_frames, int K) {
    const long fr = (long)B * max_frames;
    char* p = (char*)base;
    PitchScratch sc;
    sc.phi = (double*)p;
    p += align256(fr * K * 8);
    sc.rms = (double*)p;
    p += align256(fr * 8);
    sc.cost = (double*)p;
    p += align256(fr * NST * 8);
    sc.lag = (double*)p;
    p += align256(fr * NST * 8);
    sc.lnlag = (double*)p;
    p += align256(fr * NST * 8);
    sc.cnt = (int*)p;
    p += align256(fr * 4);
    sc.bp = (unsigned char*)p;
    return sc;
}

hipError_t pitch_nccf(const double* wav, const int* n, int B, int max_n, double scale, const PitchLags& g, double* phi, double* rms,
                      hipStream_t s) {
    if (B < 1 || B > PITCH_MAX_ROWS || max_n < 513 || g.lmin < PITCH_MIN_LAG || g.lmax > PITCH_MAX_LAG || g.lmax - g.lmin + 1 < 3)
        return hipErrorInvalidValue;
    const int max_frames = max_n / HOP + 1;
    hipLaunchKernelGGL(nccf_kernel, dim3(max_frames, B), dim3(NT), 0, s, wav, n, max_n, max_frames, scale, g, phi, rms);
    return hipGetLastError();
}

hipError_t pitch_dp(const double* phi, const double* rms, const double* stat, const int* n, int B, int max_n, const PitchLags& g, double* f0,
                    const PitchScratch& sc, hipStream_t s) {
    if (B < 1 || B > PITCH_MAX_ROWS || max_n < 513 || g.lmin < PITCH_MIN_LAG || g.lmax > PITCH_MAX_LAG || g.lmax - g.lmin + 1 < 3)
        return hipErrorInvalidValue;
    const int max_frames = max_n / HOP + 1;
    hipLaunchKernelGGL(cand_kernel, dim3(max_frames, B), dim3(NT), 0, s, phi, n, max_n, max_frames, g, sc.cost, sc.lag, sc.lnlag, sc.cnt);
    if (stat)
        hipLaunchKernelGGL(dp_kernel<true>, dim3(B), dim3(64), 0, s, rms, stat, (const double*)sc.cost, (const double*)sc.lag,
                           (const double*)sc.lnlag, (const int*)sc.cnt, n, max_n, max_frames, sc.bp, f0);
    else
        hipLaunchKernelGGL(dp_kernel<false>, dim3(B), dim3(64), 0, s, rms, stat, (const double*)sc.cost, (const double*)sc.lag,
                           (const double*)sc.lnlag, (const int*)sc.cnt, n, max_n, max_frames, sc.bp, f0);
    return hipGetLastError();
}

hipError_t pitch_stationarity(const double* wav, const int* n, int B, int max_n, double scale, double* stat, hipStream_t s) {
    if (B < 1 || B > PITCH_MAX_ROWS || max_n < 513) return hipErrorInvalidValue;
    const int max_frames = max_n / HOP + 1;
    hipLaunchKernelGGL(stat_kernel, dim3(max_frames, B), dim3(NT), 0, s, wav, n, max_n, max_frames, scale, stat);
    return hipGetLastError();
}

}  // namespace ss
