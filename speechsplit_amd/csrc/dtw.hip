// Conversion scores: mel cepstra, dynamic time warping between two cepstral sequences (the path, its cost and the mel-cepstral distortion
// along it) and F0 / voicing error along a stored path.  include/speechsplit_amd.h states the definitions completely; tests/dtw_ref.py restates
// them in numpy.  In short:
//
//   cepstra   c[b][t][d] = sum_m dct[d][m] * (double)mel[b][t][m], m = 0, 1, .. in order (multiply-adds may be fused); rows at or beyond
//             len[b] are exact zeros.
//   distance  d(i, j) = scale * sqrt(sum_k (fx[i][k] - fy[j][k])^2), k in order, the root after the sum, the scale after the root.
//   DTW       steps (1,1), (1,0), (0,1) of weight 1, both ends fixed: D(0,0) = d(0,0), D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)),
//             the candidates tried in that order with a strict <, so on a tie the diagonal wins, then (i-1, j).  Backtrack from (Tx-1, Ty-1)
//             to (0,0); the path is reported first step to last, P is its length; total = D(Tx-1,Ty-1), mcd = total / P.  No band, no slope
//             constraint.
//   F0        ln Hz with -1e10 for unvoiced frames (ss_pitch_track's convention); a frame is voiced when its value is finite and > -1e9.
//             Over the P steps: n_vv both voiced, n_vu exactly one; f0_rmse_cents = (1200 / ln 2) sqrt(sum (lx - ly)^2 / n_vv); f0_corr the
//             Pearson correlation over the both-voiced steps, means first, then centred sums, sxy / sqrt(sxx syy); vuv_error = n_vu / P.
//             Every sum runs in path order, one term at a time.
//
// Float64 throughout, no atomics, every sum in a fixed order: the same bits on every run, and a pair inside a ragged batch gives what it
// gives alone.  D depends on one add per cell, so how the lattice is tiled cannot show in the result.  The header allows fused
// multiply-adds in the cepstra and the distance; these kernels do NOT fuse them (contraction is off for this file), so that every result is the numpy
// restatement's term-by-term sum to the bit and a tie in exact arithmetic is a tie here.  It costs the distance loop a third more
// instructions (subtract, multiply, add for subtract, multiply-add).
//
// Three kernels:
//
//   cepstra_kernel  one thread per output (t, d); trivially parallel.
//   dtw_kernel      one workgroup of four wavefronts per pair.  The Tx x Ty distance matrix is never materialised.  The lattice is cut into
//                   row strips of NT = 64 rows; lane t of EVERY wavefront keeps fx[i0 + t] in registers (DIMB doubles, dim rounded up to a
//                   multiple of 8 and padded with zeros: a zero term adds exactly nothing to a non-negative sum).  The columns are swept as
//                   a skewed wavefront, lane t at column j = s - t in step s, NB = 16 steps at a time in two phases.  (A) The distances of
//                   the block's 16 x 64 cells do not hang on the recurrence: the four wavefronts compute four steps each, branch-free, into
//                   LDS.  fy comes through LDS too, transposed ([k][column], a ring of 128 columns refilled 64 at a time) so that the lanes
//                   of one read touch consecutive doubles.  (B) Wavefront 0 alone runs the recurrence over the 16 steps: D(i-1, j) is the
//                   upper lane's previous result (one cross-lane move a step, the only thing a step waits for: its distance and lane 0's
//                   boundary value are read a step ahead), D(i-1, j-1) the value that move delivered a step earlier, D(i, j-1) the lane's
//                   own previous result.  Lane 63 writes the strip's bottom row of D to scratch; it is the next strip's top boundary and is
//                   staged through LDS with the fy columns (in place: a column is read into LDS at least 63 steps before it is
//                   overwritten).  Backpointers are 2 bits a cell, four columns to a byte, each byte written once by the lane that owns the
//                   row.  Then thread 0 backtracks (positions, not stored codes, decide at the lattice's edges, so a corrupt byte changes
//                   numbers, never addresses), the workgroup moves the path to the front of its buffer and fills the rest with -1.
//                   Bound: ceil(Tx / 64) x (Ty + 63) sequential steps a pair, each one cross-lane move, two compares and an add on the
//                   chain, plus a quarter of a distance (DIMB LDS reads, subtracts, multiplies and adds, one root) per wavefront; the
//                   backtrack adds P dependent byte loads.
//   f0_kernel       one wavefront per pair: the lanes gather 64 path steps at a time into LDS, lane 0 sums them in path order (two passes:
//                   counts, squared differences and means, then the centred sums).  Path entries are clamped into the lattice.
#include "common.h"
#include "kernels.h"

#include <math.h>

// no fused multiply-adds anywhere below: see the note on arithmetic above
#pragma clang fp contract(off)

namespace ss {

namespace {

constexpr int NT = DTW_STRIP, RING = 2 * NT, NTH = 4 * NT, NB = 16;     // strip height, fy ring, threads of the DTW workgroup, steps a block
constexpr double UNVOICED_BELOW = -1e9, CENTS = 1731.2340490667560888;      // 1200 / ln 2

__device__ inline int row_len(const int* len, int b, int max_t) {
    const int v = len ? len[b] : max_t;
    return v < 1 ? 1 : (v > max_t ? max_t : v);
}

// grid = (ceil(max_t * n_ceps / 256), B), block = 256.  mel [B][max_t][n_mels] f32; dct [n_ceps][n_mels]; out [B][max_t][n_ceps].
__global__ __launch_bounds__(256) void cepstra_kernel(const float* __restrict__ mel, const int* __restrict__ len, int max_t, int n_mels,
                                                      const double* __restrict__ dct, int n_ceps, double* __restrict__ out) {
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= max_t * n_ceps) return;
    const int t = e / n_ceps, d = e - t * n_ceps;
    double acc = 0.0;
    if (t < row_len(len, b, max_t)) {
        const float* x = mel + ((long)b * max_t + t) * n_mels;
        const double* w = dct + (long)d * n_mels;
        for (int m = 0; m < n_mels; ++m) acc += w[m] * (double)x[m];
    }
    out[(long)b * max_t * n_ceps + e] = acc;
}

// grid = B, block = 256 (four wavefronts).  fx [B][max_tx][dim], fy [B][max_ty][dim]; out [B][3]; path [B][max_tx + max_ty - 1][2] or
// nullptr; bp [B][bp_stride] bytes (row i of a pair at i * ceil(max_ty / 4)); brow [B][brow_stride] doubles.
template <int DIMB>
__global__ __launch_bounds__(NTH) void dtw_kernel(const double* __restrict__ fx, const int* __restrict__ tx, const double* __restrict__ fy,
                                                  const int* __restrict__ ty, int max_tx, int max_ty, int dim, double scale,
                                                  double* __restrict__ out, int* __restrict__ path, int* __restrict__ path_len,
                                                  unsigned char* __restrict__ bp, long bp_stride, double* __restrict__ brow,
                                                  long brow_stride) {
    __shared__ double fyT[DIMB * RING];               // [k][column & (RING - 1)]
    __shared__ double top[RING];                      // the previous strip's bottom row of D, the same ring
    __shared__ double dS[(NB + 1) * NT];              // [step of the block][lane]: the distances of the block's cells (+ a row to read ahead into)
    __shared__ double total_s;
    __shared__ int plen_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (NT - 1), wave = tid / NT;
    const int Tx = row_len(tx, b, max_tx), Ty = row_len(ty, b, max_ty);
    const int ldb = (max_ty + 3) >> 2;
    fx += (long)b * max_tx * dim;
    fy += (long)b * max_ty * dim;
    bp += b * bp_stride;
    brow += b * brow_stride;
    for (int e = tid; e < DIMB * RING; e += NTH) fyT[e] = 0.0;          // the padding rows k >= dim stay zero; every column is finite
    const int strips = (Tx + NT - 1) / NT;
    for (int r = 0; r < strips; ++r) {
        const int i = r * NT + lane;                                     // every wavefront holds the strip's rows: lane t has row i0 + t
        const bool row_on = i < Tx;
        double x[DIMB];
#pragma unroll
        for (int k = 0; k < DIMB; ++k) x[k] = (row_on && k < dim) ? fx[(long)i * dim + k] : 0.0;
        const bool more = r + 1 < strips;                                // lane 63's row is the next strip's boundary
        const int steps = Ty + (Tx - r * NT < NT ? Tx - r * NT : NT) - 1;
        double mine = INFINITY, up_prev = INFINITY;
        unsigned code_acc = 0;
        for (int s0 = 0; s0 < steps; s0 += NB) {
            __syncthreads();                                             // the sweep of the block before is done with dS (and top)
            if ((s0 & (NT - 1)) == 0) {                                  // columns s0 .. s0 + 63 enter the ring
                const int cols = Ty - s0 < NT ? Ty - s0 : NT;
                for (int e = tid; e < cols * dim; e += NTH) {
                    const int jj = e / dim, k = e - jj * dim;
                    fyT[k * RING + ((s0 + jj) & (RING - 1))] = fy[(long)s0 * dim + e];
                }
                if (r > 0 && tid < cols) top[(s0 + tid) & (RING - 1)] = brow[s0 + tid];
                __syncthreads();
            }
            // the distances of the block's NB steps, NB / 4 to a wavefront, no branch: a lane whose column s - lane lies outside the lattice
            // reads some other column of the ring and its value is never used
#pragma unroll 2
            for (int u = wave; u < NB; u += NTH / NT) {
                const double* col = fyT + ((s0 + u - lane) & (RING - 1));
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < DIMB; ++k) {
                    const double df = x[k] - col[k * RING];
                    acc += df * df;
                }
                dS[u * NT + lane] = scale * sqrt(acc);
            }
            __syncthreads();
            if (wave != 0) continue;                                     // the recurrence is one wavefront's
            const int ub = steps - s0 < NB ? steps - s0 : NB;
            // the step's operands that do not hang on the recurrence are read a step ahead, so a step waits for one cross-lane move only
            double d_n = dS[lane], t_n = top[(s0 - lane) & (RING - 1)];
            for (int u = 0; u < ub; ++u) {
                const int j = s0 + u - lane;
                const double d = d_n, t = t_n;
                d_n = dS[(u + 1) * NT + lane];                           // row NB exists and is never used
                t_n = top[(j + 1) & (RING - 1)];                         // lane 0: column j + 1 of the boundary row
                double up = __shfl_up(mine, 1);                          // D(i-1, j): what the upper lane made a step ago
                if (lane == 0) up = (r > 0 && j < Ty) ? t : INFINITY;    // ... or the strip before
                const double diag0 = up_prev;                            // D(i-1, j-1): what `up` was a step ago
                up_prev = up;
                if (row_on && j >= 0 && j < Ty) {
                    const double left = j > 0 ? mine : INFINITY;
                    double best = j > 0 ? diag0 : INFINITY;
                    unsigned code = 0;
                    if (up < best) {
                        best = up;
                        code = 1;
                    }
                    if (left < best) {
                        best = left;
                        code = 2;
                    }
                    mine = (i == 0 && j == 0) ? d : d + best;
                    code_acc |= code << (2 * (j & 3));
                    if ((j & 3) == 3 || j == Ty - 1) {
                        bp[(long)i * ldb + (j >> 2)] = (unsigned char)code_acc;
                        code_acc = 0;
                    }
                    if (more && lane == NT - 1) brow[j] = mine;
                    if (i == Tx - 1 && j == Ty - 1) total_s = mine;
                }
            }
        }
    }
    __syncthreads();                                                     // publishes bp, brow (this workgroup's own stores) and total_s
    const int cap = max_tx + max_ty - 1;
    if (path) path += (long)b * cap * 2;
    if (tid == 0) {
        int i = Tx - 1, j = Ty - 1, n = 0;
        for (;;) {
            if (path) {                                                  // reversed, at the buffer's end
                path[2 * (cap - 1 - n)] = i;
                path[2 * (cap - 1 - n) + 1] = j;
            }
            ++n;
            if (i == 0 && j == 0) break;
            unsigned code = (bp[(long)i * ldb + (j >> 2)] >> (2 * (j & 3))) & 3u;
            if (i == 0) code = 2;
            else if (j == 0) code = 1;
            if (code != 2) --i;
            if (code != 1) --j;
        }
        plen_s = n;
        const double total = total_s;
        out[3 * b] = total;
        out[3 * b + 1] = (double)n;
        out[3 * b + 2] = total / (double)n;
        if (path_len) path_len[b] = n;
    }
    __syncthreads();
    if (path) {
        const int P = plen_s, off = 2 * (cap - P);                       // ints to move down by
        if (off > 0)
            for (int q = 0; q < 2 * P; q += NTH) {                       // ascending: a chunk's sources lie at or beyond its destinations
                const int v = q + tid < 2 * P ? path[q + tid + off] : 0;
                __syncthreads();
                if (q + tid < 2 * P) path[q + tid] = v;
                __syncthreads();
            }
        for (int q = 2 * P + tid; q < 2 * cap; q += NTH) path[q] = -1;
    }
}

// grid = B, block = 64.  path [B][cap][2], f0x [B][max_tx], f0y [B][max_ty], out [B][5].
__global__ __launch_bounds__(NT) void f0_kernel(const int* __restrict__ path, const int* __restrict__ path_len,
                                                const double* __restrict__ f0x, const double* __restrict__ f0y, int max_tx, int max_ty,
                                                double* __restrict__ out) {
    __shared__ double lx[NT], ly[NT];
    __shared__ int kind[NT];                                             // 2 both voiced, 1 exactly one, 0 neither
    __shared__ double mean_s[2];
    const int b = blockIdx.x, lane = threadIdx.x, cap = max_tx + max_ty - 1;
    int P = path_len ? path_len[b] : cap;
    P = P < 0 ? 0 : (P > cap ? cap : P);
    path += (long)b * cap * 2;
    f0x += (long)b * max_tx;
    f0y += (long)b * max_ty;
    double n_vv = 0.0, n_vu = 0.0, sq = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int q = 0; q < P; q += NT) {
            __syncthreads();
            if (q + lane < P) {
                int i = path[2 * (q + lane)], j = path[2 * (q + lane) + 1];
                i = i < 0 ? 0 : (i >= max_tx ? max_tx - 1 : i);
                j = j < 0 ? 0 : (j >= max_ty ? max_ty - 1 : j);
                const double a = f0x[i], c = f0y[j];
                const bool va = isfinite(a) && a > UNVOICED_BELOW, vc = isfinite(c) && c > UNVOICED_BELOW;
                lx[lane] = a;
                ly[lane] = c;
                kind[lane] = (va && vc) ? 2 : ((va || vc) ? 1 : 0);
            }
            __syncthreads();
            if (lane == 0) {
                const int n = P - q < NT ? P - q : NT;
                if (pass == 0) {
                    for (int u = 0; u < n; ++u) {
                        if (kind[u] == 2) {
                            const double df = lx[u] - ly[u];
                            n_vv += 1.0;
                            sq += df * df;
                            sx += lx[u];
                            sy += ly[u];
                        } else if (kind[u] == 1) {
                            n_vu += 1.0;
                        }
                    }
                } else {
                    const double mx = mean_s[0], my = mean_s[1];
                    for (int u = 0; u < n; ++u)
                        if (kind[u] == 2) {
                            const double a = lx[u] - mx, c = ly[u] - my;
                            sxx += a * a;
                            syy += c * c;
                            sxy += a * c;
                        }
                }
            }
        }
        if (lane == 0 && pass == 0) {
            mean_s[0] = sx / n_vv;
            mean_s[1] = sy / n_vv;
        }
    }
    if (lane == 0) {
        out[5 * b] = n_vv;
        out[5 * b + 1] = n_vu;
        out[5 * b + 2] = n_vv > 0.0 ? CENTS * sqrt(sq / n_vv) : NAN;
        out[5 * b + 3] = (n_vv >= 2.0 && sxx > 0.0 && syy > 0.0) ? sxy / sqrt(sxx * syy) : NAN;
        out[5 * b + 4] = n_vu / (double)P;
    }
}

constexpr long align256(long n) { return (n + 255) & ~255L; }

}  // namespace

long dtw_scratch_bytes(int B, int max_tx, int max_ty) {
    return (long)B * (align256((long)max_tx * ((max_ty + 3) >> 2)) + align256((long)max_ty * 8));
}

DtwScratch dtw_scratch(void* base, int B, int max_tx, int max_ty) {
    DtwScratch sc;
    sc.bp_stride = align256((long)max_tx * ((max_ty + 3) >> 2));
    sc.brow_stride = align256((long)max_ty * 8) / 8;
    sc.bp = (unsigned char*)base;
    sc.brow = (double*)((char*)base + (long)B * sc.bp_stride);
    return sc;
}

hipError_t mel_cepstra(const float* mel, const int* len, int B, int max_t, int n_mels, const double* dct, int n_ceps, double* out,
                       hipStream_t s) {
    if (B < 1 || B > DTW_MAX_ROWS || max_t < 1 || n_mels < 1 || n_ceps < 1 || n_ceps > DTW_MAX_DIM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cepstra_kernel, dim3((max_t * n_ceps + 255) / 256, B), dim3(256), 0, s, mel, len, max_t, n_mels, dct, n_ceps, out);
    return hipGetLastError();
}

hipError_t dtw(const double* fx, const int* tx, const double* fy, const int* ty, int B, int max_tx, int max_ty, int dim, double scale,
               double* out, int* path, int* path_len, const DtwScratch& sc, hipStream_t s) {
    if (B < 1 || B > DTW_MAX_ROWS || max_tx < 1 || max_ty < 1 || dim < 1 || dim > DTW_MAX_DIM) return hipErrorInvalidValue;
#define SS_DTW_LAUNCH(D)                                                                                                                  \
    hipLaunchKernelGGL(dtw_kernel<D>, dim3(B), dim3(NTH), 0, s, fx, tx, fy, ty, max_tx, max_ty, dim, scale, out, path, path_len, sc.bp, \
                       sc.bp_stride, sc.brow, sc.brow_stride)
    if (dim <= 8) SS_DTW_LAUNCH(8);
    else if (dim <= 16) SS_DTW_LAUNCH(16);
    else if (dim <= 24) SS_DTW_LAUNCH(24);
    else if (dim <= 32) SS_DTW_LAUNCH(32);
    else SS_DTW_LAUNCH(40);
#undef SS_DTW_LAUNCH
    return hipGetLastError();
}

hipError_t path_f0_stats(const int* path, const int* path_len, const double* f0x, const double* f0y, int B, int max_tx, int max_ty,
                         double* out, hipStream_t s) {
    if (B < 1 || B > DTW_MAX_ROWS || max_tx < 1 || max_ty < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_kernel, dim3(B), dim3(NT), 0, s, path, path_len, f0x, f0y, max_tx, max_ty, out);
    return hipGetLastError();
}

}  // namespace ss
