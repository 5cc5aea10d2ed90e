// Griffin-Lim vocoder: mel spectrogram -> linear magnitude -> waveform, the checkpoint-free stand-in for the last cell of the reference's
// demo.ipynb (which needs wavenet_vocoder and an external checkpoint).  It inverts exactly what features.hip computes: the reference's
// pySTFT framing (utils.py:18-31: reflect padding by 512, periodic Hann window, 1024-point rfft, hop 256) and the dB / [0, 1] scaling of
// make_spect_f0.py:59-60.  The algorithm is Griffin-Lim with momentum as published (Perraudin, Balazs, Sondergaard 2013; librosa's form):
//
//     ang = exp(i phase0);  tprev = 0
//     n_iter times:  r = STFT(ISTFT(S ang));  a = r - momentum / (1 + momentum) tprev;  tprev = r;  ang = a / (|a| + 1e-16)
//     x = ISTFT(S ang)
//
// One iteration is three launches: irfft_kernel (one workgroup per frame: S ang -> windowed time frame), ola_kernel (a gather per output
// sample over the <= 4 frames that cover it, in frame order, divided by the sum of their squared windows; no atomics) and stft_kernel with the
// projection (a, tprev, S ang) in its epilogue.  Nothing waits across workgroups, so the result is the same bits on every run.
//
// Arithmetic: float64 throughout, as features.hip -- the iteration amplifies a transform's rounding by about 10^4 over 32 rounds (measured in
// numpy), which float32 transforms would turn into an audible-level disagreement with any reference.  The transform is a real FFT:
// 60 rounds of a transform and its inverse over a batch of conditions is where features.hip's direct DFT (1024 x 513 multiply-adds a frame)
// stops being cheap.  1024-point complex radix-2 decimation in frequency, in place in LDS, output read in bit-reversed order; the twiddles come
// from sincospi, exact to double rounding.
//
// Mel -> linear: mel_to_linear_kernel applies a caller-supplied pseudo-inverse and floors; mel_nnls_kernel goes on from there to the
// non-negative magnitude whose mel is the given one, by projected FISTA, the whole iteration of a frame in one launch with the banded mel
// basis packed in LDS (include/speechsplit_amd.h, ss_mel_to_linear_nnls; zero iterations are mel_to_linear_kernel to the bit).  With an F0
// track, mel_harmonic_kernel overwrites the voiced frames with one fitted amplitude per harmonic plus a noise part, and harmonic_u_kernel /
// harmonic_phase_kernel turn the track and the harmonic share into the phases Griffin-Lim starts from (ss_mel_to_linear_harmonic,
// ss_harmonic_phase).
//
// Batches: row b has its own frame count F_b = min(max(frames[b], 4), max_frames) and n_b = 256 (F_b - 1) samples; every kernel computes row b
// as if it were alone, never reads a spectrogram frame at or beyond F_b, and writes exact zeros behind n_b.
#include "common.h"
#include "fft_lds.h"
#include "kernels.h"

namespace ss {

namespace {

using namespace fftlds;

// sample j of a row with F frames: the frames that cover padded position j + 512, in frame order, over the sum of their squared windows
__host__ __device__ inline double ola_sample(const double* __restrict__ fb, int F, int j) {
    const int p = j + NFFT / 2, q = p / HOP;
    const int lo = q - 3 > 0 ? q - 3 : 0, hi = q < F - 1 ? q : F - 1;
    double acc = 0.0, nrm = 0.0;
    for (int f = lo; f <= hi; ++f) {
        const int i = p - f * HOP;
        const double w = hann(i);
        acc += fb[(long)f * NFFT + i];
        nrm += w * w;
    }
    return acc / nrm;
}

// grid = (max_frames, B), block = 256.  wav [B][256 (max_frames - 1)]; out / mag / tprev [B][max_frames][513] (x 2 for the complex ones).
// Plain (mag == nullptr): spec rows at or beyond the row's frames are zeros.  Projection: those blocks touch nothing.
__global__ __launch_bounds__(NT) void stft_kernel(const double* __restrict__ wav, const int* __restrict__ frames, int max_frames,
                                                  double* __restrict__ out, const double* __restrict__ mag, double* __restrict__ tprev,
                                                  double coef) {
    __shared__ FftLds L;
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int F = row_frames(frames, b, max_frames);
    const long fr = (long)b * max_frames + f;
    out += fr * (2 * NBIN);
    if (f >= F) {
        if (!mag)
            for (int k = tid; k < 2 * NBIN; k += NT) out[k] = 0.0;
        return;
    }
    fft_twiddles(L, tid);
    stft_load(L, tid, wav + (long)b * HOP * (max_frames - 1), HOP * (F - 1), f);
    __syncthreads();
    for (int s = 0; s < LOGN; ++s) {
        fft_stage(L, tid, s, false);
        __syncthreads();
    }
    stft_store(L, tid, out, mag ? mag + fr * NBIN : nullptr, mag ? tprev + fr * (2 * NBIN) : nullptr, coef);
}

// grid = (max_frames, B), block = 256: spec [B][max_frames][513][2] -> frame_buf [B][max_frames][1024] = window * irfft, frames < F_b only
__global__ __launch_bounds__(NT) void irfft_kernel(const double* __restrict__ spec, const int* __restrict__ frames, int max_frames,
                                                   double* __restrict__ frame_buf) {
    __shared__ FftLds L;
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (f >= row_frames(frames, b, max_frames)) return;
    const long fr = (long)b * max_frames + f;
    fft_twiddles(L, tid);
    irfft_load(L, tid, spec + fr * (2 * NBIN));
    __syncthreads();
    for (int s = 0; s < LOGN; ++s) {
        fft_stage(L, tid, s, true);
        __syncthreads();
    }
    irfft_store(L, tid, frame_buf + fr * NFFT);
}

// grid = (max_frames - 1, B), block = 256: one output sample per thread; zeros behind the row's own samples
__global__ __launch_bounds__(NT) void ola_kernel(const double* __restrict__ frame_buf, const int* __restrict__ frames, int max_frames,
                                                 double* __restrict__ wav) {
    const int b = blockIdx.y, j = blockIdx.x * NT + threadIdx.x;
    const int F = row_frames(frames, b, max_frames);
    wav[(long)b * HOP * (max_frames - 1) + j] = j < HOP * (F - 1) ? ola_sample(frame_buf + (long)b * max_frames * NFFT, F, j) : 0.0;
}

// grid = (max_frames, B), block = 256: proj = mag exp(i phase0) (phase0 == nullptr: mag), tprev = 0, frames < F_b only
__global__ __launch_bounds__(NT) void gl_init_kernel(const double* __restrict__ mag, const double* __restrict__ phase0,
                                                     const int* __restrict__ frames, int max_frames, double* __restrict__ proj,
                                                     double* __restrict__ tprev) {
    const int f = blockIdx.x, b = blockIdx.y;
    if (f >= row_frames(frames, b, max_frames)) return;
    const long fr = (long)b * max_frames + f;
    for (int k = threadIdx.x; k < NBIN; k += NT) {
        const double m = mag[fr * NBIN + k];
        double s = 0.0, c = 1.0;
        if (phase0) sincos(phase0[fr * NBIN + k], &s, &c);
        proj[(fr * NBIN + k) * 2] = m * c;
        proj[(fr * NBIN + k) * 2 + 1] = m * s;
        tprev[(fr * NBIN + k) * 2] = 0.0;
        tprev[(fr * NBIN + k) * 2 + 1] = 0.0;
    }
}

// grid = (max_frames, B), block = 256, dynamic LDS = n_mels doubles: the inverse of melspec_kernel's last two lines, then the projection
// onto the linear bins through a caller-supplied [n_mels][513] matrix.  Rows at or beyond the row's frames: mel is not read, mag is zeros.
__global__ __launch_bounds__(NT) void mel_to_linear_kernel(const float* __restrict__ mel, const double* __restrict__ inv_basis,
                                                           const int* __restrict__ frames, int max_frames, int n_mels, double floor,
                                                           double* __restrict__ mag) {
    extern __shared__ double amp[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long fr = (long)b * max_frames + f;
    if (f >= row_frames(frames, b, max_frames)) {
        for (int k = tid; k < NBIN; k += NT) mag[fr * NBIN + k] = 0.0;
        return;
    }
    for (int m = tid; m < n_mels; m += NT) amp[m] = pow(10.0, (100.0 * (double)mel[fr * n_mels + m] - 100.0 + 16.0) / 20.0);
    __syncthreads();
    for (int k = tid; k < NBIN; k += NT) {
        double s = 0.0;
        for (int m = 0; m < n_mels; ++m) s += amp[m] * inv_basis[(long)m * NBIN + k];
        mag[fr * NBIN + k] = fmax(floor, s);
    }
}

// grid = (max_frames, B), block = 256, dynamic LDS = nnls_lds_bytes(n_mels, packed_doubles): non-negative mel inversion by projected FISTA
// (include/speechsplit_amd.h, ss_mel_to_linear_nnls), the whole iteration of one frame inside one launch.  The basis arrives packed by
// ss_mel_nnls_pack -- per band (first bin, run length), then every band's run of weights -- and is unpacked once into LDS; x and y of bins
// tid, tid + 256 and (thread 0) 512 stay in registers; per iteration y goes to LDS, a barrier, thread m < n_mels sums band m over its run in
// bin order, a barrier, every thread sums its bins' gradient over the covering bands in band order.  No global traffic inside the loop, no
// atomics, every sum in one fixed order.  Every index taken from `packed` is clamped: first bin into 0 .. 512, run length into what is left
// of the 513 bins and of the packed weights, so a corrupt buffer changes numbers, never addresses.  Rows at or beyond the row's frames: mel
// is not read, mag is zeros.  The starting product is mel_to_linear_kernel's, term for term.
__global__ __launch_bounds__(NT) void mel_nnls_kernel(const float* __restrict__ mel, const double* __restrict__ inv_basis,
                                                      const double* __restrict__ packed, int packed_doubles,
                                                      const int* __restrict__ frames, int max_frames, int n_mels, int n_iter, double step,
                                                      double floor, double* __restrict__ mag) {
    extern __shared__ double lds[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long fr = (long)b * max_frames + f;
    if (f >= row_frames(frames, b, max_frames)) {
        for (int k = tid; k < NBIN; k += NT) mag[fr * NBIN + k] = 0.0;
        return;
    }
    const int nnz = packed_doubles - 2 * n_mels;
    double* w = lds;                    // [nnz]
    double* amp = w + nnz;              // [n_mels]
    double* r = amp + n_mels;           // [n_mels]
    double* ys = r + n_mels;            // [NBIN + 1]
    int* lo = (int*)(ys + NBIN + 1);    // [n_mels]      first bin of band m
    int* off = lo + n_mels;             // [n_mels + 1]  band m's weights are w[off[m] .. off[m + 1])
    for (int m = tid; m < n_mels; m += NT) {
        amp[m] = pow(10.0, (100.0 * (double)mel[fr * n_mels + m] - 100.0 + 16.0) / 20.0);
        const double first = packed[2 * m];
        lo[m] = first >= 0.0 ? (first <= (double)(NBIN - 1) ? (int)first : NBIN - 1) : 0;       // NaN: 0
    }
    for (int i = tid; i < nnz; i += NT) w[i] = packed[2 * n_mels + i];
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int m = 0; m < n_mels; ++m) {
            const double run = packed[2 * m + 1];
            int len = run >= 0.0 ? (run <= (double)NBIN ? (int)run : NBIN) : 0;                 // NaN: 0
            len = min(len, min(NBIN - lo[m], nnz - o));
            off[m] = o;
            o += len;
        }
        off[n_mels] = o;
    }
    __syncthreads();

    constexpr int PER = (NBIN + NT - 1) / NT;   // 3: bins tid, tid + 256, tid + 512
    double x[PER], y[PER];
    int mfirst[PER], mlast[PER];                // the bands that cover the bin lie in mfirst .. mlast (empty: mfirst > mlast)
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int k = tid + j * NT;
        x[j] = y[j] = 0.0;
        mfirst[j] = n_mels;
        mlast[j] = -1;
        if (k < NBIN) {
            double s = 0.0;
            for (int m = 0; m < n_mels; ++m) s += amp[m] * inv_basis[(long)m * NBIN + k];
            x[j] = y[j] = fmax(s, 0.0);
            for (int m = 0; m < n_mels; ++m)
                if (k >= lo[m] && k - lo[m] < off[m + 1] - off[m]) {
                    mfirst[j] = min(mfirst[j], m);
                    mlast[j] = m;
                }
        }
    }
    double t = 1.0;
    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (tid + j * NT < NBIN) ys[tid + j * NT] = y[j];
        __syncthreads();
        for (int m = tid; m < n_mels; m += NT) {
            const int o = off[m], len = off[m + 1] - o, k0 = lo[m];
            double s = 0.0;
            for (int i = 0; i < len; ++i) s += ys[k0 + i] * w[o + i];
            r[m] = s - amp[m];
        }
        __syncthreads();
        const double tn = (1.0 + sqrt(1.0 + 4.0 * t * t)) / 2.0;
        const double beta = (t - 1.0) / tn;
        t = tn;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = tid + j * NT;
            double g = 0.0;
            for (int m = mfirst[j]; m <= mlast[j]; ++m) {
                const int i = k - lo[m];
                if (i >= 0 && i < off[m + 1] - off[m]) g += r[m] * w[off[m] + i];
            }
            const double xn = fmax(y[j] - step * g, 0.0);
            y[j] = xn + beta * (xn - x[j]);
            x[j] = xn;
        }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (tid + j * NT < NBIN) mag[fr * NBIN + tid + j * NT] = fmax(x[j], floor);
}

// ---- F0-guided harmonic inversion (include/speechsplit_amd.h, ss_mel_to_linear_harmonic / ss_harmonic_phase)
constexpr double HARM_BIN_HZ = 15.625;      // 16000 / 1024

// finite and inside 40 .. 1000 Hz; NaN compares false
__device__ inline bool harm_voiced(double f) { return f >= 40.0 && f <= 1000.0; }

__device__ inline int harm_count(double f, double f_top) {
    const double h = floor(f_top / f);
    return h < (double)HARM_MAX ? (h > 1.0 ? (int)h : 1) : HARM_MAX;
}

__device__ inline double sincpi(double x) { return x == 0.0 ? 1.0 : sinpi(x) / (M_PI * x); }

// the main lobe of the periodic Hann window's transform, as three shifted sincs: the closed form cancels near d = +-1
__device__ inline double hann_lobe(double d) {
    return fabs(d) < 2.0 ? 0.5 * sincpi(d) + 0.25 * sincpi(d - 1.0) + 0.25 * sincpi(d + 1.0) : 0.0;
}

// grid = (max_frames, B), block = 256, dynamic LDS = mel_harmonic_lds_bytes(n_mels, packed_doubles): one amplitude per harmonic of the
// frame's F0 by projected FISTA from zero, the whole fit of one frame inside one launch.  The basis is mel_nnls_kernel's packed image with
// the same clamping; beside it sit amp, r, the 513-bin model and its gradient, and -- because a bin's model is a gather over the
// harmonics that cover it -- every harmonic's y, first bin and four weights.  Thread h - 1 keeps harmonic h's atom, a and y in registers.
// Per round: the bins' model over the covering harmonics in ascending h, a barrier, band m's sum over its run in bin order (thread m), a
// barrier, the bins' gradient over the covering bands in band order, a barrier, each harmonic's four-term dot product and the projected
// update, a barrier.  No global traffic inside the loop, no atomics, every sum in one fixed order.  The step bound comes out of the same
// three passes run once on ones.  Frames at or beyond the row's, and unvoiced frames: mel is not read, mag is left as it is, share is zeros.
__global__ __launch_bounds__(NT) void mel_harmonic_kernel(const float* __restrict__ mel, const double* __restrict__ f0_hz,
                                                          const double* __restrict__ inv_basis, const double* __restrict__ packed,
                                                          int packed_doubles, const int* __restrict__ frames, int max_frames, int n_mels,
                                                          double f_top, int n_iter, double floor_, double* __restrict__ mag,
                                                          double* __restrict__ share) {
    extern __shared__ double lds[];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long fr = (long)b * max_frames + f;
    const double hz = f < row_frames(frames, b, max_frames) ? f0_hz[fr] : 0.0;
    if (!harm_voiced(hz)) {
        for (int k = tid; k < NBIN; k += NT) share[fr * NBIN + k] = 0.0;
        return;
    }
    const int H = harm_count(hz, f_top);
    const int nnz = packed_doubles - 2 * n_mels;
    double* w = lds;                        // [nnz]
    double* amp = w + nnz;                  // [n_mels]
    double* r = amp + n_mels;               // [n_mels]
    double* model = r + n_mels;             // [NBIN + 1]
    double* grad = model + NBIN + 1;        // [NBIN + 1]
    double* ys = grad + NBIN + 1;           // [HARM_MAX]
    double* aw = ys + HARM_MAX;             // [HARM_MAX][4]  harmonic h's weights on bins k0 .. k0 + 3
    int* lo = (int*)(aw + 4 * HARM_MAX);    // [n_mels]      first bin of band m
    int* off = lo + n_mels;                 // [n_mels + 1]  band m's weights are w[off[m] .. off[m + 1])
    int* k0s = off + n_mels + 1;            // [HARM_MAX]    first bin of harmonic h's atom
    for (int m = tid; m < n_mels; m += NT) {
        amp[m] = pow(10.0, (100.0 * (double)mel[fr * n_mels + m] - 100.0 + 16.0) / 20.0);
        const double first = packed[2 * m];
        lo[m] = first >= 0.0 ? (first <= (double)(NBIN - 1) ? (int)first : NBIN - 1) : 0;       // NaN: 0
    }
    for (int i = tid; i < nnz; i += NT) w[i] = packed[2 * n_mels + i];
    int k0 = 0;
    double wt[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid < H) {
        const double p = ((double)(tid + 1) * hz) / HARM_BIN_HZ;
        const double base = floor(p) - 1.0;
        k0 = base >= 0.0 ? (base <= (double)(NBIN - 1) ? (int)base : NBIN - 1) : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wt[j] = k0 + j < NBIN ? 512.0 * hann_lobe((double)(k0 + j) - p) : 0.0;
            aw[4 * tid + j] = wt[j];
        }
        k0s[tid] = k0;
        ys[tid] = 1.0;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int m = 0; m < n_mels; ++m) {
            const double run = packed[2 * m + 1];
            int len = run >= 0.0 ? (run <= (double)NBIN ? (int)run : NBIN) : 0;                 // NaN: 0
            len = min(len, min(NBIN - lo[m], nnz - o));
            off[m] = o;
            o += len;
        }
        off[n_mels] = o;
    }
    __syncthreads();

    constexpr int PER = (NBIN + NT - 1) / NT;   // 3: bins tid, tid + 256 and (thread 0) 512
    int mfirst[PER], mlast[PER];                // the bands that cover the bin lie in mfirst .. mlast (empty: mfirst > mlast)
    int hfirst[PER], hlast[PER];                // likewise the harmonics (0-based)
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int k = tid + j * NT;
        mfirst[j] = n_mels;
        hfirst[j] = H;
        mlast[j] = hlast[j] = -1;
        if (k < NBIN) {
            for (int m = 0; m < n_mels; ++m)
                if (k >= lo[m] && k - lo[m] < off[m + 1] - off[m]) {
                    mfirst[j] = min(mfirst[j], m);
                    mlast[j] = m;
                }
            for (int h = 0; h < H; ++h)
                if (k >= k0s[h] && k - k0s[h] < 4) {
                    hfirst[j] = min(hfirst[j], h);
                    hlast[j] = h;
                }
        }
    }
    // the three passes of a round; the caller puts a barrier between any two
    auto bins_model = [&]() {                   // model = D ys
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = tid + j * NT;
            if (k >= NBIN) continue;
            double s = 0.0;
            for (int h = hfirst[j]; h <= hlast[j]; ++h) {
                const int i = k - k0s[h];
                if (i >= 0 && i < 4) s += aw[4 * h + i] * ys[h];
            }
            model[k] = s;
        }
    };
    auto band_sum = [&](int m) {                // (model B)_m
        const int o = off[m], len = off[m + 1] - o, kb = lo[m];
        double s = 0.0;
        for (int i = 0; i < len; ++i) s += model[kb + i] * w[o + i];
        return s;
    };
    auto bins_grad = [&]() {                    // grad = B r
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = tid + j * NT;
            if (k >= NBIN) continue;
            double g = 0.0;
            for (int m = mfirst[j]; m <= mlast[j]; ++m) {
                const int i = k - lo[m];
                if (i >= 0 && i < off[m + 1] - off[m]) g += r[m] * w[off[m] + i];
            }
            grad[k] = g;
        }
    };
    auto atom_dot = [&]() {                     // (D^T grad)_h; a weight behind bin 512 is zero and its index is held inside
        double g = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) g += wt[j] * grad[min(k0 + j, NBIN - 1)];
        return g;
    };

    // L = ||A||_1 ||A||_inf for A = B^T D, which is never formed: its row sums are the band sums of the model of ones, its column sums
    // the atoms' dot products with the gradient of ones
    bins_model();
    __syncthreads();
    for (int m = tid; m < n_mels; m += NT) r[m] = band_sum(m);
    __syncthreads();
    double rows = 0.0;
    for (int m = 0; m < n_mels; ++m) rows = fmax(rows, r[m]);
    __syncthreads();
    for (int m = tid; m < n_mels; m += NT) r[m] = 1.0;
    __syncthreads();
    bins_grad();
    __syncthreads();
    if (tid < H) ys[tid] = atom_dot();
    __syncthreads();
    double cols = 0.0;
    for (int h = 0; h < H; ++h) cols = fmax(cols, ys[h]);
    __syncthreads();
    const double L = rows * cols;
    const double step = L > 0.0 ? 1.0 / L : 0.0;

    double a = 0.0, y = 0.0, t = 1.0;
    if (tid < H) ys[tid] = 0.0;
    __syncthreads();
    for (int it = 0; it < n_iter; ++it) {
        bins_model();
        __syncthreads();
        for (int m = tid; m < n_mels; m += NT) r[m] = band_sum(m) - amp[m];
        __syncthreads();
        bins_grad();
        __syncthreads();
        const double tn = (1.0 + sqrt(1.0 + 4.0 * t * t)) / 2.0;
        const double beta = (t - 1.0) / tn;
        t = tn;
        if (tid < H) {
            const double an = fmax(y - step * atom_dot(), 0.0);
            y = an + beta * (an - a);
            a = an;
            ys[tid] = y;
        }
        __syncthreads();
    }
    if (tid < H) ys[tid] = a;
    __syncthreads();
    bins_model();                               // mag_h
    __syncthreads();
    for (int m = tid; m < n_mels; m += NT) r[m] = fmax(amp[m] - band_sum(m), 0.0);
    __syncthreads();
    for (int k = tid; k < NBIN; k += NT) {
        double s = 0.0;
        for (int m = 0; m < n_mels; ++m) s += r[m] * inv_basis[(long)m * NBIN + k];
        const double mh = model[k], mn = fmax(s, 0.0);
        const double q = sqrt(mh * mh + mn * mn);
        mag[fr * NBIN + k] = fmax(q, floor_);
        share[fr * NBIN + k] = q > 0.0 ? mh / q : 0.0;
    }
}

// grid = B, block = 64 (one wave per row): the fundamental's phase at the frame centres, in cycles.  The recurrence is serial; the wave
// loads 64 frames at a time, every lane forms its frame's increment, and the chain then runs in registers over the broadcast increments,
// so no step waits for memory.  Unfused, so that the result is numpy's to the bit.  u is zero on unvoiced frames and behind the row's own.
__global__ __launch_bounds__(64) void harmonic_u_kernel(const double* __restrict__ f0_hz, const int* __restrict__ frames, int max_frames,
                                                        double* __restrict__ u) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int F = row_frames(frames, b, max_frames);
    f0_hz += (long)b * max_frames;
    u += (long)b * max_frames;
    double carry = 0.0;
    for (int i0 = 0; i0 < max_frames; i0 += 64) {
        const int i = i0 + lane;
        const double fi = i < F ? f0_hz[i] : 0.0, fp = i >= 1 && i < F ? f0_hz[i - 1] : 0.0;
        const int chained = harm_voiced(fi) && harm_voiced(fp);
        const double inc = chained ? 0.008 * (fp + fi) : 0.0;
        double mine = 0.0;
        for (int j = 0; j < 64; ++j) {
            const double tj = carry + __shfl(inc, j);
            carry = __shfl(chained, j) ? tj - floor(tj) : 0.0;
            if (lane == j) mine = carry;
        }
        if (i < max_frames) u[i] = mine;
    }
}

// grid = (max_frames, B), block = 256: phase0 = arg(w e^{i phi_h} + sqrt(1 - w^2) e^{i phi_rand}) on voiced frames, phi_rand elsewhere
// (rand == nullptr: zeros); frames at or beyond the row's: nothing is read, phase0 is zeros
__global__ __launch_bounds__(NT) void harmonic_phase_kernel(const double* __restrict__ f0_hz, const double* __restrict__ share,
                                                            const double* __restrict__ rand, const double* __restrict__ u,
                                                            const int* __restrict__ frames, int max_frames, double f_top,
                                                            double* __restrict__ phase0) {
#pragma clang fp contract(off)
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long fr = (long)b * max_frames + f;
    if (f >= row_frames(frames, b, max_frames)) {
        for (int k = tid; k < NBIN; k += NT) phase0[fr * NBIN + k] = 0.0;
        return;
    }
    const double hz = f0_hz[fr];
    if (!harm_voiced(hz)) {
        for (int k = tid; k < NBIN; k += NT) phase0[fr * NBIN + k] = rand ? rand[fr * NBIN + k] : 0.0;
        return;
    }
    const double ui = u[fr], p1 = hz / HARM_BIN_HZ, H = (double)harm_count(hz, f_top);
    for (int k = tid; k < NBIN; k += NT) {
        const double wk = share[fr * NBIN + k], pr = rand ? rand[fr * NBIN + k] : 0.0;
        const double hk = fmin(fmax(rint((double)k / p1), 1.0), H);
        const double tk = hk * ui + 0.5 * (double)(k & 1);
        double sh, ch, sr, cr;
        sincospi(2.0 * (tk - floor(tk)), &sh, &ch);
        sincos(pr, &sr, &cr);
        const double c = sqrt(fmax(1.0 - wk * wk, 0.0));
        const double re = wk * ch + c * cr, im = wk * sh + c * sr;
        phase0[fr * NBIN + k] = re == 0.0 && im == 0.0 ? pr : atan2(im, re);
    }
}

constexpr long align256(long n) { return (n + 255) & ~255L; }

}  // namespace

long mel_harmonic_lds_bytes(int n_mels, long packed_doubles) {
    // weights, amp, r, model, gradient, the harmonics' y and four weights as doubles; bands' first bins and offsets, atoms' first bins as ints
    return (packed_doubles + 2L * (NBIN + 1) + 5L * HARM_MAX) * 8 + (2L * n_mels + 1 + HARM_MAX) * 4;
}

long harmonic_phase_scratch_bytes(int B, int max_frames) { return align256((long)B * max_frames * 8); }

hipError_t mel_to_linear_harmonic(const float* mel, const double* f0_hz, const double* inv_basis, const double* packed, long packed_doubles,
                                  const int* frames, int B, int max_frames, int n_mels, double f_top, int n_iter, double floor,
                                  double* mag, double* share, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4 || n_mels < 1 || n_iter < 0 || packed_doubles < 2L * n_mels ||
        packed_doubles > NNLS_MAX_PACKED || !(f_top >= 1000.0 && f_top <= 8000.0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_harmonic_kernel, dim3(max_frames, B), dim3(NT), mel_harmonic_lds_bytes(n_mels, packed_doubles), s, mel, f0_hz,
                       inv_basis, packed, (int)packed_doubles, frames, max_frames, n_mels, f_top, n_iter, floor, mag, share);
    return hipGetLastError();
}

hipError_t harmonic_u(const double* f0_hz, const int* frames, int B, int max_frames, double* u, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(harmonic_u_kernel, dim3(B), dim3(64), 0, s, f0_hz, frames, max_frames, u);
    return hipGetLastError();
}

hipError_t harmonic_phase(const double* f0_hz, const double* share, const double* rand, const int* frames, int B, int max_frames,
                          double f_top, double* phase0, double* u, hipStream_t s) {
    if (!(f_top >= 1000.0 && f_top <= 8000.0)) return hipErrorInvalidValue;
    hipError_t e = harmonic_u(f0_hz, frames, B, max_frames, u, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(harmonic_phase_kernel, dim3(max_frames, B), dim3(NT), 0, s, f0_hz, share, rand, (const double*)u, frames, max_frames,
                       f_top, phase0);
    return hipGetLastError();
}

long mel_nnls_lds_bytes(int n_mels, long packed_doubles) {
    // weights, amp, r, y as doubles; first bins and offsets as ints
    return (packed_doubles + NBIN + 1) * 8 + (2L * n_mels + 1) * 4;
}

long vocoder_scratch_bytes(int B, int max_frames) {
    const long fr = (long)B * max_frames;
    return align256(fr * NFFT * 8) + 2 * align256(fr * NBIN * 16);
}

VocoderScratch vocoder_scratch(void* base, int B, int max_frames) {
    const long fr = (long)B * max_frames;
    char* p = (char*)base;
    VocoderScratch sc;
    sc.frame_buf = (double*)p;
    sc.proj = (double*)(p + align256(fr * NFFT * 8));
    sc.tprev = (double*)(p + align256(fr * NFFT * 8) + align256(fr * NBIN * 16));
    return sc;
}

hipError_t mel_to_linear(const float* mel, const double* inv_basis, const int* frames, int B, int max_frames, int n_mels, double floor,
                         double* mag, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4 || n_mels < 1 || n_mels > VOC_MAX_MELS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_to_linear_kernel, dim3(max_frames, B), dim3(NT), n_mels * sizeof(double), s, mel, inv_basis, frames, max_frames,
                       n_mels, floor, mag);
    return hipGetLastError();
}

hipError_t mel_to_linear_nnls(const float* mel, const double* inv_basis, const double* packed, long packed_doubles, const int* frames, int B,
                              int max_frames, int n_mels, int n_iter, double step, double floor, double* mag, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4 || n_mels < 1 || n_iter < 0 || packed_doubles < 2L * n_mels ||
        packed_doubles > NNLS_MAX_PACKED)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mel_nnls_kernel, dim3(max_frames, B), dim3(NT), mel_nnls_lds_bytes(n_mels, packed_doubles), s, mel, inv_basis, packed,
                       (int)packed_doubles, frames, max_frames, n_mels, n_iter, step, floor, mag);
    return hipGetLastError();
}

hipError_t stft(const double* wav, const int* frames, int B, int max_frames, double* spec, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stft_kernel, dim3(max_frames, B), dim3(NT), 0, s, wav, frames, max_frames, spec, (const double*)nullptr,
                       (double*)nullptr, 0.0);
    return hipGetLastError();
}

hipError_t istft(const double* spec, const int* frames, int B, int max_frames, double* wav, double* frame_buf, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(irfft_kernel, dim3(max_frames, B), dim3(NT), 0, s, spec, frames, max_frames, frame_buf);
    hipLaunchKernelGGL(ola_kernel, dim3(max_frames - 1, B), dim3(NT), 0, s, (const double*)frame_buf, frames, max_frames, wav);
    return hipGetLastError();
}

hipError_t griffinlim(const double* mag, const double* phase0, const int* frames, int B, int max_frames, int n_iter, double momentum,
                      double* wav, const VocoderScratch& sc, hipStream_t s) {
    if (B < 1 || B > VOC_MAX_ROWS || max_frames < 4 || n_iter < 0) return hipErrorInvalidValue;
    const dim3 grid(max_frames, B);
    const double coef = momentum / (1.0 + momentum);
    hipLaunchKernelGGL(gl_init_kernel, grid, dim3(NT), 0, s, mag, phase0, frames, max_frames, sc.proj, sc.tprev);
    for (int it = 0; it < n_iter; ++it) {
        hipError_t e = istft(sc.proj, frames, B, max_frames, wav, sc.frame_buf, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(stft_kernel, grid, dim3(NT), 0, s, (const double*)wav, frames, max_frames, sc.proj, mag, sc.tprev, coef);
    }
    return istft(sc.proj, frames, B, max_frames, wav, sc.frame_buf, s);
}

}  // namespace ss
