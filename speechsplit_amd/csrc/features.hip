// Offline feature extraction, the part of reference make_spect_f0.py / utils.py that can be pinned in this environment
// (SURVEY.md section 8(f) row N4): STFT magnitude (utils.py:18-31 pySTFT: reflect padding by fft/2, periodic Hann window,
// 1024-point rfft, hop 256) -> mel projection with a CALLER-SUPPLIED basis (make_spect_f0.py:15,58: librosa's filter bank is
// not available here, so it is an input) -> dB with the reference's floor and offsets (make_spect_f0.py:16,59-60) -> float32;
// and the per-utterance F0 normalisation (utils.py:35-42 + make_spect_f0.py:64-66).  Each comes twice: one utterance a call
// (ss_melspec, ss_f0_normalize) and a ragged batch a call (ss_melspec_batch, ss_f0_normalize_batch).  The Butterworth filtfilt
// and the dither's scaling are in filtfilt.hip, the pitch track in pitch.hip; only the dither DRAW stays on the host
// (speechsplit_amd/features.py): it is the speaker's numpy stream.
//
// Arithmetic: float64 throughout, as numpy computes it (the reference casts to float32 only when saving).  ss_melspec: one
// utterance is ~200 frames x 513 bins x 1024 taps = 0.2 G multiply-adds, a direct DFT from an exact twiddle table in LDS.
// ss_melspec_batch: the vocoder's 1024-point FFT in LDS (fft_lds.h), one workgroup per (frame, row).
// Batches: row b has n_b = min(max(n[b], 513), max_n) samples and F_b = n_b / 256 + 1 frames; it is computed as if it were alone
// (the framing reflects about the row's OWN end), samples at or beyond n_b are never read, frames at or beyond F_b are zeros
// (mel) or `unvoiced` (F0).
#include "common.h"
#include "fft_lds.h"
#include "kernels.h"

namespace ss {

namespace {

using namespace fftlds;   // NFFT, HOP, NBIN, padded, and the FFT phases of melspec_batch_kernel

// a row's own samples: n (nullable) clamped into [513, max_n]
__device__ __forceinline__ int row_samples(const int* __restrict__ n, int b, int max_n) {
    const int v = n ? n[b] : max_n;
    return v < NFFT / 2 + 1 ? NFFT / 2 + 1 : (v > max_n ? max_n : v);
}

// grid = (frames), block = 256: frame -> windowed samples in LDS -> |rfft| -> mag in LDS -> mel -> dB -> S
__global__ __launch_bounds__(256) void melspec_kernel(const double* __restrict__ x, int n, const double* __restrict__ mel, int n_mels,
                                                      float* __restrict__ out) {
    __shared__ double fr[NFFT];
    __shared__ double cs[NFFT], sn[NFFT];
    __shared__ double mag[NBIN];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < NFFT; i += 256) {
        const double a = 2.0 * M_PI * (double)i / (double)NFFT;
        const double w = 0.5 - 0.5 * cos(a);                       // scipy.signal.get_window('hann', N, fftbins=True)
        fr[i] = w * padded(x, n, f * HOP + i);
        cs[i] = cos(a);
        sn[i] = sin(a);
    }
    __syncthreads();
    for (int k = tid; k < NBIN; k += 256) {
        double re = 0.0, im = 0.0;
        int idx = 0;                                                // (k * t) mod NFFT, updated incrementally
        for (int t = 0; t < NFFT; ++t) {
            re += fr[t] * cs[idx];
            im -= fr[t] * sn[idx];
            idx = (idx + k) & (NFFT - 1);
        }
        mag[k] = sqrt(re * re + im * im);
    }
    __syncthreads();
    const double min_level = exp(-100.0 / 20.0 * log(10.0));       // make_spect_f0.py:16
    for (int m = tid; m < n_mels; m += 256) {
        double s = 0.0;
        for (int k = 0; k < NBIN; ++k) s += mag[k] * mel[(long)k * n_mels + m];
        const double db = 20.0 * log10(fmax(min_level, s)) - 16.0;   // :59
        out[(long)f * n_mels + m] = (float)((db + 100.0) / 100.0);    // :60, :71 (astype(float32))
    }
}

// one block, one row: mean / population std over the voiced frames (f0 != -1e10), then utils.py:35-42.  Both kernels below are this
// function, so a row of a batch comes out with the bits of the single call.  fill: unvoiced frames and out[n .. total) get `unvoiced`
// (else the -1e10 marker passes through and nothing behind n is written).
__device__ __forceinline__ void f0_norm_row(const double* __restrict__ f0, int n, float* __restrict__ out, int tid, bool fill,
                                            double unvoiced, int total) {
    __shared__ double red[256];
    __shared__ double stat[2];
    __shared__ int cnt[256];
    double s = 0.0;
    int c = 0;
    for (int i = tid; i < n; i += 256)
        if (f0[i] != -1e10) {
            s += f0[i];
            ++c;
        }
    red[tid] = s;
    cnt[tid] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[tid] += red[tid + w];
            cnt[tid] += cnt[tid + w];
        }
        __syncthreads();
    }
    const int nv = cnt[0];
    if (tid == 0) stat[0] = nv ? red[0] / nv : 0.0;
    __syncthreads();
    const double mean = stat[0];
    double q = 0.0;
    for (int i = tid; i < n; i += 256)
        if (f0[i] != -1e10) q += (f0[i] - mean) * (f0[i] - mean);
    __syncthreads();
    red[tid] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) stat[1] = nv ? sqrt(red[0] / nv) : 1.0;          // np.std: population
    __syncthreads();
    const double sd = stat[1];
    for (int i = tid; i < n; i += 256) {
        double v = f0[i];
        if (v != -1e10) {
            v = (v - mean) / sd / 4.0;
            v = fmin(fmax(v, -1.0), 1.0);
            v = (v + 1.0) / 2.0;
        } else if (fill) {
            v = unvoiced;
        }
        out[i] = (float)v;
    }
    for (int i = n + tid; i < total; i += 256) out[i] = (float)unvoiced;
}

__global__ __launch_bounds__(256) void f0_norm_kernel(const double* __restrict__ f0, int n, float* __restrict__ out) {
    f0_norm_row(f0, n, out, threadIdx.x, false, 0.0, 0);
}

// grid = (B), block = 256: f0 [B][F] -> out [B][F], row b over its own F_b frames
__global__ __launch_bounds__(256) void f0_norm_batch_kernel(const double* __restrict__ f0, const int* __restrict__ n, int max_n, int F,
                                                            double unvoiced, float* __restrict__ out) {
    const int b = blockIdx.x;
    f0_norm_row(f0 + (long)b * F, row_samples(n, b, max_n) / HOP + 1, out + (long)b * F, threadIdx.x, true, unvoiced, F);
}

// grid = (F, B), block = 256: melspec_kernel's chain with the FFT of fft_lds.h in place of the direct DFT.  wav [B][max_n], out [B][F][n_mels].
__global__ __launch_bounds__(NT) void melspec_batch_kernel(const double* __restrict__ wav, const int* __restrict__ n, int max_n,
                                                           const double* __restrict__ mel, int n_mels, float* __restrict__ out) {
    __shared__ FftLds L;
    __shared__ double mag[NBIN];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nb = row_samples(n, b, max_n);
    out += ((long)b * gridDim.x + f) * n_mels;
    if (f >= nb / HOP + 1) {
        for (int m = tid; m < n_mels; m += NT) out[m] = 0.0f;
        return;
    }
    fft_twiddles(L, tid);
    stft_load(L, tid, wav + (long)b * max_n, nb, f);
    __syncthreads();
    for (int s = 0; s < LOGN; ++s) {
        fft_stage(L, tid, s, false);
        __syncthreads();
    }
    for (int k = tid; k < NBIN; k += NT) {
        const int p = brev10(k);
        mag[k] = sqrt(L.re[p] * L.re[p] + L.im[p] * L.im[p]);
    }
    __syncthreads();
    const double min_level = exp(-100.0 / 20.0 * log(10.0));       // make_spect_f0.py:16
    for (int m = tid; m < n_mels; m += NT) {
        double s = 0.0;
        for (int k = 0; k < NBIN; ++k) s += mag[k] * mel[(long)k * n_mels + m];
        const double db = 20.0 * log10(fmax(min_level, s)) - 16.0;   // :59
        out[m] = (float)((db + 100.0) / 100.0);                      // :60, :71 (astype(float32))
    }
}

}  // namespace

hipError_t melspec(const double* x, int n, const double* mel, int n_mels, float* out, int frames, hipStream_t s) {
    if (n < NFFT / 2 + 1 || n_mels < 1 || frames < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(melspec_kernel, dim3(frames), dim3(256), 0, s, x, n, mel, n_mels, out);
    return hipGetLastError();
}

hipError_t f0_normalize(const double* f0, int n, float* out, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_norm_kernel, dim3(1), dim3(256), 0, s, f0, n, out);
    return hipGetLastError();
}

hipError_t melspec_batch(const double* wav, const int* n, int B, int max_n, const double* mel, int n_mels, float* out, hipStream_t s) {
    if (B < 1 || B > FEAT_MAX_ROWS || max_n < NFFT / 2 + 1 || n_mels < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(melspec_batch_kernel, dim3(max_n / HOP + 1, B), dim3(NT), 0, s, wav, n, max_n, mel, n_mels, out);
    return hipGetLastError();
}

hipError_t f0_normalize_batch(const double* f0, const int* n, int B, int max_n, double unvoiced, float* out, hipStream_t s) {
    if (B < 1 || max_n < NFFT / 2 + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_norm_batch_kernel, dim3(B), dim3(256), 0, s, f0, n, max_n, max_n / HOP + 1, unvoiced, out);
    return hipGetLastError();
}

}  // namespace ss
