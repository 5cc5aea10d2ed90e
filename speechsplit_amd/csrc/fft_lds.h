// The 1024-point transform the vocoder and the batched mel spectrogram share (internal; vocoder.hip, features.hip): the reference's pySTFT
// framing (utils.py:18-31: reflect padding by 512, periodic Hann window, hop 256) around a complex radix-2 decimation-in-frequency FFT, in
// place in LDS, output read in bit-reversed order; the twiddles come from sincospi, exact to double rounding.  Every phase is a
// __host__ __device__ inline function of (LDS image, thread id): a kernel of NT threads puts a workgroup barrier between any two of them, a
// host program loops tid over 0 .. NT - 1.  The names live in namespace ss::fftlds; a kernel file takes them with a using-directive.
#pragma once
#include "common.h"

namespace ss {
namespace fftlds {

constexpr int NFFT = 1024, HOP = 256, NBIN = NFFT / 2 + 1, LOGN = 10, NT = 256;

struct FftLds {
    double re[NFFT], im[NFFT];          // the transform, in place
    double wr[NFFT / 2], wi[NFFT / 2];  // exp(-2 pi i t / 1024), t < 512
};

__host__ __device__ inline double hann(int i) { return 0.5 - 0.5 * cospi((double)i / (double)(NFFT / 2)); }

__host__ __device__ inline int row_frames(const int* frames, int b, int max_frames) {
    const int F = frames ? frames[b] : max_frames;
    return F < 4 ? 4 : (F > max_frames ? max_frames : F);
}

__host__ __device__ inline int brev10(int k) {
    unsigned v = (unsigned)k;
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    v = (v >> 16) | (v << 16);
    return (int)(v >> (32 - LOGN));
}

// reflect-padded sample (numpy.pad mode='reflect': the edge sample is not repeated); needs n >= 513
__host__ __device__ inline double padded(const double* __restrict__ x, int n, int i) {
    int j = i - NFFT / 2;
    if (j < 0) j = -j;
    if (j >= n) j = 2 * (n - 1) - j;
    return x[j];
}

// The phases of a transform; the kernels put a workgroup barrier between any two of them.
__host__ __device__ inline void fft_twiddles(FftLds& L, int tid) {
    for (int t = tid; t < NFFT / 2; t += NT) {
        double s, c;
        sincospi((double)t / (double)(NFFT / 2), &s, &c);
        L.wr[t] = c;
        L.wi[t] = -s;
    }
}

// stage s of 10: butterflies of span 512 >> s; inverse conjugates the twiddles.  X[k] ends up at brev10(k).
__host__ __device__ inline void fft_stage(FftLds& L, int tid, int s, bool inverse) {
    const int half = (NFFT / 2) >> s;
    for (int b = tid; b < NFFT / 2; b += NT) {
        const int j = b & (half - 1);
        const int i0 = ((b - j) << 1) + j, i1 = i0 + half;
        const double c = L.wr[j << s], sn = inverse ? -L.wi[j << s] : L.wi[j << s];
        const double ur = L.re[i0], ui = L.im[i0], vr = L.re[i1], vi = L.im[i1];
        L.re[i0] = ur + vr;
        L.im[i0] = ui + vi;
        const double dr = ur - vr, di = ui - vi;
        L.re[i1] = dr * c - di * sn;
        L.im[i1] = dr * sn + di * c;
    }
}

__host__ __device__ inline void stft_load(FftLds& L, int tid, const double* __restrict__ x, int n, int f) {
    for (int i = tid; i < NFFT; i += NT) {
        L.re[i] = hann(i) * padded(x, n, f * HOP + i);
        L.im[i] = 0.0;
    }
}

// bins 0..512 of the frame's transform -> out [513][2].  With the projection (mag != nullptr): a = r - coef tprev, tprev = r,
// out = mag a / (|a| + 1e-16), the spectrum the next ISTFT takes.
__host__ __device__ inline void stft_store(const FftLds& L, int tid, double* __restrict__ out, const double* __restrict__ mag,
                                           double* __restrict__ tprev, double coef) {
    for (int k = tid; k < NBIN; k += NT) {
        const int p = brev10(k);
        const double rr = L.re[p], ri = L.im[p];
        if (!mag) {
            out[2 * k] = rr;
            out[2 * k + 1] = ri;
            continue;
        }
        const double ar = rr - coef * tprev[2 * k], ai = ri - coef * tprev[2 * k + 1];
        tprev[2 * k] = rr;
        tprev[2 * k + 1] = ri;
        const double d = hypot(ar, ai) + 1e-16;
        out[2 * k] = mag[k] * (ar / d);
        out[2 * k + 1] = mag[k] * (ai / d);
    }
}

// numpy.fft.irfft's reading of a half spectrum: the imaginary parts of bins 0 and 512 are ignored, the rest is mirrored conjugated
__host__ __device__ inline void irfft_load(FftLds& L, int tid, const double* __restrict__ spec) {
    for (int k = tid; k < NBIN; k += NT) {
        const bool edge = k == 0 || k == NFFT / 2;
        const double r = spec[2 * k], i = edge ? 0.0 : spec[2 * k + 1];
        L.re[k] = r;
        L.im[k] = i;
        if (!edge) {
            L.re[NFFT - k] = r;
            L.im[NFFT - k] = -i;
        }
    }
}

__host__ __device__ inline void irfft_store(const FftLds& L, int tid, double* __restrict__ frame) {
    for (int t = tid; t < NFFT; t += NT) frame[t] = (L.re[brev10(t)] * (1.0 / NFFT)) * hann(t);
}

}  // namespace fftlds
}  // namespace ss
