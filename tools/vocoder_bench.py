#!/usr/bin/env python3
"""GPU time of the Griffin-Lim vocoder (csrc/vocoder.hip), ONE process, device events, median / min / max over --reps after --warmup:
  * ss_griffinlim on --rows x --frames x --iters (default 7 x 192 x 60: the seven conditions of one demo conversion), in milliseconds;
  * per frame, the FFT-based ss_op_stft against the direct-DFT ss_melspec (features.hip; it also does the mel projection, 8 % of its
    multiply-adds) on the same --frames frames of one waveform, alternated call by call, --inner calls per timed window;
  * the mel inversion as a stage of its own, on the same --rows x --frames mels of the project's filter bank: ss_mel_to_linear against
    ss_mel_to_linear_nnls at every count of --nnls-iters (default 50 and 200), one call per timed window, alternated call by call, in
    milliseconds and as a fraction of ss_griffinlim's median on this run;
  * the F0-guided harmonic route on the same mels, every frame voiced (the worst case; per row a slow glide between 90 and 230 Hz):
    ss_mel_to_linear_harmonic alone (the magnitude already filled) at every count of --harmonic-iters (default 25 and 50),
    ss_harmonic_phase, and its serial part alone (ss_op_harmonic_u: one wave per row), the same way.
    python tools/vocoder_bench.py [--rows 7] [--frames 192] [--iters 60] [--reps 30] [--warmup 5] [--inner 20] [--nnls-iters 50 200]
                                  [--harmonic-iters 25 50]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=7)
    ap.add_argument('--frames', type=int, default=192)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--nnls-iters', type=int, nargs='+', default=[50, 200])
    ap.add_argument('--harmonic-iters', type=int, nargs='+', default=[25, 50])
    a = ap.parse_args()
    from speechsplit_amd import _capi, features, vocoder
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    B, T = a.rows, a.frames
    rng = np.random.default_rng(0)
    mag = torch.from_numpy(rng.uniform(0.0, 1.0, (B, T, 513))).to(dev)
    ph = torch.from_numpy(rng.uniform(-np.pi, np.pi, (B, T, 513))).to(dev)
    n = lib.ss_griffinlim_samples(T)
    wav = torch.from_numpy(rng.standard_normal(n) * 0.1).to(dev)
    basis = torch.from_numpy(rng.uniform(0.0, 0.1, (513, 80))).to(dev)
    spec = torch.empty(1, T, 513, 2, dtype=torch.float64, device=dev)
    mel = torch.empty(T, 80, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ss_melspec_frames(n) == T
    # the inversion's inputs: mels of non-negative spectra through the project's bank (what a mel is), its pseudo-inverse and packed form
    bank = features.mel_filter_bank().T.astype(np.float64)
    mel_in = 20.0 * np.log10(np.maximum(1e-5, (rng.uniform(0.0, 1.0, (B, T, 513)) ** 4) @ bank)) - 16.0
    mel_in = torch.from_numpy(((mel_in + 100.0) / 100.0).astype(np.float32)).to(dev)
    inv = torch.from_numpy(np.linalg.pinv(bank)).to(dev)
    packed, step = vocoder._nnls_basis(None)
    packed = torch.from_numpy(packed).to(dev)

    def gl():
        vocoder.griffin_lim_mag(mag, ph, None, a.iters, 0.99)

    def fft():
        for _ in range(a.inner):
            _capi.check(lib.ss_op_stft(p(wav), None, 1, T, p(spec), s))

    def dft():
        for _ in range(a.inner):
            _capi.check(lib.ss_melspec(p(wav), n, p(basis), 80, p(mel), s))

    def pinv():
        vocoder._mel_to_linear(mel_in, inv, None, 1e-10)

    def nnls(n_iter):
        return lambda: vocoder._mel_to_linear_nnls(mel_in, inv, packed, None, n_iter, step, 1e-10)

    # the harmonic route: every frame voiced, a glide per row; mag_h / share_h are the call's in/out and out buffers
    f0hz = torch.from_numpy(np.stack([110.0 + 20.0 * r + (20.0 + 10.0 * r) * np.sin(np.arange(T) / 17.0 + r) for r in range(B)])).to(dev)
    mag_h = vocoder._mel_to_linear(mel_in, inv, None, 1e-10)
    share_h = torch.rand(B, T, 513, dtype=torch.float64, device=dev)
    u_buf = torch.empty(B, T, dtype=torch.float64, device=dev)

    def harmonic(n_iter):
        return lambda: _capi.check(lib.ss_mel_to_linear_harmonic(p(mel_in), p(f0hz), p(inv), p(packed), packed.numel(), None, B, T, 80, 7600.0,
                                                                  n_iter, 1e-10, p(mag_h), p(share_h), s))

    def hphase():
        vocoder._harmonic_phase(f0hz, share_h, ph, None, 7600.0)

    def hu():
        _capi.check(lib.ss_op_harmonic_u(p(f0hz), None, B, T, p(u_buf), s))

    harm = [(f'mel_harmonic_{k}', harmonic(k)) for k in a.harmonic_iters] + [('harmonic_phase', hphase), ('harmonic_u', hu)]
    stages = [('griffinlim', gl), ('stft_fft', fft), ('melspec_dft', dft), ('mel_pinv', pinv)] + [(f'mel_nnls_{k}', nnls(k)) for k in a.nnls_iters] + harm
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {tag: [] for tag, _ in stages}
    for it in range(a.warmup + a.reps):
        for tag, fn in stages:
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[tag].append(ev[0].elapsed_time(ev[1]))
    med = {k: statistics.median(v) for k, v in times.items()}
    per_frame = {k: med[k] * 1e3 / (a.inner * T) for k in ('stft_fft', 'melspec_dft')}
    print(json.dumps({'rows': B, 'frames': T, 'iters': a.iters, 'reps': a.reps, 'inner': a.inner,
                      'griffinlim_ms_median': round(med['griffinlim'], 4),
                      'griffinlim_ms_minmax': [round(min(times['griffinlim']), 4), round(max(times['griffinlim']), 4)],
                      'launches': 3 + 3 * a.iters,
                      'us_per_frame_median': {k: round(v, 4) for k, v in per_frame.items()},
                      'call_ms_minmax': {k: [round(min(times[k]) / a.inner, 5), round(max(times[k]) / a.inner, 5)] for k in per_frame},
                      'dft_over_fft': round(per_frame['melspec_dft'] / per_frame['stft_fft'], 2),
                      'inversion_ms_median': {k: round(med[k], 4) for k in med if k.startswith('mel_')},
                      'inversion_ms_minmax': {k: [round(min(times[k]), 4), round(max(times[k]), 4)] for k in med if k.startswith('mel_')},
                      'inversion_over_griffinlim': {k: round(med[k] / med['griffinlim'], 4) for k in med if k.startswith('mel_')},
                      'harmonic_ms_median': {k: round(med[k], 4) for k, _ in harm},
                      'harmonic_ms_minmax': {k: [round(min(times[k]), 4), round(max(times[k]), 4)] for k, _ in harm}}))


if __name__ == '__main__':
    main()
