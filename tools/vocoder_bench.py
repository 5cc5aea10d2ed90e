#!/usr/bin/env python3
"""GPU time of the Griffin-Lim vocoder (csrc/vocoder.hip), ONE process, device events, median / min / max over --reps after --warmup:
  * ss_griffinlim on --rows x --frames x --iters (default 7 x 192 x 60: the seven conditions of one demo conversion), in milliseconds;
  * per frame, the FFT-based ss_op_stft against the direct-DFT ss_melspec (features.hip; it also does the mel projection, 8 % of its
    multiply-adds) on the same --frames frames of one waveform, alternated call by call, --inner calls per timed window.
    python tools/vocoder_bench.py [--rows 7] [--frames 192] [--iters 60] [--reps 30] [--warmup 5] [--inner 20]
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
    a = ap.parse_args()
    from speechsplit_amd import _capi, vocoder
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

    def gl():
        vocoder.griffin_lim_mag(mag, ph, None, a.iters, 0.99)

    def fft():
        for _ in range(a.inner):
            _capi.check(lib.ss_op_stft(p(wav), None, 1, T, p(spec), s))

    def dft():
        for _ in range(a.inner):
            _capi.check(lib.ss_melspec(p(wav), n, p(basis), 80, p(mel), s))

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {'griffinlim': [], 'stft_fft': [], 'melspec_dft': []}
    for it in range(a.warmup + a.reps):
        for tag, fn in (('griffinlim', gl), ('stft_fft', fft), ('melspec_dft', dft)):
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
                      'dft_over_fft': round(per_frame['melspec_dft'] / per_frame['stft_fft'], 2)}))


if __name__ == '__main__':
    main()
