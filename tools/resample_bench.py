#!/usr/bin/env python3
"""GPU time of the resampler (csrc/resample.hip), ONE process, device events, median / min / max over --reps after --warmup, at each of
--rates (default 48000 and 44100 Hz to 16 kHz) on --rows recordings of --seconds each (default 64 x 3 s) in one batch:
  * ss_resample alone, in milliseconds, beside its traffic bound: 8 bytes read an input sample and 8 written an output sample, over the
    6.29 TB/s a streaming copy measures on this chip -- and how many times the bound the call takes;
  * beside it on the same box: scipy.signal.resample_poly on one recording (one core), and whether the GPU's row equals it to the bit;
  * wall clock of features.extract_batch_sr on the recordings (upload, resampling, the chain's four calls, one copy back a batch) beside
    features.extract_batch on the same recordings resampled beforehand.
    python tools/resample_bench.py [--rows 64] [--seconds 3] [--reps 20] [--warmup 3] [--max-rows 64] [--rates 48000,44100]
The recordings are pitch_bench's harmonic glides with pauses and noise, seeded per row, brought up to the rate by scipy.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HBM_BYTES_PER_S = 6.29e12                                               # measured streaming-copy rate of the chip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--max-rows', type=int, default=64)
    ap.add_argument('--rates', default='48000,44100')
    a = ap.parse_args()
    from scipy import signal
    from pitch_bench import utterance
    from speechsplit_amd import _capi, features
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    B, n16 = a.rows, int(a.seconds * 16000) | 1
    low = [utterance(r, n16, 50.0, 250.0) for r in range(B)]
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    report = {'rows': B, 'seconds': a.seconds, 'reps': a.reps, 'max_rows': a.max_rows, 'hbm_tb_per_s': HBM_BYTES_PER_S / 1e12, 'rates': {}}
    for sr in (int(v) for v in a.rates.split(',')):
        up, down = features.rate_ratio(sr, 16000)
        recs = [signal.resample_poly(w, sr, 16000)[:int(a.seconds * sr)] for w in low]
        n = recs[0].shape[0]
        M = lib.ss_resample_len(n, up, down)
        x = torch.from_numpy(np.stack(recs)).to(dev)
        h = torch.from_numpy(features.resample_filter(up, down)).to(dev)
        y = torch.empty(B, M, dtype=torch.float64, device=dev)
        nb = lib.ss_resample_scratch_bytes(up, h.numel())
        sc = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
        times = []
        for it in range(a.warmup + a.reps):
            ev[0].record()
            _capi.check(lib.ss_resample(p(x), None, B, n, up, down, p(h), h.numel(), p(y), p(sc), nb, s))
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(ev[0].elapsed_time(ev[1]))
        t0 = time.perf_counter()
        y0 = signal.resample_poly(recs[0], up, down)
        scipy_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(y[0].cpu().numpy(), y0))
        nbytes = 8 * B * (n + M)
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        med = statistics.median(times)
        at16 = [signal.resample_poly(w, up, down) for w in recs]
        features.extract_batch_sr(recs[:2], sr, np.random.RandomState(2), 'M', max_rows=a.max_rows)      # warm-up
        features.extract_batch(at16[:2], np.random.RandomState(2), 'M', max_rows=a.max_rows)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        features.extract_batch_sr(recs, sr, np.random.RandomState(2), 'M', max_rows=a.max_rows)
        with_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        features.extract_batch(at16, np.random.RandomState(2), 'M', max_rows=a.max_rows)
        pre_ms = (time.perf_counter() - t0) * 1e3
        report['rates'][str(sr)] = {
            'up': up, 'down': down, 'n_taps': h.numel(), 'samples_in': n, 'samples_out': M,
            'multiply_adds': int(sum(min(n - 1, (m * down + h.numel() // 2) // up) - max(0, -((h.numel() // 2 - m * down) // up)) + 1
                                     for m in range(M))) * B,
            'ss_resample_ms': {'median': round(med, 4), 'min': round(min(times), 4), 'max': round(max(times), 4)},
            'traffic_bytes': nbytes, 'traffic_bound_ms': round(bound_ms, 4), 'times_the_bound': round(med / bound_ms, 2),
            'equals_scipy': same, 'scipy_resample_poly_ms_per_recording': round(scipy_ms, 3),
            'wall_ms': {'extract_batch_sr': round(with_ms, 2), 'extract_batch_on_resampled_input': round(pre_ms, 2)}}
    print(json.dumps(report))


if __name__ == '__main__':
    main()
