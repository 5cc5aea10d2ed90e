#!/usr/bin/env python3
"""GPU time of the pitch tracker (csrc/pitch.hip), ONE process, device events, median / min / max over --reps after --warmup, against the
float64 numpy restatement (tests/pitch_ref.py) on the same box:
  * ss_pitch_track on --rows utterances of --seconds each (default 64 x 3 s: 188 frames a row) for the ranges (50, 250) and (100, 600), in
    milliseconds, and its two halves alone (ss_op_nccf; ss_op_pitch_dp = candidates + dynamic programming);
  * the same with RAPT's spectral-stationarity term: ss_pitch_track_stat, ss_op_pitch_stationarity alone (the LPC analysis per frame) and
    ss_op_pitch_dp_stat (candidates + dynamic programming with the term), in the same run;
  * pitch_ref.track on the first --ref-rows of the same utterances (wall clock, one pass), per utterance, and whether the two agree there.
    python tools/pitch_bench.py [--rows 64] [--seconds 3] [--reps 20] [--warmup 3] [--ref-rows 4]
The utterances are harmonic glides with pauses and noise, seeded per row.  Prints one JSON line."""
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


def utterance(seed, n, lo, hi):
    """voiced stretches (a five-harmonic glide inside the range) between noisy pauses"""
    rng = np.random.RandomState(seed)
    f = np.interp(np.arange(n), [0, n - 1], rng.uniform(1.3 * lo, 0.7 * hi, 2))
    ph = 2.0 * np.pi * np.cumsum(f) / 16000.0
    x = sum(0.2 / h * np.sin(h * ph) for h in range(1, 6))
    gate = (np.sin(2.0 * np.pi * np.arange(n) / 16000.0 * rng.uniform(0.8, 1.6) + rng.uniform(0, 6.28)) > -0.3).astype(np.float64)
    return (x * gate + 3e-3 * rng.randn(n)).astype(np.float32).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--ref-rows', type=int, default=4)
    a = ap.parse_args()
    from speechsplit_amd import _capi
    from tests import pitch_ref as R
    from tests import pitch_stat_ref as Q
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    B, n = a.rows, int(a.seconds * 16000)
    F = lib.ss_melspec_frames(n)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {'rows': B, 'samples': n, 'frames': F, 'reps': a.reps, 'ranges': {}}
    for lo, hi in ((50.0, 250.0), (100.0, 600.0)):
        K = R.lag_range(lo, hi)[2]
        host = np.stack([utterance(b, n, lo, hi) for b in range(B)])
        wav = torch.from_numpy(host).to(dev)
        nbytes = lib.ss_pitch_scratch_bytes(B, n, lo, hi)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        f0 = torch.empty(B, F, dtype=torch.float64, device=dev)
        phi = torch.empty(B, F, K, dtype=torch.float64, device=dev)
        rms = torch.empty(B, F, dtype=torch.float64, device=dev)
        stat = torch.empty(B, F, dtype=torch.float64, device=dev)
        nbytes_stat = lib.ss_pitch_stat_scratch_bytes(B, n, lo, hi)
        scratch_stat = torch.empty(nbytes_stat, dtype=torch.uint8, device=dev)
        calls = {
            'pitch_track': lambda: lib.ss_pitch_track(p(wav), None, B, n, 32768.0, lo, hi, p(f0), p(scratch), nbytes, s),
            'nccf': lambda: lib.ss_op_nccf(p(wav), None, B, n, 32768.0, lo, hi, p(phi), p(rms), s),
            'candidates_dp': lambda: lib.ss_op_pitch_dp(p(phi), p(rms), None, B, n, lo, hi, p(f0), p(scratch), nbytes, s),
            'pitch_track_stat': lambda: lib.ss_pitch_track_stat(p(wav), None, B, n, 32768.0, lo, hi, p(f0), p(scratch_stat), nbytes_stat, s),
            'stationarity': lambda: lib.ss_op_pitch_stationarity(p(wav), None, B, n, 32768.0, p(stat), s),
            'candidates_dp_stat': lambda: lib.ss_op_pitch_dp_stat(p(phi), p(rms), p(stat), None, B, n, lo, hi, p(f0), p(scratch), nbytes, s),
        }
        times = {k: [] for k in calls}
        for it in range(a.warmup + a.reps):
            for tag, fn in calls.items():
                ev[0].record()
                _capi.check(fn())
                ev[1].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[tag].append(ev[0].elapsed_time(ev[1]))
        _capi.check(calls['pitch_track']())
        got = f0.cpu().numpy()
        t0 = time.perf_counter()
        refs = [R.track(host[b], lo, hi) for b in range(min(a.ref_rows, B))]
        ref_ms = (time.perf_counter() - t0) * 1e3 / max(len(refs), 1)
        same = all(np.array_equal(R.voiced(r), R.voiced(g)) and np.allclose(r, g, rtol=1e-10, atol=0.0) for r, g in zip(refs, got))
        _capi.check(calls['pitch_track_stat']())
        got_stat = f0.cpu().numpy()
        refs_stat = [Q.track_stat(host[b], lo, hi) for b in range(min(a.ref_rows, B))]
        same_stat = all(np.array_equal(R.voiced(r), R.voiced(g)) and np.allclose(r, g, rtol=1e-10, atol=0.0) for r, g in zip(refs_stat, got_stat))
        med = {k: statistics.median(v) for k, v in times.items()}
        out['ranges'][f'{int(lo)}-{int(hi)}'] = {
            'lags': K, 'scratch_mib': round(nbytes / 2 ** 20, 2),
            'ms_median': {k: round(v, 4) for k, v in med.items()},
            'ms_minmax': {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            'us_per_utterance': round(med['pitch_track'] * 1e3 / B, 2),
            'voiced_fraction': round(float(R.voiced(got).mean()), 3),
            'voiced_fraction_stat': round(float(R.voiced(got_stat).mean()), 3), 'stat_agrees_with_numpy': bool(same_stat),
            'numpy_ms_per_utterance': round(ref_ms, 1), 'numpy_rows': len(refs), 'agrees_with_numpy': bool(same),
            'numpy_over_gpu': round(ref_ms / (med['pitch_track'] / B), 1)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
