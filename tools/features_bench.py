#!/usr/bin/env python3
"""GPU time of the batched feature extraction (csrc/filtfilt.hip, csrc/features.hip, csrc/pitch.hip), ONE process, device events, median /
min / max over --reps after --warmup:
  * each stage on --rows recordings of --seconds each (default 64 x 3 s: 188 frames a row) in one batch, in milliseconds: ss_filtfilt (with
    gain and dither), ss_melspec_batch, ss_pitch_track in (50, 250), ss_f0_normalize_batch, and the four in a row;
  * ss_filtfilt alone on 1 row and on 16, to show that its time is the recurrence's latency and not the batch;
  * ss_mt19937_rand alone on the rows x samples draws the batch takes (csrc/mtrand.hip), also as nanoseconds per 227-word step of its chain,
    and ss_dither_rows on them;
  * beside them, wall clock on the same box: features.extract_batch on the recordings (upload, the four calls, one copy back a batch) with
    the host's draws and with device_draws=True, alternating, median / min / max over --reps after --warmup; the per-utterance
    features.extract loop, and scipy.signal.filtfilt and RandomState.rand on the host (one core).
    python tools/features_bench.py [--rows 64] [--seconds 3] [--reps 20] [--warmup 3] [--max-rows 64]
The recordings are pitch_bench's harmonic glides with pauses and noise, seeded per row.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--max-rows', type=int, default=64)
    a = ap.parse_args()
    from scipy import signal
    from pitch_bench import utterance
    from speechsplit_amd import _capi, features
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    B, n = a.rows, int(a.seconds * 16000) | 1                           # odd: the odd-length fix leaves it alone
    F = lib.ss_melspec_frames(n)
    lo, hi = 50.0, 250.0
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    host = np.stack([utterance(r, n, lo, hi) for r in range(B)])
    b, a_, = features.butter_highpass(30, 16000, order=5)
    zi = signal.lfilter_zi(b, a_)
    hp = lambda v: v.ctypes.data_as(C.c_void_p)
    x = torch.from_numpy(host).to(dev)
    r = torch.from_numpy(np.random.RandomState(1).rand(B, n)).to(dev)
    mb = torch.from_numpy(np.ascontiguousarray(features.mel_filter_bank().T, dtype=np.float64)).to(dev)
    wav = torch.empty_like(x)
    fb = lib.ss_filtfilt_scratch_bytes(B, n)
    fsc = torch.empty(fb, dtype=torch.uint8, device=dev)
    S = torch.empty(B, F, 80, device=dev)
    pb = lib.ss_pitch_scratch_bytes(B, n, lo, hi)
    psc = torch.empty(pb, dtype=torch.uint8, device=dev)
    f0 = torch.empty(B, F, dtype=torch.float64, device=dev)
    f0n = torch.empty(B, F, device=dev)
    state = torch.from_numpy(np.concatenate(np.random.RandomState(1).get_state()[1:3], axis=None).astype(np.uint32).view(np.int32)).to(dev)
    draws = torch.empty(B * n, dtype=torch.float64, device=dev)
    first = torch.arange(B, dtype=torch.int64, device=dev) * n
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)

    def filt(rows=B):
        return lib.ss_filtfilt(p(x), None, rows, n, hp(b), hp(a_), hp(zi), 0.96, p(r), 1e-06, p(wav), p(fsc), fb, s)

    mel = lambda: lib.ss_melspec_batch(p(wav), None, B, n, p(mb), 80, p(S), s)
    pitch = lambda: lib.ss_pitch_track(p(wav), None, B, n, 32768.0, lo, hi, p(f0), p(psc), pb, s)
    norm = lambda: lib.ss_f0_normalize_batch(p(f0), None, B, n, 0.0, p(f0n), s)
    calls = {'filtfilt': filt, 'melspec_batch': mel, 'pitch_track': pitch, 'f0_normalize_batch': norm,
             'all_four': lambda: filt() or mel() or pitch() or norm(),
             'filtfilt_1_row': lambda: filt(1), 'filtfilt_16_rows': lambda: filt(min(16, B)),
             'mt19937_rand': lambda: lib.ss_mt19937_rand(p(state), B * n, p(draws), s),
             'dither_rows': lambda: lib.ss_dither_rows(p(draws), B * n, p(first), p(lens), B, n, p(r), s)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in calls}
    for it in range(a.warmup + a.reps):
        for tag, fn in calls.items():
            ev[0].record()
            _capi.check(fn())
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[tag].append(ev[0].elapsed_time(ev[1]))
    _capi.check(filt())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y0 = signal.filtfilt(b, a_, host[0])
    scipy_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(wav[0].cpu().numpy(), y0 * 0.96 + (r[0].cpu().numpy() - 0.5) * 1e-06))
    fresh = np.random.RandomState(1)                                                               # the timed calls ran the state on
    rand_same = bool(np.array_equal(features.rand_dev(fresh, B * n, dev).cpu().numpy(), np.random.RandomState(1).rand(B * n)))
    t0 = time.perf_counter()
    np.random.RandomState(1).rand(B * n)
    numpy_rand_ms = (time.perf_counter() - t0) * 1e3
    recs = [host[k] for k in range(B)]
    wall = {False: [], True: []}
    for it in range(a.warmup + a.reps):
        for dd in (False, True):                                                                   # alternating: the same box, the same minute
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            features.extract_batch_sr(recs, 16000, np.random.RandomState(2), 'M', max_rows=a.max_rows, device_draws=dd)      # False: extract_batch itself
            if it >= a.warmup:
                wall[dd].append((time.perf_counter() - t0) * 1e3)
    batch_ms, batch_dev_ms = statistics.median(wall[False]), statistics.median(wall[True])
    features.extract(recs[0], np.random.RandomState(2), 'M')                                       # warm-up
    prng = np.random.RandomState(2)
    t0 = time.perf_counter()
    for w in recs:
        features.extract(w, prng, 'M')
    loop_ms = (time.perf_counter() - t0) * 1e3
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        'rows': B, 'samples': n, 'frames': F, 'reps': a.reps, 'max_rows': a.max_rows,
        'ms_median': {k: round(v, 4) for k, v in med.items()},
        'ms_minmax': {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
        'filtfilt_ns_per_step': round(med['filtfilt'] * 1e6 / (2 * (n + 36)), 2),
        'filtfilt_equals_scipy': same,
        'mt19937_draws': B * n, 'mt19937_steps': round(2 * B * n / 227),
        'mt19937_ns_per_step': round(med['mt19937_rand'] * 1e6 / (2 * B * n / 227), 2),
        'mt19937_equals_numpy': rand_same, 'numpy_rand_ms': round(numpy_rand_ms, 3),
        'scipy_filtfilt_ms_per_recording': round(scipy_ms, 3),
        'wall_ms': {'extract_batch': round(batch_ms, 2), 'extract_batch_device_draws': round(batch_dev_ms, 2), 'extract_loop': round(loop_ms, 2)},
        'wall_ms_minmax': {'extract_batch': [round(min(wall[False]), 2), round(max(wall[False]), 2)],
                           'extract_batch_device_draws': [round(min(wall[True]), 2), round(max(wall[True]), 2)]},
        'wall_us_per_recording': {'extract_batch': round(batch_ms * 1e3 / B, 1), 'extract_loop': round(loop_ms * 1e3 / B, 1)}}))


if __name__ == '__main__':
    main()
