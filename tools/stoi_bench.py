#!/usr/bin/env python3
"""The waveform scores (csrc/stoi.hip) on the GPU, ONE process:
  * device-event medians (--reps runs after --warmup) of ss_stoi (STOI and ESTOI) and of its stages through the test hooks -- energies,
    mask and compacting overlap-add (ss_op_stoi_compact), the band envelopes of one signal (ss_op_stoi_bands) -- at --rows rows of
    --frames mel frames' worth of samples (256 (frames - 1) at 16 kHz, five eighths of that at 10 kHz);
  * how far the GPU lies from the numpy restatement (tests/stoi_ref.py) on the GPU tests' pairs, beside the restatement's own two-order
    disagreement;
  * the table for DESIGN.md: STOI and ESTOI of vocoder.griffin_lim's waveform against the recording, for features.npz's u0 / u1, the three
    inversions (pinv, nnls, harmonic with F0 from features.pitch_track(wav, 50, 250)) at 0 / 8 / 32 / 60 Griffin-Lim rounds.  Recorded, not
    a bar.
    python tools/stoi_bench.py [--reps 30] [--warmup 5] [--out profiles/r05/stoi/stoi_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rows', type=int, default=7)
    ap.add_argument('--frames', type=int, default=192)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r05', 'stoi', 'stoi_bench.txt'))
    a = ap.parse_args()
    from scipy import signal
    import stoi_ref as R
    from speechsplit_amd import _capi, features, metrics, vocoder
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'features.npz'))
    lines = [f'# {torch.cuda.get_device_name(0)}; median [min .. max] ms over {a.reps} runs after {a.warmup}, device events']

    # ---- timings
    B, n = a.rows, (256 * (a.frames - 1) * 5) // 8
    rng = np.random.RandomState(0)
    base = signal.resample_poly(np.concatenate([gold['u0_wav'], gold['u1_wav']] * 3), 5, 8)[:n]
    x = np.stack([np.roll(base, 977 * r) for r in range(B)])
    y = x + 0.05 * rng.standard_normal(x.shape)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    F = metrics.stoi_frames(n)
    L = 128 * (F - 1) + 256
    lo, hi = metrics.stoi_bands()
    ilo, ihi = (C.c_int * 15)(*lo), (C.c_int * 15)(*hi)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = lib.ss_stoi_scratch_bytes(B, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, dtype=torch.float64, device=dev)
    e, inv, k = torch.empty(B, F, dtype=torch.float64, device=dev), torch.empty(B, F, dtype=torch.int32, device=dev), \
        torch.empty(B, dtype=torch.int32, device=dev)
    xp, yp = torch.empty(B, L, dtype=torch.float64, device=dev), torch.empty(B, L, dtype=torch.float64, device=dev)
    env = torch.empty(B, 15, -(-(L - 256) // 128), dtype=torch.float64, device=dev)
    calls = {
        'ss_stoi (STOI)': lambda: lib.ss_stoi(p(xd), p(yd), None, B, n, ilo, ihi, 15, 0, p(out), p(scratch), nbytes, s),
        'ss_stoi (ESTOI)': lambda: lib.ss_stoi(p(xd), p(yd), None, B, n, ilo, ihi, 15, 1, p(out), p(scratch), nbytes, s),
        'energies + mask + overlap-add': lambda: lib.ss_op_stoi_compact(p(xd), p(yd), None, B, n, 0, p(e), p(inv), p(k), p(xp), p(yp), s),
        'overlap-add alone (from the map)': lambda: lib.ss_op_stoi_compact(p(xd), p(yd), None, B, n, 1, None, p(inv), p(k), p(xp), p(yp), s),
        'band envelopes of one signal': lambda: lib.ss_op_stoi_bands(p(xp), None, B, L, ilo, ihi, 15, p(env), s),
    }
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {t: [] for t in calls}
    for it in range(a.warmup + a.reps):
        for tag, fn in calls.items():
            ev[0].record()
            _capi.check(fn())
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[tag].append(ev[0].elapsed_time(ev[1]))
    lines.append(f'{B} rows x {n} samples at 10 kHz ({a.frames} mel frames\' worth): {F} frames a row, {int(k.min())} .. {int(k.max())} kept, '
                 f'scratch {nbytes / 2 ** 20:.2f} MiB')
    for tag, v in times.items():
        lines.append(f'  {tag:<34} {statistics.median(v):8.4f} [{min(v):.4f} .. {max(v):.4f}]')

    # ---- GPU against the restatement
    lines.append('GPU against tests/stoi_ref.py (term-by-term order); beside it the restatement\'s own two orders')
    for name, seed in (('u0', 1), ('u1', 2)):
        px, py = R.make_pair(signal.resample_poly(gold[name + '_wav'].astype(np.float64), 5, 8), seed)
        for ext in (False, True):
            ref, alt = R.stoi(px, py, ext, 'loop'), R.stoi(px, py, ext, 'numpy')
            got = metrics.stoi_dev(torch.from_numpy(px).to(dev)[None], torch.from_numpy(py).to(dev)[None], None, ext)[0].cpu().numpy()
            lines.append(f'  {name} {"ESTOI" if ext else "STOI "}: GPU {got[0]:.15f}  |GPU - ref| {abs(got[0] - ref["score"]):.2e}  two orders '
                         f'{abs(ref["score"] - alt["score"]):.2e}  segments {int(got[1])} ({ref["S"]})  kept {int(got[2])} ({ref["K"]}) of {ref["F"]}')

    # ---- the vocoder routes against the recording
    lines.append('vocoder.griffin_lim against the recording (16 kHz in, resampled to 10 kHz): STOI / ESTOI; phases from numpy.random.default_rng(0)')
    lines.append(f'  {"":<4} {"route":<9} ' + ' '.join(f'{str(r) + " rounds":>17}' for r in (0, 8, 32, 60)))
    for name in ('u0', 'u1'):
        wav, mel = gold[name + '_wav'].astype(np.float64), gold[name + '_S']
        f0 = features.pitch_track(wav, 50, 250, device=dev)
        for route, kw in (('pinv', dict(inversion='pinv')), ('nnls', dict(inversion='nnls')), ('harmonic', dict(inversion='pinv', f0=f0))):
            cells = []
            for rounds in (0, 8, 32, 60):
                w = vocoder.griffin_lim(mel, n_iter=rounds, device=dev, **kw)
                st, es = (metrics.stoi(wav, w, sr=16000, extended=ext, device=dev)['stoi'] for ext in (False, True))
                cells.append(f'{st:8.4f} /{es:7.4f}')
            lines.append(f'  {name:<4} {route:<9} ' + ' '.join(f'{c:>17}' for c in cells))
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
