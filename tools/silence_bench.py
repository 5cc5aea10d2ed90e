#!/usr/bin/env python3
"""GPU time of silence removal (csrc/silence.hip), ONE process, device events, median / min / max over --reps after --warmup (default 30
after 5), of ss_remove_silence and of its three stages alone (ss_op_silence_levels, ss_op_silence_mask, ss_op_silence_gather), on two
batches: 16 rows x 4 s, and 7 rows x 192 frames' worth of samples (a training batch of the model's longest crops).  Beside each:
  * the traffic bound -- the bytes the stage has to move (levels: 8 a sample read, 8 a block written; mask: 8 a block read, 4 written; gather:
    8 a kept sample read and 8 a sample written, the map aside; the whole call: their sum) over the 6.29 TB/s a streaming copy measures on
    this chip -- and how many times the bound the stage takes (a launch alone costs microseconds: at these sizes that, not HBM, is the floor);
  * the numpy restatement's time on one row (tests/silence_ref.py, one core), and whether the GPU's row equals it to the bit.
    python tools/silence_bench.py [--reps 30] [--warmup 5] [--out profiles/r05/silence/silence_bench.txt]
The recordings are seeded noise at 1e-4 with stretches of noise at 0.3 (speech-like bursts of 0.3 .. 1.2 s and pauses of 0.1 .. 0.8 s), per row.
Prints one JSON line; --out also writes it, with a table, to a file."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_BYTES_PER_S = 6.29e12                                               # measured streaming-copy rate of the chip


def recording(seed, n):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 1e-4
    t = int(rng.uniform(0.1, 0.8) * 16000)
    while t < n:
        burst = int(rng.uniform(0.3, 1.2) * 16000)
        x[t:t + burst] += rng.standard_normal(min(burst, n - t)) * 0.3
        t += burst + int(rng.uniform(0.1, 0.8) * 16000)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import silence_ref as R
    from speechsplit_amd import _capi, features
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    opts = features.Silence(40.0, 2, 6, 8)
    g = features.silence_fade()
    gp = g.ctypes.data_as(C.POINTER(C.c_double))
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        times = []
        for it in range(a.warmup + a.reps):
            ev[0].record()
            _capi.check(call())
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(ev[0].elapsed_time(ev[1]))
        return times

    report = {'reps': a.reps, 'warmup': a.warmup, 'hbm_tb_per_s': HBM_BYTES_PER_S / 1e12,
              'options': {'top_db': opts.top_db, 'hang': opts.hang, 'edge': opts.edge, 'pause': opts.pause}, 'shapes': {}}
    for name, B, n in (('16 rows x 4 s', 16, 64000), ("7 rows x 192 frames' worth", 7, 192 * 256)):
        recs = [recording(1000 + r, n) for r in range(B)]
        x = torch.from_numpy(np.stack(recs)).to(dev)
        J = (n + 255) // 256
        y = torch.empty(B, n, dtype=torch.float64, device=dev)
        e = torch.empty(B, J, dtype=torch.float64, device=dev)
        inv = torch.empty(B, J, dtype=torch.int32, device=dev)
        m, k = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        nb = lib.ss_silence_scratch_bytes(B, n)
        sc = torch.empty(nb, dtype=torch.uint8, device=dev)
        whole = lambda: lib.ss_remove_silence(p(x), None, B, n, opts.ratio, opts.hang, opts.edge, opts.pause_blocks, gp, p(y), p(m), p(inv), p(k),
                                              p(sc), nb, s)
        t_whole = timed(whole)                                           # also leaves e's inputs' outputs (inv, k) for the stages below
        t_levels = timed(lambda: lib.ss_op_silence_levels(p(x), None, B, n, p(e), s))
        t_mask = timed(lambda: lib.ss_op_silence_mask(p(e), None, B, J, opts.ratio, opts.hang, opts.edge, opts.pause_blocks, p(inv), p(k), s))
        t_gather = timed(lambda: lib.ss_op_silence_gather(p(x), None, B, n, p(inv), p(k), gp, p(y), p(m), s))
        kept = int(m.sum())
        t0 = time.perf_counter()
        ref = R.remove_silence(recs[0], opts.ratio, opts.hang, opts.edge, opts.pause_blocks)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = bool(int(m[0]) == ref['m'] and np.array_equal(y[0, :ref['m']].cpu().numpy(), ref['y']) and
                    np.array_equal(e[0].cpu().numpy(), ref['E']))
        traffic = {'levels': 8 * B * n + 8 * B * J, 'mask': 8 * B * J + 4 * B * J, 'gather': 8 * kept + 8 * B * n + 4 * B * J}
        traffic['ss_remove_silence'] = sum(traffic.values())
        rows = {}
        for stage, times in (('ss_remove_silence', t_whole), ('levels', t_levels), ('mask', t_mask), ('gather', t_gather)):
            med, bound = statistics.median(times), traffic[stage] / HBM_BYTES_PER_S * 1e3
            rows[stage] = {'median_ms': round(med, 4), 'min_ms': round(min(times), 4), 'max_ms': round(max(times), 4),
                           'traffic_bytes': traffic[stage], 'traffic_bound_ms': round(bound, 5), 'times_the_bound': round(med / bound, 1)}
        report['shapes'][name] = {'rows': B, 'samples': n, 'blocks': J, 'samples_kept': kept, 'share_kept': round(kept / (B * n), 3),
                                  'stages': rows, 'equals_the_restatement': same, 'numpy_restatement_ms_per_row': round(numpy_ms, 2)}
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(f'# tools/silence_bench.py --reps {a.reps} --warmup {a.warmup}: device-event times of ss_remove_silence and its stages on an MI355X\n')
            f.write(f'# Silence(40, 2, 6, 8); traffic bound = bytes moved / {HBM_BYTES_PER_S / 1e12:.2f} TB/s\n')
            for name, sh in report['shapes'].items():
                f.write(f"\n{name}: {sh['rows']} x {sh['samples']} samples, {sh['blocks']} blocks a row, {100 * sh['share_kept']:.1f} % of the samples kept; "
                        f"equals the restatement to the bit: {sh['equals_the_restatement']}; numpy restatement {sh['numpy_restatement_ms_per_row']} ms a row\n")
                f.write(f"  {'stage':<20}{'median ms':>11}{'min':>9}{'max':>9}{'bytes':>12}{'bound ms':>11}{'x bound':>9}\n")
                for stage, r in sh['stages'].items():
                    f.write(f"  {stage:<20}{r['median_ms']:>11.4f}{r['min_ms']:>9.4f}{r['max_ms']:>9.4f}{r['traffic_bytes']:>12}"
                            f"{r['traffic_bound_ms']:>11.5f}{r['times_the_bound']:>9.1f}\n")
            f.write('\n' + line + '\n')


if __name__ == '__main__':
    main()
