#!/usr/bin/env python3
"""GPU time of the conversion scores (csrc/dtw.hip), ONE process, device events, median / min / max over --reps after --warmup:
  * ss_mel_cepstra, ss_dtw and ss_path_f0_stats, each alone, on B pairs of Tx x Ty frames (24 cepstra of 80 mel bands) for
    (Tx, Ty) in (135, 135), (192, 192), (1024, 1024), (4096, 4096) and B in 1, 16, 256;
  * beside ss_dtw its serial-chain bound: one wavefront sweeps ceil(Tx / 64) strips of Ty + 63 dependent steps, so time / steps is what one
    step of the chain costs (ns, and cycles at the --mhz the box reports);
  * beside them the float64 numpy restatement (tests/dtw_ref.py: cepstra, dtw, f0_stats; wall clock, one pair, one pass) where the lattice
    has at most --ref-cells cells, and whether path and total agree there.
    python tools/dtw_bench.py [--reps 5] [--warmup 2] [--out profiles/r05/dtw_bench.txt]
The mels are a random walk in time (seeded per pair), clipped to [0, 1], the second a warped noisy copy of the first."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = ((135, 135), (192, 192), (1024, 1024), (4096, 4096))
ROWS = (1, 16, 256)
STRIP = 64


def mel_pair(seed, Tx, Ty):
    import dtw_ref as R
    rng = np.random.default_rng(seed)
    x = np.clip(0.5 + np.cumsum(rng.normal(0.0, 0.03, (Tx, 80)), axis=0), 0.0, 1.0).astype(np.float32)
    return x, R.warped(x, Ty, seed + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--ref-cells', type=int, default=1100000)
    ap.add_argument('--mhz', type=float, default=2400.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r05', 'dtw_bench.txt'))
    a = ap.parse_args()
    import dtw_ref as R
    from speechsplit_amd import _capi, metrics
    lib = _capi.lib()
    dev = torch.device('cuda:0')
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dct_h = metrics.dct_basis(24, 80)
    dct = torch.from_numpy(dct_h).to(dev)
    lines = [f'# {torch.cuda.get_device_name(0)}; 24 cepstra of 80 bands; median [min .. max] ms over {a.reps} runs after {a.warmup}; '
             f'steps = ceil(Tx / {STRIP}) x (Ty + {STRIP - 1}); cycles at {a.mhz:.0f} MHz',
             f'{"Tx x Ty":>11} {"B":>4} | {"cepstra ms":>24} | {"dtw ms":>30} | {"f0 stats ms":>24} | {"steps/pair":>10} {"ns/step":>8} '
             f'{"cyc/step":>8} {"us/pair":>9} | {"scratch MiB":>11} | numpy ms/pair (cepstra, dtw, f0) agrees']
    for Tx, Ty in SHAPES:
        pairs = [mel_pair(10 * n, Tx, Ty) for n in range(4)]                               # four distinct pairs, repeated over the rows
        rng = np.random.default_rng(5)
        f0 = [np.where(rng.uniform(size=T) < 0.3, -1e10, 5.0 + 0.2 * np.sin(np.arange(T) / 7.0)) for T in (Tx, Ty)]
        ref = None
        if Tx * Ty <= a.ref_cells:
            x, y = pairs[0]
            t0 = time.perf_counter()
            cx, cy = R.cepstra(x, dct_h), R.cepstra(y, dct_h)
            t1 = time.perf_counter()
            total, path, _ = R.dtw(cx, cy)
            t2 = time.perf_counter()
            R.f0_stats(path, *f0)
            t3 = time.perf_counter()
            ref = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, total, path)
        for B in ROWS:
            mx = torch.from_numpy(np.stack([pairs[b % 4][0] for b in range(B)])).to(dev)
            my = torch.from_numpy(np.stack([pairs[b % 4][1] for b in range(B)])).to(dev)
            f0x = torch.from_numpy(np.tile(f0[0], (B, 1))).to(dev)
            f0y = torch.from_numpy(np.tile(f0[1], (B, 1))).to(dev)
            cx = torch.empty(B, Tx, 24, dtype=torch.float64, device=dev)
            cy = torch.empty(B, Ty, 24, dtype=torch.float64, device=dev)
            nbytes = lib.ss_dtw_scratch_bytes(B, Tx, Ty)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(B, 3, dtype=torch.float64, device=dev)
            path = torch.empty(B, Tx + Ty - 1, 2, dtype=torch.int32, device=dev)
            plen = torch.empty(B, dtype=torch.int32, device=dev)
            stats = torch.empty(B, 5, dtype=torch.float64, device=dev)
            _capi.check(lib.ss_mel_cepstra(p(my), None, B, Ty, 80, p(dct), 24, p(cy), s))
            calls = {
                'cepstra': lambda: lib.ss_mel_cepstra(p(mx), None, B, Tx, 80, p(dct), 24, p(cx), s),
                'dtw': lambda: lib.ss_dtw(p(cx), None, p(cy), None, B, Tx, Ty, 24, metrics.SCALE, p(out), p(path), p(plen), p(scratch), nbytes, s),
                'f0': lambda: lib.ss_path_f0_stats(p(path), p(plen), p(f0x), p(f0y), B, Tx, Ty, p(stats), s),
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
            fmt = lambda v: f'{statistics.median(v):9.4f} [{min(v):.4f} .. {max(v):.4f}]'
            steps = -(-Tx // STRIP) * (Ty + STRIP - 1)
            med = statistics.median(times['dtw'])
            ns = med * 1e6 / steps
            tail = '-'
            if ref is not None:
                P = int(plen[0])
                same = P == len(ref[4]) and np.array_equal(path[0, :P].cpu().numpy(), ref[4]) and float(out[0, 0]) == ref[3]
                tail = f'{ref[0]:.1f}, {ref[1]:.1f}, {ref[2]:.1f}  {"yes, to the bit" if same else "NO"}'
            lines.append(f'{Tx:>5} x {Ty:<4} {B:>4} | {fmt(times["cepstra"]):>24} | {fmt(times["dtw"]):>30} | {fmt(times["f0"]):>24} | '
                         f'{steps:>10} {ns:>8.1f} {ns * a.mhz / 1e3:>8.0f} {med * 1e3 / B:>9.1f} | {nbytes / 2 ** 20:>11.2f} | {tail}')
            print(lines[-1], flush=True)
            del mx, my, cx, cy, scratch, path
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
