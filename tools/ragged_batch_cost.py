#!/usr/bin/env python3
"""What ragged eval-mode batches buy on a corpus of unequal utterances: 64 synthetic utterances, lengths drawn once from a fixed seed in
96 .. 1024 frames (multiples of 8), run through Generator_3 in eval mode
    (a) one by one at batch 1 -- all a caller could do before, since padding a batch changes every row's result,
    (b) as ragged batches of --rows rows in convert.plan_batches order (sorted by length: a batch costs its longest row),
    (c) as ragged batches of --rows rows in the corpus's own order (what the sort is worth).
Each pass over the corpus is timed with hipEvents round the whole pass (inputs resident on the device, one output tensor per forward);
median of --reps passes after --warmup.  Prints one JSON line with the lengths used, utterances/s of each schedule and the ratios.
    python tools/ragged_batch_cost.py [--reps 20] [--warmup 2] [--rows 16] [--precision f32]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_UTT, SEED, LO, HI = 64, 20240, 96, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rows', type=int, default=16)
    ap.add_argument('--precision', default='f32')
    a = ap.parse_args()
    from speechsplit_amd import convert, hparams as HP, model as M
    from speechsplit_amd.engine import Engine
    dev = torch.device('cuda:0')
    hp = HP.default_hparams()
    lengths = [int(8 * n) for n in np.random.default_rng(SEED).integers(LO // 8, HI // 8 + 1, N_UTT)]
    eng = Engine('G3', hp, a.rows, 192, device=dev)
    eng.set_precision(a.precision)
    eng.load_weights(M.init_weights('G3', hp, 0))
    eng.reserve(a.rows, max(lengths))
    g = torch.Generator().manual_seed(SEED)
    utts = []
    for L in lengths:
        mel = torch.rand(1, L, hp.dim_freq, generator=g)
        onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (1, L), generator=g), hp.dim_f0).float()
        emb = torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (1,), generator=g), hp.dim_spk_emb).float()
        utts.append((torch.cat((mel, onehot), -1).to(dev), mel.to(dev), emb.to(dev)))

    def batches(plan):
        """device-resident padded inputs and the length array of every batch of a plan"""
        out = []
        for idx in plan:
            T = max(lengths[i] for i in idx)
            x_f0 = torch.zeros(len(idx), T, hp.dim_freq + hp.dim_f0, device=dev)
            mel = torch.zeros(len(idx), T, hp.dim_freq, device=dev)
            for n, i in enumerate(idx):
                x_f0[n, :lengths[i]], mel[n, :lengths[i]] = utts[i][0][0], utts[i][1][0]
            out.append((x_f0, mel, torch.cat([utts[i][2] for i in idx]), torch.tensor([lengths[i] for i in idx], dtype=torch.int32, device=dev)))
        return out

    sorted_b = batches(convert.plan_batches(lengths, a.rows))
    unsorted_b = batches([list(range(k, min(k + a.rows, N_UTT))) for k in range(0, N_UTT, a.rows)])
    schedules = {
        'batch1': lambda: [eng.g3_forward(x, m, e) for x, m, e in utts],
        'ragged_sorted': lambda: [eng.g3_forward(x, m, e, lengths=ln) for x, m, e, ln in sorted_b],
        'ragged_unsorted': lambda: [eng.g3_forward(x, m, e, lengths=ln) for x, m, e, ln in unsorted_b],
    }
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {}
    for name, run in schedules.items():
        times = []
        for it in range(a.warmup + a.reps):
            ev[0].record()
            run()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(ev[0].elapsed_time(ev[1]))
        eng.check()
        ms[name] = (statistics.median(times), min(times), max(times))
    ups = {k: N_UTT / (v[0] / 1000.0) for k, v in ms.items()}
    print(json.dumps({'model': 'G3', 'precision': a.precision, 'utterances': N_UTT, 'rows_per_batch': a.rows, 'reps': a.reps, 'seed': SEED,
                      'lengths': lengths, 'frames_total': sum(lengths),
                      'ms_per_corpus': {k: {'median': round(v[0], 3), 'min': round(v[1], 3), 'max': round(v[2], 3)} for k, v in ms.items()},
                      'utterances_per_s': {k: round(v, 1) for k, v in ups.items()},
                      'ragged_sorted_over_batch1': round(ups['ragged_sorted'] / ups['batch1'], 2),
                      'ragged_unsorted_over_batch1': round(ups['ragged_unsorted'] / ups['batch1'], 2),
                      'sorted_over_unsorted': round(ups['ragged_sorted'] / ups['ragged_unsorted'], 2)}), flush=True)


if __name__ == '__main__':
    main()
