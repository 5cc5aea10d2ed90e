#!/usr/bin/env python3
"""GPU time of the fused train step with gradient clipping (Engine.set_grad_clip) off, on with a max_norm that clips, and on with
max_norm = inf (norm and non-finite guard only): ONE process, the three modes alternated step by step so that all see the same clocks and
cache state, device events around each step, median / min / max over --reps after --warmup.  Also the number of bracketed launches per
step in each mode (ss_profile_timeline records of one step taken after the timing).
    python tools/grad_clip_cost.py [--model G3] [--batch 64] [--frames 128] [--precision f32] [--reps 30] [--force-dp]
--force-dp: the native data-parallel step on a one-rank communicator (ss_g3_dp_train_step / ss_g6_dp_train_step) instead of the fused step.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='G3')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=128)
    ap.add_argument('--precision', default='f32')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--force-dp', action='store_true', help='world-1 native data-parallel step instead of the fused one-GPU step')
    a = ap.parse_args()
    if a.reps < 30:
        ap.error('--reps: at least 30')
    from speechsplit_amd import hparams as HP, model as M
    from speechsplit_amd.engine import Engine, draw_interp
    dev = torch.device('cuda:0')
    B, T, kind = a.batch, a.frames, a.model
    hp = HP.default_hparams(max_len_pad=T, batch_size=B)
    eng = Engine(kind, hp, B, T, device=dev)
    eng.set_precision(a.precision)
    eng.load_weights(M.init_weights(kind, hp, 0))
    eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
    if a.force_dp:
        eng.comm_init(0, 1)
    g = torch.Generator().manual_seed(0)
    mel = torch.rand(B, T, hp.dim_freq, generator=g).to(dev)
    f0 = torch.rand(B, T, 1, generator=g).to(dev)
    emb = torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (B,), generator=g), hp.dim_spk_emb).float().to(dev)
    lens = torch.full((B,), T, dtype=torch.int32).to(dev)
    qidx = torch.randint(0, hp.dim_f0, (B, T), generator=g)
    onehot = torch.nn.functional.one_hot(qidx, hp.dim_f0).float().to(dev)
    qidx = qidx.to(torch.int32).to(dev)
    sc, ls = draw_interp(B, 4 if kind == 'G3' else 3, hp, generator=g)
    draws = (sc.to(dev), ls.to(dev))

    def step():
        if kind == 'G3':
            return eng.dp_train_step_native(mel, f0, emb, lens, draws) if a.force_dp else eng.g3_train_step(mel, f0, emb, lens, draws)
        return eng.g6_dp_train_step_native(mel, onehot, qidx, draws) if a.force_dp else eng.g6_train_step(mel, onehot, qidx, draws)

    # a max_norm that clips: half the norm of the first step's gradients
    eng.set_grad_clip(float('inf'))
    step()
    norm0 = float(eng.grad_clip_stats()[0])
    modes = (('off', 0.0), ('clip', 0.5 * norm0), ('inf', float('inf')))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k, _ in modes}
    for it in range(a.warmup + a.reps):
        for tag, max_norm in modes:
            eng.set_grad_clip(max_norm)
            ev[0].record()
            step()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[tag].append(ev[0].elapsed_time(ev[1]))
    stats = {}
    records = {}
    for tag, max_norm in modes:
        eng.set_grad_clip(max_norm)
        step()
        stats[tag] = [float(x) for x in eng.grad_clip_stats().cpu()]
        eng.profile('timeline')
        step()
        torch.cuda.synchronize()
        tl = eng.profile_timeline()
        eng.profile(False)
        records[tag] = {'all': len(tl), 'adam': sum(1 for r in tl if r[0] == 'adam')}
    eng.check()
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({'model': kind, 'batch': B, 'frames': T, 'precision': a.precision, 'force_dp': a.force_dp, 'reps': a.reps,
                      'step_ms_median': {k: round(v, 4) for k, v in med.items()},
                      'step_ms_minmax': {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                      'extra_ms': {'clip': round(med['clip'] - med['off'], 4), 'inf': round(med['inf'] - med['off'], 4)},
                      'first_norm': round(norm0, 6), 'last_coef': {k: round(v[1], 6) for k, v in stats.items()},
                      'timeline_records_per_step': records}))
    if a.force_dp:
        eng.lib.ss_comm_destroy(eng.h)


if __name__ == '__main__':
    main()
