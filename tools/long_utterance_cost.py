#!/usr/bin/env python3
"""GPU time of eval-mode forwards on long utterances: median of --reps forwards per shape (hipEvents round each call, after --warmup),
frames/s and the real-time factor (frames x 16 ms / time), for Generator_3 and Generator_6 in both precision modes.  One extra forward
per shape runs with the engine's profile brackets (ss_profile, every class) and reports the summed bracket time per class: how much
of a long utterance is recurrence latency (rec_fwd: decoder, enc_rec: encoder BLSTMs) against GEMMs and GroupNorm.  Brackets on
parallel branch streams overlap, so the class sums can exceed the forward's time.
    python tools/long_utterance_cost.py [--reps 20] [--warmup 3] [--precision f32 bf16]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('G3', 1, 192), ('G3', 1, 1024), ('G3', 1, 4096), ('G3', 7, 1024), ('G6', 1, 1024), ('G6', 1, 4096)]
HOP_MS = 16.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', nargs='+', default=['f32', 'bf16'])
    a = ap.parse_args()
    from speechsplit_amd import hparams as HP, model as M
    from speechsplit_amd.engine import Engine
    dev = torch.device('cuda:0')
    hp = HP.default_hparams()
    for prec in a.precision:
        engines = {}
        for kind, B, T in SHAPES:
            if kind not in engines:      # an ordinary 8 x 192 engine: the long shapes grow its workspace (Engine.reserve)
                engines[kind] = Engine(kind, hp, 8, 192, device=dev)
                engines[kind].set_precision(prec)
                engines[kind].load_weights(M.init_weights(kind, hp, 0))
            eng = engines[kind]
            g = torch.Generator().manual_seed(B * 10000 + T)
            mel = torch.rand(B, T, hp.dim_freq, generator=g).to(dev)
            onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (B, T), generator=g), hp.dim_f0).float().to(dev)
            emb = torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (B,), generator=g), hp.dim_spk_emb).float().to(dev)
            x_f0 = torch.cat((mel, onehot), -1)

            def forward():
                return eng.g3_forward(x_f0, mel, emb) if kind == 'G3' else eng.g6_forward(mel, onehot)

            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = []
            for it in range(a.warmup + a.reps):
                ev[0].record()
                forward()
                ev[1].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times.append(ev[0].elapsed_time(ev[1]))
            eng.profile('timeline')
            forward()
            torch.cuda.synchronize()
            per_class = {}
            for name, t0, t1, _ in eng.profile_timeline():
                per_class[name] = per_class.get(name, 0.0) + (t1 - t0) / 1000.0
            eng.profile(False)
            eng.check()
            ms = statistics.median(times)
            print(json.dumps({'model': kind, 'precision': prec, 'batch': B, 'frames': T, 'reps': a.reps, 'ms_median': round(ms, 3),
                              'ms_minmax': [round(min(times), 3), round(max(times), 3)],
                              'frames_per_s': round(B * T / (ms / 1000.0)), 'rtf': round(B * T * HOP_MS / ms, 1),
                              'profile_ms': {k: round(v, 3) for k, v in sorted(per_class.items(), key=lambda kv: -kv[1])}}), flush=True)


if __name__ == '__main__':
    main()
