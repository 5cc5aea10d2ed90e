#!/usr/bin/env python3
"""GPU time of the backward with the input gradients (ss_g3_backward_inputs / ss_g6_backward_inputs, every output requested) against the
plain backward (ss_g3_backward / ss_g6_backward) on the same forward: hipEvents around each call, median over --reps.
    python tools/input_grad_cost.py [--batch 64] [--frames 128] [--model G3] [--reps 30] [--training]"""
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
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=128)
    ap.add_argument('--model', default='G3')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--training', action='store_true', help='train-mode forward (resampling in the encoders) instead of eval')
    a = ap.parse_args()
    from speechsplit_amd import hparams as HP, model as M
    from speechsplit_amd.engine import Engine, draw_interp
    dev = torch.device('cuda:0')
    B, T, kind = a.batch, a.frames, a.model
    hp = HP.default_hparams(max_len_pad=T, batch_size=B)
    eng = Engine(kind, hp, B, T, device=dev)
    eng.load_weights(M.init_weights(kind, hp, 0))
    g = torch.Generator().manual_seed(0)
    mel = torch.rand(B, T, hp.dim_freq, generator=g).to(dev)
    onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (B, T), generator=g), hp.dim_f0).float().to(dev)
    emb = torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (B,), generator=g), hp.dim_spk_emb).float().to(dev)
    out_dim = hp.dim_freq if kind == 'G3' else hp.dim_f0
    d_out = torch.randn(B, T, out_dim, generator=g).to(dev)
    draws = draw_interp(B, 3, hp, generator=g) if a.training else None
    names = Engine.G3_INPUTS if kind == 'G3' else Engine.G6_INPUTS
    x_f0 = torch.cat((mel, onehot), -1)

    def forward():
        if kind == 'G3':
            eng.g3_forward(x_f0, mel, emb, draws, training=a.training)
        else:
            eng.g6_forward(mel, onehot, draws, training=a.training)

    def backward(inputs):
        return eng.g3_backward(d_out, inputs=inputs) if kind == 'G3' else eng.g6_backward(d_out, inputs=inputs)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {'plain': [], 'inputs': []}
    for it in range(a.warmup + a.reps):
        for tag, inputs in (('plain', ()), ('inputs', names)):      # alternated: both see the same clocks and cache state
            forward()
            ev[0].record()
            backward(inputs)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[tag].append(ev[0].elapsed_time(ev[1]))
    eng.check()
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({'model': kind, 'batch': B, 'frames': T, 'training': a.training, 'reps': a.reps,
                      'backward_ms_median': round(med['plain'], 4), 'backward_inputs_ms_median': round(med['inputs'], 4),
                      'extra_ms': round(med['inputs'] - med['plain'], 4),
                      'backward_ms_minmax': [round(min(times['plain']), 4), round(max(times['plain']), 4)],
                      'backward_inputs_ms_minmax': [round(min(times['inputs']), 4), round(max(times['inputs']), 4)]}))


if __name__ == '__main__':
    main()
