#!/usr/bin/env python3
"""GPU time of conversion through the codes against the forward path it replaces, ONE process, device events, median / min / max over
--reps after --warmup, the variants alternated call by call, --inner calls per timed window, at --frames frames (default 192):
  * the seven conditions of one demo conversion: the batch-7 Generator_3 forward of convert.demo_conversion against one batch-2 encode
    plus one batch-7 decode of the recombined codes (convert.demo_conversion_codes) -- the Generator_3 part only, inputs on the device;
    and a batch-7 encode plus the batch-7 decode, which repeats encoder work but keeps both calls at one (B, T): the engine re-plans
    and re-zeroes its workspace at every change of shape;
  * one utterance for --speakers speakers: one batch-N forward, and N batch-1 forwards, against one batch-1 encode plus one batch-N decode
    (convert.convert_speakers), and against the batch-N decode alone on codes kept from an earlier encode.
Before anything is timed the outputs of the variants are compared (relative max-norm, must be below 1e-4).
    python tools/codes_bench.py [--frames 192] [--speakers 16] [--reps 30] [--warmup 5] [--inner 10] [--precision f32]
Prints one JSON line.

--train: instead, the step times of training on cached codes (the differentiable decode) beside the full training step, one engine, one
process, device events, median / min / max of --reps runs after --warmup, the variants alternated run by run, at --batches x --train-frames
(default 64,16 x 128): ss_g3_train_step against the fused ss_g3_decode_train_step on that batch's codes, and the separate calls
ss_g3_decode_train / ss_g3_decode_backward (with dc_trg) / ss_adam_step_decoder.  One JSON line per batch size.
    python tools/codes_bench.py --train [--batches 64,16] [--train-frames 128] [--reps 30] [--warmup 5] [--precision f32]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train_times(a):
    import numpy as np
    from oracle import weights as W
    from oracle.gen_fixtures import draws_for, synth_batch
    from speechsplit_amd.engine import Engine
    T = a.train_frames
    hp = W.default_hparams(max_len_pad=T)
    for B in [int(b) for b in a.batches.split(',')]:
        eng = Engine('G3', hp, B, T, device='cuda:0')
        eng.set_precision(a.precision)
        eng.load_weights(W.make_weights('G3', hp, 3))
        eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
        mel, f0, emb, lens = synth_batch(31, B, T, 64)
        draws = draws_for(41, B, 4)
        d = (np.stack([x[0] for x in draws]), np.stack([x[1] for x in draws]))
        dev = eng.device
        mel, f0, emb, lens = mel.to(dev), f0.to(dev), emb.to(dev), lens.to(dev)
        d = (torch.from_numpy(d[0]).to(dev), torch.from_numpy(d[1]).to(dev))
        onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (B, T), generator=torch.Generator().manual_seed(2)), hp.dim_f0).float().to(dev)
        codes = eng.g3_encode(torch.cat((mel, onehot), -1), mel)
        d_out = torch.randn(B, T, hp.dim_freq, device=dev) / (B * T)
        variants = (('full_step', lambda: eng.g3_train_step(mel, f0, emb, lens, d)),
                    ('decode_step', lambda: eng.g3_decode_train_step(*codes, emb, mel, want_dc_trg=True)),
                    ('decode_forward', lambda: eng.g3_decode_train(*codes, emb)),
                    ('decode_backward', lambda: eng.g3_decode_backward(d_out, want=('c_trg',))),      # (follows decode_forward: the order below)
                    ('adam_decoder', lambda: eng.adam_step_decoder()))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {k: [] for k, _ in variants}
        for it in range(a.warmup + a.reps):
            for tag, fn in variants:
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[tag].append(ev[0].elapsed_time(ev[1]))
        eng.check()
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({'train': True, 'batch': B, 'frames': T, 'precision': a.precision, 'reps': a.reps,
                          'ms_median': {k: round(v, 4) for k, v in med.items()},
                          'ms_minmax': {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                          'decode_step_over_full_step': round(med['decode_step'] / med['full_step'], 3),
                          'separate_calls_sum_ms': round(med['decode_forward'] + med['decode_backward'] + med['adam_decoder'], 4)}))
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=192)
    ap.add_argument('--speakers', type=int, default=16)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--precision', default='f32', choices=('f32', 'bf16'))
    ap.add_argument('--train', action='store_true', help='time training on cached codes beside the full training step instead')
    ap.add_argument('--batches', default='64,16')
    ap.add_argument('--train-frames', type=int, default=128)
    a = ap.parse_args()
    if a.train:
        if not torch.cuda.is_available():
            raise SystemExit('codes_bench: no GPU (there is nothing to time without one)')
        return train_times(a)
    from speechsplit_amd import convert, hparams as HPM, model
    if not torch.cuda.is_available():
        raise SystemExit('codes_bench: no GPU (there is nothing to time without one)')
    dev = torch.device('cuda:0')
    hp = HPM.default_hparams(precision=a.precision)
    T, N = a.frames, a.speakers
    torch.manual_seed(0)
    G = model.Generator_3(hp, max_batch=max(N, 7)).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    mel = lambda: torch.rand(1, T, hp.dim_freq, generator=g).to(dev)
    onehot = lambda: torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (1, T), generator=g), hp.dim_f0).float().to(dev)
    spk = lambda n: torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (n,), generator=g), hp.dim_spk_emb).float().to(dev)
    x_org, x_trg, oh_org, oh_con = mel(), mel(), onehot(), onehot()
    emb_org, emb_trg, embs = spk(1), spk(1), spk(N)
    xf_org, xf_trg = torch.cat((x_org, oh_org), -1), torch.cat((x_org, oh_con), -1)
    cond = convert.CONDITIONS
    # the seven conditions as convert.demo_conversion lays them out ...
    x_f0 = torch.cat([xf_trg if 'F' in c else xf_org for c in cond])
    x_rh = torch.cat([x_trg if 'R' in c else x_org for c in cond])
    emb = torch.cat([emb_trg if 'U' in c else emb_org for c in cond])
    # ... and as convert.demo_conversion_codes does
    enc_f0, enc_rh = torch.cat((xf_org, xf_trg)), torch.cat((x_org, x_trg))
    rh = torch.tensor([1 if 'R' in c else 0 for c in cond], device=dev)
    f0 = torch.tensor([1 if 'F' in c else 0 for c in cond], device=dev)

    def seven_forward():
        return G(x_f0, x_rh, emb)

    def seven_codes():
        cx, cr, cf = G.encode(enc_f0, enc_rh)
        return G.decode(cx[:1].expand(len(cond), -1, -1), cr[rh], cf[f0], emb)

    def seven_codes_one_shape():      # the encode over all seven rows: redundant work, but both calls at one (B, T) -- no workspace re-plan between them
        return G.decode(*G.encode(x_f0, x_rh), emb)

    def grid_forward():
        return G(xf_org.expand(N, -1, -1), x_org.expand(N, -1, -1), embs)

    def grid_forward_batch1():
        return torch.cat([G(xf_org, x_org, embs[n:n + 1]) for n in range(N)])

    def grid_codes():
        cx, cr, cf = G.encode(xf_org, x_org)
        return G.decode(cx.expand(N, -1, -1), cr.expand(N, -1, -1), cf.expand(N, -1, -1), embs)

    cached = {}

    def grid_decode_cached():         # the codes of the utterance kept from an earlier encode (a cached corpus): the decode alone
        if not cached:
            cached['codes'] = tuple(c.expand(N, -1, -1).contiguous() for c in G.encode(xf_org, x_org))
        return G.decode(*cached['codes'], embs)

    rel = lambda x, y: float((x.double() - y.double()).abs().max() / y.double().abs().max())
    variants = (('seven_forward', seven_forward), ('seven_codes', seven_codes), ('seven_codes_one_shape', seven_codes_one_shape), ('grid_forward', grid_forward),
                ('grid_forward_batch1', grid_forward_batch1), ('grid_codes', grid_codes), ('grid_decode_cached', grid_decode_cached))
    with torch.no_grad():
        same = {'seven': rel(seven_codes(), seven_forward()), 'seven_one_shape': rel(seven_codes_one_shape(), seven_forward()), 'grid': rel(grid_codes(), grid_forward()),
                'grid_batch1': rel(grid_forward_batch1(), grid_forward()), 'grid_cached': rel(grid_decode_cached(), grid_forward())}
        assert all(v < 1e-4 for v in same.values()), same
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {k: [] for k, _ in variants}
        for it in range(a.warmup + a.reps):
            for tag, fn in variants:
                ev[0].record()
                for _ in range(a.inner):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[tag].append(ev[0].elapsed_time(ev[1]) / a.inner)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({'frames': T, 'speakers': N, 'precision': a.precision, 'reps': a.reps, 'inner': a.inner,
                      'ms_median': {k: round(v, 4) for k, v in med.items()},
                      'ms_minmax': {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                      'seven_forward_over_codes': round(med['seven_forward'] / med['seven_codes'], 3),
                      'grid_forward_over_codes': round(med['grid_forward'] / med['grid_codes'], 3),
                      'grid_batch1_over_codes': round(med['grid_forward_batch1'] / med['grid_codes'], 3),
                      'grid_forward_over_decode_cached': round(med['grid_forward'] / med['grid_decode_cached'], 3),
                      'rel_between_variants': {k: float(f'{v:.2e}') for k, v in same.items()}}))


if __name__ == '__main__':
    main()
