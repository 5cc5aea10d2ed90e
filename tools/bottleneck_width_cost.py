#!/usr/bin/env python3
"""What a bottleneck width costs: for the default widths and the test configurations of tests/test_capi_bottleneck_widths.py, the median
of --reps fused training steps at 64 x 128 (Generator_3; Generator_6 for P_mix), the median of --reps eval-mode forwards at 1 x 192
(hipEvents round each call, after --warmup), and the encoder BLSTM recurrences' share: the summed ss_profile brackets of class enc_rec
(SS_PROF_ENC_REC, the lstm_small_* launches) over one bracketed step / forward.  Brackets on parallel branch streams overlap, so enc_rec
can exceed what the recurrences add to the step's time.
    python tools/bottleneck_width_cost.py [--reps 20] [--warmup 3] [--configs default W_odd W_mix W_top P_mix]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import interp_np, weights as W  # noqa: E402
from oracle.gen_fixtures import draws_for, synth_batch  # noqa: E402
from tests.test_capi_bottleneck_widths import CONFIGS  # noqa: E402


def hparams_of(name, T):
    if name == 'default':
        return 'G3', W.default_hparams(max_len_pad=T)
    kind, (n1, n2, n3), (f1, f2, f3) = CONFIGS[name]
    return kind, W.default_hparams(dim_neck=n1, dim_neck_2=n2, dim_neck_3=n3, freq=f1, freq_2=f2, freq_3=f3, max_len_pad=T)


def timed(fn, warmup, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for it in range(warmup + reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(times)


def enc_rec_ms(eng, fn):
    eng.profile(['enc_rec'])
    fn()
    torch.cuda.synchronize()
    ms = sum(t1 - t0 for _, t0, t1, _ in eng.profile_timeline()) / 1000.0
    eng.profile(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--configs', nargs='+', default=['default'] + list(CONFIGS))
    a = ap.parse_args()
    from speechsplit_amd.engine import Engine
    dev = torch.device('cuda:0')
    for name in a.configs:
        kind, hp = hparams_of(name, 128)
        B, T = 64, 128
        eng = Engine(kind, hp, B, T, device=dev)
        eng.load_weights(W.make_weights(kind, hp, 3))
        eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
        mel, f0, emb, lens = synth_batch(5, B, T, 64)
        dr = draws_for(6, B, 4 if kind == 'G3' else 3)
        d = (np.stack([x[0] for x in dr]), np.stack([x[1] for x in dr]))
        if kind == 'G3':
            step = lambda: eng.g3_train_step(mel, f0, emb, lens, d)
        else:
            qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
            onehot = torch.nn.functional.one_hot(qidx, 257).float()
            step = lambda: eng.g6_train_step(mel, onehot, qidx, d)
        train_ms = timed(step, a.warmup, a.reps)
        train_rec = enc_rec_ms(eng, step)
        Te = 192
        _, hpe = hparams_of(name, Te)
        ev_eng = Engine(kind, hpe, 1, Te, device=dev)
        ev_eng.load_weights(W.make_weights(kind, hpe, 3))
        g = torch.Generator().manual_seed(7)
        mel1 = torch.rand(1, Te, 80, generator=g).to(dev)
        oh1 = torch.nn.functional.one_hot(torch.randint(0, 257, (1, Te), generator=g), 257).float().to(dev)
        emb1 = torch.nn.functional.one_hot(torch.randint(0, 82, (1,), generator=g), 82).float().to(dev)
        x_f0 = torch.cat((mel1, oh1), -1)
        fwd = (lambda: ev_eng.g3_forward(x_f0, mel1, emb1)) if kind == 'G3' else (lambda: ev_eng.g6_forward(mel1, oh1))
        eval_ms = timed(fwd, a.warmup, a.reps)
        eval_rec = enc_rec_ms(ev_eng, fwd)
        eng.check()
        ev_eng.check()
        print(json.dumps({'config': name, 'model': kind, 'widths': [hp.dim_neck, hp.dim_neck_2, hp.dim_neck_3],
                          'factors': [hp.freq, hp.freq_2, hp.freq_3], 'train_64x128_ms': round(train_ms, 3),
                          'train_enc_rec_ms': round(train_rec, 3), 'eval_1x192_ms': round(eval_ms, 3), 'eval_enc_rec_ms': round(eval_rec, 3)}),
              flush=True)
        del eng, ev_eng
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
