"""What the learning-rate schedule costs on the device: (1) the stand-alone optimiser step (ss_adam_step: one prepare launch and one Adam
launch over the whole arena) with the schedule off and with each kind on, and (2) the test hook's one-lane kernel (ss_op_lr_schedule, n = 1:
the prepare kernels' own __device__ function on one thread) per kind, which isolates the function from the arena's traffic.  Device events,
medians after warm-up runs, the forms alternating inside one process.

    python tools/lr_sched_bench.py [--kind G3] [--runs 50] [--warmup 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechsplit_amd import _capi, engine as E, hparams as HP  # noqa: E402

FORMS = {'off': dict(kind=None), 'constant': dict(kind='constant'), 'cosine': dict(kind='cosine', warmup=5, total=1000, min_lr=1e-6),
         'linear': dict(kind='linear', warmup=5, total=1000, min_lr=1e-6), 'exponential': dict(kind='exponential', warmup=5, gamma=0.999),
         'step': dict(kind='step', warmup=5, gamma=0.5, period=30)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', default='G3', choices=['G3', 'G6'])
    ap.add_argument('--runs', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    eng = E.Engine(a.kind, HP.default_hparams(max_len_pad=8), 2, 8)
    n = eng.params.numel()
    torch.manual_seed(0)
    eng.params.copy_(torch.randn(n, device=eng.device) * 0.05)
    eng.grads.copy_(torch.randn(n, device=eng.device) * 1e-3)
    eng.grads[n - 4:] = 0                                     # the status slot
    steps = torch.tensor([100], dtype=torch.int64, device=eng.device)
    out = torch.zeros(1, dtype=torch.float64, device=eng.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    step_t, hook_t = {f: [] for f in FORMS}, {f: [] for f in FORMS if f != 'off'}

    def hook(form):
        o = FORMS[form]
        _capi.check(eng.lib.ss_op_lr_schedule(E.Engine.LR_KINDS[o['kind']], 1e-4, o.get('warmup', 0), 0.1, o.get('total', 0), o.get('gamma', 0.0),
                                              o.get('period', 0), o.get('min_lr', 0.0), steps.data_ptr(), 1, out.data_ptr(), None))

    for it in range(a.warmup + a.runs):
        for form, opts in FORMS.items():
            eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 99)          # every timed step is t = 100: inside the main part of each kind
            eng.set_lr_schedule(**opts)
            torch.cuda.synchronize()
            ev[0].record()
            eng.adam_step(1.0)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                step_t[form].append(ev[0].elapsed_time(ev[1]) * 1e3)
            if form == 'off':
                continue
            ev[0].record()
            hook(form)
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                hook_t[form].append(ev[0].elapsed_time(ev[1]) * 1e3)
    eng.check()
    base = statistics.median(step_t['off'])
    print(f'{a.kind}: arena {n} floats; medians of {a.runs} after {a.warmup} warm-up runs, microseconds')
    print('ss_adam_step (prepare + Adam over the arena), device events round the call:')
    for form, ts in step_t.items():
        med = statistics.median(ts)
        print(f'  {form:12s} {med:8.1f}  [{min(ts):.1f} .. {max(ts):.1f}]  {med - base:+6.1f} us against off')
    print('the function alone on one lane (ss_op_lr_schedule, n = 1), device events round the launch:')
    cbase = statistics.median(hook_t['constant'])
    for form, ts in hook_t.items():
        med = statistics.median(ts)
        print(f'  {form:12s} {med:8.1f}  [{min(ts):.1f} .. {max(ts):.1f}]  {med - cbase:+6.1f} us against constant')


if __name__ == '__main__':
    main()
