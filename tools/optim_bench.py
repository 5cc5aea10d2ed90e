"""Time of the stand-alone optimiser step (ss_adam_step) with decoupled weight decay and the parameter EMA off and on, clipped and not, and of
a separate ema_range pass over the whole arena (what an unfused average would add): device events, medians of 30 after 5 warm-up runs, the
forms alternating inside one process.  Prints the bytes per element each form moves and the time it implies per element.

    python tools/optim_bench.py [--kind G3] [--runs 30] [--warmup 5]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechsplit_amd import _capi, engine as E, hparams as HP  # noqa: E402

# form -> (weight decay, which, EMA decay, bytes per element: read p g m v (+ ema), write p m v (+ ema))
FORMS = {'off': (0.0, 'all', None, 28), 'wd': (0.01, 'all', None, 28), 'wd_weights': (0.01, 'weights', None, 28), 'ema': (0.0, 'all', 0.999, 36),
         'both': (0.01, 'all', 0.999, 36), 'both_weights': (0.01, 'weights', 0.999, 36)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', default='G3', choices=['G3', 'G6'])
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    hp = HP.default_hparams(max_len_pad=8)
    eng = E.Engine(a.kind, hp, 2, 8)
    n = eng.params.numel()
    torch.manual_seed(0)
    eng.params.copy_(torch.randn(n, device=eng.device) * 0.05)
    eng.grads.copy_(torch.randn(n, device=eng.device) * 1e-3)
    eng.grads[n - 4:] = 0                                     # the status slot
    eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
    state = torch.zeros(64, dtype=torch.float32, device=eng.device)

    def configure(form, clip):
        wd, which, decay, _ = FORMS[form]
        eng.set_grad_clip(float('inf') if clip else 0)
        eng.set_weight_decay(wd, which)
        eng.set_ema(decay)

    def separate_pass(step):
        """the hook's ema_range over the whole arena; step < 0: under the state the step = 0 call left -- one launch, no copy, no host wait"""
        o = _capi.SSOptimExtOp()
        for k, v in dict(p=eng.params.data_ptr(), ema=eng.ema.data_ptr(), state=state.data_ptr(), lo=0, hi=n, lr=1e-4, beta1=0.9, beta2=0.999,
                         eps=1e-8, ema_decay=0.999, mode=1, step=step).items():
            setattr(o, k, v)
        _capi.check(eng.lib.ss_op_optim_ext(C.byref(o), None))

    cases = [(f, c) for c in (False, True) for f in FORMS] + [('ema_range alone', False)]
    times = {c: [] for c in cases}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for it in range(a.warmup + a.runs):
        for case in cases:
            form, clip = case
            if form == 'ema_range alone':
                configure('ema', False)
                separate_pass(0)                # fills the state (a host copy and a wait: outside the bracket)
                torch.cuda.synchronize()
                ev[0].record()
                separate_pass(-1)               # the ema_range launch alone
                ev[1].record()
            else:
                configure(form, clip)
                torch.cuda.synchronize()
                ev[0].record()
                eng.adam_step(1.0)
                ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[case].append(ev[0].elapsed_time(ev[1]) * 1e3)
    eng.check()
    base = statistics.median(times[('off', False)])
    print(f'{a.kind}: arena {n} floats; medians of {a.runs} after {a.warmup} warm-up runs, microseconds (device events round the whole ss_adam_step)')
    for (form, clip), ts in times.items():
        med, lo, hi = statistics.median(ts), min(ts), max(ts)
        if form == 'ema_range alone':
            print(f'  {"ema_range alone (one launch)":28s} {med:9.1f}  [{lo:.1f} .. {hi:.1f}]  {med / base:5.2f} x off   12 B/elt ({12 / 28:.2f} x)   '
                  f'{12 * n / med / 1e6:7.2f} TB/s')
            continue
        b = FORMS[form][3]
        print(f'  {form + (" + clip(inf)" if clip else ""):28s} {med:9.1f}  [{lo:.1f} .. {hi:.1f}]  {med / base:5.2f} x off   {b} B/elt '
              f'({b / 28:.2f} x)   {b * n / med / 1e6:7.2f} TB/s')


if __name__ == '__main__':
    main()
