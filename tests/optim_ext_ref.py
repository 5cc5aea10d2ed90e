"""Decoupled weight decay and the parameter EMA in float64 on top of adam_ref.adam_f64, stock fp32 torch as the yardstick, and the comparator
of the tests of both terms (test_gpu_optim_ext.py; proven on wrong stand-ins by test_optim_ext_ref_selftest.py).  Importing it needs no GPU;
every function works on tensors of any device.

The reference, for the step t being APPLIED (n: EMA updates applied so far), in float64 on the fp32 inputs promoted exactly:

    decayed element:  p1 = p * (1 - lr * wd)         (torch.optim.AdamW, single-tensor: param.mul_(1 - lr * weight_decay) comes first)
    every element:    p', m', v' = adam_f64(p1, g, m, v)                  (m' and v' do not see the decay; lr, not lr / bc1, in the factor)
    every element:    ema' = ema + (1 - d) * (P' - ema),  d = decay, or with warm-up min(decay, (1 + n) / (10 + n))
                      (torch.optim.swa_utils.get_ema_avg_fn(d): ema.lerp(P', 1 - d)), P' the fp32 parameter the step under test WROTE
A skipped step changes nothing, n included.  A decoder-only step (lo > 0) leaves p, m, v below lo alone and still averages everything.
wd is taken as the fp32 number the C ABI receives, as adam_ref takes grad_scale.

Errors are fp32 ulps with adam_ref's floors (see there) for m', v' and the update p - p'.  The EMA is compared the way the update is: the
average's own update ema' - ema = (1 - d) (P' - ema) is read off an ema' that is itself rounded, so its unit is at least half an ulp of the
larger of |ema| and |ema'| -- and P' - ema cancels when the average has caught up: the update is then far below an ulp of ema, the rounded
ema' may or may not move by one, and that floor is what makes both right.

BARS = adam_ref.FACTOR x YARDSTICK (the factor is justified in adam_ref: an equally valid operation order, a sqrt / division that is not
correctly rounded).  YARDSTICK is what stock fp32 torch on the CPU -- torch.optim.AdamW(foreach=False, fused=False) for the decay,
get_ema_avg_fn(d) for the average -- showed against this float64 over adam_ref.CASES x wd in WDS (3 steps each) and, for the average, x
decay in DECAYS x n in NS with and without warm-up, at 2^21 = 2 097 152 elements (measure_yardstick(1 << 21), 7 classes of 299 593 elements).
m' and v' do not depend on the decay: their bars are adam_ref's.  Without decay the update's bars are adam_ref's too.  Nothing here comes from
the engine.  test_optim_ext_ref_selftest.py re-measures at a small size and holds the result under YARDSTICK.
"""
import math

import numpy as np
import torch

from tests import adam_ref as A

WDS = (1e-2, 0.1)
DECAYS = (0.5, 0.999, 0.9999)
NS = (0, 7, 10 ** 6)

# worst error of stock fp32 torch against float64 per class (measure_yardstick(1 << 21), CPU), rounded UP to three digits
YARDSTICK = {
    'upd_wd': dict(ordinary=5.04, zero=1.66, near_eps=4.54, large=5.49, tiny=1.66, alternating=5.33, fading=5.07),
    'ema':    dict(ordinary=3.77, zero=3.77, near_eps=3.77, large=3.77, tiny=3.77, alternating=3.77, fading=3.77),
}
BARS = {q: {c: A.FACTOR * y for c, y in row.items()} for q, row in YARDSTICK.items()}


def f32(x):
    """the fp32 number the C ABI receives for the Python float x, as a Python float"""
    return float(np.float32(x))


def ema_d(decay, warmup, n):
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


# ------------------------------------------------------------------------------------------------ float64
def step_f64(p, g, m, v, *, lr, beta1, beta2, eps, t, grad_scale=1.0, wd=0.0, decayed=None, lo=0):
    """(p', m', v') of one AdamW step in float64.  decayed: bool mask of the decayed elements (None: all).  lo: a decoder-only step, the
    elements below lo keep their values."""
    p64 = p.detach().double()
    f = 1.0 - lr * f32(wd)
    p1 = p64 * f if decayed is None else torch.where(decayed, p64 * f, p64)
    pn, mn, vn = A.adam_f64(p1, g, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, t=t, grad_scale=grad_scale)
    if lo:
        for new, old in ((pn, p), (mn, m), (vn, v)):
            new[:lo] = old[:lo].double()
    return pn, mn, vn


def ema_f64(ema, p_new, decay, warmup=False, n=0):
    """The average after one update towards the fp32 parameters p_new, in float64."""
    e = ema.detach().double()
    return e + (1.0 - ema_d(decay, warmup, n)) * (p_new.detach().double() - e)


# ------------------------------------------------------------------------------------------------ stock fp32 torch
def adamw_f32_torch(p, g, m, v, *, lr, beta1, beta2, eps, t, grad_scale=1.0, wd=0.0):
    """adam_ref.adam_f32_torch with torch.optim.AdamW(weight_decay=wd): (p', m', v') in fp32 on the CPU."""
    f = lambda x: x.detach().to(device='cpu', dtype=torch.float32).clone()
    par = torch.nn.Parameter(f(p))
    opt = torch.optim.AdamW([par], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=f32(wd), amsgrad=False, foreach=False, fused=False)
    sd = opt.state_dict()
    sd['state'] = {0: dict(step=torch.tensor(float(t - 1)), exp_avg=f(m), exp_avg_sq=f(v))}
    opt.load_state_dict(sd)
    par.grad = f(g) * torch.tensor(grad_scale, dtype=torch.float32)
    opt.step()
    st = opt.state[par]
    return par.detach(), st['exp_avg'], st['exp_avg_sq']


def ema_f32_torch(ema, p_new, decay, warmup=False, n=0):
    from torch.optim.swa_utils import get_ema_avg_fn
    f = lambda x: x.detach().to(device='cpu', dtype=torch.float32).clone()
    return get_ema_avg_fn(ema_d(decay, warmup, n))(f(ema), f(p_new), n)


# ------------------------------------------------------------------------------------------------ comparator
def compare_ema(ema_got, ema_want64, ema_before, cls=None, mask=None):
    """{class: worst error} of the average, in the unit of the module docstring; a NaN or an infinity counts as an infinite error."""
    eg, ew, e0 = (x.detach().double().reshape(-1) for x in (ema_got, ema_want64, ema_before))
    upd_w, upd_g = ew - e0, eg - e0
    unit = torch.maximum(A.ulp32(upd_w), 0.5 * A.ulp32(torch.maximum(e0.abs(), ew.abs())))
    e = torch.nan_to_num((upd_g - upd_w).abs() / unit, nan=float('inf'), posinf=float('inf'))
    if mask is not None:
        e = torch.where(mask, e, torch.zeros_like(e))
    return dict(zip(A.CLASSES, A._per_class(e, cls).tolist()))


def bars_for(wd_on):
    """the bars of m', v', the update and the average for a step with (without) decay"""
    return {'m': A.BARS['m'], 'v': A.BARS['v'], 'upd': BARS['upd_wd'] if wd_on else A.BARS['upd'], 'ema': BARS['ema']}


def check(got, before, g, hp, t, *, grad_scale=1.0, wd=0.0, decayed=None, decay=None, warmup=False, n=0, lo=0, cls=None, mask=None,
          real=False):
    """One APPLIED step: got = (p', m', v', ema' or None) against float64 from before = (p, m, v, ema or None) and the gradients g.  The
    average is compared on got's own p'.  Returns (report, [(quantity, class, error, bar)] beyond the bars); real: real gradients (adam_ref's
    cancellation floor, every class at the 'ordinary' bar)."""
    want = step_f64(before[0], g, before[1], before[2], t=t, grad_scale=grad_scale, wd=wd, decayed=decayed, lo=lo, **hp)
    rep = A.compare(got[:3], want, before[:3], cls, mask, cancel_floor=real)
    bars = bars_for(wd > 0)
    only = 'ordinary' if real else None
    bad = A.excess(rep, bars=bars, only=only)
    if decay is not None:
        rep['ema'] = compare_ema(got[3], ema_f64(before[3], got[0], decay, warmup, n), before[3], cls, mask)
        bad += [('ema', c, e, bars['ema'][only or c]) for c, e in rep['ema'].items() if not e <= bars['ema'][only or c]]
    return rep, bad


def check_skipped(got, before, n_got, n_before):
    """A SKIPPED step: every arena keeps its bits and the EMA counter its value.  Returns the list of what moved."""
    names = ('p', 'm', 'v', 'ema')
    bad = [names[i] for i, (a, b) in enumerate(zip(got, before)) if a is not None and not A.bits_equal(a, b)]
    return bad + (['n'] if int(n_got) != int(n_before) else [])


def merge(into, rep):
    A.merge(into, rep)
    if 'ema' in rep:
        row = into.setdefault('ema', dict.fromkeys(A.CLASSES, 0.0))
        for c, e in rep['ema'].items():
            row[c] = max(row[c], e)
    return into


def table(rep):
    return '\n'.join(f'    {q:4s}' + ''.join(f' {c} {rep[q][c]:.3g}' for c in A.CLASSES) for q in ('m', 'v', 'upd', 'ema') if q in rep)


# ------------------------------------------------------------------------------------------------ controlled inputs
def make_ema(p, device='cpu'):
    """The average a case starts from, by flat index mod 3 (coprime to the 7 gradient classes and to the kernels' float4): 0 the parameter
    itself (caught up: P' - ema is the step's own update), 1 the parameter off by up to 10^-3 of itself, 2 a value of its own."""
    n = p.numel()
    k = torch.arange(n, dtype=torch.int64, device=device) % 3
    p64 = p.detach().double().reshape(-1)
    near = p64 * (1.0 + 1e-3 * (A._u(n, 9, device) - 0.5))
    own = torch.where(A._u(n, 10, device) < 0.5, -1.0, 1.0) * 10.0 ** (-3.0 + 3.0 * A._u(n, 11, device))
    return torch.where(k == 0, p64, torch.where(k == 1, near, own)).float()


def decayed_mask(table_, n, which, device='cpu'):
    """bool [n]: the elements ss_set_weight_decay(which) decays among the PARAMETER elements of an engine's table [(name, offset, shape)]:
    'all' every parameter, 'weights' the tensors with ndim >= 2."""
    mask = torch.zeros(n, dtype=torch.bool, device=device)
    for _, off, shape in table_:
        if which == 'all' or len(shape) >= 2:
            mask[off:off + int(np.prod(shape))] = True
    return mask


# ------------------------------------------------------------------------------------------------ the yardstick
def measure_yardstick(n, steps=3, report=None):
    """Stock fp32 torch against this float64 over the grid of the module docstring at n elements: {'upd_wd': {class: worst}, 'ema': ..}."""
    cls = A.classes(n)
    out = {'upd_wd': dict.fromkeys(A.CLASSES, 0.0), 'ema': dict.fromkeys(A.CLASSES, 0.0)}
    for name, hp, restored, gs in A.CASES:
        for wd in WDS:
            p = A.make_params(n)
            m, v = A.make_moments(n, restored, hp['eps'], gs)
            ema = make_ema(p)
            for k in range(1, steps + 1):
                g = A.make_grad(n, k, hp['eps'])
                t = restored + k
                got = adamw_f32_torch(p, g, m, v, t=t, grad_scale=gs, wd=wd, **hp)
                want = step_f64(p, g, m, v, t=t, grad_scale=gs, wd=wd, **hp)
                rep = A.compare(got, want, (p, m, v), cls)
                for c, e in rep['upd'].items():
                    out['upd_wd'][c] = max(out['upd_wd'][c], e)
                for decay in DECAYS:
                    for nn in NS:
                        for warm in (False, True):
                            if not warm and nn != NS[0]:
                                continue                       # without warm-up n does not enter
                            eg = ema_f32_torch(ema, got[0], decay, warm, nn)
                            r = compare_ema(eg, ema_f64(ema, got[0], decay, warm, nn), ema, cls)
                            for c, e in r.items():
                                out['ema'][c] = max(out['ema'][c], e)
                ema = ema_f32_torch(ema, got[0], DECAYS[k % len(DECAYS)], False, 0)
                p, m, v = got
            if report:
                report(name, wd, out)
    return out


if __name__ == '__main__':
    import sys
    res = measure_yardstick(int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 21, report=lambda *a: print(a[0], a[1], flush=True))
    for q, row in res.items():
        print(q, {c: float(f'{e:.5g}') for c, e in row.items()})
