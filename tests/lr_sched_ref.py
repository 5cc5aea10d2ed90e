"""The learning-rate schedule of ss_set_lr_schedule restated in float64, the torch.optim.lr_scheduler objects it corresponds to, and the
comparators of its tests (test_gpu_lr_sched.py; proven on wrong variants by test_lr_sched_ref_selftest.py).  Importing it needs no GPU.

The definition (include/speechsplit_amd.h), for the optimiser step t being APPLIED (1-based, the t of the bias corrections), s = t - 1,
base the rate of ss_set_adam:

    warm-up, W > 0 and s < W:   lr_t = base * (sf + (1 - sf) * (s / W))
    otherwise, k = s - W:       constant     base
                                cosine       kk = min(k, N); min_lr + (base - min_lr) * (0.5 * (1 + cospi(kk / N)))
                                linear       kk = min(k, N); base + (min_lr - base) * (kk / N)
                                exponential  max(base * gamma^k, min_lr)
                                step         max(base * gamma^(k // P), min_lr)

every product and sum a float64 operation of its own, in this order.  The consumers: step_size = float32(lr_t / bc1) and the decay factor
float32(1 - lr_t * wd); an AdamW step under the schedule is optim_ext_ref's step with lr replaced by lr_t (hp_at).

In torch: SequentialLR(opt, [LinearLR(opt, sf, 1.0, W), main], [W]), or main alone when W = 0, main = CosineAnnealingLR(T_max=N,
eta_min=min_lr), LinearLR(1.0, min_lr / base, N), ExponentialLR(gamma) or StepLR(P, gamma), the rate read before each optimizer.step()
(torch_lrs).  Two deliberate differences: past N cosine STAYS at min_lr (torch's turns back up), and min_lr floors the geometric kinds.

TORCH_WORST is what max |lr_at - torch| / base showed per kind over W + N + 2 steps, W in {0, 1, 5}, N = 12, P in {1, 4}, min_lr = 0 for
the geometric kinds (measure_torch(), torch 2.10 on the CPU: 1.81e-16 for every kind, one ulp of the rate in torch's chained warm-up),
rounded UP to two digits.  LR_BAR, the bar of a device evaluation against lr_at relative to max(base, min_lr), is 100 x that figure and at least
100 x 2^-52: one factor of ten for a third rounding of the same operations, one for the device's pow and cospi.  Nothing here comes from the
engine.
"""
import math
import warnings

import numpy as np

KINDS = ('constant', 'cosine', 'linear', 'exponential', 'step')
KIND_ID = {'off': 0, 'constant': 1, 'cosine': 2, 'linear': 3, 'exponential': 4, 'step': 5}
TORCH_BAR = 1e-12                        # lr_at against the torch objects, relative to base
# measure_torch(): worst |lr_at - torch| / base per kind
TORCH_WORST = {'constant': 1.9e-16, 'cosine': 1.9e-16, 'linear': 1.9e-16, 'exponential': 1.9e-16, 'step': 1.9e-16}
EPS64 = 2.0 ** -52
LR_BAR = {k: max(100.0 * w, 100.0 * EPS64) for k, w in TORCH_WORST.items()}


def sched(kind, W=0, sf=0.1, N=None, gamma=None, P=None, min_lr=0.0):
    return dict(kind=kind, W=W, sf=sf, N=N, gamma=gamma, P=P, min_lr=min_lr)


def cospi(x):
    """cos(pi x) for 0 <= x <= 1, exact at 0, 1/2 and 1 as the device's is"""
    return 0.0 if x == 0.5 else math.cos(math.pi * x)


def lr_at(t, base, kind, W=0, sf=0.1, N=None, gamma=None, P=None, min_lr=0.0, variant=None):
    """lr_t of the applied step t.  variant: the one thing a wrong implementation gets wrong (the self-test's stand-ins)."""
    s = t if variant == 's_is_t' else t - 1
    if kind == 'off':
        return base
    if W > 0 and s < W:
        return base * (sf + (1.0 - sf) * (float(s) / float(W - 1 if variant == 'warmup_ends_early' and W > 1 else W)))
    k = s if variant == 'warmup_not_subtracted' else s - W
    lo = 0.0 if variant == 'min_lr_ignored' else min_lr
    if kind == 'cosine':
        kk = min(k, N)
        half = 1.0 if variant == 'cosine_without_half' else 0.5
        return lo + (base - lo) * (half * (1.0 + cospi(float(kk) / float(N))))
    if kind == 'linear':
        kk = min(k, N)
        return base + (lo - base) * (float(kk) / float(N))
    if kind == 'exponential':
        return max(base * math.pow(gamma, float(k + 1 if variant == 'gamma_k_plus_1' else k)), lo)
    if kind == 'step':
        q = -((-k) // P) if variant == 'step_ceil' else k // P
        return max(base * math.pow(gamma, float(q)), lo)
    assert kind == 'constant', kind
    return base


def hp_at(hp, t, sc):
    """the Adam hyper-parameters of the applied step t under the schedule sc: lr replaced by lr_t (adam_ref / optim_ext_ref take them)"""
    return dict(hp, lr=lr_at(t, hp['lr'], **sc))


def step_size64(hp, t, sc):
    """lr_t / bc1 in float64: what the prepare kernels round ONCE, to float32"""
    return lr_at(t, hp['lr'], **sc) / (1.0 - hp['beta1'] ** t)


def step_size32(hp, t, sc):
    return np.float32(step_size64(hp, t, sc))


def decay_mul32(hp, t, sc, wd):
    """the weight-decay factor of the applied step t: float32(1 - lr_t * wd), wd the fp32 number the C ABI receives"""
    return np.float32(1.0 - lr_at(t, hp['lr'], **sc) * float(np.float32(wd)))


def lr_error(got, want, base, min_lr=0.0):
    """|got - want| relative to max(base, min_lr); a NaN counts as an infinite error"""
    e = abs(float(got) - float(want)) / max(base, min_lr)
    return e if e == e else float('inf')


# ------------------------------------------------------------------------------------------------ torch
def torch_lrs(steps, base, kind, W=0, sf=0.1, N=None, gamma=None, P=None, min_lr=0.0, optimizer=None):
    """[rate torch reads before optimizer.step() number t, t = 1 .. steps] under the scheduler objects of the module docstring.  optimizer:
    drive this one (its lr is base; its step() is called here, so its gradients must be set); None: a throw-away SGD."""
    opt, sch = torch_scheduler(base, kind, W, sf, N, gamma, P, min_lr, optimizer)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for _ in range(steps):
            out.append(float(opt.param_groups[0]['lr']))
            opt.step()
            sch.step()
    return out


def torch_scheduler(base, kind, W=0, sf=0.1, N=None, gamma=None, P=None, min_lr=0.0, optimizer=None):
    import torch
    from torch.optim import lr_scheduler as L
    opt = optimizer
    if opt is None:
        par = torch.nn.Parameter(torch.zeros(1))
        par.grad = torch.zeros(1)
        opt = torch.optim.SGD([par], lr=base)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if kind == 'cosine':
            main = L.CosineAnnealingLR(opt, T_max=N, eta_min=min_lr)
        elif kind == 'linear':
            main = L.LinearLR(opt, start_factor=1.0, end_factor=min_lr / base, total_iters=N)
        elif kind == 'exponential':
            main = L.ExponentialLR(opt, gamma=gamma)
        elif kind == 'step':
            main = L.StepLR(opt, step_size=P, gamma=gamma)
        else:
            main = L.ConstantLR(opt, factor=1.0, total_iters=0)
        if W > 0:
            main = L.SequentialLR(opt, [L.LinearLR(opt, start_factor=sf, end_factor=1.0, total_iters=W), main], milestones=[W])
    return opt, main


BASE, N_REF, GAMMA = 3e-4, 12, 0.8


def grid(min_lr_geometric=0.0, min_lr_annealed=3e-6):
    """(schedule, steps up to which torch and the definition agree) over every kind, W in {0, 1, 5} and P in {1, 4}.  Cosine agrees up to
    k = N (W + N + 1 steps), everything else for as long as one likes (W + N + 2 here)."""
    out = []
    for W in (0, 1, 5):
        out.append((sched('constant', W=W), W + N_REF + 2))
        out.append((sched('cosine', W=W, N=N_REF, min_lr=min_lr_annealed), W + N_REF + 1))
        out.append((sched('linear', W=W, N=N_REF, min_lr=min_lr_annealed), W + N_REF + 2))
        out.append((sched('exponential', W=W, gamma=GAMMA, min_lr=min_lr_geometric), W + N_REF + 2))
        for P in (1, 4):
            out.append((sched('step', W=W, gamma=GAMMA, P=P, min_lr=min_lr_geometric), W + N_REF + 2))
    return out


def measure_torch(base=BASE):
    """{kind: worst |lr_at - torch| / base} over grid()"""
    worst = dict.fromkeys(KINDS, 0.0)
    for sc, steps in grid():
        got = torch_lrs(steps, base, **sc)
        for t, lr in enumerate(got, 1):
            worst[sc['kind']] = max(worst[sc['kind']], lr_error(lr_at(t, base, **sc), lr, base))
    return worst


if __name__ == '__main__':
    print({k: float(f'{e:.3g}') for k, e in measure_torch().items()})
