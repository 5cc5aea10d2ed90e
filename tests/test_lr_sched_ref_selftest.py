"""CPU self-test of tests/lr_sched_ref.py: the float64 restatement agrees with the torch.optim.lr_scheduler objects it names within 1e-12
of the base rate (worst measured: 1.81e-16, every kind -- one ulp of the rate in torch's chained warm-up), the two stated differences are
differences, an AdamW step with the rate replaced by lr_t matches stock torch.optim.AdamW driven by the scheduler within optim_ext_ref's
bars, and each of ten wrong variants is reported at 100 times the bar or more in the quantity it bears on."""
import math

import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import lr_sched_ref as L
from tests import optim_ext_ref as R

N = 7 * 3 * 4 * 50                       # every gradient class x every EMA start x every float4 lane


def test_written_figures_hold():
    worst = L.measure_torch()
    for k, e in worst.items():
        assert e <= L.TORCH_WORST[k] <= L.TORCH_BAR, (k, e)
        assert L.LR_BAR[k] == max(100.0 * L.TORCH_WORST[k], 100.0 * 2.0 ** -52)


@pytest.mark.parametrize('sc,agree', L.grid(), ids=lambda x: '{kind}_W{W}_P{P}'.format(**x) if isinstance(x, dict) else str(x))
def test_agrees_with_torch(sc, agree):
    """W + N + 2 steps of every kind; for cosine the last of them (k = N + 1) is the first stated difference and is asserted as one"""
    steps = sc['W'] + L.N_REF + 2
    got = L.torch_lrs(steps, L.BASE, **sc)
    for t, lr in enumerate(got, 1):
        mine = L.lr_at(t, L.BASE, **sc)
        if t <= agree:
            assert L.lr_error(mine, lr, L.BASE) <= L.TORCH_BAR, (sc, t, mine, lr)
        else:
            assert sc['kind'] == 'cosine' and mine == sc['min_lr'] and lr > sc['min_lr'] * (1.0 + 1e-3), (sc, t, mine, lr)


@pytest.mark.parametrize('W', (0, 1, 5))
def test_past_N_cosine_and_linear_stay_at_min_lr(W):
    for kind in ('cosine', 'linear'):
        sc = L.sched(kind, W=W, N=L.N_REF, min_lr=3e-6)
        far = L.torch_lrs(W + 2 * L.N_REF + 1, L.BASE, **sc)
        for t in (W + L.N_REF + 1, W + L.N_REF + 2, W + 2 * L.N_REF + 1, 2 ** 31 + 7):
            mine = L.lr_at(t, L.BASE, **sc)      # cosine to the bit at kk = N and ever after; linear is base + (min_lr - base): one rounding
            assert mine == 3e-6 if kind == 'cosine' else (mine == L.lr_at(W + L.N_REF + 1, L.BASE, **sc) and abs(mine - 3e-6) <= 1e-12 * L.BASE)
        # torch's linear stays as well; torch's cosine has turned all the way back up after another N steps
        assert (abs(far[-1] - L.BASE) <= 1e-12 * L.BASE) if kind == 'cosine' else (abs(far[-1] - 3e-6) <= 1e-12 * L.BASE), (kind, far[-1])


@pytest.mark.parametrize('kind,P', [('exponential', None), ('step', 1), ('step', 4)])
def test_min_lr_floors_the_geometric_kinds(kind, P):
    floor = L.BASE * L.GAMMA ** 2.5                  # between two values of the sequence
    sc = L.sched(kind, W=0, gamma=L.GAMMA, P=P, min_lr=floor)      # (the warm-up is not floored: it is not part of the geometric sequence)
    steps = 6 * (P or 1)
    theirs = L.torch_lrs(steps, L.BASE, **dict(sc, min_lr=0.0))
    mine = [L.lr_at(t, L.BASE, **sc) for t in range(1, steps + 1)]
    below = [t for t, lr in enumerate(theirs, 1) if lr < floor]
    assert below and len(below) < steps
    for t, (a, b) in enumerate(zip(mine, theirs), 1):
        if t in below:
            assert a == floor and b < floor * (1.0 - 1e-3), (t, a, b)
        else:
            assert L.lr_error(a, b, L.BASE) <= L.TORCH_BAR, (t, a, b)
    assert [L.lr_at(t, L.BASE, **dict(sc, min_lr=0.0)) for t in range(1, steps + 1)] == pytest.approx(theirs, rel=1e-12, abs=0.0)


# ------------------------------------------------------------------------------------------------ the AdamW step under the schedule
def torch_adamw_run(hp, sc, wd, steps):
    """stock fp32 torch.optim.AdamW(foreach=False, fused=False) driven by the scheduler objects: [(before, g, got)] per step"""
    p0 = A.make_params(N)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([par], lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'], weight_decay=R.f32(wd), amsgrad=False,
                            foreach=False, fused=False)
    _, sch = L.torch_scheduler(hp['lr'], optimizer=opt, **sc)
    out = []
    m = v = torch.zeros(N)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for t in range(1, steps + 1):
            g = A.make_grad(N, t, hp['eps'])
            before = (par.detach().clone(), m.clone(), v.clone())
            par.grad = g.clone()
            opt.step()
            sch.step()
            st = opt.state[par]
            m, v = st['exp_avg'].clone(), st['exp_avg_sq'].clone()
            out.append((before, g, (par.detach().clone(), m, v)))
    return out


@pytest.mark.parametrize('kind', L.KINDS)
@pytest.mark.parametrize('wd', (0.0, 0.1))
def test_adamw_under_the_schedule_matches_stock_torch(kind, wd):
    hp = A.HP_FAST
    sc = L.sched(kind, W=2, N=3, gamma=L.GAMMA, P=2, min_lr=0.0 if kind in ('exponential', 'step') else 1e-5)
    steps = 2 + 3 + 1                                # through k = N: torch's cosine agrees that far
    cls = A.classes(N)
    for t, (before, g, got) in enumerate(torch_adamw_run(hp, sc, wd, steps), 1):
        rep, bad = R.check(got + (None,), before + (None,), g, L.hp_at(hp, t, sc), t, wd=wd, cls=cls)
        assert not bad, (kind, wd, t, bad)


# ------------------------------------------------------------------------------------------------ wrong variants
SC = {
    's_is_t': L.sched('cosine', W=5, N=L.N_REF, min_lr=3e-6),
    'warmup_not_subtracted': L.sched('cosine', W=5, N=L.N_REF, min_lr=3e-6),
    'warmup_ends_early': L.sched('linear', W=5, N=L.N_REF, min_lr=3e-6),
    'cosine_without_half': L.sched('cosine', W=1, N=L.N_REF, min_lr=3e-6),
    'gamma_k_plus_1': L.sched('exponential', W=1, gamma=L.GAMMA),
    'step_ceil': L.sched('step', W=0, gamma=L.GAMMA, P=4),
    'min_lr_ignored': L.sched('exponential', W=0, gamma=L.GAMMA, min_lr=L.BASE * L.GAMMA ** 2.5),
}


@pytest.mark.parametrize('variant', sorted(SC))
def test_wrong_schedule_is_reported(variant):
    """the quantity: lr_t, relative to max(base, min_lr); the bar: LR_BAR (the GPU test's)"""
    sc = SC[variant]
    ts = range(1, sc['W'] + L.N_REF + 3)
    worst = max(L.lr_error(L.lr_at(t, L.BASE, variant=variant, **sc), L.lr_at(t, L.BASE, **sc), L.BASE, sc['min_lr']) for t in ts)
    assert worst >= 100.0 * L.LR_BAR[sc['kind']], (variant, worst)
    assert max(L.lr_error(L.lr_at(t, L.BASE, **sc), L.lr_at(t, L.BASE, **sc), L.BASE) for t in ts) == 0.0


def standin(before, g, hp, t, sc, *, wd=0.0, variant=None, lr_t=None):
    """One fp32 AdamW step in the kernel's operation order under the schedule: (p', m', v').  variant: what it gets wrong."""
    p, m, v = (x.clone() for x in before)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    lr_t = L.lr_at(t, hp['lr'], **sc) if lr_t is None else lr_t
    bc1, bc2 = 1.0 - hp['beta1'] ** t, 1.0 - hp['beta2'] ** t
    mul = f32(1.0 - (hp['lr'] if variant == 'decay_from_base' else lr_t) * R.f32(wd))
    m1 = m + f32(1.0 - hp['beta1']) * (g - m)
    v1 = v * f32(hp['beta2']) + f32(1.0 - hp['beta2']) * g * g
    denom = v1.sqrt() / f32(math.sqrt(bc2)) + f32(hp['eps'])
    p1 = p * mul if wd else p
    return p1 - f32(lr_t / bc1) * (m1 / denom), m1, v1


def worst_over_bar(bad):
    return max((e / b for _, _, e, b in bad), default=0.0)


def test_decay_factor_from_the_base_rate_is_reported():
    """the quantity: the update of a decayed parameter, optim_ext_ref's unit and bar"""
    hp, sc, wd, t = A.HP_FAST, L.sched('constant', W=5, sf=0.1), 0.5, 1          # first warm-up step: lr_t = base / 10
    before = (A.make_params(N), *A.make_moments(N, 0, hp['eps']))
    g = A.make_grad(N, 1, hp['eps'])
    check = lambda got: R.check(got + (None,), before + (None,), g, L.hp_at(hp, t, sc), t, wd=wd, cls=A.classes(N))[1]
    assert not check(standin(before, g, hp, t, sc, wd=wd))
    bad = check(standin(before, g, hp, t, sc, wd=wd, variant='decay_from_base'))
    assert bad and all(q == 'upd' for q, *_ in bad) and worst_over_bar(bad) >= 100.0, bad


def test_schedule_advancing_on_a_skipped_step_is_reported():
    """a skipped step, then an applied one: t did not move, so the applied step carries lr_t of the SAME t; one that advanced the schedule
    on the skip applies the rate of t + 1 under the bias corrections of t.  The quantity: the update, adam_ref's unit and bar."""
    hp, sc, t = A.HP_FAST, L.sched('cosine', W=2, sf=0.1, N=L.N_REF), 1
    before = (A.make_params(N), *A.make_moments(N, 0, hp['eps']))
    g = A.make_grad(N, 1, hp['eps'])
    check = lambda got: R.check(got + (None,), before + (None,), g, L.hp_at(hp, t, sc), t, cls=A.classes(N))[1]
    assert not check(standin(before, g, hp, t, sc))
    bad = check(standin(before, g, hp, t, sc, lr_t=L.lr_at(t + 1, hp['lr'], **sc)))
    assert bad and all(q == 'upd' for q, *_ in bad) and worst_over_bar(bad) >= 100.0, bad


def test_rate_applied_after_rounding_base_over_bc1_is_reported():
    """The quantity: the float64 step size lr_t / bc1 that is rounded ONCE to float32, relative to itself; the bar: LR_BAR.  A variant that
    rounds base / bc1 to float32 first and multiplies the schedule's factor in afterwards carries that rounding (up to 2^-24 = 6e-8) into
    the product; the float32 it ends up with differs from step_size32 in its bits as well."""
    hp, sc = A.HP_MID, L.sched('cosine', W=5, N=L.N_REF, min_lr=3e-6)
    worst, bits = 0.0, 0
    for t in range(1, sc['W'] + L.N_REF + 3):
        want = L.step_size64(hp, t, sc)
        factor = L.lr_at(t, hp['lr'], **sc) / hp['lr']
        wrong = float(np.float32(hp['lr'] / (1.0 - hp['beta1'] ** t))) * factor
        worst = max(worst, abs(wrong - want) / want)
        bits += int(np.float32(wrong).view(np.uint32) != L.step_size32(hp, t, sc).view(np.uint32))
    assert worst >= 100.0 * L.LR_BAR['cosine'], worst
    assert bits > 0
