"""CPU self-test of tests/optim_ext_ref.py: the yardstick re-measured at a small size stays under the written one, stock fp32 torch
(AdamW + get_ema_avg_fn) passes the bars, and each of eleven wrong optimisers -- fp32 stand-ins for what a kernel or a schedule could get
wrong -- is reported by the same check()/check_skipped() the GPU tests use."""
import math

import pytest
import torch

from tests import adam_ref as A
from tests import optim_ext_ref as R

N = 7 * 3 * 4 * 250                      # every gradient class x every EMA start x every float4 lane
LO = N // 3 // 4 * 4                     # the 'decoder range' of the stand-in arena starts here
# a stand-in parameter table: weights (ndim 2) and biases (ndim 1) alternating
TABLE = [(f't{i}', off, shape) for i, (off, shape) in enumerate([(0, (50, 40)), (2000, (500,)), (2500, (100, 80)), (10500, (10, 5, 5)), (10750, (10250,))])]


def start(case, wd_on=True):
    name, hp, restored, gs = case
    p = A.make_params(N)
    m, v = A.make_moments(N, restored, hp['eps'], gs)
    return hp, restored, gs, (p, m, v, R.make_ema(p))


def standin(before, g, hp, t, gs, *, wd=0.0, decayed=None, decay=None, warmup=False, n=0, lo=0, skipped=False, variant=None):
    """One step of an fp32 optimiser in the kernel's operation order: (p', m', v', ema', n').  variant: the one thing it gets wrong."""
    p, m, v, ema = (x.clone() for x in before)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    bc1, bc2 = 1.0 - hp['beta1'] ** t, 1.0 - hp['beta2'] ** t
    mul = f32(1.0 - (hp['lr'] / bc1 if variant == 'decay_lr_bc1' else hp['lr']) * R.f32(wd))
    dec = torch.ones(N, dtype=torch.bool) if (decayed is None or variant == 'bias_decayed') else decayed
    sel = torch.arange(N) >= lo
    if skipped:
        if variant == 'decay_on_skip':
            p = torch.where(dec & sel, p * mul, p)
        return p, m, v, ema, n + (1 if variant == 'n_on_skip' else 0)
    gg = g * f32(gs)
    if variant == 'l2':
        gg = gg + f32(R.f32(wd)) * torch.where(dec, p, torch.zeros_like(p))
    m1 = m + f32(1.0 - hp['beta1']) * (gg - m)
    v1 = v * f32(hp['beta2']) + f32(1.0 - hp['beta2']) * gg * gg
    denom = v1.sqrt() / f32(math.sqrt(bc2)) + f32(hp['eps'])
    upd = f32(hp['lr'] / bc1) * (m1 / denom)
    if variant in ('l2',) or wd == 0:
        p1 = p - upd
    elif variant == 'decay_after':
        p1 = torch.where(dec, (p - upd) * mul, p - upd)
    else:
        p1 = torch.where(dec, p * mul, p) - upd
    pn, mn, vn = torch.where(sel, p1, p), torch.where(sel, m1, m), torch.where(sel, v1, v)
    if decay is None:
        return pn, mn, vn, ema, n
    nn = n + 1 if variant == 'warmup_off_by_one' else n
    d = R.ema_d(decay, warmup, nn)
    w = f32(d if variant == 'ema_swapped' else 1.0 - d)
    src = p if variant == 'ema_from_old_p' else pn
    e1 = ema + w * (src - ema)
    if variant == 'ema_encoder_left':
        e1 = torch.where(sel, e1, ema)
    return pn, mn, vn, e1, n + 1


def report(got, before, g, hp, t, gs, **kw):
    return R.check(got[:4], before, g, hp, t, grad_scale=gs, cls=A.classes(N), **kw)[1]


def test_yardstick_at_a_small_size_stays_under_the_written_one():
    small = R.measure_yardstick(N, steps=2)
    for q, row in small.items():
        for c, e in row.items():
            assert e <= R.YARDSTICK[q][c], (q, c, e, R.YARDSTICK[q][c])
        assert max(row.values()) > 0.3 * max(R.YARDSTICK[q].values()), (q, row)      # and it measures something


@pytest.mark.parametrize('case', A.CASES, ids=[c[0] for c in A.CASES])
def test_stock_torch_and_the_right_standin_pass(case):
    hp, restored, gs, before = start(case)
    dmask = R.decayed_mask(TABLE, N, 'weights')
    for k, (wd, decay, warm, n) in enumerate([(1e-2, 0.999, False, 0), (0.1, 0.5, True, 7), (0.1, 0.9999, True, 10 ** 6), (0.0, 0.999, True, 0)], 1):
        g = A.make_grad(N, k, hp['eps'])
        t = restored + k
        pn, mn, vn = R.adamw_f32_torch(before[0], g, before[1], before[2], t=t, grad_scale=gs, wd=wd, **hp)
        got = (pn, mn, vn, R.ema_f32_torch(before[3], pn, decay, warm, n))
        assert not report(got, before, g, hp, t, gs, wd=wd, decay=decay, warmup=warm, n=n), (case[0], k)
        for decayed, lo in ((None, 0), (dmask, 0), (dmask, LO)):
            mine = standin(before, g, hp, t, gs, wd=wd, decayed=decayed, decay=decay, warmup=warm, n=n, lo=lo)
            assert mine[4] == n + 1
            assert not report(mine, before, g, hp, t, gs, wd=wd, decayed=decayed, decay=decay, warmup=warm, n=n, lo=lo), (case[0], k, lo)
            if lo:
                assert all(A.bits_equal(a[:lo], b[:lo]) for a, b in zip(mine[:3], before[:3])) and not A.bits_equal(mine[3][:lo], before[3][:lo])
        before = got


CASE = A.CASES[2]                        # mid, restored step 7: 1 - beta1^t is far from 1, so lr / bc1 is not lr
WRONG_APPLIED = {
    'l2': dict(wd=0.1), 'decay_after': dict(wd=0.1), 'decay_lr_bc1': dict(wd=0.1),
    'ema_from_old_p': dict(decay=0.5), 'ema_swapped': dict(decay=0.999), 'warmup_off_by_one': dict(decay=0.999, warmup=True, n=7),
}


@pytest.mark.parametrize('variant', sorted(WRONG_APPLIED))
def test_wrong_applied_step_is_reported(variant):
    hp, restored, gs, before = start(CASE)
    kw = WRONG_APPLIED[variant]
    g = A.make_grad(N, 1, hp['eps'])
    assert not report(standin(before, g, hp, restored + 1, gs, **kw), before, g, hp, restored + 1, gs, **kw)
    assert report(standin(before, g, hp, restored + 1, gs, variant=variant, **kw), before, g, hp, restored + 1, gs, **kw), variant


def test_biases_decayed_under_weights_only_is_reported():
    hp, restored, gs, before = start(CASE)
    g = A.make_grad(N, 1, hp['eps'])
    dmask = R.decayed_mask(TABLE, N, 'weights')
    assert dmask.any() and not dmask.all() and not dmask[2000:2500].any() and dmask[10500:10750].all()
    got = standin(before, g, hp, restored + 1, gs, wd=0.1, decayed=dmask, variant='bias_decayed')
    assert report(got, before, g, hp, restored + 1, gs, wd=0.1, decayed=dmask)


@pytest.mark.parametrize('variant,moved', [('decay_on_skip', ['p']), ('n_on_skip', ['n'])])
def test_wrong_skipped_step_is_reported(variant, moved):
    hp, restored, gs, before = start(CASE)
    g = A.make_grad(N, 1, hp['eps'])
    right = standin(before, g, hp, restored + 1, gs, wd=0.1, decay=0.999, n=5, skipped=True)
    assert R.check_skipped(right[:4], before, right[4], 5) == []
    got = standin(before, g, hp, restored + 1, gs, wd=0.1, decay=0.999, n=5, skipped=True, variant=variant)
    assert R.check_skipped(got[:4], before, got[4], 5) == moved


def test_ema_updated_on_every_micro_batch_is_reported():
    """a two-micro-batch cycle: the first micro-batch takes no optimiser step, so it may not average either -- one that does has moved the
    average twice (and counted twice) by the end of the cycle"""
    hp, restored, gs, before = start(CASE)
    g = A.make_grad(N, 1, hp['eps'])
    w = torch.tensor(1.0 - 0.5, dtype=torch.float32)
    early = (before[0], before[1], before[2], before[3] + w * (before[0] - before[3]))      # the wrong first micro-batch: an EMA pass
    got = standin(early, g, hp, restored + 1, gs, decay=0.5, n=1)
    assert got[4] == 2
    assert report(got, before, g, hp, restored + 1, gs, decay=0.5, n=0)
    right = standin(before, g, hp, restored + 1, gs, decay=0.5, n=0)
    assert right[4] == 1 and not report(right, before, g, hp, restored + 1, gs, decay=0.5, n=0)


def test_encoder_range_of_the_ema_left_alone_is_reported():
    hp, restored, gs, before = start(CASE)
    g = A.make_grad(N, 1, hp['eps'])
    got = standin(before, g, hp, restored + 1, gs, wd=0.1, decay=0.5, lo=LO, variant='ema_encoder_left')
    assert report(got, before, g, hp, restored + 1, gs, wd=0.1, decay=0.5, lo=LO)
