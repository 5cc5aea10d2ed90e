"""Self-test of tests/adam_ref.py on the CPU: deliberately wrong fp32 optimisers written in plain torch must each be reported by
compare() under the bars the GPU tests use (adam_ref.BARS), on the same controlled inputs at a small size, and stock torch.optim.Adam --
as well as a correct fp32 step in the engine's operation order -- must not be.  This is the proof that test_gpu_optimizer.py can fail,
and that its margins are tight enough; no HIP kernel is ever built wrong for it."""
import math

import pytest
import torch

from tests import adam_ref as A

N = 7 * 4 * 250                      # every class 1000 times, every class in every float4 lane
SEAM = N // 2                        # a multiple of 28: element SEAM is 'ordinary', element SEAM - 1 'fading'
CLS = A.classes(N)


def f32_step(p, g, m, v, *, lr, beta1, beta2, eps, t, grad_scale=1.0, bug=None, restored=0):
    """An fp32 Adam step in the engine's operation order (adam_kernel of csrc/elementwise.hip) -- correct for bug=None, else wrong in one way."""
    f = torch.float32
    t32 = lambda x: torch.tensor(x, dtype=f)
    if bug == 'beta2_fixed':
        beta2 = 0.999
    if bug == 'beta1_fixed':
        beta1 = 0.9
    if bug == 'step_not_advanced':
        t = t - 1
    if bug == 'restored_step_ignored':
        t = t - restored
    gm = g * t32(grad_scale)
    gv = g if bug in ('scale_on_m_only', 'v_before_scaling') else gm
    m1 = m + t32(1.0 - beta1) * (gm - m)
    v1 = v * t32(beta2) + t32(1.0 - beta2) * gv * gv
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    bc2s, e32 = t32(math.sqrt(bc2)), t32(eps)
    if bug == 'eps_before_division':
        denom = (v1.sqrt() + e32) / bc2s
    elif bug == 'bc2_omitted':
        denom = v1.sqrt() + e32
    else:
        denom = v1.sqrt() / bc2s + e32
    p1 = p - t32(lr / bc1) * (m1 / denom)
    if bug in ('seam_twice', 'seam_never'):
        i = SEAM if bug == 'seam_twice' else SEAM - 1
        if bug == 'seam_twice':        # the element just above the seam is in both ranges: the same step state applied to its own result
            p2, m2, v2 = f32_step(p1, g, m1, v1, lr=lr, beta1=beta1, beta2=beta2, eps=eps, t=t, grad_scale=grad_scale)
        else:                          # the element just below it is in neither
            p2, m2, v2 = p, m, v
        p1, m1, v1 = p1.clone(), m1.clone(), v1.clone()
        p1[i], m1[i], v1[i] = p2[i], m2[i], v2[i]
    return p1, m1, v1


def run(case, stepper, steps=3):
    """`steps` steps of a case of the grid; every step is compared from the state stock torch.optim.Adam left (as the GPU test compares every
    step from the engine's own state).  Returns the running worst and the list of everything beyond the bars."""
    _, hp, restored, gs = case
    p = A.make_params(N)
    m, v = A.make_moments(N, restored, hp['eps'], gs)
    worst, bad = {}, []
    for k in range(1, steps + 1):
        g = A.make_grad(N, k, hp['eps'])
        kw = dict(hp, t=restored + k, grad_scale=gs)
        want = A.adam_f64(p, g, m, v, **kw)
        got = stepper(p, g, m, v, **kw)
        rep = A.compare(got, want, (p, m, v), CLS)
        A.merge(worst, rep)
        bad += [(k,) + x for x in A.excess(rep)]
        if stepper is not A.adam_f32_torch:
            zero = CLS == 1
            if not all(A.bits_equal(a, b, zero) for a, b in zip(got, (p, m, v))):
                bad.append((k, 'bits', 'zero', float('nan'), 0.0))
        p, m, v = A.adam_f32_torch(p, g, m, v, **kw)
    return worst, bad


CASE = {c[0]: c for c in A.CASES}


def test_bars_are_four_times_a_measured_yardstick():
    for q in ('m', 'v', 'upd'):
        assert set(A.BARS[q]) == set(A.CLASSES)
        for c in A.CLASSES:
            if (q, c) == ('v', 'tiny'):
                assert A.BARS[q][c] == 1.0           # one smallest normal: flushed and kept subnormals both pass, nothing larger does
                continue
            assert A.BARS[q][c] == 4.0 * A.YARDSTICK[q][c], (q, c)
            assert A.BARS[q][c] <= 64.0, (q, c)      # "a few ulps"
    assert all(A.BARS[q]['zero'] == 0.0 for q in ('m', 'v', 'upd'))      # the always-zero class: bit-identical or reported


@pytest.mark.parametrize('case', A.CASES, ids=[c[0] for c in A.CASES])
def test_stock_fp32_adam_is_accepted_and_within_the_recorded_yardstick(case):
    worst, bad = run(case, A.adam_f32_torch, steps=9)
    assert not bad, bad
    for q in ('m', 'v', 'upd'):                      # these N elements are the first N of the arena-sized measurement
        for c in A.CLASSES:
            assert worst[q][c] <= A.YARDSTICK[q][c], (q, c, worst[q][c])


@pytest.mark.parametrize('case', A.CASES, ids=[c[0] for c in A.CASES])
def test_correct_fp32_step_in_the_engines_operation_order_is_accepted(case):
    _, hp, restored, _ = case
    worst, bad = run(case, lambda *a, **k: f32_step(*a, **k, restored=restored), steps=9)
    print(A.table(worst))
    assert not bad, bad


STAND_INS = [
    ('eps_before_division', 'default_t0_gs1'),        # 1  eps added before the division by sqrt(bc2)
    ('bc2_omitted', 'default_t7_gs1'),                # 2
    ('beta2_fixed', 'mid_t7_gs2m10'),                 # 3  0.999 where 0.98 was asked for
    ('beta1_fixed', 'fast_t0_gs05'),                  # 4  0.9 where 0.5 was asked for
    ('step_not_advanced', 'default_t7_gs1'),          # 5  the corrections of t - 1
    ('restored_step_ignored', 'default_t999_gs05'),   # 6  the counter starts from 0
    ('scale_on_m_only', 'fast_t0_gs05'),              # 7  grad_scale applied to m but not to v
    ('v_before_scaling', 'mid_t7_gs2m10'),            # 8  v updated with g before scaling
    ('seam_twice', 'default_t7_gs1'),                 # 9  one element at a range seam updated twice
    ('seam_never', 'default_t7_gs1'),                 # 10 one element at a range seam never updated
]


@pytest.mark.parametrize('bug,case', STAND_INS, ids=[b for b, _ in STAND_INS])
def test_wrong_stand_in_is_reported(bug, case):
    _, hp, restored, _ = CASE[case]
    worst, bad = run(CASE[case], lambda *a, **k: f32_step(*a, **k, bug=bug, restored=restored))
    assert bad, (bug, worst)
    assert worst['worst'][2] > 2.0 * max(A.BARS[worst['worst'][0]].values()), (bug, worst['worst'])     # and not by a hair
    if bug.startswith('seam'):
        assert worst['worst'][1] == (SEAM if bug == 'seam_twice' else SEAM - 1), worst['worst']          # reported where it is


@pytest.mark.parametrize('bug,case', [('step_not_advanced', 'fast_t1e6_gs1'), ('restored_step_ignored', 'mid_t1e6_gs2m10')])
def test_a_wrong_counter_at_a_million_steps_is_reported_once_it_matters(bug, case):
    """At t = 10^6 both corrections are exactly 1, so the corrections of t - 1 are the right ones and must pass; a counter that restarts at 0
    gives 1 - beta^k and must not."""
    _, hp, restored, _ = CASE[case]
    worst, bad = run(CASE[case], lambda *a, **k: f32_step(*a, **k, bug=bug, restored=restored))
    assert bool(bad) == (bug == 'restored_step_ignored'), (bug, bad[:3])


def test_compare_counts_nan_and_inf_and_honours_the_mask():
    _, hp, restored, gs = CASE['default_t7_gs1']
    p, g = A.make_params(N), A.make_grad(N, 1, hp['eps'])
    m, v = A.make_moments(N, restored, hp['eps'], gs)
    kw = dict(hp, t=restored + 1, grad_scale=gs)
    want = A.adam_f64(p, g, m, v, **kw)
    for val in (float('nan'), float('inf')):
        got = [x.clone() for x in A.adam_f32_torch(p, g, m, v, **kw)]
        got[0][14] = val
        rep = A.compare(got, want, (p, m, v), CLS)
        assert rep['worst'][:2] == ('upd', 14) and rep['worst'][2] == float('inf') and A.excess(rep)
        mask = torch.ones(N, dtype=torch.bool)
        mask[14] = False                                 # an alignment gap: not compared
        assert not A.excess(A.compare(got, want, (p, m, v), CLS, mask))


def test_cancel_floor_only_ever_loosens_where_m_cancels():
    """Real gradients: beta1 m + (1 - beta1) g may cancel; the unit of m' is then an ulp of m.  Without cancellation the two metrics agree."""
    _, hp, restored, gs = CASE['default_t7_gs1']
    p, g = A.make_params(N), A.make_grad(N, 1, hp['eps'])
    m, v = A.make_moments(N, restored, hp['eps'], gs)
    kw = dict(hp, t=restored + 1, grad_scale=gs)
    want, got = A.adam_f64(p, g, m, v, **kw), A.adam_f32_torch(p, g, m, v, **kw)
    a, b = A.compare(got, want, (p, m, v), CLS), A.compare(got, want, (p, m, v), CLS, cancel_floor=True)
    for c in ('ordinary', 'near_eps', 'large', 'tiny'):             # same sign of m and g: |m'| >= |beta1 m|, at most one binade below |m|
        assert 0.5 * a['m'][c] <= b['m'][c] <= a['m'][c]
    g2 = (-(hp['beta1'] / (1 - hp['beta1'])) * m.double() * (1 + 1e-6)).float()      # cancels to ~1e-6 of its terms
    want, got = A.adam_f64(p, g2, m, v, **kw), A.adam_f32_torch(p, g2, m, v, **kw)
    nz = CLS != 1
    a, b = A.compare(got, want, (p, m, v), None, nz), A.compare(got, want, (p, m, v), None, nz, cancel_floor=True)
    assert a['m']['ordinary'] > 1e3 and A.excess(a, only='ordinary')               # ulps of the result: no fp32 Adam passes
    assert not A.excess(b, only='ordinary'), b
