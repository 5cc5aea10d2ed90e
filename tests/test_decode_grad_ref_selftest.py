"""The float64 restatement of the differentiable decode (tests/decode_grad_ref.py) checked on the CPU: against the oracle's forward,
against central finite differences in float64, and on the mistakes a kernel or an engine could make -- each has to show at least
WRONG_FACTOR (100) bars on the kind of inputs tests/test_gpu_decode_grad.py uses, or that test could not tell it from the right answer."""
import pytest
import torch

from oracle import ref_model, weights as W
from tests import adam_ref, decode_grad_ref as R
from tests.test_capi_bottleneck_widths import hparams_of as widths_hparams

HP = W.default_hparams()
HP_MIX = widths_hparams('W_mix')               # factors (4, 16, 8), widths (12, 3, 24): the three factors differ
CASES = {'G3': ('G3', HP, 2, 16), 'G3_mix': ('G3', HP_MIX, 2, 32), 'G6': ('G6', HP, 2, 16)}
_CACHE = {}


def case(name):
    """the reference of a case, computed once"""
    if name not in _CACHE:
        kind, hp, B, T = CASES[name]
        P = R.p64(kind, hp)
        codes, emb, d_out = R.make_inputs(kind, hp, B, T, seed=5)
        _CACHE[name] = (kind, hp, P, codes, emb, d_out, R.decode_grad(kind, P, hp, codes, emb, d_out))
    return _CACHE[name]


@pytest.mark.parametrize('name', list(CASES))
def test_out_is_the_oracles_forward_of_the_upsampled_codes(name):
    kind, hp, P, codes, emb, _, ref = case(name)
    with torch.no_grad():
        enc = R.dec_input(kind, hp, [c.double() for c in codes], emb.double() if emb is not None else None)
        want = ref_model.decoder(enc, P, 3 if kind == 'G3' else 2)
    assert R.rel(ref['out'], want) < 1e-12
    assert enc.shape[-1] == sum(w for _, _, w in R.factors(kind, hp)) + (hp.dim_spk_emb if kind == 'G3' else 0)


@pytest.mark.parametrize('name', list(CASES))
def test_gradients_match_central_differences(name):
    """<grad, u> against (L(x + h u) - L(x - h u)) / 2h in float64, one random direction u per tensor: every code, the speaker rows, every
    decoder / head parameter.  h = 1e-5 at unit-scale tensors: truncation ~ h^2, cancellation ~ 1e-16 / h -- both far below 1e-6."""
    kind, hp, P, codes, emb, d_out, ref = case(name)
    layers = 3 if kind == 'G3' else 2
    g = torch.Generator().manual_seed(17)
    d64 = d_out.double()
    Pd = R.dec_params(P, grad=False)

    def loss(cs, e, prm):
        with torch.no_grad():
            return float((ref_model.decoder(R.dec_input(kind, hp, cs, e), prm, layers) * d64).sum())
    cs0 = [c.double() for c in codes]
    e0 = emb.double() if emb is not None else None
    h = 1e-5
    worst = 0.0

    def check(tag, grad, lo, hi):
        nonlocal worst
        u = getattr(check, 'u')
        fd = (hi - lo) / (2 * h)
        an = float((grad * u).sum())
        scale = float(grad.abs().max() * u.abs().sum()) + 1e-30
        worst = max(worst, abs(fd - an) / scale)
        assert abs(fd - an) <= 1e-6 * scale, (name, tag, fd, an)
    for i, c in enumerate(cs0):
        check.u = u = torch.randn(c.shape, generator=g, dtype=torch.float64)
        mk = lambda s: [x + s * h * u if j == i else x for j, x in enumerate(cs0)]
        check(f'code{i}', ref['d_codes'][i], loss(mk(-1), e0, Pd), loss(mk(+1), e0, Pd))
    if emb is not None:
        check.u = u = torch.randn(e0.shape, generator=g, dtype=torch.float64)
        check('c_trg', ref['dc_trg'], loss(cs0, e0 - h * u, Pd), loss(cs0, e0 + h * u, Pd))
    for k in Pd:
        check.u = u = torch.randn(Pd[k].shape, generator=g, dtype=torch.float64)
        check(k, ref['grads'][k], loss(cs0, e0, dict(Pd, **{k: Pd[k] - h * u})), loss(cs0, e0, dict(Pd, **{k: Pd[k] + h * u})))
    print(f'[{name}] worst |fd - analytic| / (max|grad| sum|u|) = {worst:.2e}')


@pytest.mark.parametrize('name', list(CASES))
def test_code_gradients_are_block_sums_and_wrong_reductions_are_far_off(name):
    kind, hp, _, _, _, _, ref = case(name)
    right = R.reduce_codes(kind, hp, ref['d_in'])
    for a, b in zip(right, ref['d_codes']):
        assert R.rel(a, b) < 1e-12
    fs = [f for _, f, _ in R.factors(kind, hp)]
    for v in R.CODE_VARIANTS:
        if v == 'factors_swapped' and fs[0] == fs[1]:
            continue                                       # equal factors cannot tell: the W_mix case does
        wrong = R.reduce_codes(kind, hp, ref['d_in'], v)
        worst = max(R.rel(w, r) for w, r in zip(wrong, right))
        print(f'[{name}] {v}: {worst / R.BAR:.0f} bars')
        assert worst >= R.WRONG_FACTOR * R.BAR, (name, v, worst)
        if v != 'factors_swapped':
            assert min(R.rel(w, r) for w, r in zip(wrong, right)) >= R.WRONG_FACTOR * R.BAR, (name, v)     # every code shows it
    assert name != 'G3_mix' or len(set(fs)) == 3


def test_the_swapped_factors_case_exists():
    assert any(len({f for _, f, _ in R.factors(k, hp)}) > 1 for k, hp, _, _ in CASES.values())


@pytest.mark.parametrize('name', ['G3', 'G3_mix'])
def test_dc_trg_is_per_row_and_needs_both_directions(name):
    kind, hp, P, codes, emb, d_out, ref = case(name)
    out, g_f, g_r = R.dc_trg_by_direction(P, hp, codes, emb, d_out)
    assert R.rel(out, ref['out']) < 1e-12
    assert R.rel(g_f + g_r, ref['dc_trg']) < 1e-10
    for tag, wrong in (('forward only', g_f), ('reverse only', g_r), ('batch-summed', R.dc_batch_summed(ref['dc_trg']))):
        r = R.rel(wrong, ref['dc_trg'])
        print(f'[{name}] dc_trg {tag}: {r / R.BAR:.0f} bars')
        assert r >= R.WRONG_FACTOR * R.BAR, (name, tag, r)


def test_decoder_only_adam_and_its_wrong_variants():
    """On the arena state the GPU test sets up (adam_ref's case default_t7_gs1: restored step 7, non-zero moments everywhere; here with
    exact-zero gradients below the split, as a decode backward leaves them) an update of the whole
    arena moves every encoder element (the GPU test asks for equal bits there), and a step counter that did not advance shows in the
    following full step far beyond the optimiser bars."""
    n, split = 4096, 1024
    hpar = adam_ref.HP_DEFAULT
    p = adam_ref.make_params(n)
    m, v = adam_ref.make_moments(n, 7, hpar['eps'])
    ordinary = adam_ref.classes(n) == 0
    g = adam_ref.make_grad(n, 2, hpar['eps'])
    g[:split] = 0
    right = R.adam_decoder(p, g, m, v, split, t=8, **hpar)
    for a, b in zip(right, (p, m, v)):
        assert torch.equal(a[:split], b[:split].double())
    want = adam_ref.adam_f64(p[split:], g[split:], m[split:], v[split:], t=8, **hpar)
    for a, b in zip(right, want):
        assert torch.equal(a[split:], b)
    whole = R.adam_decoder(p, g, m, v, split, t=8, variant='whole_arena', **hpar)
    moved = (whole[0][:split].float() != p[:split]) & ordinary[:split]
    assert int(moved.sum()) == int(ordinary[:split].sum())            # every ordinary element's fp32 bits change
    for a, b in zip(whole[1:], (m, v)):                                # ... and both moments decay: no bit pattern survives either
        assert int(((a[:split].float() != b[:split]) & ordinary[:split]).sum()) == int(ordinary[:split].sum())
    # the following full step: t = 9 (right) against t = 8 again (counter not advanced)
    p1, m1, v1 = (x.float() for x in right)
    g2 = adam_ref.make_grad(n, 3, hpar['eps'])
    nxt = adam_ref.adam_f64(p1, g2, m1, v1, t=9, **hpar)
    stuck = adam_ref.adam_f64(p1, g2, m1, v1, t=8, **hpar)
    rep = adam_ref.compare(stuck, nxt, (p1, m1, v1), mask=ordinary)
    print(f'step counter not advanced: upd {rep["upd"]["ordinary"]:.3g} units (bar {adam_ref.BARS["upd"]["ordinary"]:.3g})')
    assert rep['upd']['ordinary'] >= R.WRONG_FACTOR * adam_ref.BARS['upd']['ordinary']


def test_sum_order_budget_covers_an_fp32_sum_in_order_and_is_exact_for_one_term():
    g = torch.Generator().manual_seed(3)
    for f in (1, 4, 8, 16):
        x = torch.randn(4096, f, generator=g)
        acc = x[:, 0].clone()
        for u in range(1, f):
            acc = acc + x[:, u]
        err = (acc.double() - x.double().sum(1)).abs()
        budget = R.sum_order_budget(x.double().abs().sum(1), f)
        assert bool((err <= budget).all()), f
        assert f > 1 or float(budget.max()) == 0.0


def test_train_decoder_f64_moves_only_the_decoder_and_lowers_the_loss():
    kind, hp, P, codes, emb, _, ref = case('G3')
    target = ref['out'].float() + 0.1
    losses, Pd = R.train_decoder_f64(kind, P, hp, codes, emb, target, 3)
    assert set(Pd) == {k for k in P if k.startswith('decoder.')} and len(Pd) == 26
    assert losses[2] < losses[0]
    assert all(not torch.equal(Pd[k], P[k]) for k in Pd)
