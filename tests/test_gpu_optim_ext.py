"""Decoupled weight decay and the parameter EMA (adam_ext_kernel, ema_range_kernel, arena_swap_kernel and the prepare kernels,
csrc/elementwise.hip; their call sites in csrc/engine.hip) against float64 on every element of the arena and on every route to the optimiser.
Runs on the GPU box: pytest -m gpu.

The reference and the bars are tests/optim_ext_ref.py (float64 on top of adam_ref.adam_f64; bars = 4 x what stock fp32 torch.optim.AdamW and
get_ema_avg_fn show against it on the CPU; nothing in them comes from the engine).  Every step is compared FROM THE ENGINE'S OWN STATE BEFORE
IT, the average on the engine's own new parameters.  Shapes are the smallest the engine takes (B = 2, T = max_len_pad = 8, a bucket at 16):
the arena is full size whatever the shape.

  1 controlled gradients   ss_adam_step on adam_ref's seven classes: wd alone, EMA alone, both, both under clipping (coefficient exactly 0.5
                           -- max_norm is chosen so that it is a power of two and the scaled gradient stays exact -- and exactly 1), which = 0
                           and 1, warm-up on and off, a restored n
  2 routes                 real gradients, three steps: fused, SS_STEP_BUCKET, SS_STEP_NO_ADAM + ss_adam_step, split + ss_train_finish, the
                           native data-parallel step on one rank, a two-micro-batch accumulation cycle, ss_adam_step_decoder,
                           ss_g3_decode_train_step; after each step p, m, v and the EMA against float64 AND bit for bit against a twin engine
                           that takes the stand-alone step from the same state and gradient arena
  3 off means off          three fused steps on an engine that never heard of the calls, on one that called them with 0 / None, and on one
                           that switched both on and off again: the same bits
  4 skip                   an inf behind SS_STEP_NO_ADAM under clipping at +inf: nothing moves, n included; the next step applies with n + 1
  5 swap                   ema_weights(): the forward of an engine loaded with the average, bit for bit; the bits back afterwards; no training inside
  6 containment            the kernels on guarded buffers (tests/guarded.py) at lengths that are and are not a multiple of the grid's stride
  7 solver                 train, save, resume: the next step bit for bit, EMA and n included; 'model_ema' loads into a fresh Generator_3
  8 refusals               the bad arguments of the four calls, which they name after the binding (so not without a device)
The tests print their worst errors (profiles/r05/optim_ext/test_figures.txt keeps a run's).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import interp_np, weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from speechsplit_amd import _capi
from tests import adam_ref as A
from tests import guarded as G
from tests import optim_ext_ref as R

pytestmark = pytest.mark.gpu
B, T, T_BUCKET = 2, 8, 16
INF = float('inf')


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


@pytest.fixture
def deterministic(E):
    E.tune('deterministic', 1)
    try:
        yield
    finally:
        E.tune('deterministic', 0)


_ENGINES = {}


def get_engine(E, kind, slot=0, precision='f32'):
    """One engine per generator, slot and precision for the whole module (slot 1: the twin that takes the stand-alone step; the precision of
    an engine is chosen before its first step, so the bf16 mode has an engine of its own)."""
    key = (kind, slot, precision)
    if key not in _ENGINES:
        eng = E.Engine(kind, W.default_hparams(max_len_pad=T), B, T_BUCKET)
        eng.set_precision(precision)
        n = eng.params.numel()
        mask = torch.zeros(n, dtype=torch.bool, device=eng.device)
        for _, off, shape in eng.table:
            mask[off:off + int(np.prod(shape))] = True
        eng.is_param = mask
        eng.cls = A.classes(n, eng.device)
        eng.decayed = {'all': None, 'weights': R.decayed_mask(eng.table, n, 'weights', eng.device)}
        _ENGINES[key] = eng
    eng = _ENGINES[key]
    eng.set_grad_clip(0)
    eng.set_weight_decay(0)
    eng.set_ema(None)
    return eng


def fill(eng, arena, flat):
    views = eng.views(arena)
    for n, off, shape in eng.table:
        views[n].copy_(flat[off:off + int(np.prod(shape))].view(*shape))


def snapshot(eng):
    return tuple(x.clone() if x is not None else None for x in (eng.params, eng.adam_m, eng.adam_v, eng.ema))


def state(eng):
    return (eng.params, eng.adam_m, eng.adam_v, eng.ema)


def same_bits(eng, snap, sel=None):
    return [name for name, a, b in zip(('p', 'm', 'v', 'ema'), state(eng), snap) if a is not None and b is not None and not A.bits_equal(a, b, sel)]


def ema_n(eng):
    return int(eng.ema_stats()[0].item())


# ------------------------------------------------------------------------------------------------ 1: controlled gradients
#           id                  kind  adam_ref case  wd    which      decay   warmup n0       clip
CONTROLLED = [
    ('g3_wd_all',               'G3', 0,             1e-2, 'all',     None,   False, 0,       None),
    ('g3_wd_weights',           'G3', 1,             0.1,  'weights', None,   False, 0,       None),
    ('g3_ema',                  'G3', 2,             0.0,  'all',     0.999,  False, 0,       None),
    ('g3_both_warm_restored',   'G3', 3,             0.1,  'weights', 0.9999, True,  10 ** 6, None),
    ('g3_both_clip_half',       'G3', 4,             1e-2, 'all',     0.5,    True,  7,       'half'),
    ('g3_both_clip_one',        'G3', 5,             0.1,  'weights', 0.999,  False, 0,       'one'),
    ('g6_both_warm',            'G6', 6,             1e-2, 'weights', 0.9999, True,  0,       None),
    ('g6_ema_clip_half',        'G6', 0,             0.0,  'all',     0.5,    False, 0,       'half'),
]


@pytest.mark.parametrize('cfg', CONTROLLED, ids=[c[0] for c in CONTROLLED])
def test_standalone_step_on_controlled_gradients(E, cfg):
    """Three ss_adam_step calls on adam_ref's controlled gradients with the terms of `cfg` on; after each, every parameter element of p, m, v
    and the EMA against float64 at the bars of optim_ext_ref, and the update counter."""
    tag, kind, case, wd, which, decay, warm, n0, clip = cfg
    name, hp, restored, gs = A.CASES[case]
    eng = get_engine(E, kind)
    n, dev, cls = eng.params.numel(), eng.device, eng.cls
    eng.zero_grads()
    p0 = A.make_params(n, dev)
    fill(eng, eng.params, p0)
    m0, v0 = A.make_moments(n, restored, hp['eps'], gs, dev)
    fill(eng, eng.adam_m, m0)
    fill(eng, eng.adam_v, v0)
    eng.set_adam(hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], restored)
    eng.set_weight_decay(wd, which)
    if decay is not None:
        eng.set_ema(decay, warm, state=(R.make_ema(p0, dev), n0))
        assert ema_n(eng) == n0
    zero = eng.is_param & (cls == 1)
    worst = {}
    for k in range(1, 4):
        fill(eng, eng.grads, A.make_grad(n, k, hp['eps'], dev))
        coef = 1.0
        if clip == 'one':
            eng.set_grad_clip(INF)
        elif clip == 'half':        # coef = max_norm / (norm + 1e-6) in fp32: exactly 0.5 when max_norm is half that fp32 sum
            norm = np.float32(eng.grad_norm(gs).item())
            eng.set_grad_clip(float(np.float32(0.5) * (norm + np.float32(1e-6))))
            coef = 0.5
        before = snapshot(eng)
        eng.adam_step(gs)
        if clip:
            st = eng.grad_clip_stats().cpu()
            assert float(st[1]) == coef and int(st[3]) == 0, (tag, k, st)
        g_eff = eng.grads.double() * coef           # exact: the coefficient is a power of two
        rep, bad = R.check(state(eng), before, g_eff, hp, restored + k, grad_scale=gs, wd=wd, decayed=eng.decayed[which], decay=decay, warmup=warm,
                           n=n0 + k - 1, cls=cls, mask=eng.is_param)
        assert not bad, (tag, k, bad, rep['worst'])
        if decay is not None:
            assert ema_n(eng) == n0 + k, (tag, k)
            s = eng.ema_stats().cpu()
            assert abs(float(s[1]) - R.ema_d(decay, warm, n0 + k - 1)) <= 1e-7
        if wd:
            assert float(eng.ema_stats()[2]) == float(np.float32(1.0 - hp['lr'] * R.f32(wd)))
        if not wd or which == 'weights':            # an element that is not decayed and sees no gradient keeps its bits
            still = zero if not wd else zero & ~eng.decayed['weights']
            assert not [q for q in same_bits(eng, before[:3] + (None,), still)], (tag, k, 'always-zero class moved')
        R.merge(worst, rep)
    eng.check()
    assert eng.status() == 0
    print(f'[{tag} / {name}] engine against float64 over 3 steps, worst per class (worst element: {worst["worst"]}):\n{R.table(worst)}')


# ------------------------------------------------------------------------------------------------ 2: every route, real gradients
def batch_of(kind, seed, frames):
    mel, f0, emb, lens = synth_batch(seed, B, frames, frames)
    if kind == 'G3':
        return mel, f0, emb, lens
    q = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
    return mel, torch.nn.functional.one_hot(q, 257).float(), q


def stack_draws(draws):
    return np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])


_WEIGHTS = {}


def weights_of(kind):
    if kind not in _WEIGHTS:
        _WEIGHTS[kind] = W.make_weights(kind, W.default_hparams(max_len_pad=T), 11)
    return _WEIGHTS[kind]


def codes_of(eng, kind, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = eng.code_shapes(B, T)
    codes = [torch.randn(shapes[k], generator=g) * 0.5 for k in (('x', 'r', 'f0') if kind == 'G3' else ('r', 'f0'))]
    emb = torch.randn(B, eng.hp.dim_spk_emb, generator=g) * 0.1
    out_dim = eng.hp.dim_freq if kind == 'G3' else eng.hp.dim_f0
    return codes, emb, torch.randn(B, T, out_dim, generator=g)


def route_step(eng, kind, route, it):
    """One optimiser step through `route`; returns (grad_scale of the optimiser step, first element the step covers)."""
    ncalls = 4 if kind == 'G3' else 3
    step = (lambda b, d, **kw: eng.g3_train_step(*b, d, **kw)) if kind == 'G3' else (lambda b, d, **kw: eng.g6_train_step(*b, d, **kw))
    frames = T_BUCKET if route == 'bucket' else T
    batch, draws = batch_of(kind, 60 + it, frames), stack_draws(draws_for(160 + it, B, ncalls))
    if route == 'fused':
        step(batch, draws)
    elif route == 'bucket':
        step(batch, draws, bucket=True)
    elif route == 'no_adam':
        step(batch, draws, no_adam=True)
        eng.adam_step()
    elif route == 'split':
        step(batch, draws, no_adam=True, split_backward=True)
        eng.train_finish(no_adam=False)
    elif route == 'dp_native':
        eng.comm_init(0, 1)
        try:
            (eng.dp_train_step_native if kind == 'G3' else eng.g6_dp_train_step_native)(*batch, draws)
            torch.cuda.synchronize()
        finally:
            eng.lib.ss_comm_destroy(eng.h)
    elif route == 'accum':
        before = snapshot(eng)
        n = ema_n(eng)
        step(batch, draws, no_adam=True)
        assert not same_bits(eng, before) and ema_n(eng) == n, 'a micro-batch without an optimiser step decayed or averaged'
        step(batch_of(kind, 80 + it, frames), stack_draws(draws_for(180 + it, B, ncalls)), accumulate=True, grad_scale=0.5)
        return 0.5, 0
    elif route in ('decoder_step', 'decode_train_step'):
        codes, emb, rnd = codes_of(eng, kind, 90 + it)
        if route == 'decode_train_step':
            eng.g3_decode_train_step(*codes, emb, rnd)
        elif kind == 'G3':
            eng.g3_decode_train(*codes, emb)
            eng.g3_decode_backward(1e-3 * rnd)
            eng.adam_step_decoder()
        else:
            eng.g6_decode_train(*codes)
            eng.g6_decode_backward(1e-3 * rnd)
            eng.adam_step_decoder()
        return 1.0, eng.grad_split
    else:
        raise ValueError(route)
    return 1.0, 0


ROUTES = [('G3', r, c) for r, c in (('fused', 0), ('fused', INF), ('bucket', 0), ('no_adam', 0), ('split', 0), ('dp_native', 0), ('accum', 0),
                                    ('decoder_step', 0), ('decoder_step', INF), ('decode_train_step', 0))]
ROUTES += [('G6', r, c) for r, c in (('fused', 0), ('bucket', 0), ('no_adam', INF), ('dp_native', 0), ('accum', 0), ('decoder_step', 0))]
ROUTES = [r + ('f32',) for r in ROUTES] + [('G3', 'fused', 0, 'bf16'), ('G3', 'split', 0, 'bf16'), ('G3', 'fused', INF, 'bf16')]
WD, WHICH, DECAY, N0, HP, RESTORED = 0.1, 'weights', 0.999, 3, A.HP_FAST, 500


@pytest.mark.parametrize('kind,route,clip,precision', ROUTES, ids=[f'{k.lower()}-{r}-{"clip_inf" if c else "noclip"}-{p}' for k, r, c, p in ROUTES])
def test_route_matches_float64_and_the_standalone_step(E, kind, route, clip, precision):
    """Three optimiser steps through one route with decay (which = 1) and a warmed-up EMA on, from a restored step 500: after each, p, m, v and
    the EMA against float64 from the snapshot before the step and the gradient arena as it stands; the encoder range of p, m, v bit-unchanged
    on the decoder routes while its EMA moved; n advanced once; and the same bits as a twin engine that takes the stand-alone optimiser step
    (ss_adam_step, or ss_adam_step_decoder) from the same state and the same gradient arena."""
    eng, twin = get_engine(E, kind, 0, precision), get_engine(E, kind, 1)      # (the twin only takes optimiser steps: no precision there)
    n, dev = eng.params.numel(), eng.device
    eng.load_weights(weights_of(kind))
    fill(eng, eng.adam_m, (1e-3 * (A._u(n, 7, dev) - 0.5)).float())
    fill(eng, eng.adam_v, (1e-6 * (0.01 + A._u(n, 8, dev))).float())
    eng.set_adam(HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], RESTORED)
    for e in (eng, twin):
        e.set_grad_clip(clip)
        e.set_weight_decay(WD, WHICH)
    eng.set_ema(DECAY, True, state=(eng.params * (1.0 + 1e-2 * (A._u(n, 12, dev).float() - 0.5)), N0))
    worst = {}
    for it in range(3):
        before = snapshot(eng)
        gs, lo = route_step(eng, kind, route, it)
        t, nb = RESTORED + it + 1, N0 + it
        rep, bad = R.check(state(eng), before, eng.grads, HP, t, grad_scale=gs, wd=WD, decayed=eng.decayed[WHICH], decay=DECAY, warmup=True, n=nb,
                           lo=lo, mask=eng.is_param, real=True)
        assert not bad, (kind, route, it, bad, rep['worst'])
        assert ema_n(eng) == nb + 1
        if lo:
            enc = slice(0, lo)
            assert not same_bits(eng, before[:3] + (None,), enc), 'the encoder range of p, m, v moved on a decoder-only step'
            assert not A.bits_equal(eng.ema[enc], before[3][enc]), 'the encoder range of the EMA did not move'
        assert same_bits(eng, before) == ['p', 'm', 'v', 'ema']
        # the twin: the same state, the same gradient arena, the stand-alone call
        for dst, src in zip((twin.params, twin.adam_m, twin.adam_v, twin.grads), before[:3] + (eng.grads,)):
            dst.copy_(src)
        twin.set_adam(HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], t - 1)
        twin.set_ema(DECAY, True, state=(before[3], nb))
        (twin.adam_step_decoder if lo else twin.adam_step)(gs)
        assert not same_bits(twin, state(eng)), (kind, route, it, 'differs from the stand-alone step', same_bits(twin, state(eng)))
        assert ema_n(twin) == nb + 1
        R.merge(worst, rep)
    eng.check()
    twin.check()
    assert eng.status() == 0
    covered = eng.is_param.clone()
    covered[:lo] = False
    moved = float((eng.grads[covered] != 0).float().mean())
    assert moved > 0.5, moved                      # real gradients: the step was not compared on an arena of zeros
    w = {q: float(f'{worst[q]["ordinary"]:.3g}') for q in ('m', 'v', 'upd', 'ema')}
    print(f'[{kind} {route} clip={clip} {precision}] engine against float64 over 3 steps, every element: {w}, worst element {worst["worst"][:3]}')


# ------------------------------------------------------------------------------------------------ 3: off means off
@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_off_means_off(E, deterministic, kind):
    hp = W.default_hparams(max_len_pad=T)

    def run(prepare):
        eng = E.Engine(kind, hp, B, T)
        eng.load_weights(weights_of(kind))
        eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
        prepare(eng)
        for it in range(3):
            ncalls = 4 if kind == 'G3' else 3
            batch, draws = batch_of(kind, 30 + it, T), stack_draws(draws_for(130 + it, B, ncalls))
            (eng.g3_train_step if kind == 'G3' else eng.g6_train_step)(*batch, draws)
        eng.check()
        return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()

    def zeros(eng):
        eng.set_weight_decay(0)
        eng.set_ema(None)

    def on_and_off(eng):
        eng.set_weight_decay(0.1, 'weights')
        eng.set_ema(0.999, True)
        batch, draws = batch_of(kind, 29, T), stack_draws(draws_for(129, B, 4 if kind == 'G3' else 3))
        p = eng.params.clone()
        (eng.g3_train_step if kind == 'G3' else eng.g6_train_step)(*batch, draws)
        assert not A.bits_equal(eng.params, p)
        eng.load_weights(weights_of(kind))                      # back to the start: parameters, moments, step
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
        zeros(eng)

    base = run(lambda eng: None)
    for other in (zeros, on_and_off):
        got = run(other)
        assert all(A.bits_equal(a, b) for a, b in zip(got, base)), other.__name__


# ------------------------------------------------------------------------------------------------ 4: skip
def test_a_skipped_step_changes_nothing(E):
    kind = 'G3'
    eng = get_engine(E, kind)
    eng.load_weights(weights_of(kind))
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
    eng.set_grad_clip(INF)
    eng.set_weight_decay(0.1, 'all')
    eng.set_ema(0.5, True)
    step = lambda it, **kw: eng.g3_train_step(*batch_of(kind, 40 + it, T), stack_draws(draws_for(140 + it, B, 4)), **kw)
    step(0)                                                     # one applied step: non-zero moments, the average apart from p, n = 1
    assert ema_n(eng) == 1 and not A.bits_equal(eng.ema, eng.params)
    before, stats_before = snapshot(eng), eng.ema_stats().cpu()
    step(1, no_adam=True)
    _, off, _ = eng.table[len(eng.table) // 2]
    eng.grads[off + 1] = INF                                    # an ordinary store into the caller-owned gradient arena
    eng.adam_step()
    torch.cuda.synchronize()
    assert R.check_skipped(state(eng), before, ema_n(eng), 1) == []
    assert torch.equal(eng.ema_stats().cpu(), stats_before)
    clip = eng.grad_clip_stats().cpu()
    assert not math.isfinite(float(clip[0])) and float(clip[1]) == 0.0 and int(clip[3]) == 1
    assert eng.status() == 0
    eng.grads[off + 1] = 0.0
    eng.adam_step()                                             # the next step applies: t = 2, n from 1 to 2
    rep, bad = R.check(state(eng), before, eng.grads, dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), 2, wd=0.1, decay=0.5, warmup=True, n=1,
                       mask=eng.is_param, real=True)
    assert not bad, bad
    assert ema_n(eng) == 2 and int(eng.grad_clip_stats()[3]) == 1
    eng.check()


# ------------------------------------------------------------------------------------------------ 5: swap
def test_ema_weights_swaps_and_restores(E):
    kind = 'G3'
    hp = W.default_hparams(max_len_pad=T)
    eng = get_engine(E, kind)
    eng.load_weights(weights_of(kind))
    n, dev = eng.params.numel(), eng.device
    avg = eng.params * (1.0 + 0.05 * (A._u(n, 13, dev).float() - 0.5))
    eng.set_ema(0.999, False, state=(avg, 5))
    other = E.Engine(kind, hp, B, T_BUCKET)
    other.load_weights({k: v.clone() for k, v in eng.ema_views().items()})
    mel, f0, emb, lens = batch_of(kind, 50, T)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy())), 257).float()
    x_f0 = torch.cat((mel, onehot), -1)
    p_bits, e_bits = eng.params.clone(), eng.ema.clone()
    plain = eng.g3_forward(x_f0, mel, emb).clone()
    with eng.ema_weights():
        assert A.bits_equal(eng.params, e_bits) and A.bits_equal(eng.ema, p_bits)
        inside = eng.g3_forward(x_f0, mel, emb).clone()
        for call in (lambda: eng.g3_train_step(mel, f0, emb, lens, stack_draws(draws_for(150, B, 4))), eng.adam_step, eng.adam_step_decoder,
                     lambda: eng.train_finish(no_adam=False), lambda: eng.dp_train_step_native(mel, f0, emb, lens, stack_draws(draws_for(150, B, 4)))):
            with pytest.raises(RuntimeError, match='ema_weights'):
                call()
        with pytest.raises(RuntimeError, match='ema_weights'):
            with eng.ema_weights():
                pass
    assert A.bits_equal(eng.params, p_bits) and A.bits_equal(eng.ema, e_bits)
    want = other.g3_forward(x_f0, mel, emb)
    assert A.bits_equal(inside, want) and not A.bits_equal(inside, plain)
    assert A.bits_equal(eng.g3_forward(x_f0, mel, emb), plain)
    assert ema_n(eng) == 5
    eng.check()
    g6 = get_engine(E, 'G6')
    with pytest.raises(RuntimeError, match='no EMA'):
        g6.ema_weights().__enter__()


# ------------------------------------------------------------------------------------------------ 6: containment
STRIDE4 = 4096 * 256                        # float4 elements one sweep of the largest grid covers
LENGTHS = [4 * 256 * 3, 4 * (256 * 3 + 5), 4 * 2 * STRIDE4, 4 * (STRIDE4 + 257)]


def op(**kw):
    o = _capi.SSOptimExtOp()
    for k, v in kw.items():
        setattr(o, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return o


def run_op(o):
    _capi.check(_capi.lib().ss_op_optim_ext(C.byref(o), None))
    torch.cuda.synchronize()


@pytest.mark.parametrize('n', LENGTHS, ids=[f'n{n}' for n in LENGTHS])
@pytest.mark.parametrize('form', ['wd', 'wd_tab', 'ema', 'both', 'both_tab_clip', 'skip'])
def test_update_kernels_stay_inside_their_arenas(E, form, n):
    """The extended Adam update on guarded p, m, v, ema and a guarded input g, over [lo, hi) inside them: no guard word changes, the elements
    outside [lo, hi) keep their bits, the ones inside match float64.  Lengths: below one sweep of the grid with and without a whole number of
    workgroups, and above it with and without a whole number of sweeps."""
    dev = torch.device('cuda')
    hp, t0, gs = A.HP_MID, 7, 0.5
    cls = A.classes(n, dev)
    p0 = A.make_params(n, dev)
    m0, v0 = A.make_moments(n, t0, hp['eps'], gs, dev)
    e0 = R.make_ema(p0, dev)
    g0 = A.make_grad(n, 1, hp['eps'], dev)
    bufs = {k: G.out((n,), dev, fill=x, name=k) for k, x in (('p', p0), ('m', m0), ('v', v0), ('ema', e0))}
    gin = G.inp(g0, dev, name='g')
    st = torch.zeros(64, dtype=torch.float32, device=dev)
    skip = torch.ones(1, dtype=torch.float32, device=dev)
    lo, hi = 8, n - 12
    wd = 0.0 if form == 'ema' else 0.1
    ema = form in ('ema', 'both', 'both_tab_clip', 'skip')
    tab = 'tab' in form
    coef = 0.5 if 'clip' in form else 0.0
    decayed = torch.ones(n, dtype=torch.bool, device=dev)
    if tab:
        edges = [0] + sorted({(n * k // 23) // 4 * 4 for k in range(1, 23)}) + [n]
        nr = len(edges) - 1
        starts = (C.c_long * nr)(*edges[:-1])
        lens = (C.c_int * nr)(*[b - a for a, b in zip(edges[:-1], edges[1:])])
        decs = (C.c_int * nr)(*[k % 2 for k in range(nr)])
        for k in range(nr):
            decayed[edges[k]:edges[k + 1]] = bool(k % 2)
    o = op(p=bufs['p'].t, g=gin.t, m=bufs['m'].t, v=bufs['v'].t, ema=bufs['ema'].t if ema else None, state=st, lo=lo, hi=hi, lr=hp['lr'],
           beta1=hp['beta1'], beta2=hp['beta2'], eps=hp['eps'], step=t0, grad_scale=gs, clip_coef=coef, weight_decay=wd, ema_decay=0.999,
           ema_warmup=1, ema_updates=3, mode=0, skip_status=skip if form == 'skip' else None)
    if tab:
        o.n_runs, o.run_start, o.run_len, o.run_decayed = nr, starts, lens, decs
    run_op(o)
    G.check_all(list(bufs.values()) + [gin])
    got = (bufs['p'].t, bufs['m'].t, bufs['v'].t, bufs['ema'].t)
    before = (p0, m0, v0, e0)
    inside = torch.zeros(n, dtype=torch.bool, device=dev)
    inside[lo:hi] = True
    for a, b in zip(got, before):
        assert A.bits_equal(a, b, ~inside), 'an element outside [lo, hi) moved'
    if form == 'skip':
        assert all(A.bits_equal(a, b) for a, b in zip(got, before))
        return
    if not ema:
        assert A.bits_equal(got[3], e0)
    rep, bad = R.check(got, before, g0.double() * (coef or 1.0), hp, t0 + 1, grad_scale=gs, wd=wd, decayed=decayed if tab else None,
                       decay=0.999 if ema else None, warmup=True, n=3, cls=cls, mask=inside)
    assert not bad, (form, n, bad, rep['worst'])


@pytest.mark.parametrize('n', LENGTHS, ids=[f'n{n}' for n in LENGTHS])
def test_ema_range_and_arena_swap_stay_inside_their_arenas(E, n):
    dev = torch.device('cuda')
    p0 = A.make_params(n, dev)
    e0 = R.make_ema(p0, dev)
    lo, hi = 4, n - 8
    inside = torch.zeros(n, dtype=torch.bool, device=dev)
    inside[lo:hi] = True
    st = torch.zeros(64, dtype=torch.float32, device=dev)
    # ema_range: p is an input
    pin, eout = G.inp(p0, dev, name='p'), G.out((n,), dev, fill=e0, name='ema')
    base = dict(state=st, lo=lo, hi=hi, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=0, grad_scale=1.0, ema_decay=0.9999, ema_warmup=1,
                ema_updates=10 ** 6)
    run_op(op(p=pin.t, ema=eout.t, mode=1, **base))
    G.check_all([pin, eout])
    assert A.bits_equal(eout.t, e0, ~inside) and A.bits_equal(pin.t, p0)
    r = R.compare_ema(eout.t, R.ema_f64(e0, p0, 0.9999, True, 10 ** 6), e0, A.classes(n, dev), inside)
    assert max(r.values()) <= R.BARS['ema']['ordinary'], r
    skip = torch.ones(1, dtype=torch.float32, device=dev)
    keep = eout.t.clone()
    run_op(op(p=pin.t, ema=eout.t, mode=1, skip_status=skip, **base))
    assert A.bits_equal(eout.t, keep)
    # arena_swap: both are outputs; twice restores
    a, b = G.out((n,), dev, fill=p0, name='a'), G.out((n,), dev, fill=e0, name='b')
    run_op(op(p=a.t, ema=b.t, state=st, lo=lo, hi=hi, mode=2))
    G.check_all([a, b])
    assert A.bits_equal(a.t, torch.where(inside, e0, p0)) and A.bits_equal(b.t, torch.where(inside, p0, e0))
    run_op(op(p=a.t, ema=b.t, state=st, lo=lo, hi=hi, mode=2))
    G.check_all([a, b])
    assert A.bits_equal(a.t, p0) and A.bits_equal(b.t, e0)


# ------------------------------------------------------------------------------------------------ 7: the solver
def test_resumed_solver_with_decay_and_ema_takes_the_same_next_step(E, tmp_path):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver
    from speechsplit_amd.engine import draw_interp
    from speechsplit_amd.model import Generator_3
    hp = HP.default_hparams(batch_size=4, max_len_pad=128)
    np.random.seed(0)
    torch.manual_seed(0)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = SimpleNamespace(num_iters=3, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False,
                          device_id=0, log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path),
                          log_step=1, sample_step=1000, model_save_step=3, weight_decay=0.01, weight_decay_which='weights', ema_decay=0.999,
                          ema_warmup=True)
    s = solver.Solver(loader, cfg, hp)
    s.train()
    ckpt = torch.load(str(tmp_path / '3-G.ckpt'), map_location='cpu', weights_only=False)
    assert ckpt['ema_updates'] == 3 and set(ckpt['model_ema']) == set(ckpt['model'])
    group = ckpt['optimizer']['param_groups'][0]
    assert group['weight_decay'] == 0.01 and group['weight_decay_which'] == 'weights'
    fresh = Generator_3(hp)
    fresh.load_state_dict(ckpt['model_ema'])
    name = s.eng.table[0][0]
    assert not torch.equal(ckpt['model_ema'][name], ckpt['model'][name])
    s2 = solver.Solver(loader, SimpleNamespace(**{**vars(cfg), 'resume_iters': 3, 'num_iters': 1}), hp)
    s2.restore_model(3)
    assert s2.step_count == 3 == s.step_count and ema_n(s2.eng) == 3 == ema_n(s.eng)
    for k, v in s.eng.ema_views().items():
        assert torch.equal(v, s2.eng.ema_views()[k]), k
    batch = next(iter(loader))
    draws = draw_interp(batch[0].shape[0], 4, hp, generator=torch.Generator().manual_seed(5))
    E.tune('deterministic', 1)
    try:
        la, lb = s.train_on_batch(batch, draws), s2.train_on_batch(batch, draws)
        s.eng.check()
        s2.eng.check()
    finally:
        E.tune('deterministic', 0)
    assert float(la) == float(lb)
    for name in ('params', 'adam_m', 'adam_v'):
        assert A.bits_equal(getattr(s.eng, name), getattr(s2.eng, name)), name
    for k, v in s.eng.ema_views().items():
        assert A.bits_equal(v, s2.eng.ema_views()[k]), k
    assert ema_n(s.eng) == ema_n(s2.eng) == 4
    assert torch.equal(s.eng.ema_stats(), s2.eng.ema_stats())


def test_checkpoint_without_the_terms_has_todays_keys(E, tmp_path, capsys):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver
    hp = HP.default_hparams(batch_size=4, max_len_pad=128)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = SimpleNamespace(num_iters=1, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False, device_id=0,
                          log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path), log_step=1, sample_step=1000,
                          model_save_step=1)
    s = solver.Solver(loader, cfg, hp)
    s.save_model(0)
    ckpt = torch.load(str(tmp_path / '0-G.ckpt'), map_location='cpu', weights_only=False)
    assert set(ckpt) == {'model', 'optimizer'}
    group = ckpt['optimizer']['param_groups'][0]
    assert group['weight_decay'] == 0 and type(group['weight_decay']) is int and 'weight_decay_which' not in group
    # resuming from it with a decay and an average configured: the configured decay stays in force (the stored 0 does not switch it off),
    # the average starts from the restored parameters, and both are said
    capsys.readouterr()
    s2 = solver.Solver(loader, SimpleNamespace(**vars(cfg), weight_decay=0.05, weight_decay_which='weights', ema_decay=0.9), hp)
    s2.restore_model(0)
    out = capsys.readouterr().out
    assert s2.weight_decay == 0.05 and s2.weight_decay_which == 'weights' and 'written without weight decay' in out and 'holds no parameter average' in out
    assert A.bits_equal(s2.eng.ema, s2.eng.params) and ema_n(s2.eng) == 0
    s2.train_on_batch(next(iter(loader)))
    assert float(s2.eng.ema_stats()[2]) == float(np.float32(1.0 - 1e-4 * R.f32(0.05)))
    s2.save_model(1)
    # ... and the other way round: an average in the checkpoint that nobody asked for is reported, not silently dropped
    s.restore_model(1)
    out = capsys.readouterr().out
    assert "holds a parameter average ('model_ema', 1 updates) but no ema_decay is configured" in out
    assert s.weight_decay == 0.05 and s.eng.ema is None                     # the decay the checkpoint was trained with wins


# ------------------------------------------------------------------------------------------------ 8: refusals on a bound engine
def test_bad_arguments_are_refused_by_name(E):
    eng = get_engine(E, 'G6')
    lib, h = eng.lib, eng.h
    err = lambda: lib.ss_last_error().decode()
    for wd, which, why in ((-1.0, 0, 'weight_decay must be'), (float('nan'), 0, 'weight_decay must be'), (INF, 0, 'weight_decay must be'),
                           (0.1, 2, 'which must be'), (0.1, -1, 'which must be')):
        assert lib.ss_set_weight_decay(h, wd, which, None) != 0 and err().startswith('ss_set_weight_decay: ') and why in err(), err()
    buf = torch.zeros(eng.params.numel() + 4, device=eng.device)
    for ptr, decay, why in ((buf.data_ptr(), 1.0, 'decay must lie in [0, 1)'), (buf.data_ptr(), -0.1, 'decay must lie'), (buf.data_ptr(), float('nan'), 'decay must lie'),
                            (buf.data_ptr() + 4, 0.9, '16-byte aligned'), (eng.params.data_ptr(), 0.9, 'an arena of its own')):
        assert lib.ss_set_ema(h, ptr, decay, 0, -1, None) != 0 and err().startswith('ss_set_ema: ') and why in err(), err()
    assert lib.ss_ema_swap(h, None) != 0 and err() == 'ss_ema_swap: no EMA arena (call ss_set_ema first)'
    assert lib.ss_ema_stats(h, None, None) != 0 and err() == 'ss_ema_stats: null pointer'
    # the kernel hook's run table: a hole, an overlap and a table that stops short of hi are refused by the launcher
    dev = eng.device
    bufs = [torch.zeros(64, device=dev) for _ in range(6)]
    bufs[0].fill_(1.0)                                          # an update would decay it
    for starts, lens in (((0, 32), (16, 32)), ((0, 16), (32, 32)), ((0, 32), (32, 16)), ((8, 32), (24, 32))):
        o = op(p=bufs[0], g=bufs[1], m=bufs[2], v=bufs[3], ema=bufs[4], state=bufs[5], lo=0, hi=64, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
               grad_scale=1.0, weight_decay=0.1, ema_decay=0.5, mode=0, n_runs=2)
        o.run_start, o.run_len, o.run_decayed = (C.c_long * 2)(*starts), (C.c_int * 2)(*lens), (C.c_int * 2)(1, 0)
        assert lib.ss_op_optim_ext(C.byref(o), None) != 0, (starts, lens)
        torch.cuda.synchronize()
        assert bool((bufs[0] == 1.0).all()) and float(bufs[4].abs().max()) == 0.0, 'a refused table still updated something'
    with pytest.raises(ValueError):
        eng.set_weight_decay(0.1, which='biases')
    assert torch.equal(eng.ema_stats().cpu(), torch.zeros(4))          # nothing above took effect
