"""The Adam update (adam_kernel and its prepare kernels, csrc/elementwise.hip; the range split of the fused step, csrc/engine.hip) against
float64, on every element of the arena, on every route to the optimiser and past step one.  Runs on the GPU box: pytest -m gpu.

The reference is tests/adam_ref.py: adam_f64 evaluates torch.optim.Adam's single-tensor formulas in float64, on the device, FROM THE
ENGINE'S OWN STATE BEFORE THE STEP, so errors do not accumulate and the bar is a few ulps: adam_ref.BARS = 4 x what stock fp32
torch.optim.Adam shows against the same float64 on the same inputs (measured on the CPU, adam_ref.YARDSTICK; nothing in it comes from the
engine).  test_adam_ref_selftest.py proves on the CPU that ten wrong optimisers are reported under these bars.

Part 1 (test_standalone_step_*): ss_adam_step on controlled gradients -- seven magnitude classes as a fixed function of the flat index
(adam_ref.make_grad), three hyper-parameter sets, restored steps 0 / 7 / 999 / 10^6 with random moments, grad_scale 1 / 0.5 / 2^-10; nine
consecutive steps per case, the ninth being the check of the step counter.  The always-zero class is held bit-identical.
Part 2 (test_route_*): real gradients, five steps through the fused step (whose update goes out in two launches split at ss_grad_split),
SS_STEP_NO_ADAM + ss_adam_step, the split backward + ss_train_finish, and SS_STEP_BUCKET; from zero moments and from a restored step 500.
Real gradients are compared with adam_ref's cancellation floor (see there) at the 'ordinary' bars.
Part 3: one deterministic step of a resumed solver against the same step of the uninterrupted one, bit for bit.

Worst errors in the units of adam_ref (fp32 ulps of the float64 value).  Yardstick: stock fp32 torch.optim.Adam on the CPU over the whole
grid at 19.4 M elements; bar = 4 x yardstick; engine: measured on MI355X over every case of part 1, both generators (the tests print it):
    class          m' yardstick / bar / engine    v' yardstick / bar / engine      update yardstick / bar / engine
    ordinary       1.54 / 6.16 / 1.53             2.27 / 9.08 / 2.72               6.28 / 25.1 / 4.89
    zero           0 / 0 / 0 (bit-identical)      0 / 0 / 0                        0 / 0 / 0
    near_eps       1.53 / 6.12 / 1.53             2.25 / 9.00 / 2.71               5.19 / 20.8 / 4.07
    large          1.53 / 6.12 / 1.53             2.27 / 9.08 / 2.70               5.16 / 20.6 / 4.60
    tiny           1.54 / 6.16 / 1.53             1.2e-7 / 1 (flush or keep) / 1.2e-7   1.72e-6 / 6.9e-6 / 1.72e-6 (p unchanged on both sides)
    alternating    9.61 / 38.4 / 9.60             2.26 / 9.04 / 2.26               6.96 / 27.8 / 6.85
    fading         0.625 / 2.5 / 0.75             2.26 / 9.04 / 2.26               4.84 / 19.4 / 4.18
The engine needs at most 0.30 x its bar in any class (its v' sits 0.45 ulp further out than torch's, its update closer in).  Part 2, real
gradients, all routes, every element: m' 2.40, v' 2.74, update 4.86 against the 'ordinary' bars.
"""

import numpy as np
import pytest
import torch

from oracle import interp_np, weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from tests import adam_ref as A

pytestmark = pytest.mark.gpu
B, T, T_BUCKET = 2, 64, 56


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


_ENGINES = {}


def get_engine(E, kind, precision='f32'):
    """One engine per generator and precision for the whole module (as get_engine of test_gpu_parity.py): Adam's cost does not depend on the
    shape.  The precision of an engine is chosen before its first step, so the bf16 mode has an engine of its own."""
    key = (kind, precision)
    if key not in _ENGINES:
        eng = E.Engine(kind, W.default_hparams(max_len_pad=T), 8, T)
        eng.set_precision(precision)
        n = eng.params.numel()
        mask = torch.zeros(n, dtype=torch.bool, device=eng.device)
        edges = []
        for _, off, shape in eng.table:
            k = int(np.prod(shape))
            mask[off:off + k] = True
            edges += [off, off + k - 1]
        assert not bool(mask[n - 4:].any())                                  # the status slot is no parameter
        eng.is_param = mask
        eng.cls = A.classes(n, eng.device)
        s = eng.grad_split
        seam = list(range(max(s - 8, 0), min(s + 8, n - 4)))
        eng.explicit = torch.tensor(sorted(set(i for i in edges + seam if bool(mask[i]))), dtype=torch.int64, device=eng.device)
        _ENGINES[key] = eng
    return _ENGINES[key]


def fill(eng, arena, flat):
    """Write a flat arena-sized tensor into an arena through the parameter views only (gaps and the status slot are left alone)."""
    views = eng.views(arena)
    for n, off, shape in eng.table:
        views[n].copy_(flat[off:off + int(np.prod(shape))].view(*shape))


def snapshot(eng):
    return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()


def unchanged(eng, snap):
    return all(A.bits_equal(a, b) for a, b in zip((eng.params, eng.adam_m, eng.adam_v), snap))


def check_step(eng, before, hp, t, grad_scale, cls, tag, real):
    """The step the engine just took against adam_f64 from `before` and the gradient arena as it stands: every parameter element at the
    bars, then the seam of ss_grad_split and the first and last element of every tensor once more on their own."""
    got = (eng.params, eng.adam_m, eng.adam_v)
    want = A.adam_f64(before[0], eng.grads, before[1], before[2], t=t, grad_scale=grad_scale, **hp)
    rep = A.compare(got, want, before, cls, eng.is_param, cancel_floor=real)
    only = 'ordinary' if real else None
    assert not A.excess(rep, only=only), (tag, t, A.excess(rep, only=only), rep['worst'])
    ix = eng.explicit
    sub = A.compare([x[ix] for x in got], [x[ix] for x in want], [x[ix] for x in before], None if cls is None else cls[ix], None, cancel_floor=real)
    assert not A.excess(sub, only=only), (tag, t, 'seam / tensor edges', A.excess(sub, only=only), int(ix[sub['worst'][1]]))
    return rep


# ------------------------------------------------------------------------------------------------ part 1: the stand-alone step
G6_CASES = ('default_t0_gs1', 'mid_t7_gs2m10')
PART1 = [('G3', c) for c in A.CASES] + [('G6', c) for c in A.CASES if c[0] in G6_CASES]


@pytest.mark.parametrize('kind,case', PART1, ids=[f'{k.lower()}_{c[0]}' for k, c in PART1])
def test_standalone_step_on_controlled_gradients(E, kind, case):
    """Nine ss_adam_step calls on the controlled gradients; each compared from the engine's own state before it, the ninth (t = restored + 9)
    being the evidence that the counter advanced once per step.  Yardstick (stock fp32 torch.optim.Adam, CPU) and the engine's measured
    worst per class: adam_ref.YARDSTICK and the table in DESIGN.md section 2; the engine needs at most 0.30 x the bar in any class (module docstring)."""
    name, hp, restored, gs = case
    eng = get_engine(E, kind)
    n, dev, cls = eng.params.numel(), eng.device, eng.cls
    eng.zero_grads()
    fill(eng, eng.params, A.make_params(n, dev))
    m0, v0 = A.make_moments(n, restored, hp['eps'], gs, dev)
    fill(eng, eng.adam_m, m0)
    fill(eng, eng.adam_v, v0)
    assert float(eng.adam_v.min()) >= 0.0
    eng.set_adam(hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], restored)
    zero = eng.is_param & (cls == 1)
    worst = {}
    for k in range(1, 10):
        fill(eng, eng.grads, A.make_grad(n, k, hp['eps'], dev))
        before = snapshot(eng)
        eng.adam_step(gs)
        rep = check_step(eng, before, hp, restored + k, gs, cls, f'{kind} {name} step {k}', real=False)
        assert all(A.bits_equal(a, b, zero) for a, b in zip((eng.params, eng.adam_m, eng.adam_v), before)), (name, k, 'always-zero class moved')
        A.merge(worst, rep)
    eng.check()
    assert eng.status() == 0
    print(f'[{kind} {name}] engine against float64 over 9 steps, worst per class (worst element: {worst["worst"]}):\n{A.table(worst)}')


# ------------------------------------------------------------------------------------------------ part 2: every route, real gradients
def batch_of(kind, seed, frames):
    mel, f0, emb, lens = synth_batch(seed, B, frames, frames - 7)
    if kind == 'G3':
        return mel, f0, emb, lens
    q = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
    return mel, torch.nn.functional.one_hot(q, 257).float(), q


_WEIGHTS = {}


def weights_of(kind):
    if kind not in _WEIGHTS:
        _WEIGHTS[kind] = W.make_weights(kind, W.default_hparams(max_len_pad=T), 11)
    return _WEIGHTS[kind]


def stack_draws(draws):
    return np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])


def route_step(eng, kind, route, batch, draws, before):
    """One training step through `route`; where the forward and backward run with SS_STEP_NO_ADAM, nothing may change before the optimiser is called."""
    if kind == 'G3':
        step = lambda **kw: eng.g3_train_step(*batch, draws, **kw)
    else:
        step = lambda **kw: eng.g6_train_step(*batch, draws, **kw)
    if route == 'fused':
        step()
    elif route == 'bucket':
        step(bucket=True)
    elif route == 'no_adam':
        step(no_adam=True)
        assert unchanged(eng, before), 'SS_STEP_NO_ADAM changed parameters or moments'
        eng.adam_step()
    elif route == 'split':
        step(no_adam=True, split_backward=True)
        assert unchanged(eng, before), 'the split backward changed parameters or moments'
        eng.train_finish(no_adam=False)
    else:
        raise ValueError(route)


STARTS = {'zero_default': (A.HP_DEFAULT, 0), 'restored500_fast': (A.HP_FAST, 500), 'zero_fast': (A.HP_FAST, 0), 'restored500_default': (A.HP_DEFAULT, 500)}
MODELS = {'g3_f32': ('G3', 'f32', ('fused', 'no_adam', 'split', 'bucket')), 'g3_bf16': ('G3', 'bf16', ('fused', 'no_adam', 'split', 'bucket')),
          'g6_f32': ('G6', 'f32', ('fused', 'no_adam', 'bucket'))}
# both starting states and both hyper-parameter sets on every route of every model; the crossed pairs on the fused route, where the seam is
PART2 = [(mdl, r, s) for mdl, (_, _, routes) in MODELS.items() for r in routes for s in ('zero_default', 'restored500_fast')]
PART2 += [(mdl, 'fused', s) for mdl in MODELS for s in ('zero_fast', 'restored500_default')]


@pytest.mark.parametrize('model,route,start', PART2, ids=['-'.join(x) for x in PART2])
def test_route_matches_float64_on_real_gradients(E, model, route, start):
    """Five training steps through one route; after each, the gradient arena still holds that step's raw gradients, and the engine's p, m and
    v must equal adam_f64 applied to them and to the snapshot taken before the step -- every parameter element, and the 8 elements either
    side of ss_grad_split and the first and last element of every tensor once more explicitly.  Then: status clean, and a probe ss_adam_step
    on the same gradients matches t + 1 (the counter advanced once per step)."""
    kind, precision, _ = MODELS[model]
    hp, restored = STARTS[start]
    eng = get_engine(E, kind, precision)
    n, dev = eng.params.numel(), eng.device
    frames = T_BUCKET if route == 'bucket' else T
    eng.load_weights(weights_of(kind))
    if restored:                                   # random non-zero moments at the scale of this model's gradients
        fill(eng, eng.adam_m, (1e-3 * (A._u(n, 7, dev) - 0.5)).float())
        fill(eng, eng.adam_v, (1e-6 * (0.01 + A._u(n, 8, dev))).float())
    else:
        eng.adam_m.zero_()
        eng.adam_v.zero_()
    eng.set_adam(hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], restored)
    worst = {}
    ncalls = 4 if kind == 'G3' else 3
    for it in range(5):
        batch = batch_of(kind, 60 + it, frames)
        draws = stack_draws(draws_for(160 + it, B, ncalls))
        before = snapshot(eng)
        route_step(eng, kind, route, batch, draws, before)
        rep = check_step(eng, before, hp, restored + it + 1, 1.0, None, f'{model} {route} {start} step {it}', real=True)
        A.merge(worst, rep)
        assert not unchanged(eng, before)
    eng.check()
    assert eng.status() == 0
    moved = float((eng.grads[eng.is_param] != 0).float().mean())
    assert moved > 0.5, moved                      # real gradients: the step was not compared on an arena of zeros
    before = snapshot(eng)                         # the probe: one more update on the gradients that are there
    eng.adam_step()
    check_step(eng, before, hp, restored + 6, 1.0, None, f'{model} {route} {start} probe', real=True)
    eng.check()
    w = {q: worst[q]['ordinary'] for q in ('m', 'v', 'upd')}
    print(f'[{model} {route} {start}] engine against float64 over 5 steps, every element: {w}, worst element {worst["worst"][:3]}')


# ------------------------------------------------------------------------------------------------ part 3: the resumed solver
def test_resumed_solver_takes_the_same_next_step_bit_for_bit(E, tmp_path):
    """test_solver_trains_and_checkpoints (test_gpu_parity.py) checks the restored step count and exp_avg_sq.  Here the resumed solver and the
    uninterrupted one each take the next step on the same batch and draws in deterministic mode: parameters and both moments are equal
    bit for bit (a restored counter off by one, or moments that lost bits on the way, would show in every element)."""
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver
    from speechsplit_amd.engine import draw_interp
    hp = HP.default_hparams(batch_size=4, max_len_pad=128)
    np.random.seed(0)
    torch.manual_seed(0)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = SimpleNamespace(num_iters=3, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False,
                          device_id=0, log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path),
                          log_step=1, sample_step=1000, model_save_step=3)
    s = solver.Solver(loader, cfg, hp)
    s.train()
    s2 = solver.Solver(loader, SimpleNamespace(**{**vars(cfg), 'resume_iters': 3, 'num_iters': 1}), hp)
    s2.restore_model(3)
    assert s2.step_count == 3 == s.step_count
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
    assert float(s.eng.adam_m.abs().max()) > 0 and s.step_count == s2.step_count == 4
