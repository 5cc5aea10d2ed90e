"""The learning-rate schedule (lr_schedule and lr_prepare in the two prepare kernels, lr_schedule_eval_kernel, csrc/elementwise.hip; its call
sites in csrc/engine.hip) against the float64 restatement and on every route to the optimiser.  Runs on the GPU box: pytest -m gpu.

The restatement, its agreement with torch's scheduler objects and the bar of the function are tests/lr_sched_ref.py; the optimiser step
under a rate lr_t is tests/optim_ext_ref.py's float64 step with lr replaced by lr_t, at that module's bars.  Nothing in either comes from
the engine.  Shapes are test_gpu_optim_ext.py's (B = 2, T = max_len_pad = 8, a bucket at 16), and so are its batches, routes and helpers.

  1 the function alone     ss_op_lr_schedule at t in {1, 2, W, W + 1, W + 2, W + N, W + N + 1, W + N + 1000, 2^31 + 7}, every kind, W in
                           {0, 1, 5}, P in {1, 4}, against lr_at within LR_BAR (100 x the restatement-vs-torch figure, at least 100 x 2^-52,
                           relative to max(base, min_lr)); cosine at kk = N is min_lr and constant is base, to the bit
  2 controlled gradients   ss_adam_step on adam_ref's classes, positioned by set_adam(step=...) inside the warm-up, at its last step, at the
                           first main step and past N; with and without decay (which 0 and 1), EMA and clipping; p, m, v and the EMA against
                           float64; lr_stats()[0] = (float)lr_t of the hook and ema_stats()[2] = (float)(1 - lr_t * wd), to the bit
  3 routes                 three steps across the warm-up boundary on every route of test_gpu_optim_ext.py, against float64 and bit for bit
                           against a twin engine that takes the stand-alone step from the same state and gradient arena
  4 off means off          three fused steps: never called / kind 0 / on and off again / constant with W = 0: the same bits
  5 skip                   an inf behind SS_STEP_NO_ADAM under clipping at +inf: nothing moves, lr_stats included; the next applied step
                           carries lr_t of the SAME t
  6 containment            the hook kernel on guarded buffers at n in {1, 63, 64, 257}
  7 solver                 train across the warm-up boundary, save, resume: the next step bit for bit, lr_stats included
  8 refusals               on a bound engine, by name
The tests print their worst figures (profiles/r05/lr_sched/test_figures.txt keeps a run's).
"""
import math

import numpy as np
import pytest
import torch

from oracle import weights as W
from oracle.gen_fixtures import draws_for
from speechsplit_amd import _capi
from tests import adam_ref as A
from tests import guarded as G
from tests import lr_sched_ref as L
from tests import optim_ext_ref as R
from tests import test_gpu_optim_ext as X

pytestmark = pytest.mark.gpu
B, T, T_BUCKET = X.B, X.T, X.T_BUCKET
INF = float('inf')
BASE, N_REF, GAMMA, MIN_LR = L.BASE, L.N_REF, L.GAMMA, 3e-6


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
    """test_gpu_optim_ext.get_engine with a cache of this module's own (an engine of that module must never be left with a schedule on),
    every optimiser option off"""
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
    eng.set_lr_schedule(None)
    return eng


def set_schedule(eng, sc):
    eng.set_lr_schedule(sc['kind'], warmup=sc['W'], warmup_start=sc['sf'], total=sc['N'], gamma=sc['gamma'], period=sc['P'], min_lr=sc['min_lr'])


def device_lr(ts, base, sc, steps=None, out=None):
    """the hook: lr_t at every t of ts as float64, by the prepare kernels' own __device__ function"""
    dev = torch.device('cuda')
    steps = torch.tensor(list(ts), dtype=torch.int64, device=dev) if steps is None else steps
    out = torch.full((steps.numel(),), float('nan'), dtype=torch.float64, device=dev) if out is None else out
    _capi.check(_capi.lib().ss_op_lr_schedule(L.KIND_ID[sc['kind']], base, sc['W'], sc['sf'], sc['N'] or 0, sc['gamma'] or 0.0, sc['P'] or 0,
                                              sc['min_lr'], steps.data_ptr(), steps.numel(), out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().tolist()


def bits32(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1: the function alone
def function_grid():
    out = []
    for Wm in (0, 1, 5):
        out.append(L.sched('constant', W=Wm))
        out.append(L.sched('cosine', W=Wm, N=N_REF, min_lr=MIN_LR))
        out.append(L.sched('linear', W=Wm, N=N_REF, min_lr=MIN_LR))
        out.append(L.sched('exponential', W=Wm, gamma=GAMMA))
        out.append(L.sched('exponential', W=Wm, gamma=GAMMA, min_lr=BASE * GAMMA ** 2.5))
        for P in (1, 4):
            out.append(L.sched('step', W=Wm, gamma=GAMMA, P=P))
            out.append(L.sched('step', W=Wm, gamma=GAMMA, P=P, min_lr=BASE * GAMMA ** 2.5))
    return out


def test_the_function_alone_matches_the_restatement():
    worst = dict.fromkeys(L.KINDS, 0.0)
    for sc in function_grid():
        Wm = sc['W']
        ts = sorted({t for t in (1, 2, Wm, Wm + 1, Wm + 2, Wm + N_REF, Wm + N_REF + 1, Wm + N_REF + 1000, 2 ** 31 + 7) if t >= 1})
        got = device_lr(ts, BASE, sc)
        for t, lr in zip(ts, got):
            want = L.lr_at(t, BASE, **sc)
            e = L.lr_error(lr, want, BASE, sc['min_lr'])
            worst[sc['kind']] = max(worst[sc['kind']], e)
            assert e <= L.LR_BAR[sc['kind']], (sc, t, lr, want, e)
            s = t - 1
            if sc['kind'] == 'constant' and not (Wm > 0 and s < Wm):
                assert lr == BASE, (sc, t, lr)                       # to the bit
            if sc['kind'] == 'cosine' and s - Wm >= N_REF:
                assert lr == MIN_LR, (sc, t, lr)                     # cospi(1) = -1: the bracket is exactly zero
    print('[function alone] worst |device - restatement| / max(base, min_lr) per kind: '
          + ', '.join(f'{k} {worst[k]:.3g} (bar {L.LR_BAR[k]:.3g})' for k in L.KINDS))


# ------------------------------------------------------------------------------------------------ 2: controlled gradients
COS = L.sched('cosine', W=5, N=N_REF, min_lr=1e-6)
#           id                        kind  hp          schedule                                          restored       wd    which      decay  clip
CONTROLLED = [
    ('g3_inside_warmup',              'G3', A.HP_DEFAULT, COS,                                            1,             0.0,  'all',     None,  None),
    ('g3_warmup_end_wd_all_ema',      'G3', A.HP_FAST,    COS,                                            4,             0.1,  'all',     0.999, None),
    ('g3_linear_reaches_N_wd_w_clip', 'G3', A.HP_MID,     L.sched('linear', W=5, N=N_REF, min_lr=1e-6),   5 + N_REF - 1, 0.1,  'weights', None,  'half'),
    ('g3_past_N_wd_ema_clip_one',     'G3', A.HP_FAST,    COS,                                            5 + N_REF + 3, 1e-2, 'all',     0.5,   'one'),
    ('g6_exponential_wd_w_ema',       'G6', A.HP_MID,     L.sched('exponential', W=5, gamma=GAMMA),       4,             0.1,  'weights', 0.999, None),
    ('g6_step_first_steps_clip',      'G6', A.HP_FAST,    L.sched('step', W=1, gamma=0.5, P=1),           0,             0.0,  'all',     None,  'half'),
]


@pytest.mark.parametrize('cfg', CONTROLLED, ids=[c[0] for c in CONTROLLED])
def test_standalone_step_on_controlled_gradients(E, cfg):
    """Two ss_adam_step calls on adam_ref's controlled gradients from a position set_adam(step=...) chose; after each, every parameter
    element of p, m, v and the EMA against float64 under the restatement's lr_t at optim_ext_ref's bars, and the stats words to the bit."""
    tag, kind, hp, sc, restored, wd, which, decay, clip = cfg
    gs = 0.5
    eng = get_engine(E, kind)
    n, dev, cls = eng.params.numel(), eng.device, eng.cls
    eng.zero_grads()
    p0 = A.make_params(n, dev)
    X.fill(eng, eng.params, p0)
    m0, v0 = A.make_moments(n, restored, hp['eps'], gs, dev)
    X.fill(eng, eng.adam_m, m0)
    X.fill(eng, eng.adam_v, v0)
    set_schedule(eng, sc)                                          # before set_adam: the schedule survives it, and the step positions it
    eng.set_adam(hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], restored)
    eng.set_weight_decay(wd, which)
    if decay is not None:
        eng.set_ema(decay, False, state=(R.make_ema(p0, dev), 0))
    assert eng.lr_stats().cpu().tolist() == [0.0, 0.0, 0.0, float(L.KIND_ID[sc['kind']])]
    worst = {}
    for k in range(1, 3):
        t = restored + k
        X.fill(eng, eng.grads, A.make_grad(n, k, hp['eps'], dev))
        coef = 1.0
        if clip == 'one':
            eng.set_grad_clip(INF)
        elif clip == 'half':
            norm = np.float32(eng.grad_norm(gs).item())
            eng.set_grad_clip(float(np.float32(0.5) * (norm + np.float32(1e-6))))
            coef = 0.5
        before = X.snapshot(eng)
        eng.adam_step(gs)
        if clip:
            st = eng.grad_clip_stats().cpu()
            assert float(st[1]) == coef and int(st[3]) == 0, (tag, k, st)
        hp_t = L.hp_at(hp, t, sc)
        rep, bad = R.check(X.state(eng), before, eng.grads.double() * coef, hp_t, t, grad_scale=gs, wd=wd, decayed=eng.decayed[which], decay=decay,
                           n=k - 1, cls=cls, mask=eng.is_param)
        assert not bad, (tag, k, bad, rep['worst'])
        lr_dev = device_lr([t], hp['lr'], sc)[0]                   # the same double the prepare kernel formed
        assert L.lr_error(lr_dev, hp_t['lr'], hp['lr'], sc['min_lr']) <= L.LR_BAR[sc['kind']]
        s = eng.lr_stats().cpu()
        assert bits32(s[0]) == bits32(lr_dev), (tag, t, float(s[0]), lr_dev)
        assert bits32(s[1]) == bits32(lr_dev / hp['lr']) and float(s[2]) == t and float(s[3]) == L.KIND_ID[sc['kind']], (tag, t, s)
        if wd:
            assert bits32(eng.ema_stats()[2].item()) == bits32(1.0 - lr_dev * R.f32(wd)), (tag, t)
        R.merge(worst, rep)
    eng.check()
    assert eng.status() == 0
    print(f'[{tag}] engine against float64 under lr_t over 2 steps, worst per class (worst element: {worst["worst"]}):\n{R.table(worst)}')


# ------------------------------------------------------------------------------------------------ 3: every route, real gradients
# every route with the schedule alone (the plain prepare launches), and a few with decay and the EMA on as well (the extended ones)
EXT_TOO = {('G3', 'fused', 0, 'f32'), ('G3', 'fused', INF, 'f32'), ('G3', 'decoder_step', INF, 'f32'), ('G3', 'accum', 0, 'f32'),
           ('G6', 'no_adam', INF, 'f32'), ('G6', 'dp_native', 0, 'f32'), ('G3', 'fused', 0, 'bf16')}
ROUTES = [r + (False,) for r in X.ROUTES] + [r + (True,) for r in X.ROUTES if r in EXT_TOO]
HP, RESTORED, WD, WHICH, DECAY, N0 = A.HP_FAST, 1, 0.1, 'weights', 0.999, 3
ROUTE_SC = L.sched('cosine', W=2, sf=0.25, N=4, min_lr=1e-5)      # t = 2 the warm-up's last step, t = 3 and 4 the first two main steps


@pytest.mark.parametrize('kind,route,clip,precision,ext', ROUTES,
                         ids=[f'{k.lower()}-{r}-{"clip_inf" if c else "noclip"}-{p}-{"ext" if x else "plain"}' for k, r, c, p, x in ROUTES])
def test_route_matches_float64_and_the_standalone_step(E, kind, route, clip, precision, ext):
    eng, twin = get_engine(E, kind, 0, precision), get_engine(E, kind, 1)
    n, dev = eng.params.numel(), eng.device
    eng.load_weights(X.weights_of(kind))
    X.fill(eng, eng.adam_m, (1e-3 * (A._u(n, 7, dev) - 0.5)).float())
    X.fill(eng, eng.adam_v, (1e-6 * (0.01 + A._u(n, 8, dev))).float())
    eng.set_adam(HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], RESTORED)
    wd = WD if ext else 0.0
    for e in (eng, twin):
        e.set_grad_clip(clip)
        e.set_weight_decay(wd, WHICH)
        set_schedule(e, ROUTE_SC)
    if ext:
        eng.set_ema(DECAY, True, state=(eng.params * (1.0 + 1e-2 * (A._u(n, 12, dev).float() - 0.5)), N0))
    worst = {}
    for it in range(3):
        before = X.snapshot(eng)
        gs, lo = X.route_step(eng, kind, route, it)
        t, nb = RESTORED + it + 1, N0 + it
        rep, bad = R.check(X.state(eng), before, eng.grads, L.hp_at(HP, t, ROUTE_SC), t, grad_scale=gs, wd=wd, decayed=eng.decayed[WHICH],
                           decay=DECAY if ext else None, warmup=True, n=nb, lo=lo, mask=eng.is_param, real=True)
        assert not bad, (kind, route, it, bad, rep['worst'])
        s = eng.lr_stats().cpu()
        assert bits32(s[0]) == bits32(device_lr([t], HP['lr'], ROUTE_SC)[0]) and float(s[2]) == t, (kind, route, it, s)
        if lo:
            assert not X.same_bits(eng, before[:3] + (None,), slice(0, lo)), 'the encoder range of p, m, v moved on a decoder-only step'
        # the twin: the same state, the same gradient arena, the stand-alone call
        for dst, src in zip((twin.params, twin.adam_m, twin.adam_v, twin.grads), before[:3] + (eng.grads,)):
            dst.copy_(src)
        twin.set_adam(HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], t - 1)
        if ext:
            twin.set_ema(DECAY, True, state=(before[3], nb))
        (twin.adam_step_decoder if lo else twin.adam_step)(gs)
        assert not X.same_bits(twin, X.state(eng)), (kind, route, it, 'differs from the stand-alone step', X.same_bits(twin, X.state(eng)))
        assert torch.equal(twin.lr_stats().cpu(), s)
        R.merge(worst, rep)
    eng.check()
    twin.check()
    assert eng.status() == 0
    w = {q: float(f'{worst[q]["ordinary"]:.3g}') for q in ('m', 'v', 'upd', 'ema') if q in worst}
    print(f'[{kind} {route} clip={clip} {precision} ext={ext}] engine against float64 under lr_t over 3 steps, every element: {w}')


# ------------------------------------------------------------------------------------------------ 4: off means off
@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_off_means_off(E, deterministic, kind):
    hp = W.default_hparams(max_len_pad=T)
    step = lambda eng, seed: (eng.g3_train_step if kind == 'G3' else eng.g6_train_step)(
        *X.batch_of(kind, seed, T), X.stack_draws(draws_for(100 + seed, B, 4 if kind == 'G3' else 3)))

    def run(prepare):
        eng = E.Engine(kind, hp, B, T)
        eng.load_weights(X.weights_of(kind))
        eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
        prepare(eng)
        for it in range(3):
            step(eng, 30 + it)
        eng.check()
        return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.lr_stats().cpu()

    def kind0(eng):
        eng.set_lr_schedule(None)

    def on_and_off(eng):
        eng.set_lr_schedule('cosine', warmup=3, total=5)
        p = eng.params.clone()
        step(eng, 29)
        assert not A.bits_equal(eng.params, p) and float(eng.lr_stats()[2]) == 1.0
        eng.load_weights(X.weights_of(kind))                    # back to the start: parameters, moments, step
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
        eng.set_lr_schedule('off')

    def constant(eng):
        eng.set_lr_schedule('constant', warmup=0)

    base = run(lambda eng: None)
    assert base[3].tolist() == [0.0] * 4                        # off: the stats words are never written
    for other in (kind0, on_and_off, constant):
        got = run(other)
        assert all(A.bits_equal(a, b) for a, b in zip(got[:3], base[:3])), other.__name__
        if other is constant:
            assert got[3].tolist() == [float(np.float32(1e-3)), 1.0, 3.0, 1.0]
        else:
            assert got[3].tolist() == [0.0] * 4, other.__name__


# ------------------------------------------------------------------------------------------------ 5: skip
def test_a_skipped_step_changes_nothing_and_keeps_the_position(E):
    kind, hp = 'G3', dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    sc = L.sched('cosine', W=3, sf=0.1, N=5)
    eng = get_engine(E, kind)
    eng.load_weights(X.weights_of(kind))
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], 0)
    eng.set_grad_clip(INF)
    eng.set_weight_decay(0.1, 'all')
    set_schedule(eng, sc)
    step = lambda it, **kw: eng.g3_train_step(*X.batch_of(kind, 40 + it, T), X.stack_draws(draws_for(140 + it, B, 4)), **kw)
    step(0)                                                     # one applied step: t = 1
    before, lr_before, ema_before = X.snapshot(eng), eng.lr_stats().cpu(), eng.ema_stats().cpu()
    assert float(lr_before[2]) == 1.0 and bits32(lr_before[0]) == bits32(L.lr_at(1, hp['lr'], **sc))
    step(1, no_adam=True)
    _, off, _ = eng.table[len(eng.table) // 2]
    eng.grads[off + 1] = INF                                    # an ordinary store into the caller-owned gradient arena
    eng.adam_step()
    torch.cuda.synchronize()
    assert R.check_skipped(X.state(eng), before, 0, 0) == []
    assert torch.equal(eng.lr_stats().cpu(), lr_before) and torch.equal(eng.ema_stats().cpu(), ema_before)
    clip = eng.grad_clip_stats().cpu()
    assert not math.isfinite(float(clip[0])) and float(clip[1]) == 0.0 and int(clip[3]) == 1
    assert eng.status() == 0
    eng.grads[off + 1] = 0.0
    eng.adam_step()                                             # the next step applies: t = 2 and the rate of t = 2, not of t = 3
    rep, bad = R.check(X.state(eng), before, eng.grads, L.hp_at(hp, 2, sc), 2, wd=0.1, mask=eng.is_param, real=True)
    assert not bad, bad
    s = eng.lr_stats().cpu()
    lr2, lr3 = device_lr([2, 3], hp['lr'], sc)
    assert float(s[2]) == 2.0 and bits32(s[0]) == bits32(lr2) != bits32(lr3)
    assert bits32(eng.ema_stats()[2].item()) == bits32(1.0 - lr2 * R.f32(0.1))
    eng.check()


# ------------------------------------------------------------------------------------------------ 6: containment
@pytest.mark.parametrize('n', [1, 63, 64, 257])
def test_the_hook_kernel_stays_inside_its_buffers(n):
    dev = torch.device('cuda')
    sc = L.sched('cosine', W=5, N=N_REF, min_lr=MIN_LR)
    ts = [1 + (7 * i) % (5 + N_REF + 3) for i in range(n)]
    steps = G.inp(torch.tensor(ts, dtype=torch.int64), dev, name='steps')
    out = G.out((n,), dev, dtype=torch.float64, name='lr')
    got = device_lr(None, BASE, sc, steps=steps.t, out=out.t)
    G.check_all([steps, out])
    assert steps.t.cpu().tolist() == ts
    for t, lr in zip(ts, got):
        assert L.lr_error(lr, L.lr_at(t, BASE, **sc), BASE) <= L.LR_BAR['cosine'], (t, lr)


# ------------------------------------------------------------------------------------------------ 7: the solver
def solver_cfg(tmp_path, **kw):
    from types import SimpleNamespace
    return SimpleNamespace(num_iters=3, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False, device_id=0,
                           log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path), log_step=1, sample_step=1000,
                           model_save_step=3, **kw)


def test_resumed_solver_lands_on_the_same_point_of_the_schedule(E, tmp_path, capsys):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HPM, solver
    from speechsplit_amd.engine import draw_interp
    hp = HPM.default_hparams(batch_size=4, max_len_pad=128)
    np.random.seed(0)
    torch.manual_seed(0)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = solver_cfg(tmp_path, lr_schedule='cosine', lr_warmup=2, lr_warmup_start=0.25, lr_total=4, lr_min=1e-6, weight_decay=0.01)
    sc = L.sched('cosine', W=2, sf=0.25, N=4, min_lr=1e-6)
    s = solver.Solver(loader, cfg, hp)
    assert s.lr_schedule == dict(kind='cosine', warmup=2, warmup_start=0.25, total=4, gamma=None, period=None, min_lr=1e-6)
    s.train()                                                   # t = 1, 2 the warm-up, t = 3 the first main step
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith('Elapsed')]
    assert len(lines) == 3 and all(', lr: ' in ln for ln in lines), out
    assert [float(ln.split(', lr: ')[1]) for ln in lines] == [float(f'{float(np.float32(L.lr_at(t, 1e-4, **sc))):.8e}') for t in (1, 2, 3)]
    ckpt = torch.load(str(tmp_path / '3-G.ckpt'), map_location='cpu', weights_only=False)
    assert set(ckpt) == {'model', 'optimizer', 'lr_schedule'} and ckpt['lr_schedule'] == s.lr_schedule
    assert ckpt['optimizer']['param_groups'][0]['lr'] == 1e-4                        # the base rate
    # resumed with ANOTHER schedule configured: the checkpoint's wins, and that is said
    other = {**vars(cfg), 'resume_iters': 3, 'num_iters': 1, 'lr_schedule': 'linear', 'lr_warmup': 0, 'lr_total': 9}
    s2 = solver.Solver(loader, SimpleNamespace(**other), hp)
    s2.restore_model(3)
    assert "the checkpoint's learning-rate schedule" in capsys.readouterr().out and s2.lr_schedule == s.lr_schedule
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
    st = s.eng.lr_stats().cpu()
    assert torch.equal(st, s2.eng.lr_stats().cpu()) and float(st[2]) == 4.0 and bits32(st[0]) == bits32(device_lr([4], 1e-4, sc)[0])
    assert bits32(s.eng.ema_stats()[2].item()) == bits32(1.0 - device_lr([4], 1e-4, sc)[0] * R.f32(0.01))


def test_checkpoint_and_log_without_the_option_are_todays(E, tmp_path, capsys):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HPM, solver
    hp = HPM.default_hparams(batch_size=4, max_len_pad=128)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = solver_cfg(tmp_path)
    cfg.num_iters, cfg.model_save_step = 1, 1
    s = solver.Solver(loader, cfg, hp)
    assert s.lr_schedule is None
    s.train()
    out = capsys.readouterr().out
    assert ', lr: ' not in out and 'G/loss_id' in out
    ckpt = torch.load(str(tmp_path / '1-G.ckpt'), map_location='cpu', weights_only=False)
    assert set(ckpt) == {'model', 'optimizer'}
    assert s.eng.lr_stats().cpu().tolist() == [0.0] * 4
    # resuming from it with a schedule configured: the configured one applies from here on, positioned by the restored step, and that is said
    s2 = solver.Solver(loader, SimpleNamespace(**{**vars(cfg), 'lr_schedule': 'exponential', 'lr_gamma': 0.5}), hp)
    s2.restore_model(1)
    assert 'written without a learning-rate schedule' in capsys.readouterr().out
    s2.train_on_batch(next(iter(loader)))
    st = s2.eng.lr_stats().cpu()
    assert float(st[2]) == 2.0 and bits32(st[0]) == bits32(1e-4 * 0.5) and float(st[3]) == 4.0


# ------------------------------------------------------------------------------------------------ 8: refusals on a bound engine
def test_bad_arguments_are_refused_by_name_on_a_bound_engine(E):
    from tests.test_capi_lr_sched import BAD
    eng = get_engine(E, 'G6')
    lib, h = eng.lib, eng.h
    err = lambda: lib.ss_last_error().decode()
    for args, why in BAD:
        assert lib.ss_set_lr_schedule(h, *args, None) != 0 and err().startswith('ss_set_lr_schedule: ') and why in err(), (args, err())
    assert lib.ss_lr_stats(h, None, None) != 0 and err() == 'ss_lr_stats: null pointer'
    with pytest.raises(ValueError):
        eng.set_lr_schedule('cyclic')
    for kw, why in ((dict(kind='cosine'), 'total_steps'), (dict(kind='exponential'), 'gamma'), (dict(kind='step', gamma=0.5), 'period')):
        with pytest.raises(RuntimeError, match=why):
            eng.set_lr_schedule(**kw)
    assert eng.lr_stats().cpu().tolist() == [0.0] * 4            # nothing above took effect: the schedule is still off
    eng.set_lr_schedule('step', gamma=0.5, period=2)
    assert eng.lr_stats().cpu().tolist() == [0.0, 0.0, 0.0, 5.0]
    eng.set_lr_schedule(None)
