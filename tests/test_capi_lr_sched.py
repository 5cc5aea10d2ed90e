"""CPU-only checks of the learning-rate schedule (ss_set_lr_schedule / ss_lr_stats, the test hook ss_op_lr_schedule): symbols, the header's
definition and the version, every refusal that comes before anything is enqueued, the Solver's option parsing and the checkpoint's keys
with and without the option.  No kernel is launched here.  The two engine calls name a bad argument AFTER a missing binding, so the
argument refusals are checked here on the engine-free hook, which shares the refusal and its words with ss_set_lr_schedule;
tests/test_gpu_lr_sched.py repeats them on a bound engine."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from speechsplit_amd import _capi, hparams as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)       # non-null, aligned stand-in for a device pointer: the calls below refuse before they touch it
NAN, INF = float('nan'), float('inf')
# (kind, warmup_steps, warmup_start, total_steps, gamma, period, min_lr)
GOOD = {1: (1, 0, 0.1, 0, 0.0, 0, 0.0), 2: (2, 5, 0.1, 12, 0.0, 0, 1e-6), 3: (3, 5, 1.0, 1, 0.0, 0, 0.0), 4: (4, 0, 0.5, 0, 1.0, 0, 0.0),
        5: (5, 1, 0.1, 0, 0.5, 1, 0.0)}
BAD = [
    ((6, 0, 0.1, 1, 0.5, 1, 0.0), 'kind must be'), ((-1, 0, 0.1, 1, 0.5, 1, 0.0), 'kind must be'),
    ((1, -1, 0.1, 0, 0.0, 0, 0.0), 'warmup_steps must be >= 0'),
    ((1, 3, 0.0, 0, 0.0, 0, 0.0), 'warmup_start must lie in (0, 1]'), ((2, 3, 1.5, 12, 0.0, 0, 0.0), 'warmup_start must lie in (0, 1]'),
    ((3, 3, NAN, 12, 0.0, 0, 0.0), 'warmup_start must lie in (0, 1]'), ((1, 0, -0.1, 0, 0.0, 0, 0.0), 'warmup_start must lie in (0, 1]'),
    ((2, 0, 0.1, 0, 0.0, 0, 0.0), 'total_steps must be >= 1'), ((3, 0, 0.1, -4, 0.0, 0, 0.0), 'total_steps must be >= 1'),
    ((4, 0, 0.1, 0, 0.0, 0, 0.0), 'gamma must lie in (0, 1]'), ((4, 0, 0.1, 0, 1.5, 0, 0.0), 'gamma must lie in (0, 1]'),
    ((5, 0, 0.1, 0, NAN, 4, 0.0), 'gamma must lie in (0, 1]'), ((5, 0, 0.1, 0, -0.5, 4, 0.0), 'gamma must lie in (0, 1]'),
    ((5, 0, 0.1, 0, 0.5, 0, 0.0), 'period must be >= 1'), ((5, 0, 0.1, 0, 0.5, -2, 0.0), 'period must be >= 1'),
    ((1, 0, 0.1, 0, 0.0, 0, -1e-9), 'min_lr must be >= 0 and finite'), ((2, 0, 0.1, 12, 0.0, 0, INF), 'min_lr must be >= 0 and finite'),
    ((4, 0, 0.1, 0, 0.5, 0, NAN), 'min_lr must be >= 0 and finite'),
]


def _engine(kind):
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    h = lib.ss_create(kind, C.byref(hps), 2, 192)
    assert h
    return lib, h


def _err(lib):
    return lib.ss_last_error().decode()


def test_symbols_header_text_and_the_version():
    vp, d, i, l = C.c_void_p, C.c_double, C.c_int, C.c_long
    assert _capi.SYMBOLS['ss_set_lr_schedule'] == (i, [vp, i, i, d, i, d, i, d, vp])
    assert _capi.SYMBOLS['ss_lr_stats'] == (i, [vp, vp, vp])
    assert _capi.SYMBOLS['ss_op_lr_schedule'] == (i, [i, d, i, d, i, d, i, d, vp, l, vp, vp])
    lib = _capi.lib()
    for name in ('ss_set_lr_schedule', 'ss_lr_stats', 'ss_op_lr_schedule'):
        assert getattr(lib, name).restype is C.c_int
    assert lib.ss_abi_version() == 2
    text = re.sub(r'\s+', ' ', re.sub(r'\n \* ', '\n', open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()))
    for decl in ('int ss_set_lr_schedule(ss_engine* e, int kind, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, '
                 'double min_lr, void* stream);',
                 'int ss_lr_stats(ss_engine* e, float* out4_dev, void* stream);',
                 'int ss_op_lr_schedule(int kind, double base, int warmup_steps, double warmup_start, int total_steps, double gamma, int period, '
                 'double min_lr, const long* steps_dev, long n, double* lr_dev, void* stream);'):
        assert decl in text, decl
    for phrase in ('s = t - 1', 'lr_t = base * (sf + (1 - sf) * ((double)s / (double)W))', 'k = s - W',
                   'lr_t = min_lr + (base - min_lr) * (0.5 * (1 + cospi((double)kk / (double)N)))',
                   'lr_t = base + (min_lr - base) * ((double)kk / (double)N)', 'lr_t = max(base * pow(gamma, (double)k), min_lr)',
                   'lr_t = max(base * pow(gamma, (double)(k / P)), min_lr), integer division', 'step_size = (float)(lr_t / bc1)',
                   '(float)(1 - lr_t * weight_decay)', 'SequentialLR(opt, [LinearLR(opt, sf, 1.0, W), main], [W])', 'CosineAnnealingLR(T_max=N,', 'eta_min=min_lr)',
                   'LinearLR(1.0, min_lr / base, N)', 'ExponentialLR(gamma)', 'StepLR(P, gamma)', "torch's cosine turns back up",
                   'min_lr also floors the two geometric kinds', 'carries the rate of the SAME t', 'kind 0 is off', 'what ss_bind restores',
                   'ss_set_adam(..., step) positions it', 'counts optimiser steps, not micro-batches'):
        assert phrase in text, phrase


@pytest.mark.parametrize('name,args', [('ss_set_lr_schedule', GOOD[2]), ('ss_lr_stats', (FAKE,))])
def test_null_wrong_kind_and_unbound_engines_are_refused(name, args):
    lib = _capi.lib()
    fn = getattr(lib, name)
    assert fn(None, *args, None) != 0
    assert _err(lib) == name + ': null engine'
    lib0, h0 = _engine(0)
    try:
        assert fn(h0, *args, None) != 0
        assert name in _err(lib) and 'is not a Generator_3 or a Generator_6: it is InterpLnr-only' in _err(lib)
    finally:
        lib0.ss_destroy(h0)
    for kind in (3, 6):
        _, h = _engine(kind)
        try:
            assert fn(h, *args, None) != 0
            assert _err(lib) == name + ': engine is not bound (call ss_bind first)'
        finally:
            lib.ss_destroy(h)


@pytest.mark.parametrize('args,why', BAD, ids=[f'{a[0]}-{w[:14]}-{k}' for k, (a, w) in enumerate(BAD)])
def test_bad_options_are_refused_by_name(args, why):
    lib, h = _engine(3)
    try:                        # on an unbound engine the binding is what is reported, bad options or not
        assert lib.ss_set_lr_schedule(h, *args, None) != 0
        assert _err(lib) == 'ss_set_lr_schedule: engine is not bound (call ss_bind first)'
    finally:
        lib.ss_destroy(h)
    # the hook refuses the options with the words ss_set_lr_schedule uses, in front of its pointers
    steps, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    assert lib.ss_op_lr_schedule(args[0], 1e-4, *args[1:], steps, 4, out, None) != 0
    assert _err(lib).startswith('ss_op_lr_schedule: ') and why in _err(lib), _err(lib)


@pytest.mark.parametrize('kind', sorted(GOOD))
def test_good_options_and_off_are_refused_on_an_unbound_engine(kind):
    lib, h = _engine(6)
    try:
        for args in (GOOD[kind], (0, -5, NAN, -1, NAN, -1, NAN)):      # off reads none of the others
            assert lib.ss_set_lr_schedule(h, *args, None) != 0
            assert _err(lib) == 'ss_set_lr_schedule: engine is not bound (call ss_bind first)'
    finally:
        lib.ss_destroy(h)


def test_the_hook_refuses_its_own_arguments():
    lib = _capi.lib()
    steps, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    for a, n, b, why in ((None, 4, out, 'null pointer'), (steps, 4, None, 'null pointer'), (steps, 0, out, 'n must lie in'),
                         (steps, -1, out, 'n must lie in'), (steps, (1 << 24) + 1, out, 'n must lie in'),
                         (C.c_void_p(0x2004), 4, out, '8-byte aligned'), (steps, 4, C.c_void_p(0x3004), '8-byte aligned')):
        assert lib.ss_op_lr_schedule(2, 1e-4, 5, 0.1, 12, 0.0, 0, 0.0, a, n, b, None) != 0
        assert _err(lib).startswith('ss_op_lr_schedule: ') and why in _err(lib), _err(lib)
    _, h = _engine(3)
    try:
        assert lib.ss_lr_stats(h, None, None) != 0 and _err(lib) == 'ss_lr_stats: engine is not bound (call ss_bind first)'
    finally:
        lib.ss_destroy(h)


def test_solver_options_from_config_and_environment():
    from speechsplit_amd.solver import lr_schedule_options as opt
    cfg = lambda **kw: SimpleNamespace(num_iters=100, **kw)
    assert opt(cfg(), {}) is None
    assert opt(cfg(), {'SS_LR_SCHEDULE': ''}) is None and opt(cfg(), {'SS_LR_SCHEDULE': 'off'}) is None
    assert opt(cfg(lr_schedule=None), {'SS_LR_SCHEDULE': 'cosine'}) is None          # an attribute on the config wins, None included
    assert opt(cfg(), {'SS_LR_SCHEDULE': 'constant'}) == dict(kind='constant', warmup=0, warmup_start=0.1, total=None, gamma=None, period=None,
                                                              min_lr=0.0)
    env = {'SS_LR_SCHEDULE': 'cosine', 'SS_LR_WARMUP': '5', 'SS_LR_WARMUP_START': '0.25', 'SS_LR_MIN': '1e-6'}
    assert opt(cfg(), env) == dict(kind='cosine', warmup=5, warmup_start=0.25, total=95, gamma=None, period=None, min_lr=1e-6)
    assert opt(cfg(), dict(env, SS_LR_TOTAL='40'))['total'] == 40
    assert opt(cfg(lr_schedule='linear', lr_warmup=10), {})['total'] == 90
    assert opt(cfg(lr_schedule='exponential', lr_gamma=0.99, lr_total=7), {}) == dict(kind='exponential', warmup=0, warmup_start=0.1, total=None,
                                                                                      gamma=0.99, period=None, min_lr=0.0)
    assert opt(cfg(), {'SS_LR_SCHEDULE': 'step', 'SS_LR_GAMMA': '0.5', 'SS_LR_PERIOD': '30'}) == dict(
        kind='step', warmup=0, warmup_start=0.1, total=None, gamma=0.5, period=30, min_lr=0.0)
    for bad in ({'SS_LR_SCHEDULE': 'cyclic'}, {'SS_LR_SCHEDULE': 'cosine', 'SS_LR_WARMUP': '-1'}, {'SS_LR_SCHEDULE': 'cosine', 'SS_LR_WARMUP': '100'},
                {'SS_LR_SCHEDULE': 'cosine', 'SS_LR_WARMUP_START': '0'}, {'SS_LR_SCHEDULE': 'linear', 'SS_LR_WARMUP_START': '1.5'},
                {'SS_LR_SCHEDULE': 'linear', 'SS_LR_TOTAL': '0'}, {'SS_LR_SCHEDULE': 'exponential'}, {'SS_LR_SCHEDULE': 'exponential', 'SS_LR_GAMMA': '1.1'},
                {'SS_LR_SCHEDULE': 'step', 'SS_LR_GAMMA': '0.5'}, {'SS_LR_SCHEDULE': 'step', 'SS_LR_GAMMA': '0.5', 'SS_LR_PERIOD': '0'},
                {'SS_LR_SCHEDULE': 'constant', 'SS_LR_MIN': '-1'}, {'SS_LR_SCHEDULE': 'constant', 'SS_LR_MIN': 'nan'}):
        with pytest.raises(ValueError):
            opt(cfg(), bad)


def test_engine_methods_exist_with_the_stated_signatures():
    import inspect
    from speechsplit_amd.engine import Engine
    sig = inspect.signature(Engine.set_lr_schedule).parameters
    assert list(sig) == ['self', 'kind', 'warmup', 'warmup_start', 'total', 'gamma', 'period', 'min_lr']
    assert [sig[k].default for k in list(sig)[1:]] == [None, 0, 0.1, None, None, None, 0.0]
    assert callable(Engine.lr_stats)
    assert Engine.LR_KINDS == {None: 0, 'off': 0, 'constant': 1, 'cosine': 2, 'linear': 3, 'exponential': 4, 'step': 5}


class _FakeEngine:
    """what Solver.save_model and optimizer_state_dict touch, without a device"""
    ema = None
    adam_m = adam_v = None

    def views(self, flat):
        return {'w': torch.zeros(3)}


@pytest.mark.parametrize('sched', [None, dict(kind='cosine', warmup=5, warmup_start=0.1, total=95, gamma=None, period=None, min_lr=0.0)])
def test_checkpoint_keys_with_and_without_the_option(sched, tmp_path):
    from speechsplit_amd.solver import Solver
    s = object.__new__(Solver)
    s.model_save_dir, s.eng, s.step_count = str(tmp_path), _FakeEngine(), 3
    s.G = SimpleNamespace(state_dict=lambda: {'w': torch.ones(3)}, _names=['w'])
    s.g_lr, s.beta1, s.beta2, s.weight_decay, s.weight_decay_which, s.lr_schedule = 1e-4, 0.9, 0.999, 0.0, 'all', sched
    s.save_model(3)
    ckpt = torch.load(os.path.join(str(tmp_path), '3-G.ckpt'), weights_only=False)
    assert set(ckpt) == ({'model', 'optimizer'} | ({'lr_schedule'} if sched else set()))
    if sched:
        assert ckpt['lr_schedule'] == sched and ckpt['lr_schedule'] is not sched
    assert ckpt['optimizer']['param_groups'][0]['lr'] == 1e-4          # the base rate, schedule or not
    assert set(ckpt['optimizer']['param_groups'][0]) == {'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable',
                                                         'differentiable', 'fused', 'params'}
