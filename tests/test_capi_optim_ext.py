"""CPU-only checks of decoupled weight decay and the parameter EMA (ss_set_weight_decay / ss_set_ema / ss_ema_swap / ss_ema_stats, the test
hooks ss_op_optim_ext / ss_op_wd_runs): symbols and arities, the refusals that come before anything is enqueued, the decayed-run table of
which = 1 against the parameter table of both generators, and the Solver's option parsing.  No kernel is launched here.  The four engine
calls name a bad argument AFTER a missing binding, so their argument refusals need a bound engine: tests/test_gpu_optim_ext.py has those."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from speechsplit_amd import _capi, hparams as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)       # non-null, 256-byte aligned stand-in for a device pointer: the calls below refuse before they touch it
CALLS = {
    'ss_set_weight_decay': 'int ss_set_weight_decay(ss_engine* e, float weight_decay, int which, void* stream);',
    'ss_set_ema': 'int ss_set_ema(ss_engine* e, float* ema_dev, double decay, int warmup, long updates, void* stream);',
    'ss_ema_swap': 'int ss_ema_swap(ss_engine* e, void* stream);',
    'ss_ema_stats': 'int ss_ema_stats(ss_engine* e, float* out4_dev, void* stream);',
}
ARGS = {'ss_set_weight_decay': (0.01, 1), 'ss_set_ema': (FAKE, 0.999, 0, -1), 'ss_ema_swap': (), 'ss_ema_stats': (FAKE,)}
BAD_ARGS = {'ss_set_weight_decay': (-1.0, 7), 'ss_set_ema': (FAKE, 1.5, 0, -1), 'ss_ema_swap': (), 'ss_ema_stats': (None,)}


def _engine(kind):
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    h = lib.ss_create(kind, C.byref(hps), 2, 192)
    assert h
    return lib, h


def _err(lib):
    return lib.ss_last_error().decode()


def test_symbols_arities_and_the_version():
    vp, f, d, i, l = C.c_void_p, C.c_float, C.c_double, C.c_int, C.c_long
    assert _capi.SYMBOLS['ss_set_weight_decay'] == (i, [vp, f, i, vp])
    assert _capi.SYMBOLS['ss_set_ema'] == (i, [vp, vp, d, i, l, vp])
    assert _capi.SYMBOLS['ss_ema_swap'] == (i, [vp, vp])
    assert _capi.SYMBOLS['ss_ema_stats'] == (i, [vp, vp, vp])
    lib = _capi.lib()
    for name in list(CALLS) + ['ss_op_optim_ext', 'ss_op_wd_runs']:
        assert getattr(lib, name).restype is C.c_int
    assert lib.ss_abi_version() == 2
    text = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read())
    for decl in CALLS.values():
        assert decl in text, decl
    assert 'int ss_op_optim_ext(const ss_optim_ext_op* op, void* stream);' in text
    assert set(re.findall(r'#define (SS_STEP_\w+) ', text)) == {'SS_STEP_NO_ADAM', 'SS_STEP_SPLIT_BACKWARD', 'SS_STEP_SPLIT_NO_JOIN', 'SS_STEP_ACCUMULATE',
                                                               'SS_STEP_BUCKET'}
    for phrase in ('p1 = p * (float)(1 - lr * weight_decay)', 'not lr / bc1', "ema' = ema + w * (p' - ema)", 'min(decay, (1 + n) / (10 + n))',
                   'a step skipped on the device changes nothing', 'only the cycle\'s one optimiser step decays and averages',
                   'trains the AVERAGED weights', 'a second call restores the original bits', 'ss_bind restores'):
        assert phrase.lower() in text.lower(), phrase


def test_the_optim_ext_descriptor_has_the_layout_of_the_header():
    text = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    body = re.search(r'typedef struct ss_optim_ext_op \{(.*?)\} ss_optim_ext_op;', text, flags=re.S).group(1)
    names = [n.strip().lstrip('*') for decl in body.split(';') if decl.strip() for n in decl.strip().split(',')]
    names = [n.split()[-1].lstrip('*') for n in names]
    assert names == [n for n, _ in _capi.SSOptimExtOp._fields_]


@pytest.mark.parametrize('name', sorted(CALLS))
def test_null_wrong_kind_and_unbound_engines_are_refused_in_that_order(name):
    lib = _capi.lib()
    fn = getattr(lib, name)
    for args in (ARGS[name], BAD_ARGS[name]):                 # bad arguments as well: the engine is what is reported
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


def _op(**kw):
    o = _capi.SSOptimExtOp()
    base = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, ema=0x5000, state=0x6000, lo=0, hi=64, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=0,
                grad_scale=1.0, clip_coef=0.0, weight_decay=0.01, ema_decay=0.999, mode=0)
    base.update(kw)
    for k, v in base.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize('kw,why', [
    (dict(p=None), 'null pointer'), (dict(state=None), 'null pointer'), (dict(g=None), 'needs g, m and v'), (dict(m=None), 'needs g, m and v'),
    (dict(mode=1, ema=None), 'need ema'), (dict(mode=2, ema=None), 'need ema'), (dict(mode=3), 'mode must be'), (dict(mode=-1), 'mode must be'),
    (dict(lo=2), 'multiples of 4'), (dict(hi=66), 'multiples of 4'), (dict(lo=8, hi=4), 'multiples of 4'), (dict(lo=-4), 'multiples of 4'),
    (dict(p=0x1004), '16-byte aligned'), (dict(ema=0x5008), '16-byte aligned'), (dict(state=0x6010), '256-byte aligned'),
    (dict(weight_decay=-0.1), 'weight_decay must be'), (dict(weight_decay=float('nan')), 'weight_decay must be'), (dict(ema_decay=1.0), 'ema_decay in [0, 1)'),
    (dict(ema_decay=-0.1), 'ema_decay in [0, 1)'), (dict(n_runs=97), 'n_runs in 0 .. 96'), (dict(n_runs=2), 'n_runs in 0 .. 96'),
])
def test_the_kernel_hook_refuses_before_it_enqueues(kw, why):
    lib = _capi.lib()
    assert lib.ss_op_optim_ext(C.byref(_op(**kw)), None) != 0
    assert _err(lib).startswith('ss_op_optim_ext: ') and why in _err(lib), _err(lib)
    assert lib.ss_op_optim_ext(None, None) != 0 and 'null pointer' in _err(lib)


def _runs(kind, hp=None):
    lib = _capi.lib()
    hps = _capi.hparams_struct(hp or HP.default_hparams())
    st, ln, dc = (C.c_long * 128)(), (C.c_int * 128)(), (C.c_int * 128)()
    n = lib.ss_op_wd_runs(kind, C.byref(hps), st, ln, dc, 128)
    assert 0 < n <= 96, _err(lib)
    return [(st[k], ln[k], dc[k]) for k in range(n)]


def _table(kind):
    lib, h = _engine(kind)
    try:
        name = C.create_string_buffer(256)
        off, nd, shp = C.c_long(), C.c_int(), (C.c_long * 3)()
        out = []
        for i in range(lib.ss_num_params(h)):
            assert lib.ss_param_info(h, i, name, 256, C.byref(off), C.byref(nd), shp) == 0
            out.append((name.value.decode(), off.value, tuple(shp[k] for k in range(nd.value))))
        return out, lib.ss_arena_numel(h)
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('kind', [3, 6])
def test_the_decayed_runs_are_the_tensors_with_two_or_more_dimensions(kind):
    table, arena = _table(kind)
    runs = _runs(kind)
    # the runs tile [0, arena) in float4 steps, alternate, and end with the status slot's run
    pos = 0
    for k, (start, length, dec) in enumerate(runs):
        assert start == pos and length > 0 and start % 4 == 0 and length % 4 == 0 and dec in (0, 1)
        assert k == 0 or dec != runs[k - 1][2], 'neighbouring runs of one class were not merged'
        pos += length
    assert pos == arena and runs[-1][2] == 0
    decayed = np.zeros(arena, bool)
    for start, length, dec in runs:
        decayed[start:start + length] = bool(dec)
    seen = {1: 0, 2: 0, 3: 0}
    for name, off, shape in table:
        k = int(np.prod(shape))
        seen[len(shape)] += 1
        if len(shape) >= 2:
            assert decayed[off:off + k].all(), name
            assert 'weight' in name
        else:
            assert not decayed[off:off + k].any(), name
            assert 'bias' in name or name.endswith('.1.weight'), name         # biases and the GroupNorm affine (gamma is '<block>.1.weight')
    assert seen[1] and seen[2] and seen[3]
    assert not decayed[arena - 4:].any()


def test_interp_only_and_small_caps():
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    st, ln, dc = (C.c_long * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    assert lib.ss_op_wd_runs(0, C.byref(hps), st, ln, dc, 4) < 0 and 'ss_op_wd_runs' in _err(lib)
    assert lib.ss_op_wd_runs(3, C.byref(hps), None, ln, dc, 4) < 0 and 'null pointer' in _err(lib)
    n = lib.ss_op_wd_runs(3, C.byref(hps), st, ln, dc, 2)          # a cap below the count: the count comes back, cap entries are written
    assert n == len(_runs(3)) and st[2] == 0 and ln[1] > 0


def test_solver_options_from_config_and_environment():
    from speechsplit_amd.solver import optim_ext_options as opt
    assert opt(SimpleNamespace(), {}) == (0.0, 'all', None, False)
    env = {'SS_WEIGHT_DECAY': '0.01', 'SS_WEIGHT_DECAY_WHICH': 'weights', 'SS_EMA_DECAY': '0.999', 'SS_EMA_WARMUP': '1'}
    assert opt(SimpleNamespace(), env) == (0.01, 'weights', 0.999, True)
    # an attribute on the config wins over the environment, None included (as grad_clip)
    cfg = SimpleNamespace(weight_decay=None, weight_decay_which='all', ema_decay=0.5, ema_warmup=False)
    assert opt(cfg, env) == (0.0, 'all', 0.5, False)
    assert opt(SimpleNamespace(weight_decay=0.1), {'SS_EMA_WARMUP': 'off', 'SS_EMA_DECAY': '0'}) == (0.1, 'all', 0.0, False)
    assert opt(SimpleNamespace(), {'SS_WEIGHT_DECAY': '', 'SS_EMA_DECAY': ''}) == (0.0, 'all', None, False)
    for bad in ({'SS_WEIGHT_DECAY': '-1'}, {'SS_WEIGHT_DECAY': 'nan'}, {'SS_WEIGHT_DECAY': 'inf'}, {'SS_WEIGHT_DECAY_WHICH': 'biases'},
                {'SS_EMA_DECAY': '1'}, {'SS_EMA_DECAY': '-0.5'}, {'SS_EMA_DECAY': 'nan'}, {'SS_EMA_WARMUP': 'maybe'}):
        with pytest.raises(ValueError):
            opt(SimpleNamespace(), bad)


def test_engine_methods_exist_with_the_stated_signatures():
    import inspect
    from speechsplit_amd.engine import Engine
    assert list(inspect.signature(Engine.set_weight_decay).parameters) == ['self', 'wd', 'which']
    assert inspect.signature(Engine.set_weight_decay).parameters['which'].default == 'all'
    assert list(inspect.signature(Engine.set_ema).parameters) == ['self', 'decay', 'warmup', 'state']
    for name in ('ema_views', 'ema_stats', 'ema_weights'):
        assert callable(getattr(Engine, name))
    assert Engine.WD_WHICH == {'all': 0, 'weights': 1}
