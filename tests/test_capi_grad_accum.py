"""CPU-only checks of the gradient-accumulation surface of the C ABI (SS_STEP_ACCUMULATE, ss_grad_accum_count) and of its Python binding.
No kernel is launched here; what accumulation computes is tests/test_gpu_grad_accum.py's business."""
import ctypes as C
import inspect
import os
import re

from speechsplit_amd import _capi, hparams as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()


def step_flags():
    return {n: int(v) for n, v in re.findall(r'#define\s+(SS_STEP_[A-Z_]+)\s+(\d+)', HEADER)}


def test_header_defines_the_flag_as_the_free_bit():
    flags = step_flags()
    assert flags['SS_STEP_ACCUMULATE'] == 8
    # one bit each, none shared: the flag composes with every other
    assert sorted(flags.values()) == [1, 2, 4, 8, 16]
    assert flags == {'SS_STEP_NO_ADAM': 1, 'SS_STEP_SPLIT_BACKWARD': 2, 'SS_STEP_SPLIT_NO_JOIN': 4, 'SS_STEP_ACCUMULATE': 8, 'SS_STEP_BUCKET': 16}


def test_header_states_the_semantics():
    text = ' '.join(re.sub(r'\n \*', ' ', HEADER).split())          # comment lines joined, their leading ' *' dropped
    for phrase in ('plain SUM', 'mean of the micro-batches\' means', 'ONE precision mode', 'takes no accumulate flag of its own',
                   '1 / (world * ss_grad_accum_count)', 'adds to it'):
        assert phrase in text, phrase
    assert re.search(r'long\s+ss_grad_accum_count\s*\(\s*const\s+ss_engine\s*\*\s*e\s*\)\s*;', HEADER)


def test_library_exports_the_count_and_keeps_the_abi_version():
    lib = _capi.lib()
    assert 'ss_grad_accum_count' in _capi.SYMBOLS
    assert hasattr(lib, 'ss_grad_accum_count')
    assert lib.ss_grad_accum_count.restype is C.c_long
    assert lib.ss_abi_version() == 2


def test_count_is_zero_before_anything_ran():
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    for kind in (3, 6):
        h = lib.ss_create(kind, C.byref(hps), 2, 192)
        assert h
        assert lib.ss_grad_accum_count(h) == 0                   # valid on an engine that is not bound: nothing was ever summed
        # an accumulating step on an unbound engine is refused like any other, and counts nothing
        assert lib.ss_g3_train_step(h, None, None, None, None, None, None, 2, 192, 1.0, 8, None, None) != 0
        assert lib.ss_grad_accum_count(h) == 0
        lib.ss_destroy(h)
    assert lib.ss_grad_accum_count(None) == 0


def test_python_surface_takes_accumulate():
    from speechsplit_amd.engine import Engine
    for name in ('g3_train_step', 'g6_train_step', 'dp_train_step_native', 'g6_dp_train_step_native', 'dp_train_step', 'dp_g6_train_step'):
        p = inspect.signature(getattr(Engine, name)).parameters
        assert 'accumulate' in p and p['accumulate'].default is False, name
    assert isinstance(Engine.grad_accum_count, property)
    assert 'accumulate' not in inspect.signature(Engine.train_finish).parameters


def test_solver_reads_accum_steps(monkeypatch):
    """config.accum_steps, or SS_ACCUM_STEPS for a config without the attribute (the unchanged main.py), default 1.  The constructor reads it
    before it asks for a GPU; here it is told there is none, so it stops right behind."""
    import pytest
    import torch
    from types import SimpleNamespace
    from speechsplit_amd import solver
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    base = dict(num_iters=1, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None)

    def accum_steps_of(cfg):
        s = solver.Solver.__new__(solver.Solver)
        with pytest.raises(RuntimeError, match='ROCm GPU'):
            solver.Solver.__init__(s, None, cfg, HP.default_hparams())
        return s.accum_steps

    monkeypatch.delenv('SS_ACCUM_STEPS', raising=False)
    assert accum_steps_of(SimpleNamespace(**base)) == 1
    assert accum_steps_of(SimpleNamespace(accum_steps=4, **base)) == 4
    monkeypatch.setenv('SS_ACCUM_STEPS', '3')
    assert accum_steps_of(SimpleNamespace(**base)) == 3
    assert accum_steps_of(SimpleNamespace(accum_steps=2, **base)) == 2     # the attribute wins over the environment
    s = solver.Solver.__new__(solver.Solver)
    with pytest.raises(ValueError, match='accum_steps'):
        solver.Solver.__init__(s, None, SimpleNamespace(accum_steps=0, **base), HP.default_hparams())
