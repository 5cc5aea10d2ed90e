"""CPU-only checks of the gradient-clipping entry points (ss_set_grad_clip / ss_grad_norm / ss_grad_clip_stats): declarations, and the
argument checks that come before anything is enqueued, on an engine that was never bound to a device."""
import ctypes as C
import os
import re

import pytest

from speechsplit_amd import _capi, hparams as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)       # non-null stand-in for a device pointer: the calls below refuse before they touch it


def _engine(kind):
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    h = lib.ss_create(kind, C.byref(hps), 2, 192)
    assert h
    return lib, h


def _err(lib):
    return lib.ss_last_error().decode()


def test_symbols_are_declared_with_the_stated_signatures():
    vp, f, i = C.c_void_p, C.c_float, C.c_int
    assert _capi.SYMBOLS['ss_set_grad_clip'] == (i, [vp, f, vp])
    assert _capi.SYMBOLS['ss_grad_norm'] == (i, [vp, f, vp, vp])
    assert _capi.SYMBOLS['ss_grad_clip_stats'] == (i, [vp, vp, vp])
    lib = _capi.lib()
    for name in ('ss_set_grad_clip', 'ss_grad_norm', 'ss_grad_clip_stats'):
        assert getattr(lib, name).restype is C.c_int


def test_header_declares_the_three_calls():
    text = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read())
    assert 'int ss_set_grad_clip(ss_engine* e, float max_norm, void* stream);' in text
    assert 'int ss_grad_norm(ss_engine* e, float grad_scale, float* norm_dev, void* stream);' in text
    assert 'int ss_grad_clip_stats(ss_engine* e, float* out4_dev, void* stream);' in text


def test_abi_version_is_unchanged():
    assert _capi.lib().ss_abi_version() == 2


@pytest.mark.parametrize('kind', [3, 6])
@pytest.mark.parametrize('bad', [-1.0, -0.0001, float('-inf'), float('nan')])
def test_negative_and_nan_max_norm_are_refused(kind, bad):
    lib, h = _engine(kind)
    try:
        assert lib.ss_set_grad_clip(h, bad, None) < 0
        assert 'ss_set_grad_clip' in _err(lib) and 'max_norm' in _err(lib)
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('kind', [3, 6])
@pytest.mark.parametrize('max_norm', [0.0, 1.0, float('inf')])
def test_set_grad_clip_on_an_unbound_engine_is_refused_with_a_message(kind, max_norm):
    lib, h = _engine(kind)
    try:
        assert lib.ss_set_grad_clip(h, max_norm, None) < 0
        # the engine's own refusal, not a HIP error from an attempted launch (there is no device here)
        assert _err(lib) == 'ss_set_grad_clip: engine is not bound (call ss_bind first)'
    finally:
        lib.ss_destroy(h)


def test_norm_and_stats_refuse_an_unbound_engine_and_null_outputs():
    lib, h = _engine(3)
    try:
        assert lib.ss_grad_norm(h, 1.0, FAKE, None) < 0
        assert 'ss_grad_norm' in _err(lib) and 'not bound' in _err(lib)
        assert lib.ss_grad_clip_stats(h, FAKE, None) < 0
        assert 'ss_grad_clip_stats' in _err(lib) and 'not bound' in _err(lib)
        assert lib.ss_grad_norm(h, 1.0, None, None) < 0 and 'null' in _err(lib)
        assert lib.ss_grad_clip_stats(h, None, None) < 0 and 'null' in _err(lib)
    finally:
        lib.ss_destroy(h)
