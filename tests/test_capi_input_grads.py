"""CPU-only checks of the input-gradient entry points (ss_g3_backward_inputs / ss_g6_backward_inputs): their argument checks come
first and fail before anything is enqueued, so they run on an engine that was never bound to a device."""
import ctypes as C

import pytest

from speechsplit_amd import _capi, hparams as HP

# non-null stand-ins for device pointers: the calls below must refuse before they touch any of them
FAKE = [C.c_void_p(0x1000 * (i + 1)) for i in range(4)]


def _engine(kind):
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    h = lib.ss_create(kind, C.byref(hps), 2, 192)
    assert h
    return lib, h


def _err(lib):
    return lib.ss_last_error().decode()


def test_symbols_are_declared_with_their_argument_types():
    assert _capi.SYMBOLS['ss_g3_backward_inputs'][1] == [C.c_void_p] * 6
    assert _capi.SYMBOLS['ss_g6_backward_inputs'][1] == [C.c_void_p] * 5
    lib = _capi.lib()
    assert lib.ss_g3_backward_inputs.restype is C.c_int and lib.ss_g6_backward_inputs.restype is C.c_int


@pytest.mark.parametrize('outputs', [(None, None, None), tuple(FAKE[1:4])])
def test_g6_entry_point_refuses_a_generator3_engine(outputs):
    lib, h = _engine(3)
    try:
        assert lib.ss_g6_backward_inputs(h, FAKE[0], outputs[0], outputs[1], None) < 0
        assert 'Generator_3' in _err(lib) and 'ss_g6_backward_inputs' in _err(lib)
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('outputs', [(None, None, None), tuple(FAKE[1:4])])
def test_g3_entry_point_refuses_a_generator6_engine(outputs):
    lib, h = _engine(6)
    try:
        assert lib.ss_g3_backward_inputs(h, FAKE[0], *outputs, None) < 0
        assert 'Generator_6' in _err(lib) and 'ss_g3_backward_inputs' in _err(lib)
    finally:
        lib.ss_destroy(h)


def test_kind_is_checked_before_the_forward():
    # neither engine has run a forward: the message must still be about the kind
    lib, h = _engine(3)
    try:
        assert lib.ss_g6_backward_inputs(h, FAKE[0], FAKE[1], FAKE[2], None) < 0
        assert 'Generator_3' in _err(lib)
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('kind', [3, 6])
def test_backward_inputs_without_a_forward_fail_without_launching(kind):
    lib, h = _engine(kind)
    try:
        if kind == 3:
            rc = lib.ss_g3_backward_inputs(h, FAKE[0], FAKE[1], FAKE[2], FAKE[3], None)
        else:
            rc = lib.ss_g6_backward_inputs(h, FAKE[0], FAKE[1], FAKE[2], None)
        assert rc < 0
        # the engine's own refusal, not a HIP error from an attempted launch or copy (there is no device here)
        assert _err(lib) == 'backward without a preceding forward'
        # all outputs null: the same refusal as the plain backward
        if kind == 3:
            assert lib.ss_g3_backward_inputs(h, FAKE[0], None, None, None, None) < 0
        else:
            assert lib.ss_g6_backward_inputs(h, FAKE[0], None, None, None) < 0
        assert _err(lib) == 'backward without a preceding forward'
    finally:
        lib.ss_destroy(h)


def test_module_asks_only_for_what_autograd_needs():
    from speechsplit_amd import model

    class Ctx:
        needs_input_grad = (False, True, False, True, False)
    assert model._wanted(Ctx, 1, ('x_f0', 'x_org', 'c_trg')) == ('x_f0', 'c_trg')
    Ctx.needs_input_grad = (False,) * 5
    assert model._wanted(Ctx, 1, ('x_f0', 'x_org', 'c_trg')) == ()
