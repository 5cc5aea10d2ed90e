"""CPU-only checks of the long-utterance surface: the host-only workspace query ss_plan_bytes, the refusals of ss_set_workspace on an
engine that was never bound, and the padding rule of the conversion.  None of them touches a device."""
import ctypes as C

import pytest

from speechsplit_amd import _capi, hparams as HP


def _engine(kind, B=2, T=192):
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    h = lib.ss_create(kind, C.byref(hps), B, T)
    assert h
    return lib, h


def _err(lib):
    return lib.ss_last_error().decode()


def test_symbols_are_exported_with_their_types():
    lib = _capi.lib()
    assert _capi.SYMBOLS['ss_plan_bytes'] == (C.c_long, [C.c_void_p, C.c_int, C.c_int])
    assert _capi.SYMBOLS['ss_set_workspace'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p])
    assert lib.ss_plan_bytes.restype is C.c_long and lib.ss_set_workspace.restype is C.c_int


@pytest.mark.parametrize('kind', [3, 6])
@pytest.mark.parametrize('maxB,maxT', [(2, 192), (16, 192), (4, 256)])
def test_plan_of_the_create_limits_is_the_workspace(kind, maxB, maxT):
    lib, h = _engine(kind, maxB, maxT)
    try:
        plan = lib.ss_plan_bytes(h, maxB, maxT)
        assert 0 < plan <= lib.ss_workspace_bytes(h)
        assert plan == lib.ss_workspace_bytes(h)
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('kind', [3, 6])
def test_plan_grows_with_batch_times_frames(kind):
    lib, h = _engine(kind, 8, 192)
    try:
        sizes = [lib.ss_plan_bytes(h, B, T) for B, T in [(1, 192), (1, 1024), (1, 4096), (1, 8192)]]
        assert all(s > 0 for s in sizes)
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
        assert lib.ss_plan_bytes(h, 1, 1024) < lib.ss_plan_bytes(h, 7, 1024)
        # the activation plan scales with B * T: twice the frames costs about what twice the batch costs
        d_t = lib.ss_plan_bytes(h, 1, 2048) - lib.ss_plan_bytes(h, 1, 1024)
        d_b = lib.ss_plan_bytes(h, 2, 1024) - lib.ss_plan_bytes(h, 1, 1024)
        assert d_t > 0 and d_b > 0 and 0.9 < d_t / d_b < 1.1
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('B,T,what', [(1, 1020, 'multiple'), (1, 1001, 'multiple'), (1, 8200, 'SS_MAX_EVAL_FRAMES'),
                                      (1, 0, 'frames'), (0, 192, 'batch'), (9, 192, 'batch')])
def test_plan_refuses_invalid_shapes(B, T, what):
    lib, h = _engine(3, 8, 192)
    try:
        assert lib.ss_plan_bytes(h, B, T) == -1
        assert what in _err(lib)
    finally:
        lib.ss_destroy(h)


def test_plan_accepts_the_longest_eval_shape():
    lib, h = _engine(6, 1, 192)
    try:
        assert lib.ss_plan_bytes(h, 1, 8192) > lib.ss_workspace_bytes(h)
    finally:
        lib.ss_destroy(h)


def test_batch16_engine_holds_a_2000_frame_utterance():
    # a 16 x 192 Generator_3 workspace (about 3 100 slab rows) runs a 1 x 2000 conversion without new memory
    lib, h = _engine(3, 16, 192)
    try:
        assert lib.ss_plan_bytes(h, 1, 2000) <= lib.ss_workspace_bytes(h)
        assert lib.ss_plan_bytes(h, 1, 4096) > lib.ss_workspace_bytes(h)
    finally:
        lib.ss_destroy(h)


def test_set_workspace_needs_a_bound_engine():
    lib, h = _engine(3)
    try:
        assert lib.ss_set_workspace(h, C.c_void_p(0x10000), lib.ss_workspace_bytes(h), None) < 0
        assert 'not bound' in _err(lib)
    finally:
        lib.ss_destroy(h)


def test_create_limits_are_unchanged():
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    assert not lib.ss_create(3, C.byref(hps), 2, 264)
    assert 'max_frames <= 256' in _err(lib)


def test_conversion_padding_rule():
    from speechsplit_amd.convert import conversion_frames
    assert conversion_frames((150, 120)) == 192
    assert conversion_frames((192, 192)) == 192
    assert conversion_frames((500, 430)) == 504
    assert conversion_frames((430, 500)) == 504
    assert conversion_frames((193, 10)) == 200
    assert conversion_frames((2000, 64)) == 2000
    assert conversion_frames((300, 20), max_len_pad=320) == 320
