"""CPU-only checks of the codes interface (ss_g3_encode / ss_g3_decode / ss_g6_encode / ss_g6_decode): the symbols and their signatures,
every refusal the host can reach without a GPU, and the argument errors of the Python layers.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

from speechsplit_amd import _capi, convert, hparams as HP, model
from speechsplit_amd.engine import Engine

_vp, _i = C.c_void_p, C.c_int
SIGNATURES = {
    'ss_g3_encode': [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp],      # e, x_f0, x_org, len, B, T, codes_x, codes_r, codes_f0, stream
    'ss_g3_decode': [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],      # e, codes_x, codes_r, codes_f0, c_trg, len, B, T, out, stream
    'ss_g6_encode': [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],           # e, x_org, f0_trg, len, B, T, codes_r, codes_f0, stream
    'ss_g6_decode': [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp],                # e, codes_r, codes_f0, len, B, T, out, stream
}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'speechsplit_amd.h')
P = C.c_void_p(16)                 # a non-null pointer that is never dereferenced: every call below is refused before anything is enqueued


def err(lib):
    return lib.ss_last_error().decode()


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, args in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        res, got = _capi.SYMBOLS[name]
        assert res is _i and list(got) == args, name
        fn = getattr(lib, name)
        assert fn.restype is _i and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2                     # additive change


def test_header_declares_the_four_calls_and_states_the_contract():
    text = open(HEADER).read()
    for name in SIGNATURES:
        assert re.search(r'\bint ' + name + r'\(ss_engine\* e,', text), name
    for phrase in ('codes: the encoders alone', 'bit-identical', 'SS_PROF_REC_FWD', 'SS_PROF_ENC_REC', 'NaN included', 'all NULL is an error'):
        assert phrase in text, phrase


@pytest.fixture(scope='module')
def engines():
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    g3, g6 = lib.ss_create(3, C.byref(hps), 2, 192), lib.ss_create(6, C.byref(hps), 2, 192)
    assert g3 and g6
    yield lib, g3, g6
    lib.ss_destroy(g3)
    lib.ss_destroy(g6)


def calls(lib, g3, g6, B=2, T=192, p=P, o=P):
    """the four calls on the engines of their own kind; p: every input pointer, o: every output pointer"""
    return {
        'ss_g3_encode': lambda e=g3: lib.ss_g3_encode(e, p, p, None, B, T, o, o, o, None),
        'ss_g3_decode': lambda e=g3: lib.ss_g3_decode(e, p, p, p, p, None, B, T, o, None),
        'ss_g6_encode': lambda e=g6: lib.ss_g6_encode(e, p, p, None, B, T, o, o, None),
        'ss_g6_decode': lambda e=g6: lib.ss_g6_decode(e, p, p, None, B, T, o, None),
    }


def test_unbound_engine_is_refused_by_name(engines):
    lib, g3, g6 = engines
    for name, call in calls(lib, g3, g6).items():
        assert call() != 0, name
        assert name in err(lib) and 'not bound' in err(lib), (name, err(lib))


def test_wrong_engine_kind_and_null_engine_are_refused_by_name(engines):
    lib, g3, g6 = engines
    for name, call in calls(lib, g3, g6).items():
        assert call(g6 if 'g3' in name else g3) != 0, name
        assert name in err(lib) and ('Generator_3' if 'g3' in name else 'Generator_6') in err(lib), (name, err(lib))
        assert call(None) != 0, name
        assert name in err(lib) and 'null engine' in err(lib), (name, err(lib))


def test_kind_is_checked_before_the_binding(engines):
    """the order of the refusals: kind, binding, pointers, shape -- an unbound engine of the wrong kind reports the kind"""
    lib, g3, g6 = engines
    assert lib.ss_g3_encode(g6, None, None, None, 0, 0, None, None, None, None) != 0
    assert 'Generator_3' in err(lib)
    assert lib.ss_g6_decode(g3, None, None, None, 0, 0, None, None) != 0
    assert 'Generator_6' in err(lib)


def test_engine_methods_exist_with_lengths():
    import inspect
    for name in ('g3_encode', 'g3_decode', 'g6_encode', 'g6_decode'):
        sig = inspect.signature(getattr(Engine, name))
        assert sig.parameters['lengths'].default is None, name
    for cls in (model.Generator_3, model.Generator_6):
        for name in ('encode', 'decode'):
            assert inspect.signature(getattr(cls, name)).parameters['lengths'].default is None, (cls, name)
    assert list(inspect.signature(model.Generator_3.encode).parameters)[1:3] == ['x_f0', 'x_org']
    assert list(inspect.signature(model.Generator_3.decode).parameters)[1:5] == ['codes_x', 'codes_2', 'codes_f0', 'c_trg']
    assert callable(convert.demo_conversion_codes) and callable(convert.convert_speakers)
    assert list(inspect.signature(convert.demo_conversion_codes).parameters) == list(inspect.signature(convert.demo_conversion).parameters)


def test_modules_refuse_training_mode_grad_inputs_and_the_cpu():
    hp = HP.default_hparams()
    G, P6 = model.Generator_3(hp), model.Generator_6(hp)
    x_f0, x_org = torch.zeros(1, 8, hp.dim_freq + hp.dim_f0), torch.zeros(1, 8, hp.dim_freq)
    with pytest.raises(RuntimeError, match='eval-mode only'):
        G.encode(x_f0, x_org)                                    # a fresh module is in training mode
    with pytest.raises(RuntimeError, match='eval-mode only'):
        P6.decode(torch.zeros(1, 1, 2), torch.zeros(1, 1, 64))
    G.eval(), P6.eval()
    with pytest.raises(RuntimeError, match='not autograd-connected'):
        G.encode(x_f0, x_org.clone().requires_grad_())
    with pytest.raises(RuntimeError, match='not autograd-connected'):
        G.decode(torch.zeros(1, 1, 16), torch.zeros(1, 1, 2), torch.zeros(1, 1, 64), torch.zeros(1, hp.dim_spk_emb).requires_grad_())
    with torch.no_grad():                                        # grad disabled: the same input passes that check and reaches the next
        with pytest.raises(RuntimeError, match='ROCm GPU only'):
            G.encode(x_f0, x_org.clone().requires_grad_())
    with pytest.raises(RuntimeError, match='ROCm GPU only'):
        P6.encode(x_org, torch.zeros(1, 8, hp.dim_f0))


class _Shapes(Engine):
    """the argument checks of Engine.g*_encode / g*_decode without a device: every check below raises before the library is called"""

    def __init__(self, kind):
        self.kind, self.hp, self.device = kind, HP.default_hparams(), torch.device('cpu')
        self.max_frames, self._fwd_bt, self._alloc = 192, None, None

    def __del__(self):
        pass


def test_engine_argument_errors():
    e = _Shapes('G3')
    hp = e.hp
    assert e.code_shapes(2, 16) == {'x': (2, 2, 16), 'r': (2, 2, 2), 'f0': (2, 2, 64)}
    assert _Shapes('G6').code_shapes(1, 8) == {'r': (1, 1, 2), 'f0': (1, 1, 64)}
    x_f0, x_org = torch.zeros(2, 16, hp.dim_freq + hp.dim_f0), torch.zeros(2, 16, hp.dim_freq)
    with pytest.raises(ValueError, match='want'):
        e.g3_encode(x_f0, x_org, want=())
    with pytest.raises(ValueError, match='want'):
        e.g3_encode(x_f0, x_org, want=('x', 'speaker'))
    with pytest.raises(ValueError, match='x_f0 must have shape'):
        e.g3_encode(x_f0[:, :8], x_org)
    with pytest.raises(ValueError, match='multiple'):
        e.g3_encode(x_f0, x_org, lengths=[16, 12])
    cx, cr, cf, emb = torch.zeros(2, 2, 16), torch.zeros(2, 2, 2), torch.zeros(2, 2, 64), torch.zeros(2, hp.dim_spk_emb)
    with pytest.raises(ValueError, match='codes_x must have shape'):
        e.g3_decode(cx[:, :1], cr, cf, emb)
    with pytest.raises(ValueError, match='codes_f0 must have shape'):
        e.g3_decode(cx, cr, cf[..., :32], emb)
    with pytest.raises(ValueError, match='codes_r must be'):
        e.g3_decode(cx, cr[0], cf, emb)
    with pytest.raises(ValueError, match='c_trg must be'):
        e.g3_decode(cx, cr, cf, emb[:, :80])
    with pytest.raises(ValueError, match='c_trg must be'):
        e.g3_decode(cx, cr, cf, torch.zeros(3, hp.dim_spk_emb))
    with pytest.raises(ValueError, match='outside'):
        e.g3_decode(cx, cr, cf, emb, lengths=[16, 24])
    e6 = _Shapes('G6')
    with pytest.raises(ValueError, match='f0_trg must have shape'):
        e6.g6_encode(x_org, torch.zeros(2, 16, 80))
    with pytest.raises(ValueError, match='codes_f0 must have shape'):
        e6.g6_decode(cr, cf[:1])
    with pytest.raises(ValueError, match='want'):
        e6.g6_encode(x_org, torch.zeros(2, 16, hp.dim_f0), want=('x',))
