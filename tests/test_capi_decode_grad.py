"""CPU-only checks of the differentiable decode (ss_*_decode_train / ss_*_decode_backward / ss_adam_step_decoder /
ss_g3_decode_train_step and the test hook ss_op_dec_in_codes_grad): the symbols and their signatures, every refusal the host can reach
without a GPU, and the argument errors of the Python layers.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from speechsplit_amd import _capi, convert, hparams as HP, model
from speechsplit_amd.engine import Engine

_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
SIGNATURES = {
    'ss_g3_decode_train': [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],            # e, codes_x, codes_r, codes_f0, c_trg, B, T, out, stream
    'ss_g3_decode_backward': [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp],             # e, d_out, d_codes_x, d_codes_r, d_codes_f0, dc_trg, flags, stream
    'ss_g6_decode_train': [_vp, _vp, _vp, _i, _i, _vp, _vp],                      # e, codes_r, codes_f0, B, T, out, stream
    'ss_g6_decode_backward': [_vp, _vp, _vp, _vp, _i, _vp],                       # e, d_out, d_codes_r, d_codes_f0, flags, stream
    'ss_adam_step_decoder': [_vp, _f, _vp],                                       # e, grad_scale, stream
    # e, codes_x, codes_r, codes_f0, c_trg, target_mel, B, T, grad_scale, flags, loss, dc_trg, stream
    'ss_g3_decode_train_step': [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp],
    'ss_op_dec_in_codes_grad': [C.POINTER(_capi.SSCodeSrc), _i, _vp, _i, _i, _i, _i, _vp],      # src, nsrc, d_in, ld, B, T, f, stream
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


def test_header_declares_the_calls_and_states_the_contract():
    text = open(HEADER).read()
    for name in SIGNATURES:
        assert re.search(r'\bint ' + name + r'\(', text), name
    for phrase in ('differentiable decode', 'NOT summed over the batch', 'SS_PROF_WGRAD', 'exact zeros', 'the last forward was a decode',
                   'keeps its bits', 'T > max_frames included', 'without atomics'):
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


def calls(lib, g3, g6, B=2, T=192, p=P, flags=0):
    """the engine calls on the engines of their own kind; p: every pointer"""
    return {
        'ss_g3_decode_train': lambda e=g3: lib.ss_g3_decode_train(e, p, p, p, p, B, T, p, None),
        'ss_g3_decode_backward': lambda e=g3: lib.ss_g3_decode_backward(e, p, p, p, p, p, flags, None),
        'ss_g6_decode_train': lambda e=g6: lib.ss_g6_decode_train(e, p, p, B, T, p, None),
        'ss_g6_decode_backward': lambda e=g6: lib.ss_g6_decode_backward(e, p, p, p, flags, None),
        'ss_g3_decode_train_step': lambda e=g3: lib.ss_g3_decode_train_step(e, p, p, p, p, p, B, T, 1.0, flags, p, p, None),
    }


def test_unbound_engine_is_refused_by_name(engines):
    lib, g3, g6 = engines
    for name, call in calls(lib, g3, g6).items():
        assert call() != 0, name
        assert name in err(lib) and 'not bound' in err(lib), (name, err(lib))
    assert lib.ss_adam_step_decoder(g3, 1.0, None) != 0
    assert 'ss_adam_step_decoder' in err(lib) and 'not bound' in err(lib), err(lib)


def test_wrong_engine_kind_and_null_engine_are_refused_by_name(engines):
    lib, g3, g6 = engines
    for name, call in calls(lib, g3, g6).items():
        assert call(g6 if 'g3' in name else g3) != 0, name
        assert name in err(lib) and ('Generator_3' if 'g3' in name else 'Generator_6') in err(lib), (name, err(lib))
        assert call(None) != 0, name
        assert name in err(lib) and 'null engine' in err(lib), (name, err(lib))
    assert lib.ss_adam_step_decoder(None, 1.0, None) != 0
    assert 'ss_adam_step_decoder' in err(lib) and 'null engine' in err(lib), err(lib)


def test_kind_is_checked_before_the_binding_and_the_pointers(engines):
    """the order of the refusals is that of the code calls: kind, binding, pointers, shape"""
    lib, g3, g6 = engines
    assert lib.ss_g3_decode_train(g6, None, None, None, None, 0, 0, None, None) != 0
    assert 'Generator_3' in err(lib)
    assert lib.ss_g6_decode_backward(g3, None, None, None, 255, None) != 0
    assert 'Generator_6' in err(lib)


def test_the_engines_stay_usable_after_the_refusals(engines):
    lib, g3, g6 = engines
    for call in calls(lib, g3, g6).values():
        call()
    assert lib.ss_num_params(g3) > 0 and lib.ss_grad_split(g3) > 0 and lib.ss_grad_split(g3) % 4 == 0
    assert lib.ss_grad_split(g6) > 0 and lib.ss_grad_split(g6) % 4 == 0


def test_the_kernel_hook_refuses_bad_descriptors():
    """ss_op_dec_in_codes_grad needs no engine: its refusals are the neighbours' (a null pointer, counts, T % freq, columns beyond ld, the
    compact form with another freq), each before anything is launched"""
    lib = _capi.lib()

    def run(src, nsrc, d_in, ld, B, T, f):
        arr = (_capi.SSCodeSrc * max(len(src), 1))(*[_capi.SSCodeSrc(None, d, H, fr, col, l) for d, H, fr, col, l in src])
        return lib.ss_op_dec_in_codes_grad(arr, nsrc, d_in, ld, B, T, f, None)
    ok = (16, 8, 8, 0, 16)             # d_o, H, freq, col, ld_i
    cases = [
        ('null d_in', ([ok], 1, None, 64, 1, 8, 0), 'null pointer'),
        ('null dst', ([(None, 8, 8, 0, 16)], 1, P, 64, 1, 8, 0), 'slab pointer is null'),
        ('no source', ([ok], 0, P, 64, 1, 8, 0), 'number of sources'),
        ('four sources', ([ok] * 4, 4, P, 64, 1, 8, 0), 'number of sources'),
        ('B', ([ok], 1, P, 64, 0, 8, 0), 'B >= 1'),
        ('T % freq', ([ok], 1, P, 64, 1, 12, 0), 'multiple'),
        ('columns', ([(16, 8, 8, 56, 16)], 1, P, 64, 1, 8, 0), 'beyond ld'),
        ('ld_i', ([(16, 8, 8, 0, 8)], 1, P, 64, 1, 8, 0), 'below 2 H'),
        ('f', ([ok], 1, P, 64, 1, 8, 3), 'divisor'),
        ('compact freq', ([(16, 8, 4, 0, 16)], 1, P, 64, 1, 8, 8), 'freq == f'),
    ]
    for tag, args, phrase in cases:
        assert run(*args) != 0, tag
        assert 'ss_op_dec_in_codes_grad' in err(lib) and phrase in err(lib), (tag, err(lib))


def test_python_surface_exists():
    for name in ('g3_decode_train', 'g3_decode_backward', 'g3_decode_train_step', 'g6_decode_train', 'g6_decode_backward', 'adam_step_decoder'):
        assert callable(getattr(Engine, name)), name
    assert list(inspect.signature(model.Generator_3.decode_grad).parameters)[1:] == ['codes_x', 'codes_2', 'codes_f0', 'c_trg']
    assert list(inspect.signature(model.Generator_6.decode_grad).parameters)[1:] == ['codes_2', 'codes_f0']
    sig = inspect.signature(convert.adapt_speaker)
    assert list(sig.parameters)[:6] == ['G', 'entries', 'steps', 'lr', 'train_decoder', 'emb0']
    assert sig.parameters['lr'].default == 1e-4 and sig.parameters['train_decoder'].default is True and sig.parameters['emb0'].default is None
    import dropin.convert
    assert dropin.convert.adapt_speaker is convert.adapt_speaker


def test_decode_and_encode_keep_their_refusals_and_decode_grad_needs_a_gpu():
    hp = HP.default_hparams()
    G, P6 = model.Generator_3(hp), model.Generator_6(hp)
    codes = torch.zeros(1, 1, 16), torch.zeros(1, 1, 2), torch.zeros(1, 1, 64), torch.zeros(1, hp.dim_spk_emb)
    with pytest.raises(RuntimeError, match='eval-mode only'):
        G.decode(*codes)                                         # a fresh module is in training mode: decode still refuses it ...
    with pytest.raises(RuntimeError, match='ROCm GPU only'):
        G.decode_grad(*codes)                                    # ... decode_grad does not, and reaches the device check
    G.eval()
    with pytest.raises(RuntimeError, match='not autograd-connected'):
        G.decode(codes[0], codes[1], codes[2], codes[3].clone().requires_grad_())
    with pytest.raises(RuntimeError, match='ROCm GPU only'):
        G.decode_grad(codes[0], codes[1], codes[2], codes[3].clone().requires_grad_())
    with pytest.raises(RuntimeError, match='ROCm GPU only'):
        P6.decode_grad(codes[1], codes[2])
    assert [n for n in G._dec_names()] == [n for n in G._names if n.startswith('decoder.')] and len(G._dec_names()) == 26
    assert len(P6._dec_names()) == 18


class _Shapes(Engine):
    """the argument checks of the Engine methods without a device: every check below raises before the library is called"""

    def __init__(self, kind):
        self.kind, self.hp, self.device = kind, HP.default_hparams(), torch.device('cpu')
        self.max_frames, self._fwd_bt, self._alloc = 192, None, None

    def __del__(self):
        pass


def test_engine_argument_errors():
    e = _Shapes('G3')
    hp = e.hp
    cx, cr, cf, emb = torch.zeros(2, 2, 16), torch.zeros(2, 2, 2), torch.zeros(2, 2, 64), torch.zeros(2, hp.dim_spk_emb)
    with pytest.raises(ValueError, match='codes_x must have shape'):
        e.g3_decode_train(cx[:, :1], cr, cf, emb)
    with pytest.raises(ValueError, match='codes_r must be'):
        e.g3_decode_train(cx, cr[0], cf, emb)
    with pytest.raises(ValueError, match='c_trg must be'):
        e.g3_decode_train(cx, cr, cf, torch.zeros(3, hp.dim_spk_emb))
    with pytest.raises(ValueError, match='target_mel must have shape'):
        e.g3_decode_train_step(cx, cr, cf, emb, torch.zeros(2, 8, hp.dim_freq))
    with pytest.raises(ValueError, match='want'):
        e.g3_decode_backward(torch.zeros(2, 16, hp.dim_freq), want=('speaker',))
    e6 = _Shapes('G6')
    with pytest.raises(ValueError, match='codes_f0 must have shape'):
        e6.g6_decode_train(cr, cf[:1])
    with pytest.raises(ValueError, match='want'):
        e6.g6_decode_backward(torch.zeros(2, 16, hp.dim_f0), want=('x',))


def test_adapt_speaker_argument_errors():
    with pytest.raises(ValueError, match='at least one entry'):
        convert.adapt_speaker(model.Generator_3(HP.default_hparams()), [], 3)
