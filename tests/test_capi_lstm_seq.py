"""CPU-only checks of the persistent-recurrence test hooks ss_op_lstm_seq_fwd / ss_op_lstm_seq_bwd: the C symbols and their signatures, the
header's declarations and the contract text of every option, and every refusal -- each is made before anything is enqueued, so fake
non-null device pointers are enough and no device is needed.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re

from speechsplit_amd import _capi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
SIGNATURES = {
    # gates, whh_f, whh_b, out, csave, scratch, floats, xc, xf, out_img, img_bf16, hi_only, len, B, T, H, stream
    'ss_op_lstm_seq_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _vp]),
    # gates, whh_f, whh_b, d_out, csave, scratch, floats, amax, gbias_f, gbias_b, dgs, xf, dimg, img_only, hi_only, B, T, H, stream
    'ss_op_lstm_seq_bwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    # the hooks they stand beside keep their signatures
    'ss_op_lstm_fwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp]),
    'ss_op_lstm_bwd': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i, _vp]),
}
PTR = C.c_void_p(1 << 20)                                   # fake, non-null, 256-byte aligned; never dereferenced
B, T, H = 5, 40, 256


def scratch_floats(B, H, backward):
    """The header's formulas, in floats."""
    nbt = (B + 15) // 16
    return ((4 * nbt * (H // 16) ** 2 if backward else 8 * nbt * (H // 32)) * 1024 + 8192) // 4


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_declares_them_and_states_every_option():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('int ss_op_lstm_seq_fwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, float* out_dev, float* csave_dev, '
                 'float* scratch_dev, long scratch_floats, const float* xc_dev, int xf, float* out_img_dev, int img_bf16, int hi_only, '
                 'const int* len_dev, int B, int T, int H, void* stream);',
                 'int ss_op_lstm_seq_bwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, const float* d_out_dev, '
                 'const float* csave_dev, float* scratch_dev, long scratch_floats, float* amax_dev, float* gbias_f_dev, float* gbias_b_dev, '
                 'float* dgs_dev, int xf, float* dimg_dev, int img_only, int hi_only, int B, int T, int H, void* stream);',
                 'int ss_op_lstm_fwd(float* gates_dev, const float* whh_f_dev, const float* whh_b_dev, float* out_dev, float* csave_dev, '
                 'float* scratch_dev, long scratch_floats, int B, int T, int H, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_lstm_bwd(') < raw.index(' ss_op_lstm_seq_fwd(') < raw.index(' ss_op_lstm_seq_bwd(') < raw.index(' ss_op_lstm_wgrad(')
    whole = re.sub(r'[\s*]+', ' ', raw)
    for phrase in ('No fall-back', 'refused before anything is enqueued', '8 ceil(B/16) (H/32) 1024 + 8192 bytes (forward)',
                   '4 ceil(B/16) (H/16)^2 1024 + 8192 bytes (backward)', 'which the hooks zero', 'xf >= 1, T % xf == 0', 'the gates slab is only written',
                   'base 32-byte aligned', 'base 8-byte aligned', 'round to nearest even', 'high fp16 pieces', 'zeros for t >= len[b]',
                   'it only ever grows: zero it first', 'ADDED to both halves', 'every element overwritten', 'forward direction: t descending',
                   'img_only != 0 (needs dimg_dev)', "keeps the forward's activated gates"):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def _fwd(**k):
    args = (('gates', PTR), ('whh_f', PTR), ('whh_b', PTR), ('out', PTR), ('csave', PTR), ('scratch', PTR), ('floats', scratch_floats(B, H, False)),
            ('xc', None), ('xf', 0), ('out_img', None), ('img_bf16', 0), ('hi_only', 0), ('len', None), ('B', B), ('T', T), ('H', H), ('stream', None))
    assert set(k) <= {a for a, _ in args}
    return _capi.lib().ss_op_lstm_seq_fwd(*[k.get(a, d) for a, d in args])


def _bwd(**k):
    args = (('gates', PTR), ('whh_f', PTR), ('whh_b', PTR), ('d_out', PTR), ('csave', PTR), ('scratch', PTR), ('floats', scratch_floats(B, H, True)),
            ('amax', None), ('gbias_f', None), ('gbias_b', None), ('dgs', None), ('xf', 0), ('dimg', None), ('img_only', 0), ('hi_only', 0),
            ('B', B), ('T', T), ('H', H), ('stream', None))
    assert set(k) <= {a for a, _ in args}
    return _capi.lib().ss_op_lstm_seq_bwd(*[k.get(a, d) for a, d in args])


def test_forward_refusals_each_with_its_own_text():
    for name in ('gates', 'whh_f', 'whh_b', 'out', 'csave', 'scratch'):
        _refused(_fwd(**{name: None}), 'ss_op_lstm_seq_fwd: null pointer')
    for shape in (dict(B=0), dict(T=0), dict(T=-4)):
        _refused(_fwd(**shape), 'ss_op_lstm_seq_fwd: empty shape')
    for xf in (0, -1, 3, 16, 41):                           # T = 40
        _refused(_fwd(xc=PTR, xf=xf), 'ss_op_lstm_seq_fwd: xc_dev needs xf >= 1 and T % xf == 0')
    for off in (4, 8, 16):
        _refused(_fwd(out_img=C.c_void_p((1 << 20) + off)), 'out_img_dev (format v2) is not 32-byte aligned')
    for off in (2, 4, 6):
        _refused(_fwd(out_img=C.c_void_p((1 << 20) + off), img_bf16=1), 'out_img_dev (bf16) is not 8-byte aligned')
    _refused(_fwd(gates=C.c_void_p((1 << 20) + 4)), 'not 16-byte aligned')
    _refused(_fwd(xc=C.c_void_p((1 << 20) + 8), xf=8), 'not 16-byte aligned')
    _refused(_fwd(floats=scratch_floats(B, H, False) - 1), 'ss_op_lstm_seq_fwd: scratch too small')
    _refused(_fwd(B=17, floats=scratch_floats(16, H, False)), 'ss_op_lstm_seq_fwd: scratch too small')        # a second tile doubles it
    _refused(_fwd(floats=-1), 'scratch too small')
    # a shape lstm_seq_supported rejects, every other argument in order (no fall-back to the per-step kernels)
    for Hq in (64, 128, 32, 384):
        _refused(_fwd(H=Hq, floats=1 << 30), 'ss_op_lstm_seq_fwd: shape not supported by the persistent kernels')
    _refused(_fwd(B=16 * 9, floats=1 << 30), 'shape not supported')                                           # 2 * 9 * 16 = 288 workgroups > 256


def test_backward_refusals_each_with_its_own_text():
    for name in ('gates', 'whh_f', 'whh_b', 'd_out', 'csave', 'scratch'):
        _refused(_bwd(**{name: None}), 'ss_op_lstm_seq_bwd: null pointer')
    for shape in (dict(B=0), dict(T=0)):
        _refused(_bwd(**shape), 'ss_op_lstm_seq_bwd: empty shape')
    for xf in (0, -1, 3, 16, 41):
        _refused(_bwd(dgs=PTR, xf=xf), 'ss_op_lstm_seq_bwd: dgs_dev needs xf >= 1 and T % xf == 0')
    _refused(_bwd(img_only=1), 'ss_op_lstm_seq_bwd: img_only without dimg_dev')
    _refused(_bwd(img_only=1, amax=PTR, gbias_f=PTR, gbias_b=PTR), 'img_only without dimg_dev')
    for off in (2, 4, 6):
        _refused(_bwd(dimg=C.c_void_p((1 << 20) + off)), 'dimg_dev (bf16) is not 8-byte aligned')
        _refused(_bwd(dimg=C.c_void_p((1 << 20) + off), img_only=1), 'dimg_dev (bf16) is not 8-byte aligned')
    _refused(_bwd(d_out=C.c_void_p((1 << 20) + 4)), 'not 16-byte aligned')
    _refused(_bwd(amax=C.c_void_p((1 << 20) + 2)), 'not 16-byte aligned')
    _refused(_bwd(floats=scratch_floats(B, H, True) - 1), 'ss_op_lstm_seq_bwd: scratch too small')
    _refused(_bwd(floats=scratch_floats(B, H, False)), 'ss_op_lstm_seq_bwd: scratch too small')               # the forward's size does not do
    for Hq in (64, 128, 32, 384):
        _refused(_bwd(H=Hq, floats=1 << 30), 'ss_op_lstm_seq_bwd: shape not supported by the persistent kernels')


def test_python_hook_signature():
    sig = inspect.signature(engine.seq_recurrence)
    assert list(sig.parameters) == ['pre_or_xc', 'w_hh', 'd_out', 'xf', 'out_img', 'hi_only', 'lengths', 'amax0', 'gbias0', 'dgs', 'dimg', 'img_only']
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, 0, None, False, None, None, None, False, False, False]
    sig = inspect.signature(engine.blstm_recurrence)        # unchanged
    assert list(sig.parameters) == ['gates', 'w_hh', 'd_out', 'lengths', 'place']
