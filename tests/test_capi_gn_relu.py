"""CPU-only checks of the GroupNorm + ReLU test hooks ss_op_gn_relu_fwd / _mask / _bwd / _scratch: the C symbols and their signatures, the
header's declarations and contract text, the host-side plan contract of the Python wrappers, and every refusal -- each is made before
anything is enqueued, so fake non-null device pointers are enough and no device is needed.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from speechsplit_amd import _capi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
SIGNATURES = {
    'ss_op_gn_relu_scratch': (_l, [_i, _i, _i]),
    # x, x_ld, x_bs, y, y_ld, y_bs, gamma, beta, stats, len, i0, lam, nrows, P, y_img, img_scale, img_bf16, scratch, bytes, B, T, C, stream
    'ss_op_gn_relu_fwd': (_i, [_vp, _l, _l, _vp, _l, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _l, _i, _i, _i, _vp]),
    # x, x_ld, x_bs, gamma, beta, stats, mask, B, T, C, stream
    'ss_op_gn_relu_mask': (_i, [_vp, _l, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    # x, x_ld, x_bs, dy, dy_ld, dy_bs, gamma, beta, stats, g_gamma, g_beta, g_bias, amax, part, lam, start, P, src, src_ld, src_bs, dy_img, B, T, C, stream
    'ss_op_gn_relu_bwd': (_i, [_vp, _l, _l, _vp, _l, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _l, _l, _vp, _i, _i, _i, _vp]),
    # the hook they stand beside keeps its signature
    'ss_op_conv_block_scratch': (_l, [_i, _i, _i, _i]),
}
BASE = 1 << 20
PTR = C.c_void_p(BASE)                                      # fake, non-null, 256-byte aligned; never dereferenced
B, T, CH, LD = 3, 40, 128, 136


def off(n):
    return C.c_void_p(BASE + n)


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2                        # symbols were only added


def test_header_declares_them_and_states_the_contracts():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('long ss_op_gn_relu_scratch(int B, int T, int C);',
                 'int ss_op_gn_relu_fwd(const float* x_dev, long x_ld, long x_bs, float* y_dev, long y_ld, long y_bs, const float* gamma_dev, '
                 'const float* beta_dev, float* stats_dev, const int* len_dev, const int* i0_dev, const float* lam_dev, const int* nrows_dev, int P, '
                 'float* y_img_dev, const float* img_scale_dev, int img_bf16, void* scratch_dev, long scratch_bytes, int B, int T, int C, void* stream);',
                 'int ss_op_gn_relu_mask(const float* x_dev, long x_ld, long x_bs, const float* gamma_dev, const float* beta_dev, '
                 'const float* stats_dev, float* mask_dev, int B, int T, int C, void* stream);',
                 'int ss_op_gn_relu_bwd(const float* x_dev, long x_ld, long x_bs, float* dy_dev, long dy_ld, long dy_bs, const float* gamma_dev, '
                 'const float* beta_dev, const float* stats_dev, float* g_gamma_dev, float* g_beta_dev, float* g_bias_dev, float* amax_dev, '
                 'float* part_dev, const float* lam_dev, const int* start_dev, int P, const float* src_dev, long src_ld, long src_bs, '
                 'float* dy_img_dev, int B, int T, int C, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_lstm_wgrad(') < raw.index(' ss_op_gn_relu_scratch(') < raw.index(' ss_op_gn_relu_fwd(') < raw.index(' ss_op_gn_relu_mask(') \
        < raw.index(' ss_op_gn_relu_bwd(') < raw.index(' ss_op_split_image(')
    whole = re.sub(r'[\s*]+', ' ', raw)
    for phrase in ('no convolution, no engine, no copy into private slabs', 'Refused before anything is enqueued', 'ld >= C, ld % 4 == 0, bs % 4 == 0',
                   'eps 1e-5 inside the square root', 'biased variance', '2 B (C/16) ceil(T/64) float64 words', 'x rows t >= L are never read',
                   'its stats entries are then NaN', 'never returns success without the image it was asked for', 'act row T reads as zeros',
                   'stats as the plain form\'s, bit for bit', 'base 32-byte aligned', 'base 16-byte aligned', 'round to nearest even',
                   'it only ever grows: zero it first', 'used only under ss_tune("deterministic", 1)', 'dy on entry is NOT read',
                   'dy[t] = sum_{i0[r] == t} (1 - lam[r]) src[r] + sum_{i0[r] == t - 1} lam[r] src[r] over r < nrows', 'PLAN CONTRACT',
                   '0 <= i0[b][r] < T', '0 <= nrows[b] <= P <= 258', 'number of rows r < nrows[b] with i0[b][r] < i', 'ADDED to g_gamma_dev',
                   'The Python wrappers assert this on the host'):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


FWD = (('x', PTR), ('x_ld', LD), ('x_bs', LD * (T + 4)), ('y', PTR), ('y_ld', LD), ('y_bs', LD * (T + 4)), ('gamma', PTR), ('beta', PTR),
       ('stats', PTR), ('len', None), ('i0', None), ('lam', None), ('nrows', None), ('P', 0), ('y_img', None), ('img_scale', None), ('img_bf16', 0),
       ('scratch', None), ('bytes', 0), ('B', B), ('T', T), ('C', CH), ('stream', None))
MASK = (('x', PTR), ('x_ld', LD), ('x_bs', LD * (T + 4)), ('gamma', PTR), ('beta', PTR), ('stats', PTR), ('mask', PTR), ('B', B), ('T', T), ('C', CH),
        ('stream', None))
BWD = (('x', PTR), ('x_ld', LD), ('x_bs', LD * (T + 4)), ('dy', PTR), ('dy_ld', LD), ('dy_bs', LD * (T + 4)), ('gamma', PTR), ('beta', PTR),
       ('stats', PTR), ('g_gamma', PTR), ('g_beta', PTR), ('g_bias', PTR), ('amax', None), ('part', None), ('lam', None), ('start', None), ('P', 0),
       ('src', None), ('src_ld', 0), ('src_bs', 0), ('dy_img', None), ('B', B), ('T', T), ('C', CH), ('stream', None))
PLAN = dict(i0=PTR, lam=PTR, nrows=PTR, P=T)
SCAT = dict(lam=PTR, start=PTR, P=T, src=PTR, src_ld=LD, src_bs=LD * (T + 4))


def _call(fn, spec, k):
    assert set(k) <= {a for a, _ in spec}, set(k) - {a for a, _ in spec}
    return getattr(_capi.lib(), fn)(*[k.get(a, d) for a, d in spec])


def _fwd(**k):
    return _call('ss_op_gn_relu_fwd', FWD, k)


def _mask(**k):
    return _call('ss_op_gn_relu_mask', MASK, k)


def _bwd(**k):
    return _call('ss_op_gn_relu_bwd', BWD, k)


def test_scratch_formula():
    lib = _capi.lib()
    for b, t, c in ((1, 1, 64), (3, 256, 192), (2, 257, 64), (3, 320, 192), (1, 8192, 64), (2, 321, 128)):
        want = 0 if t <= 256 else 2 * b * (c // 16) * -(-t // 64) * 8
        assert lib.ss_op_gn_relu_scratch(b, t, c) == want == engine.gn_relu_scratch(b, t, c)
    assert lib.ss_op_gn_relu_scratch(1, 8192, 64) == 2 * 4 * 128 * 8                    # GN_MAXCH chunks
    assert lib.ss_op_gn_relu_scratch(0, 300, 64) == 0 and lib.ss_op_gn_relu_scratch(1, 300, 65) == 0


def test_forward_refusals_each_with_its_own_text():
    for name in ('x', 'y', 'gamma', 'beta', 'stats'):
        _refused(_fwd(**{name: None}), 'ss_op_gn_relu_fwd: null pointer')
    for shape in (dict(B=0), dict(T=0), dict(T=-3)):
        _refused(_fwd(**shape), 'ss_op_gn_relu_fwd: needs B >= 1 and T >= 1')
    for c in (0, 16, 65, 96, -64):
        _refused(_fwd(C=c), 'ss_op_gn_relu_fwd: needs C % 64 == 0')
    _refused(_fwd(T=8193, scratch=PTR, bytes=1 << 40), 'T above SS_MAX_EVAL_FRAMES')
    # strides and bases
    _refused(_fwd(x_ld=CH - 4), 'ss_op_gn_relu_fwd: x: row stride below C')
    _refused(_fwd(y_ld=CH - 4), 'ss_op_gn_relu_fwd: y: row stride below C')
    for bad in (dict(x_ld=LD + 1), dict(x_bs=LD * (T + 4) + 2), dict(y_ld=LD + 2), dict(y_bs=LD * (T + 4) + 3)):
        _refused(_fwd(**bad), 'stride is not a multiple of 4 floats')
    _refused(_fwd(x=off(4)), 'ss_op_gn_relu_fwd: x: base is not 16-byte aligned')
    _refused(_fwd(y=off(8)), 'ss_op_gn_relu_fwd: y: base is not 16-byte aligned')
    _refused(_fwd(gamma=off(4)), 'gamma_dev / beta_dev are not 16-byte aligned')
    _refused(_fwd(beta=off(8)), 'gamma_dev / beta_dev are not 16-byte aligned')
    _refused(_fwd(stats=off(2)), 'a word array is not 4-byte aligned')
    _refused(_fwd(len=off(2)), 'a word array is not 4-byte aligned')
    # the long path's scratch
    need = _capi.lib().ss_op_gn_relu_scratch(B, 300, CH)
    big = dict(T=300, x_bs=LD * 304, y_bs=LD * 304)
    _refused(_fwd(**big), 'ss_op_gn_relu_fwd: scratch too small')
    _refused(_fwd(scratch=PTR, bytes=need - 1, **big), 'ss_op_gn_relu_fwd: scratch too small')
    _refused(_fwd(scratch=None, bytes=need, **big), 'ss_op_gn_relu_fwd: scratch too small')
    _refused(_fwd(scratch=off(4), bytes=need, **big), 'ss_op_gn_relu_fwd: scratch_dev is not 8-byte aligned')
    # the gather form
    for part in ('i0', 'lam', 'nrows'):
        _refused(_fwd(**{**PLAN, part: None}), 'the gather form needs i0_dev, lam_dev and nrows_dev')
    for p in (0, -1, 259, 512):
        _refused(_fwd(**{**PLAN, 'P': p}), 'the gather form needs 1 <= P <= 258')
    _refused(_fwd(T=257, x_bs=LD * 261, y_bs=LD * 261, scratch=PTR, bytes=1 << 30, **PLAN), 'T > 256 runs the plain and ragged forms only')
    _refused(_fwd(len=PTR, **PLAN), 'len_dev and a plan exclude each other')
    _refused(_fwd(y_img=PTR), 'y_img_dev without a plan')
    # an image the launcher would silently drop is refused
    _refused(_fwd(y_img=PTR, y_ld=LD + 4, **PLAN), 'y_img_dev needs y_ld % 8 == 0 and y_bs % 8 == 0')
    _refused(_fwd(y_img=PTR, y_bs=LD * (T + 4) + 4, **PLAN), 'y_img_dev needs y_ld % 8 == 0 and y_bs % 8 == 0')
    for o in (4, 8, 16):
        _refused(_fwd(y_img=off(o), **PLAN), 'y_img_dev (format v2) is not 32-byte aligned')
    for o in (2, 4, 8):
        _refused(_fwd(y_img=off(o), img_bf16=1, **PLAN), 'y_img_dev (bf16) is not 16-byte aligned')
    _refused(_fwd(y_img=PTR, img_scale=off(2), **PLAN), 'a word array is not 4-byte aligned')


def test_mask_refusals():
    for name in ('x', 'gamma', 'beta', 'stats', 'mask'):
        _refused(_mask(**{name: None}), 'ss_op_gn_relu_mask: null pointer')
    _refused(_mask(T=0), 'ss_op_gn_relu_mask: needs B >= 1 and T >= 1')
    _refused(_mask(C=96), 'ss_op_gn_relu_mask: needs C % 64 == 0')
    _refused(_mask(T=257), 'ss_op_gn_relu_mask: T > 256 has no backward and no mask')
    _refused(_mask(x_ld=CH - 4), 'ss_op_gn_relu_mask: x: row stride below C')
    _refused(_mask(x=off(4)), 'ss_op_gn_relu_mask: x: base is not 16-byte aligned')
    _refused(_mask(mask=off(2)), 'ss_op_gn_relu_mask: an operand is not 4-byte aligned')


def test_backward_refusals_each_with_its_own_text():
    for name in ('x', 'dy', 'gamma', 'beta', 'stats', 'g_gamma', 'g_beta', 'g_bias'):
        _refused(_bwd(**{name: None}), 'ss_op_gn_relu_bwd: null pointer')
    for shape in (dict(B=0), dict(T=0)):
        _refused(_bwd(**shape), 'ss_op_gn_relu_bwd: needs B >= 1 and T >= 1')
    for c in (32, 100):
        _refused(_bwd(C=c), 'ss_op_gn_relu_bwd: needs C % 64 == 0')
    for t in (257, 300, 8192):
        _refused(_bwd(T=t), 'ss_op_gn_relu_bwd: T > 256 has no backward')
        _refused(_bwd(T=t, **SCAT), 'ss_op_gn_relu_bwd: T > 256 has no backward')
    for part in ('lam', 'start', 'src'):
        _refused(_bwd(**{**SCAT, part: None}), 'the scatter form needs lam_dev, start_dev and src_dev')
    for p in (0, 259):
        _refused(_bwd(**{**SCAT, 'P': p}), 'the scatter form needs 1 <= P <= 258')
    _refused(_bwd(x_ld=CH - 4), 'ss_op_gn_relu_bwd: x: row stride below C')
    _refused(_bwd(dy_ld=LD + 2), 'ss_op_gn_relu_bwd: dy: row / batch stride is not a multiple of 4 floats')
    _refused(_bwd(dy=off(4)), 'ss_op_gn_relu_bwd: dy: base is not 16-byte aligned')
    _refused(_bwd(**{**SCAT, 'src_ld': CH - 4}), 'ss_op_gn_relu_bwd: src: row stride below C')
    _refused(_bwd(**{**SCAT, 'src_bs': LD * (T + 4) + 1}), 'ss_op_gn_relu_bwd: src: row / batch stride is not a multiple of 4 floats')
    _refused(_bwd(**{**SCAT, 'src': off(8)}), 'ss_op_gn_relu_bwd: src: base is not 16-byte aligned')
    _refused(_bwd(gamma=off(4)), 'gamma_dev / beta_dev are not 16-byte aligned')
    for name in ('stats', 'g_gamma', 'g_beta', 'g_bias', 'amax', 'part'):
        _refused(_bwd(**{name: off(2)}), 'a word array is not 4-byte aligned')
    _refused(_bwd(dy_img=PTR, dy_ld=LD + 4), 'dy_img_dev needs dy_ld % 8 == 0 and dy_bs % 8 == 0')
    _refused(_bwd(dy_img=PTR, dy_bs=LD * (T + 4) + 4), 'dy_img_dev needs dy_ld % 8 == 0 and dy_bs % 8 == 0')
    for o in (2, 4, 6):
        _refused(_bwd(dy_img=off(o)), 'dy_img_dev (bf16) is not 8-byte aligned')


def test_python_wrappers_and_the_host_side_plan_contract():
    sig = inspect.signature(engine.gn_relu_fwd)
    assert list(sig.parameters) == ['x', 'y', 'gamma', 'beta', 'stats', 'lengths', 'plan', 'y_img', 'img_scale', 'scratch']
    sig = inspect.signature(engine.gn_relu_bwd)
    assert list(sig.parameters) == ['x', 'dy', 'gamma', 'beta', 'stats', 'g_gamma', 'g_beta', 'g_bias', 'amax', 'part', 'scatter', 'src', 'dy_img']
    assert list(inspect.signature(engine.gn_relu_mask).parameters) == ['x', 'gamma', 'beta', 'stats', 'out']
    Tq, P = 8, 6
    i0 = torch.tensor([[0, 0, 3, 7, 7, 2]], dtype=torch.int32)              # row 5 is past nrows: anything
    lam = torch.rand(1, P)
    nrows = torch.tensor([5], dtype=torch.int32)
    start = engine.gn_plan_start(i0, nrows, Tq)
    assert start.tolist() == [[0, 2, 2, 2, 3, 3, 3, 3, 5]]
    assert engine.check_gn_plan(Tq, P, i0=i0, lam=lam, nrows=nrows, start=start) == 1
    bad = lambda **k: pytest.raises(ValueError, engine.check_gn_plan, Tq, k.pop('P', P), **{**dict(i0=i0, lam=lam, nrows=nrows, start=start), **k})
    bad(i0=torch.tensor([[0, 0, 3, 8, 8, 2]], dtype=torch.int32))           # i0 == T
    bad(i0=torch.tensor([[0, -1, 3, 7, 7, 2]], dtype=torch.int32))
    bad(i0=torch.tensor([[0, 3, 2, 7, 7, 2]], dtype=torch.int32))           # decreasing within the live rows
    bad(nrows=torch.tensor([7], dtype=torch.int32))                         # nrows > P
    bad(nrows=torch.tensor([-1], dtype=torch.int32))
    bad(start=start + 1)                                                    # does not rise from 0, leaves 0 .. P at the end
    bad(start=torch.tensor([[0, 2, 1, 2, 3, 3, 3, 3, 5]], dtype=torch.int32))
    bad(start=torch.tensor([[0, 2, 2, 2, 3, 3, 3, 3, 7]], dtype=torch.int32))
    bad(start=torch.tensor([[0, 2, 2, 2, 3, 3, 3, 3, 4]], dtype=torch.int32))      # start[T] != nrows
    bad(lam=torch.full((1, P), float('nan')))
    bad(i0=i0.long())
    bad(start=start[:, :-1].contiguous())
    with pytest.raises(ValueError):
        engine.check_gn_plan(Tq, 259)
    assert engine.check_gn_plan(Tq, P, i0=i0, lam=lam, nrows=torch.tensor([0], dtype=torch.int32)) == 1      # nrows = 0: nothing is live
