"""CPU-only checks of the test hooks of the kernels between the heavy families of a training step -- ss_op_mse_loss, ss_op_ce_loss,
ss_op_colsum[_scratch_doubles], ss_op_dec_in / _grad / _codes and ss_op_spk_grad: the C symbols and their signatures, the header's
declarations and contract text, the scratch formula, and every refusal -- each is made before anything is enqueued, so fake non-null device
pointers are enough and no device is needed.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest

import step_ops_ref as R
from speechsplit_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_src = C.POINTER(_capi.SSCodeSrc)
SIGNATURES = {
    'ss_op_mse_loss': (_i, [_vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _i, _i, _i, _f, _vp, _vp, _vp]),
    'ss_op_ce_loss': (_i, [_vp, _l, _l, _vp, _vp, _l, _l, _i, _i, _i, _f, _vp, _vp, _vp]),
    'ss_op_colsum_scratch_doubles': (_l, [_i]),
    'ss_op_colsum': (_i, [_vp, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _l, _vp, _i, _vp]),
    'ss_op_dec_in': (_i, [_src, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    'ss_op_dec_in_grad': (_i, [_src, _i, _vp, _i, _i, _i, _i, _vp]),
    'ss_op_dec_in_codes': (_i, [_src, _i, _vp, _i, _i, _vp, _l, _vp, _i, _i, _i, _i, _vp]),
    'ss_op_spk_grad': (_i, [_vp, _l, _l, _i, _vp, _vp, _l, _i, _i, _i, _vp, _i, _vp]),
}
BASE = 1 << 20
PTR = C.c_void_p(BASE)                                      # fake, non-null, aligned; never dereferenced


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2                        # symbols were only added
    assert C.sizeof(_capi.SSCodeSrc) == 32 and _capi.SSCodeSrc.ld.offset == 28


def test_header_declares_them_and_states_the_contracts():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('int ss_op_mse_loss(const float* out_dev, long out_ld, long out_bs, const float* tgt_dev, long tgt_ld, long tgt_bs, float* d_out_dev, '
                 'long d_ld, long d_bs, int B, int T, int C, float grad_scale, float* partials_dev, float* loss_dev, void* stream);',
                 'int ss_op_ce_loss(const float* logits_dev, long ld, long bs, const int* tgt_dev, float* d_out_dev, long d_ld, long d_bs, int B, int T, '
                 'int C, float grad_scale, float* partials_dev, float* loss_dev, void* stream);',
                 'long ss_op_colsum_scratch_doubles(int cols);',
                 'int ss_op_colsum(const float* in_dev, long ld, int R, int C, int two_dir, float* o0_dev, float* o1_dev, float* o2_dev, float* o3_dev, '
                 'double* part_dev, long part_doubles, unsigned* ctr_dev, int ctr_words, void* stream);',
                 'typedef struct ss_code_src { const float* o; float* d_o; int H, freq, col, ld; } ss_code_src;',
                 'int ss_op_dec_in(const ss_code_src* src, int nsrc, const float* emb_dev, int emb_dim, int emb_col, float* dst_dev, int ld, int B, int T, '
                 'int f, void* stream);',
                 'int ss_op_dec_in_grad(const ss_code_src* src, int nsrc, const float* d_in_dev, int ld, int B, int T, int f, void* stream);',
                 'int ss_op_dec_in_codes(const ss_code_src* src, int nsrc, const float* emb_dev, int emb_dim, int emb_col, float* codes_dev, '
                 'long codes_floats, float* dst_dev, int ld, int B, int T, int f, void* stream);',
                 'int ss_op_spk_grad(const float* dg_dev, long ld, long b_stride, int rows, const float* w_f_dev, const float* w_r_dev, long w_ld, int col0, '
                 'int H4, int E, float* out_dev, int B, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_gn_relu_bwd(') < raw.index(' ss_op_mse_loss(') < raw.index(' ss_op_spk_grad(') < raw.index(' ss_op_split_image(')
    whole = re.sub(r'[\s*]+', ' ', raw)
    for phrase in ('no engine, no copy into private buffers', 'Every refusal is made before anything is enqueued', 'p being frame 0 (no halo is added)',
                   'at least 8 B floats of scratch', 'at least B T floats', 'TARGETS MUST LIE IN [0, C)', 'NOT CHECKED there', 'shift-invariant',
                   '(ceil(1024 / nb) + 1) nb 64 with nb = ceil(cols / 64)', 'ADDED to the outputs', 'o1 .. o3 must be NULL',
                   'ZERO on entry and zero again when the launch retires', 'The sums are the same bits whatever the arrival order',
                   'forward half at the LAST frame', 'backward half at its FIRST frame', 'halo rows untouched', 'every other column of the ld is written zero',
                   'fp32, frames ascending', 'and nowhere else', 'T % freq_i != 0', 'ld_i < 2 H_i', 'the compact form with a freq_i != f',
                   'ld < 2 H4', 'w_ld < col0 + E', 'more than 64 KiB of LDS'):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def _call(fn, spec, k):
    assert set(k) <= {a for a, _ in spec}, set(k) - {a for a, _ in spec}
    return getattr(_capi.lib(), fn)(*[k.get(a, d) for a, d in spec])


B, T, CH, LD = 3, 8, 80, 88
MSE = (('out', PTR), ('out_ld', LD), ('out_bs', LD * T), ('tgt', PTR), ('tgt_ld', LD), ('tgt_bs', LD * T), ('d_out', PTR), ('d_ld', LD), ('d_bs', LD * T),
       ('B', B), ('T', T), ('C', CH), ('gs', 1.0), ('partials', PTR), ('loss', PTR), ('stream', None))
CE = (('logits', PTR), ('ld', LD), ('bs', LD * T), ('tgt', PTR), ('d_out', PTR), ('d_ld', LD), ('d_bs', LD * T), ('B', B), ('T', T), ('C', CH), ('gs', 1.0),
      ('partials', PTR), ('loss', PTR), ('stream', None))


def test_loss_refusals():
    for p in ('out', 'tgt', 'd_out', 'partials', 'loss'):
        _refused(_call('ss_op_mse_loss', MSE, {p: None}), 'ss_op_mse_loss: null pointer')
    for d in ('B', 'T', 'C'):
        _refused(_call('ss_op_mse_loss', MSE, {d: 0}), 'ss_op_mse_loss: needs B >= 1')
        _refused(_call('ss_op_mse_loss', MSE, {d: -3}), 'ss_op_mse_loss: needs B >= 1')
    for s in ('out_ld', 'tgt_ld', 'd_ld'):
        _refused(_call('ss_op_mse_loss', MSE, {s: CH - 1}), 'ss_op_mse_loss: row stride below C')
    for p in ('logits', 'tgt', 'd_out', 'partials', 'loss'):
        _refused(_call('ss_op_ce_loss', CE, {p: None}), 'ss_op_ce_loss: null pointer')
    for d in ('B', 'T', 'C'):
        _refused(_call('ss_op_ce_loss', CE, {d: 0}), 'ss_op_ce_loss: needs B >= 1')
    for s in ('ld', 'd_ld'):
        _refused(_call('ss_op_ce_loss', CE, {s: CH - 1}), 'ss_op_ce_loss: row stride below C')


COLS = 257
COL = (('in', PTR), ('ld', 2 * COLS + 3), ('R', 33), ('C', COLS), ('two_dir', 0), ('o0', PTR), ('o1', None), ('o2', None), ('o3', None), ('part', PTR),
       ('part_doubles', R.colsum_scratch_doubles(2 * COLS)), ('ctr', PTR), ('ctr_words', 16), ('stream', None))


def test_colsum_scratch_formula():
    lib = _capi.lib()
    for cols in (1, 8, 63, 64, 65, 257, 512, 4096, 65536, 65537):
        nb = -(-cols // 64)
        assert lib.ss_op_colsum_scratch_doubles(cols) == (-(-1024 // nb) + 1) * nb * 64 == R.colsum_scratch_doubles(cols)
    assert lib.ss_op_colsum_scratch_doubles(0) == 0 and lib.ss_op_colsum_scratch_doubles(-5) == 0


def test_colsum_refusals():
    def col(**k):
        return _call('ss_op_colsum', COL, k)
    two = dict(two_dir=1, o2=PTR)
    _refused(col(**{'in': None}), 'ss_op_colsum: null pointer')
    _refused(col(o0=None), 'ss_op_colsum: null pointer')
    _refused(col(R=0), 'needs R >= 1')
    _refused(col(C=0), 'needs R >= 1')
    _refused(col(two_dir=1), 'the two-direction form needs o2_dev')
    _refused(col(o1=PTR), 'o1_dev .. o3_dev must be NULL')
    _refused(col(o3=PTR), 'o1_dev .. o3_dev must be NULL')
    _refused(col(ld=COLS - 1), 'row stride below the number of columns')
    _refused(col(ld=2 * COLS - 1, **two), 'row stride below the number of columns')
    _refused(col(part=None), 'part_dev and ctr_dev come together')
    _refused(col(ctr=None), 'part_dev and ctr_dev come together')
    _refused(col(part_doubles=R.colsum_scratch_doubles(COLS) - 1), 'part_dev too small')
    _refused(col(part_doubles=R.colsum_scratch_doubles(2 * COLS) - 1, **two), 'part_dev too small')
    _refused(col(ctr_words=4), 'fewer than ceil(cols / 64) counters')                       # 257 columns: five blocks
    _refused(col(ctr_words=8, **two), 'fewer than ceil(cols / 64) counters')                # 514 columns: nine
    _refused(col(part=C.c_void_p(BASE + 4)), 'not 8-byte aligned')
    _refused(col(ctr=C.c_void_p(BASE + 2)), 'not 8-byte aligned or ctr_dev not 4-byte aligned')


def _srcs(*rows):
    arr = (_capi.SSCodeSrc * len(rows))()
    for i, (o, d_o, H, freq, col, ld) in enumerate(rows):
        arr[i] = _capi.SSCodeSrc(o, d_o, H, freq, col, ld)
    return arr


P = BASE
GOOD = ((P, P, 8, 8, 0, 16), (P, P, 1, 8, 16, 2), (P, P, 32, 8, 18, 64))
DEC = (('src', None), ('nsrc', 3), ('emb', PTR), ('emb_dim', 82), ('emb_col', 82), ('dst', PTR), ('ld', 170), ('B', B), ('T', 16), ('f', 0), ('stream', None))
GRAD = (('src', None), ('nsrc', 3), ('d_in', PTR), ('ld', 170), ('B', B), ('T', 16), ('f', 0), ('stream', None))
CODES = (('src', None), ('nsrc', 3), ('emb', PTR), ('emb_dim', 82), ('emb_col', 82), ('codes', PTR), ('codes_floats', 1 << 20), ('dst', PTR), ('ld', 170),
         ('B', B), ('T', 16), ('f', 0), ('stream', None))


@pytest.mark.parametrize('fn,spec', (('ss_op_dec_in', DEC), ('ss_op_dec_in_grad', GRAD), ('ss_op_dec_in_codes', CODES)))
def test_dec_in_refusals(fn, spec):
    good = _srcs(*GOOD)
    io = 'd_in' if fn == 'ss_op_dec_in_grad' else 'dst'

    def call(rows=None, **k):
        k.setdefault('src', _srcs(*rows) if rows is not None else good)
        return _call(fn, spec, k)

    def with_src(i, **ch):
        rows = [list(r) for r in GOOD]
        for key, v in ch.items():
            rows[i][('o', 'd_o', 'H', 'freq', 'col', 'ld').index(key)] = v
        return rows
    _refused(_call(fn, spec, {}), fn + ': null pointer')                                     # src == NULL
    _refused(call(**{io: None}), fn + ': null pointer')
    _refused(call(nsrc=0), 'number of sources out of range')
    _refused(call(nsrc=4 if fn == 'ss_op_dec_in_codes' else 5), 'number of sources out of range')
    _refused(call(B=0), 'needs B >= 1')
    _refused(call(T=0), 'needs B >= 1')
    _refused(call(f=-1), 'f must be 0')
    _refused(call(f=5), 'f must be 0')                                                       # 16 % 5
    _refused(call(f=4), "the compact form needs every source's freq == f")
    _refused(call(with_src(1, freq=4), f=8), "the compact form needs every source's freq == f")
    _refused(call(with_src(0, **{'d_o' if fn == 'ss_op_dec_in_grad' else 'o': None})), "a source's slab pointer is null")
    _refused(call(with_src(2, H=0)), 'a source needs H >= 1')
    _refused(call(with_src(2, freq=0)), 'a source needs H >= 1')
    _refused(call(with_src(2, col=-1)), 'a source needs H >= 1')
    _refused(call(with_src(1, freq=3)), "T is not a multiple of a source's freq")
    _refused(call(with_src(2, col=170 - 63)), "a source's columns lie beyond ld")
    _refused(call(with_src(0, ld=15)), "a source's row stride is below 2 H")
    _refused(call(with_src(1, ld=1)), "a source's row stride is below 2 H")
    if fn != 'ss_op_dec_in_grad':
        _refused(call(emb=None), 'emb_dim > 0 without emb_dev')
        _refused(call(emb_dim=-1), 'bad speaker columns')
        _refused(call(emb_col=89), 'speaker columns beyond ld')
    if fn == 'ss_op_dec_in_codes':
        need = sum((B * (16 // f) * 2 * H + 3) // 4 * 4 for _, _, H, f, _, _ in GOOD)
        _refused(call(codes_floats=need - 1), 'codes_dev too small')
        _refused(call(codes=None), 'codes_dev too small')
        _refused(call(codes=C.c_void_p(BASE + 4)), 'not 16-byte aligned')


SPK = (('dg', PTR), ('ld', 40), ('b_stride', 40 * 12), ('rows', 12), ('w_f', PTR), ('w_r', PTR), ('w_ld', 100), ('col0', 7), ('H4', 16), ('E', 81),
       ('out', PTR), ('B', B), ('stream', None))


def test_spk_grad_refusals():
    def spk(**k):
        return _call('ss_op_spk_grad', SPK, k)
    for p in ('dg', 'w_f', 'w_r', 'out'):
        _refused(spk(**{p: None}), 'ss_op_spk_grad: null pointer')
    for k in (dict(E=0), dict(E=1025), dict(H4=0), dict(rows=0), dict(B=0), dict(col0=-1)):
        _refused(spk(**k), 'needs 1 <= E <= 1024')
    _refused(spk(H4=7800, ld=1 << 20), "64 KiB of LDS")                 # 2 * 7800 + 12 * 81 floats
    _refused(spk(ld=31), 'row stride below 2 H4')
    _refused(spk(w_ld=87), 'w_ld below col0 + E')
