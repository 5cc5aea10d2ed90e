"""CPU-only checks of the test hooks of the resampling kernels -- ss_op_interp_plan, ss_op_interp_gather, ss_op_interp_quant and
ss_op_interp_scatter: the C symbols and their signatures, the header's declarations and contract text, and every refusal -- each is made before
anything is enqueued, so fake non-null device pointers are enough and no device is needed.  No kernel is launched here."""
import ctypes as C
import os
import re

from speechsplit_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
SIGNATURES = {
    'ss_op_interp_plan': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'ss_op_interp_gather': (_i, [_vp, _vp, _vp, _i, _vp, _l, _l, _vp, _l, _l, _i, _i, _vp, _vp, _vp]),
    'ss_op_interp_quant': (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _l, _l, _vp, _l, _l, _i, _vp, _i, _vp]),
    'ss_op_interp_scatter': (_i, [_vp, _vp, _i, _i, _vp, _l, _l, _vp, _l, _l, _i, _i, _vp]),
}
BASE = 1 << 20
PTR = C.c_void_p(BASE)                                      # fake, non-null, 32-byte aligned; never dereferenced


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
    for decl in ('int ss_op_interp_plan(const float* scales_dev, const int* len_seg_dev, const int* len_seq_dev, int len_seq_const, int S, int ncand, '
                 'int P, int T, int B, int* i0_dev, float* lam_dev, int* nrows_dev, int* counts_dev, int* start_dev, void* stream);',
                 'int ss_op_interp_gather(const int* i0_dev, const float* lam_dev, const int* nrows_dev, int P, const float* x_dev, long x_ld, long x_bs, '
                 'float* y_dev, long y_ld, long y_bs, int C, int B, float* y_img_dev, const float* img_scale_dev, void* stream);',
                 'int ss_op_interp_quant(const int* i0_dev, const float* lam_dev, const int* nrows_dev, int P, int T, const float* mel_dev, '
                 'const float* f0_dev, int CM, float* ymel_dev, long ym_ld, long ym_bs, float* yoh_dev, long yo_ld, long yo_bs, int NOH, int* qidx_dev, '
                 'int B, void* stream);',
                 'int ss_op_interp_scatter(const float* lam_dev, const int* start_dev, int P, int T, const float* dy_dev, long dy_ld, long dy_bs, '
                 'float* dx_dev, long dx_ld, long dx_bs, int C, int B, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_spk_grad(') < raw.index(' ss_op_interp_plan(') < raw.index(' ss_op_interp_scatter(') < raw.index(' ss_op_conv_pack(')
    whole = re.sub(r'[\s*]+', ' ', raw)
    for phrase in ('bit-exact to the reference', 'IEEE division', 'fl < len_seg[b S + s] - 1', 'fl + off < len - 1', 'nrows[b] = min(counts[b], P)',
                   'ZERO in both for nrows[b] <= r < P', 'the number of rows r < nrows[b] with i0[b][r] < i, for i = 0 .. T',
                   'ncand <= 64, P <= 512', 'NOT CHECKED', 'the two products and the sum rounded separately', 'subnormal products kept',
                   'are never read', 'the launcher would drop the image silently', 'rint to nearest even', 'min(rint(f 255) + 1, NOH - 1)',
                   'unvoiced, -0.0, NaN', 'for ALL yo_ld columns of the row', 'one fp32 chain of fused multiply-adds from 0',
                   'the weight 1 - lam_r rounded to fp32 first', '+0.0 where no row contributes', 'The same bits on every call'):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def _call(fn, spec, k):
    assert set(k) <= {a for a, _ in spec}, set(k) - {a for a, _ in spec}
    return getattr(_capi.lib(), fn)(*[k.get(a, d) for a, d in spec])


PLAN = (('scales', PTR), ('len_seg', PTR), ('len_seq', PTR), ('const', 0), ('S', 7), ('ncand', 64), ('P', 192), ('T', 224), ('B', 4), ('i0', PTR),
        ('lam', PTR), ('nrows', PTR), ('counts', PTR), ('start', PTR), ('stream', None))


def test_plan_refusals():
    def plan(**k):
        return _call('ss_op_interp_plan', PLAN, k)
    for p in ('scales', 'len_seg', 'i0', 'lam', 'nrows', 'counts', 'start'):
        _refused(plan(**{p: None}), 'ss_op_interp_plan: null pointer')
    for d in ('B', 'S', 'T'):
        _refused(plan(**{d: 0}), 'ss_op_interp_plan: needs B >= 1, S >= 1 and T >= 1')
    _refused(plan(ncand=0), 'ncand outside 1 .. 64')
    _refused(plan(ncand=65), 'ncand outside 1 .. 64')                                         # what the launcher refuses
    _refused(plan(P=0), 'P outside 1 .. 512')
    _refused(plan(P=513), 'P outside 1 .. 512')
    _refused(plan(len_seq=None, const=-1), 'len_seq_const outside 0 .. T')
    _refused(plan(len_seq=None, const=225), 'len_seq_const outside 0 .. T')
    _refused(plan(start=off(2)), 'a word array is not 4-byte aligned')
    _refused(plan(len_seq=off(1)), 'a word array is not 4-byte aligned')


GATHER = (('i0', PTR), ('lam', PTR), ('nrows', PTR), ('P', 48), ('x', PTR), ('x_ld', 68), ('x_bs', 68 * 64), ('y', PTR), ('y_ld', 72), ('y_bs', 72 * 48),
          ('C', 64), ('B', 8), ('y_img', PTR), ('img_scale', PTR), ('stream', None))


def test_gather_refusals():
    def gather(**k):
        return _call('ss_op_interp_gather', GATHER, k)
    for p in ('i0', 'lam', 'nrows', 'x', 'y'):
        _refused(gather(**{p: None}), 'ss_op_interp_gather: null pointer')
    _refused(gather(B=0), 'B outside 1 .. 65535')
    _refused(gather(B=65536), 'B outside 1 .. 65535')
    _refused(gather(P=0), 'P outside 1 .. 65535')
    _refused(gather(C=0), 'needs C >= 1 and row strides of at least C')
    _refused(gather(x_ld=63), 'needs C >= 1 and row strides of at least C')
    _refused(gather(y_ld=63, y_img=None, img_scale=None), 'needs C >= 1 and row strides of at least C')
    _refused(gather(y_img=None), 'img_scale_dev without y_img_dev')
    _refused(gather(lam=off(2)), 'a word array is not 4-byte aligned')
    # the alignment rule of the image: every condition under which the launcher would drop it
    for k in (dict(C=60, x_ld=64), dict(x_ld=70), dict(y_ld=68), dict(x_bs=68 * 64 + 2), dict(y_bs=72 * 48 + 4), dict(x=off(8)), dict(y=off(8)),
              dict(y_img=off(16))):
        _refused(gather(**k), 'the launcher would drop the image')


QUANT = (('i0', PTR), ('lam', PTR), ('nrows', PTR), ('P', 256), ('T', 256), ('mel', PTR), ('f0', PTR), ('CM', 80), ('ymel', PTR), ('ym_ld', 84),
         ('ym_bs', 84 * 260), ('yoh', PTR), ('yo_ld', 260), ('yo_bs', 260 * 260), ('NOH', 257), ('qidx', PTR), ('B', 3), ('stream', None))
SCATTER = (('lam', PTR), ('start', PTR), ('P', 48), ('T', 64), ('dy', PTR), ('dy_ld', 67), ('dy_bs', 67 * 48), ('dx', PTR), ('dx_ld', 69),
           ('dx_bs', 69 * 64), ('C', 64), ('B', 8), ('stream', None))


def test_quant_and_scatter_refusals():
    def quant(**k):
        return _call('ss_op_interp_quant', QUANT, k)
    for p in ('i0', 'lam', 'nrows', 'mel', 'f0', 'ymel', 'yoh', 'qidx'):
        _refused(quant(**{p: None}), 'ss_op_interp_quant: null pointer')
    _refused(quant(B=0), 'B outside 1 .. 65535')
    _refused(quant(P=65536), 'P outside 1 .. 65535')
    for k in (dict(T=1), dict(CM=0), dict(NOH=1)):
        _refused(quant(**k), 'needs T >= 2, CM >= 1 and NOH >= 2')
    _refused(quant(ym_ld=79), 'row stride below CM (ymel) or below NOH (yoh)')
    _refused(quant(yo_ld=256), 'row stride below CM (ymel) or below NOH (yoh)')
    _refused(quant(qidx=off(2)), 'an operand is not 4-byte aligned')

    def scatter(**k):
        return _call('ss_op_interp_scatter', SCATTER, k)
    for p in ('lam', 'start', 'dy', 'dx'):
        _refused(scatter(**{p: None}), 'ss_op_interp_scatter: null pointer')
    _refused(scatter(B=0), 'B outside 1 .. 65535')
    _refused(scatter(P=0), 'P outside 1 .. 65535')
    for k in (dict(T=0), dict(C=0), dict(dy_ld=63), dict(dx_ld=63)):
        _refused(scatter(**k), 'needs T >= 1, C >= 1 and row strides of at least C')
    _refused(scatter(dx=off(2)), 'an operand is not 4-byte aligned')
