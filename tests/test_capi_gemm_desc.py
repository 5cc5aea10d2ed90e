"""CPU-only checks of the descriptor-level GEMM test hooks ss_op_gemm_desc / ss_op_gemm_img_desc: the C symbols, the struct layouts against
the header, and every refusal -- each is made before anything is enqueued, so fake non-null device pointers are enough and no device is
needed.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re

from speechsplit_amd import _capi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20                                                 # fake, non-null, 256-byte aligned; never dereferenced


def _header():
    return open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()


def _struct_fields(name):
    """[(c type, field)] of `typedef struct <name> { ... }` in the header, in declaration order."""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), _header(), re.S).group(1)
    out = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'(const float|const void|float|long|int)\s*(.*)', decl, re.S)
        base = m.group(1)
        for f in m.group(2).split(','):
            f = f.strip()
            out.append((base + '*' if f.startswith('*') or decl.startswith(base + '*') else base, f.lstrip('* ')))
    return out


def test_symbols_and_struct_layouts_match_the_header():
    lib = _capi.lib()
    for name, st in (('ss_op_gemm_desc', _capi.SSGemmDesc), ('ss_op_gemm_img_desc', _capi.SSGemmImgDesc)):
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 2 and args[0]._type_ is st and args[1] is C.c_void_p
        assert getattr(lib, name).restype is C.c_int
    for cname, st in (('ss_gemm_desc', _capi.SSGemmDesc), ('ss_gemm_img_desc', _capi.SSGemmImgDesc)):
        fields = _struct_fields(cname)
        assert [f for _, f in fields] == [f for f, _ in st._fields_], cname
        for (ctype, f), (_, pyt) in zip(fields, st._fields_):
            assert pyt is {'long': C.c_long, 'int': C.c_int}.get(ctype, C.c_void_p), (cname, f, ctype)
    # every GemmDesc / ImgGemmDesc field a product launch sets has its place (diag, queue and the work-queue fields are left out)
    assert {f for f, _ in _capi.SSGemmDesc._fields_} == {
        'a', 'lda', 'a_bstride', 'a_seglen', 'a_segstride', 'b', 'ldb', 'b_bstride', 'b_seglen', 'b_segstride', 'c', 'ldc', 'cstride', 'bias', 'M', 'N', 'K',
        'batch', 'flags', 'want', 'row_period', 'row_off', 'row_lo', 'row_hi', 'ksplit', 'amax_a', 'amax_b', 'a_pre', 'b_pre', 'a_pre_scale', 'b_pre_scale',
        'part'}
    assert {f for f, _ in _capi.SSGemmImgDesc._fields_} == {
        'a', 'lda', 'a_bstride', 'a_seglen', 'a_segstride', 'b', 'ldb', 'b_bstride', 'b_seglen', 'b_segstride', 'c', 'ldc', 'cstride', 'bias', 'M', 'N', 'K',
        'batch', 'ksplit', 'flags', 'row_period', 'row_off', 'row_lo', 'row_hi', 'rm_T', 'rm_TP', 'part', 'scale_a', 'scale_b', 'zeros', 'cfg', 'bf16'}
    whole = re.sub(r'[\s*]+', ' ', _header())
    for phrase in ('TEST HOOKS of the two GEMM launchers', 'Refused before anything is enqueued', 'The work-queue form stays with ss_op_gemm_img',
                   'a row mask with ksplit > 1'):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def _gemm(**k):
    f = dict(a=P, b=P, c=P, lda=64, ldb=64, ldc=64, M=64, N=64, K=64, batch=1, ksplit=1)
    f.update(k)
    d = _capi.SSGemmDesc(**f)
    return _capi.lib().ss_op_gemm_desc(C.byref(d), None)


def _img(**k):
    f = dict(a=P, b=P, c=P, lda=64, ldb=64, ldc=64, M=64, N=64, K=64, batch=1, ksplit=1, cfg=-1, zeros=P)
    f.update(k)
    d = _capi.SSGemmImgDesc(**f)
    return _capi.lib().ss_op_gemm_img_desc(C.byref(d), None)


def test_gemm_desc_refusals_each_with_its_own_text():
    _refused(_capi.lib().ss_op_gemm_desc(None, None), 'ss_op_gemm_desc: null descriptor')
    for name in ('a', 'b', 'c'):
        _refused(_gemm(**{name: None}), 'ss_op_gemm_desc: null pointer')
    for name in ('M', 'N', 'K', 'batch', 'ksplit', 'want', 'a_seglen', 'b_seglen'):
        _refused(_gemm(**{name: -1}), 'ss_op_gemm_desc: negative size')
    for flags in (32, 64, 128, 1 << 20):                    # 32 / 64 are the launcher's own image bits
        _refused(_gemm(flags=flags), 'ss_op_gemm_desc: unknown flag')
    for flags in (0, 1, 2, 3, 8, 16):
        for ks in (2, 3, 16):
            _refused(_gemm(flags=flags, ksplit=ks), 'ss_op_gemm_desc: ksplit > 1 needs the accumulate flag')
            _refused(_gemm(flags=flags, ksplit=ks, part=P), 'ksplit > 1 needs the accumulate flag')
    for mask in (dict(row_period=-1), dict(row_period=10, row_off=-1), dict(row_period=10, row_lo=-1, row_hi=4), dict(row_period=10, row_lo=2, row_hi=11),
                 dict(row_period=10, row_lo=5, row_hi=4)):
        _refused(_gemm(**mask), 'ss_op_gemm_desc: bad row mask')


def test_gemm_img_desc_refusals_each_with_its_own_text():
    _refused(_capi.lib().ss_op_gemm_img_desc(None, None), 'ss_op_gemm_img_desc: null descriptor')
    for name in ('a', 'b', 'c'):
        _refused(_img(**{name: None}), 'ss_op_gemm_img_desc: null pointer')
    for name in ('M', 'N', 'K', 'batch', 'ksplit', 'a_seglen', 'b_seglen', 'rm_T', 'rm_TP'):
        _refused(_img(**{name: -1}), 'ss_op_gemm_img_desc: negative size')
    for flags in (8, 16, 32):
        _refused(_img(flags=flags), 'ss_op_gemm_img_desc: unknown flag')
    for ks in (2, 3):
        _refused(_img(ksplit=ks), 'ss_op_gemm_img_desc: ksplit > 1 needs part_dev')
    _refused(_img(row_period=10, row_lo=2, row_hi=11), 'ss_op_gemm_img_desc: bad row mask')
    _refused(_img(rm_T=36, rm_TP=35), 'ss_op_gemm_img_desc: rm_TP < rm_T')
    for cfg in (-2, 4):
        _refused(_img(cfg=cfg), 'ss_op_gemm_img_desc: cfg outside -1 .. 3')
    # what gemm_img_supported refuses
    not_supported = 'ss_op_gemm_img_desc: shape / alignment / option not supported by the image GEMM'
    for bad in (dict(M=0), dict(K=0), dict(N=62), dict(K=40), dict(a=P + 16), dict(b=P + 8), dict(lda=68), dict(a_bstride=4, batch=2),
                dict(a_seglen=16, a_segstride=64), dict(b_seglen=32, b_segstride=36), dict(flags=1, M=60), dict(flags=2, K=40, zeros=None),
                dict(rm_T=16, rm_TP=20), dict(rm_T=36, rm_TP=40, flags=1), dict(rm_T=36, rm_TP=40, row_period=40, row_lo=2, row_hi=38),
                dict(bf16=1, K=32), dict(bf16=1, a_seglen=32, a_segstride=64)):
        _refused(_img(**bad), not_supported)
    # a row mask on a split reduction: the partial slabs carry no mask, so the ordered reduction would write the masked rows
    _refused(_img(row_period=40, row_off=2, row_lo=2, row_hi=38, ksplit=2, part=P, K=128), not_supported)


def test_python_hook_signatures():
    sig = inspect.signature(engine.gemm_desc)
    assert list(sig.parameters) == ['a', 'a_geom', 'b', 'b_geom', 'c', 'c_geom', 'M', 'N', 'K', 'batch', 'ta', 'tb', 'accumulate', 'bf16', 'f16x2', 'bias',
                                    'want', 'row_mask', 'ksplit', 'amax_a', 'amax_b', 'a_img', 'b_img', 'a_pre_scale', 'b_pre_scale', 'part']
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[9:])
    sig = inspect.signature(engine.gemm_img_desc)
    assert list(sig.parameters) == ['a_img', 'a_geom', 'b_img', 'b_geom', 'c', 'c_geom', 'M', 'N', 'K', 'batch', 'ta', 'tb', 'accumulate', 'bias', 'row_mask',
                                    'rm', 'ksplit', 'part', 'scale_a', 'scale_b', 'zeros', 'cfg']
    assert list(inspect.signature(engine.gemm).parameters)[:6] == ['a', 'b', 'bias', 'ta', 'tb', 'ksplit']      # the existing hooks are unchanged
