"""CPU-only checks of the test hooks of the re-layout and guard kernels -- ss_op_conv_pack / _many / _dx, ss_op_conv_unpack / _many, ss_op_prep,
ss_op_transpose, ss_op_copy_rows, ss_op_act_scales and ss_op_param_guard: the C symbols and their signatures, the header's declarations and
contract text, and every refusal -- each is made before anything is enqueued, so fake non-null device pointers are enough and no device is
needed.  No kernel is launched here."""
import ctypes as C
import os
import re

from speechsplit_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
SIGNATURES = {
    'ss_op_conv_pack': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    'ss_op_conv_pack_many': (_i, [C.POINTER(_capi.SSConvPackTask), _i, _i, _vp]),
    'ss_op_conv_pack_dx': (_i, [_vp, _i, _i, _vp, _vp]),
    'ss_op_conv_unpack': (_i, [_vp, _i, _i, _i, _vp, _i, _vp]),
    'ss_op_conv_unpack_many': (_i, [C.POINTER(_capi.SSConvUnpackTask), _i, _i, _vp]),
    'ss_op_prep': (_i, [C.POINTER(_capi.SSPrepTask), _i, _i, _vp]),
    'ss_op_transpose': (_i, [_vp, _i, _i, _vp, _vp]),
    'ss_op_copy_rows': (_i, [_vp, _l, _l, _vp, _l, _l, _vp, _i, _i, _i, _vp]),
    'ss_op_act_scales': (_i, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i), _i, _i, _vp, _vp]),
    'ss_op_param_guard': (_i, [_vp, _l, _f, _vp, _vp]),
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
    assert C.sizeof(_capi.SSConvPackTask) == 56 and _capi.SSConvPackTask.Co.offset == 40
    assert C.sizeof(_capi.SSConvUnpackTask) == 32 and _capi.SSConvUnpackTask.Co.offset == 16
    assert C.sizeof(_capi.SSPrepTask) == 40 and _capi.SSPrepTask.n.offset == 24 and _capi.SSPrepTask.img.offset == 32


def test_header_declares_them_and_states_the_contracts():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('typedef struct ss_conv_pack_task { const float* w; float *wf, *wb, *wf_img, *wb_img; int Co, Ci, Cp; } ss_conv_pack_task;',
                 'typedef struct ss_conv_unpack_task { const float* gp; float* g; int Co, Ci, Cp; } ss_conv_unpack_task;',
                 'typedef struct ss_prep_task { const float* a; const float* b; float* dst; long n; float* img; } ss_prep_task;',
                 'int ss_op_conv_pack(const float* w_dev, int Co, int Ci, int Cp, float* wf_dev, float* wb_dev, float* wf_img_dev, float* wb_img_dev, '
                 'int img_bf16, void* stream);',
                 'int ss_op_conv_pack_many(const ss_conv_pack_task* t, int n, int img_bf16, void* stream);',
                 'int ss_op_conv_pack_dx(const float* w_dev, int Co, int Ci, float* wb_dev, void* stream);',
                 'int ss_op_conv_unpack(const float* gp_dev, int Co, int Ci, int Cp, float* g_dev, int acc, void* stream);',
                 'int ss_op_conv_unpack_many(const ss_conv_unpack_task* t, int n, int acc, void* stream);',
                 'int ss_op_prep(const ss_prep_task* t, int n, int img_bf16, void* stream);',
                 'int ss_op_transpose(const float* in_dev, int R, int C, float* out_dev, void* stream);',
                 'int ss_op_copy_rows(const float* src_dev, long s_ld, long s_bs, float* dst_dev, long d_ld, long d_bs, const int* len_dev, int B, int T, '
                 'int C, void* stream);',
                 'int ss_op_act_scales(const float* const* gamma_dev, const float* const* beta_dev, const int* C, int n, int T, float* out_dev, '
                 'void* stream);',
                 'int ss_op_param_guard(const float* p_dev, long n, float limit, unsigned* sticky_dev, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_spk_grad(') < raw.index(' ss_op_conv_pack(') < raw.index(' ss_op_param_guard(') < raw.index(' ss_op_split_image(')
    whole = re.sub(r'[\s*]+', ' ', raw)
    for phrase in ('each hands its operands to one kernel launcher and does nothing else', 'Every move is exact', 'n % 8 == 0, base 32-byte aligned',
                   'to nearest even', 'ZERO for Ci <= c < Cp', 'w[co][ci][4 - k]', 'wb_img without wb', 'the same bits as one ss_op_conv_pack each',
                   'for any Ci and Co', 'the columns Ci <= c < Cp of gp are never read', 'COPY OF THE BITS of a, -0.0 and NaN payloads included',
                   'the kernel would drop the image', 'R above 65535 32', 'min(max(len[b], 0), T) of src are never read and dst gets +0.0 there',
                   'halo rows and row gaps keep their bits', 'fmaf(sqrtf(16 T), max|gamma_i|, max|beta_i|)', 'one fused multiply-add',
                   'the largest power of two s >= 2^-20', 'A bound of +inf KEEPS 16', 'A NaN element does not enter the maxima',
                   '|p| >= limit; no other bit of the word changes and a clean arena leaves it as it was', 'n not a positive multiple of 4'):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def _call(fn, spec, k):
    assert set(k) <= {a for a, _ in spec}, set(k) - {a for a, _ in spec}
    return getattr(_capi.lib(), fn)(*[k.get(a, d) for a, d in spec])


PACK = (('w', PTR), ('Co', 8), ('Ci', 3), ('Cp', 4), ('wf', PTR), ('wb', PTR), ('wf_img', PTR), ('wb_img', PTR), ('bf16', 0), ('stream', None))
PACK_BAD = ((dict(w=None), 'null pointer'), (dict(wf=None), 'null pointer'), (dict(Co=0), 'needs Co >= 1'), (dict(Ci=0), 'needs Co >= 1'),
            (dict(Cp=-4), 'needs Co >= 1'), (dict(Co=6), 'needs Co % 4 == 0 and Cp % 4 == 0'), (dict(Cp=6), 'needs Co % 4 == 0 and Cp % 4 == 0'),
            (dict(Ci=5), 'Cp below Ci'), (dict(wb=None), 'wb_img without wb'), (dict(wf=off(8)), 'wf / wb not 16-byte aligned'),
            (dict(wb=off(4)), 'wf / wb not 16-byte aligned'), (dict(w=off(2)), 'w is not 4-byte aligned'),
            (dict(wf_img=off(16)), 'format-v2 image is not 32-byte aligned'), (dict(wb_img=off(8)), 'format-v2 image is not 32-byte aligned'),
            (dict(Co=4, Ci=1), 'element count that is a multiple of 8'),                    # wb: 1 x 5 x 4 = 20 elements
            (dict(bf16=1, wf_img=off(4)), 'bf16 image is not 8-byte aligned'), (dict(bf16=1, wb_img=off(2)), 'bf16 image is not 8-byte aligned'))


def test_conv_pack_refusals():
    for k, word in PACK_BAD:
        rc = _call('ss_op_conv_pack', PACK, k)
        _refused(rc, 'ss_op_conv_pack: ')
        _refused(rc, word)


def _pack_tasks(*rows):
    arr = (_capi.SSConvPackTask * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = _capi.SSConvPackTask(*[v.value if isinstance(v, C.c_void_p) else v for v in r])
    return arr


def test_conv_pack_many_refusals():
    lib = _capi.lib()
    names = ('w', 'wf', 'wb', 'wf_img', 'wb_img', 'Co', 'Ci', 'Cp')
    good = dict(w=PTR, wf=PTR, wb=PTR, wf_img=PTR, wb_img=PTR, Co=8, Ci=3, Cp=4)
    _refused(lib.ss_op_conv_pack_many(None, 1, 0, None), 'ss_op_conv_pack_many: null pointer')
    one = _pack_tasks([good[n] for n in names])
    _refused(lib.ss_op_conv_pack_many(one, 0, 0, None), 'number of tasks out of range (1 .. 8)')
    _refused(lib.ss_op_conv_pack_many(one, 9, 0, None), 'number of tasks out of range (1 .. 8)')
    for k, word in PACK_BAD:                                # a bad task behind a good one
        bf16 = k.get('bf16', 0)
        bad = dict(good, **{n: v for n, v in k.items() if n != 'bf16'})
        two = _pack_tasks([good[n] for n in names], [bad[n] for n in names])
        _refused(lib.ss_op_conv_pack_many(two, 2, bf16, None), 'ss_op_conv_pack_many: ')
        _refused(lib.ss_op_conv_pack_many(two, 2, bf16, None), word)


def test_conv_pack_dx_and_unpack_refusals():
    lib = _capi.lib()
    _refused(lib.ss_op_conv_pack_dx(None, 4, 4, PTR, None), 'ss_op_conv_pack_dx: null pointer')
    _refused(lib.ss_op_conv_pack_dx(PTR, 4, 4, None, None), 'ss_op_conv_pack_dx: null pointer')
    _refused(lib.ss_op_conv_pack_dx(PTR, 0, 4, PTR, None), 'ss_op_conv_pack_dx: needs Co >= 1 and Ci >= 1')
    _refused(lib.ss_op_conv_pack_dx(PTR, 4, -1, PTR, None), 'ss_op_conv_pack_dx: needs Co >= 1 and Ci >= 1')
    _refused(lib.ss_op_conv_pack_dx(PTR, 4, 4, off(2), None), 'ss_op_conv_pack_dx: an operand is not 4-byte aligned')
    UNP = (('gp', PTR), ('Co', 8), ('Ci', 3), ('Cp', 4), ('g', PTR), ('acc', 0), ('stream', None))
    bad = ((dict(gp=None), 'null pointer'), (dict(g=None), 'null pointer'), (dict(Co=0), 'needs Co >= 1'), (dict(Ci=0), 'needs Co >= 1'),
           (dict(Cp=0), 'needs Co >= 1'), (dict(Ci=5), 'Cp below Ci'), (dict(g=off(1)), 'an operand is not 4-byte aligned'))
    for acc in (0, 1):
        for k, word in bad:
            _refused(_call('ss_op_conv_unpack', UNP, dict(k, acc=acc)), 'ss_op_conv_unpack: ' + word)
    _refused(lib.ss_op_conv_unpack_many(None, 1, 0, None), 'ss_op_conv_unpack_many: null pointer')
    good = (BASE, BASE, 8, 3, 4)
    arr = (_capi.SSConvUnpackTask * 2)(_capi.SSConvUnpackTask(*good), _capi.SSConvUnpackTask(*good))
    _refused(lib.ss_op_conv_unpack_many(arr, 0, 0, None), 'number of tasks out of range (1 .. 8)')
    _refused(lib.ss_op_conv_unpack_many(arr, 9, 0, None), 'number of tasks out of range (1 .. 8)')
    for k, word in bad:
        t = dict(zip(('gp', 'g', 'Co', 'Ci', 'Cp'), good))
        t.update({n: (v.value if isinstance(v, C.c_void_p) else v) for n, v in k.items()})
        arr[1] = _capi.SSConvUnpackTask(t['gp'], t['g'], t['Co'], t['Ci'], t['Cp'])
        _refused(lib.ss_op_conv_unpack_many(arr, 2, 1, None), 'ss_op_conv_unpack_many: ' + word)


def test_prep_refusals():
    lib = _capi.lib()

    def run(bf16=0, n_tasks=2, **k):
        t = dict(a=BASE, b=BASE, dst=BASE, n=64, img=BASE)
        t.update(k)
        arr = (_capi.SSPrepTask * 2)(_capi.SSPrepTask(BASE, None, BASE, 5, None), _capi.SSPrepTask(t['a'], t['b'], t['dst'], t['n'], t['img']))
        return lib.ss_op_prep(arr, n_tasks, bf16, None)
    _refused(lib.ss_op_prep(None, 1, 0, None), 'ss_op_prep: null pointer')
    _refused(run(n_tasks=0), 'number of tasks out of range (1 .. 48)')
    _refused(run(n_tasks=49), 'number of tasks out of range (1 .. 48)')
    _refused(run(a=None), "a task's a or dst is null")
    _refused(run(dst=None), "a task's a or dst is null")
    _refused(run(n=0), 'a task needs n >= 1')
    _refused(run(a=BASE + 2, img=None), 'an operand is not 4-byte aligned')
    for k in (dict(n=66), dict(a=BASE + 4), dict(b=BASE + 8), dict(dst=BASE + 12)):          # the scalar path would drop the image
        _refused(run(**k), 'a task with an image needs n % 4 == 0 and a, b, dst 16-byte aligned')
    _refused(run(n=68), 'element count that is a multiple of 8')
    _refused(run(img=BASE + 16), 'format-v2 image is not 32-byte aligned')
    _refused(run(bf16=1, img=BASE + 4), 'bf16 image is not 8-byte aligned')


def test_transpose_and_copy_rows_refusals():
    lib = _capi.lib()
    _refused(lib.ss_op_transpose(None, 4, 4, PTR, None), 'ss_op_transpose: null pointer')
    _refused(lib.ss_op_transpose(PTR, 4, 4, None, None), 'ss_op_transpose: null pointer')
    _refused(lib.ss_op_transpose(PTR, 0, 4, PTR, None), 'ss_op_transpose: needs R >= 1 and C >= 1')
    _refused(lib.ss_op_transpose(PTR, 4, 0, PTR, None), 'ss_op_transpose: needs R >= 1 and C >= 1')
    _refused(lib.ss_op_transpose(PTR, 65535 * 32 + 1, 1, PTR, None), 'ss_op_transpose: R above 65535 * 32')
    _refused(lib.ss_op_transpose(off(2), 4, 4, PTR, None), 'ss_op_transpose: an operand is not 4-byte aligned')
    CP = (('src', PTR), ('s_ld', 83), ('s_bs', 83 * 9), ('dst', PTR), ('d_ld', 88), ('d_bs', 88 * 13), ('len', PTR), ('B', 3), ('T', 9), ('C', 83),
          ('stream', None))
    for k, word in ((dict(src=None), 'null pointer'), (dict(dst=None), 'null pointer'), (dict(B=0), 'needs 1 <= B <= 65535'),
                    (dict(B=65536), 'needs 1 <= B <= 65535'), (dict(T=0), 'needs 1 <= B <= 65535'), (dict(C=0), 'needs 1 <= B <= 65535'),
                    (dict(s_ld=82), 'row stride below C'), (dict(d_ld=82), 'row stride below C'), (dict(len=off(2)), 'an operand is not 4-byte aligned')):
        _refused(_call('ss_op_copy_rows', CP, k), 'ss_op_copy_rows: ' + word)


def test_act_scales_and_param_guard_refusals():
    lib = _capi.lib()

    def act(n=2, T=64, out=PTR, g=(BASE, BASE), b=(BASE, BASE), c=(64, 100), arrays=(True, True, True)):
        ga, ba, ca = (C.c_void_p * 8)(*g), (C.c_void_p * 8)(*b), (C.c_int * 8)(*c)
        return lib.ss_op_act_scales(ga if arrays[0] else None, ba if arrays[1] else None, ca if arrays[2] else None, n, T, out, None)
    for arrays in ((False, True, True), (True, False, True), (True, True, False)):
        _refused(act(arrays=arrays), 'ss_op_act_scales: null pointer')
    _refused(act(out=None), 'ss_op_act_scales: null pointer')
    _refused(act(n=0), 'number of blocks out of range (1 .. 8)')
    _refused(act(n=9), 'number of blocks out of range (1 .. 8)')
    _refused(act(T=0), 'ss_op_act_scales: needs T >= 1')
    _refused(act(c=(64, -1)), "a block's C is negative")
    _refused(act(g=(BASE, None)), 'a block with C > 0 needs gamma and beta')
    _refused(act(b=(None, BASE)), 'a block with C > 0 needs gamma and beta')
    _refused(act(g=(BASE, BASE + 2)), 'gamma / beta is not 4-byte aligned')
    _refused(act(out=off(2)), 'out_dev is not 4-byte aligned')
    _refused(lib.ss_op_param_guard(None, 8, 2048.0, PTR, None), 'ss_op_param_guard: null pointer')
    _refused(lib.ss_op_param_guard(PTR, 8, 2048.0, None, None), 'ss_op_param_guard: null pointer')
    for n in (0, -4, 6, 3):
        _refused(lib.ss_op_param_guard(PTR, n, 2048.0, PTR, None), 'n must be a positive multiple of 4')
    _refused(lib.ss_op_param_guard(off(8), 8, 2048.0, PTR, None), 'p_dev is not 16-byte aligned')
    _refused(lib.ss_op_param_guard(PTR, 8, 2048.0, off(2), None), 'sticky_dev not 4-byte aligned')
