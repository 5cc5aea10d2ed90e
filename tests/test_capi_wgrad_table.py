"""CPU-only checks of ss_op_lstm_wgrad_table and its two size functions: symbols and signatures, the header's declarations and contract text,
the size formulas, and every refusal -- each is made before anything is enqueued, so fake non-null device pointers are enough and no device
is needed.  No kernel is launched here."""
import ctypes as C
import os
import re

import wgrad_ref as R
from speechsplit_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
_task = C.POINTER(_capi.SSWgradTask)
SIGNATURES = {
    'ss_op_lstm_wgrad_table_floats': (_l, [_task, _i, _i]),
    'ss_op_lstm_wgrad_table_counters': (_i, [_task, _i]),
    'ss_op_lstm_wgrad_table': (_i, [_task, _i, _i, _vp, _l, _vp, _i, _vp]),
}
BASE = 1 << 20
PTR = C.c_void_p(BASE)
GOOD = dict(dg=BASE, x=BASE, x_ld=204, hout=BASE, h_ld=64, gwih=BASE, gwhh=BASE, gb=BASE, H=32, In=200, R=1059)
SMALL = dict(GOOD, H=3, In=63, x_ld=64, h_ld=8, R=65)


def tasks(*rows):
    arr = (_capi.SSWgradTask * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = _capi.SSWgradTask(**r)
    return arr


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2                        # symbols were only added
    assert C.sizeof(_capi.SSWgradTask) == 80 and _capi.SSWgradTask.H.offset == 64 and _capi.SSWgradTask.R.offset == 72


def test_header_declares_them_and_states_the_contract():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('typedef struct ss_wgrad_task { const float* dg; const float* x; long x_ld; const float* hout; long h_ld; float *gwih, *gwhh, *gb; '
                 'int H, In; long R; } ss_wgrad_task;',
                 'long ss_op_lstm_wgrad_table_floats(const ss_wgrad_task* t, int n, int row_groups);',
                 'int ss_op_lstm_wgrad_table_counters(const ss_wgrad_task* t, int n);',
                 'int ss_op_lstm_wgrad_table(const ss_wgrad_task* t, int n, int row_groups, float* part_dev, long part_floats, unsigned* ctr_dev, '
                 'int ctr_words, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_spk_grad(') < raw.index(' ss_op_lstm_wgrad_table(') < raw.index(' ss_op_interp_plan(')
    whole = re.sub(r'[\s*]+', ' ', raw)
    for phrase in ('a TABLE of 1 .. 8 tasks in one launch', 'the columns behind 2 H are never read', 'sum_r dg[r + 1][n] hout[r][k]',
                   'sum_r dg[r][4H + n] hout[r + 1][H + k]', 'b_ih and b_hh have the same gradient', 'ceil(ceil(R / row_groups) / 64) 64 rows',
                   'one fp32 chain of fused multiply-adds in row order', 'added in float64 in group order, rounded to fp32 once and added (fp32) to what '
                   'the output holds', 'whatever the order the workgroups arrive in', 'tiles row_groups 4096 floats',
                   'ZERO on entry and zero again when the launch retires', 'ceil(8 H / 64) (ceil(In / 64) + (4 H % 64 == 0 ? 1 : 2))',
                   'return 0 for a table the hook would refuse', 'dg not 16-byte aligned', 'ROW 0 OF dg MUST BE ZERO', 'summed beside its W_hh, over dg[r + 1]'):
        assert phrase in whole, phrase


def test_size_functions():
    lib = _capi.lib()
    for H, In in ((1, 1), (3, 63), (8, 64), (16, 65), (17, 64), (31, 1), (32, 200), (32, 4096)):
        t = tasks(dict(GOOD, H=H, In=In, x_ld=In, h_ld=2 * H))
        for rg in (1, 7, 16):
            assert lib.ss_op_lstm_wgrad_table_floats(t, 1, rg) == R.tiles(H, In) * rg * 4096
        assert lib.ss_op_lstm_wgrad_table_counters(t, 1) == R.tiles(H, In)
    three = tasks(GOOD, SMALL, dict(GOOD, H=8, In=64, x_ld=64, h_ld=16))
    assert lib.ss_op_lstm_wgrad_table_counters(three, 3) == R.tiles(32, 200) + R.tiles(3, 63) + R.tiles(8, 64)
    assert lib.ss_op_lstm_wgrad_table_floats(three, 3, 9) == (R.tiles(32, 200) + R.tiles(3, 63) + R.tiles(8, 64)) * 9 * 4096
    assert lib.ss_op_lstm_wgrad_table_floats(None, 1, 16) == 0 and lib.ss_op_lstm_wgrad_table_floats(three, 3, 0) == 0
    assert lib.ss_op_lstm_wgrad_table_counters(tasks(dict(GOOD, H=33)), 1) == 0


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and b'ss_op_lstm_wgrad_table: ' in msg and word.encode() in msg, (word, msg)


def test_refusals():
    lib = _capi.lib()
    need = R.tiles(32, 200) + R.tiles(3, 63)

    def run(second=SMALL, n=2, rg=16, part=PTR, floats=None, ctr=PTR, words=need):
        return lib.ss_op_lstm_wgrad_table(tasks(GOOD, second), n, rg, part, need * rg * 4096 if floats is None else floats, ctr, words, None)
    _refused(lib.ss_op_lstm_wgrad_table(None, 1, 16, PTR, 1 << 30, PTR, 64, None), 'null pointer')
    _refused(run(n=0), 'number of tasks out of range (1 .. 8)')
    _refused(run(n=9), 'number of tasks out of range (1 .. 8)')
    _refused(run(rg=0), 'row_groups outside 1 .. 1024')
    _refused(run(rg=1025), 'row_groups outside 1 .. 1024')
    for p in ('dg', 'x', 'hout', 'gwih', 'gwhh', 'gb'):
        _refused(run(dict(SMALL, **{p: None})), "a task's pointer is null")
    for k in (dict(H=0), dict(H=33), dict(In=0), dict(R=0)):
        _refused(run(dict(SMALL, **k)), 'a task needs H in 1 .. 32, In >= 1 and R >= 1')
    _refused(run(dict(SMALL, x_ld=62)), "a task's x_ld is below In")
    _refused(run(dict(SMALL, h_ld=5)), "a task's h_ld is below 2 H")
    _refused(run(dict(SMALL, dg=BASE + 8)), "a task's dg is not 16-byte aligned")
    _refused(run(dict(SMALL, x=BASE + 2)), "a task's operand is not 4-byte aligned")
    _refused(run(dict(GOOD, In=64 * 16400, x_ld=64 * 16400)), 'more than 65535 tiles')
    _refused(run(part=None), 'part_dev too small')
    _refused(run(floats=need * 16 * 4096 - 1), 'part_dev too small')
    _refused(run(ctr=None), 'fewer counters than tiles')
    _refused(run(words=need - 1), 'fewer counters than tiles')
    _refused(run(part=C.c_void_p(BASE + 8)), 'part_dev is not 16-byte aligned')
    _refused(run(ctr=C.c_void_p(BASE + 2)), 'ctr_dev not 4-byte aligned')
