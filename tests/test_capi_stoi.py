"""CPU-only checks of the waveform scores' interface: the C symbols and their header text, the scratch arithmetic, every refusal (each is
made before anything is enqueued, so a fake non-null pointer is enough and no device is needed), the band table, and the host side of
metrics.stoi and convert.conversion_stoi with the device call replaced by the numpy restatement.  No kernel is launched here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import stoi_ref as R
from speechsplit_amd import _capi, convert, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
_pi = C.POINTER(C.c_int)
SIGNATURES = {
    'ss_stoi_scratch_bytes': (_l, [_i, _i]),                                              # B, max_n
    # x, y, n, B, max_n, band_lo, band_hi, n_bands, extended, out, scratch, bytes, stream
    'ss_stoi': (_i, [_vp, _vp, _vp, _i, _i, _pi, _pi, _i, _i, _vp, _vp, _l, _vp]),
    'ss_op_stoi_compact': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),  # x, y, n, B, max_n, from_map, e, inv, k, xp, yp, stream
    'ss_op_stoi_bands': (_i, [_vp, _vp, _i, _i, _pi, _pi, _i, _vp, _vp]),                 # sig, len, B, max_len, lo, hi, n_bands, env, stream
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null, 256-byte aligned; never dereferenced
LO, HI = (C.c_int * 15)(*R.LO), (C.c_int * 15)(*R.HI)


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2                                                       # additive: the version is unchanged


def test_header_declares_them_between_the_conversion_scores_and_collate():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))                 # comments out: declarations carry inline ones
    for decl in ('long ss_stoi_scratch_bytes(int B, int max_n);',
                 'int ss_stoi(const double* x_dev, const double* y_dev, const int* n_dev, int B, int max_n, const int* band_lo, '
                 'const int* band_hi, int n_bands, int extended, double* out_dev , void* scratch_dev, long scratch_bytes, void* stream);',
                 'int ss_op_stoi_compact(const double* x_dev, const double* y_dev, const int* n_dev, int B, int max_n, int from_map, '
                 'double* e_dev , int* inv_dev , int* k_dev , double* xp_dev , double* yp_dev , void* stream);',
                 'int ss_op_stoi_bands(const double* sig_dev, const int* len_dev, int B, int max_len, const int* band_lo, '
                 'const int* band_hi, int n_bands, double* env_dev , void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_path_f0_stats(') < raw.index('long ss_stoi_scratch_bytes(') < raw.index(' ss_stoi(') \
        < raw.index(' ss_op_stoi_compact(') < raw.index(' ss_op_stoi_bands(') < raw.index('int ss_collate(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('eps = 2^-52', '0.5 - 0.5 cos(2 pi (i + 1) / 257)', 'e_f > max_f e_f - 40', 'the earlier frame\'s term first',
                   'strictly below len - 256', '(1 + 10^(15/20))', 'the score is NaN and S is reported as 0', 'parity with pystoi is unpinned',
                   'a corrupt scratch changes numbers, never addresses', 'lo = 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174',
                   'hi = 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219', 'to the bit'):
        assert phrase in whole, phrase


def test_band_table_is_the_headers():
    lo, hi = metrics.stoi_bands()
    assert lo == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert hi == [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]
    assert (lo, hi) == R.bands() and all(type(v) is int for v in lo + hi)
    assert [metrics.stoi_frames(n) for n in (1, 255, 256, 383, 384, 4096)] == [R.n_frames(n) for n in (1, 255, 256, 383, 384, 4096)]


def _a256(v):
    return -(-v // 256) * 256


def test_scratch_bytes_arithmetic_and_monotonicity():
    lib = _capi.lib()
    sb = lib.ss_stoi_scratch_bytes
    for B, n in ((1, 256), (1, 383), (1, 384), (1, 4096), (7, 30720), (16, 100000), (65535, 256), (3, 2 ** 31 - 1)):
        F = (n - 256) // 128 + 1
        L, M = 128 * (F - 1) + 256, F - 1
        S = max(M - 29, 0)
        want = _a256(8 * B * F) + _a256(4 * B * F) + _a256(4 * B) + 2 * _a256(8 * B * L) + 2 * _a256(8 * B * 32 * M) + _a256(8 * B * S)
        assert sb(B, n) == want and want % 256 == 0, (B, n, sb(B, n), want)
    assert sb(65535, 2 ** 31 - 1) > 2 ** 40                                                # long arithmetic
    for a in range(1, 20):
        assert sb(a + 1, 5000) >= sb(a, 5000) and sb(3, 256 + 100 * (a + 1)) >= sb(3, 256 + 100 * a)
    for args, word in (((0, 4096), b'B'), ((-1, 4096), b'B'), ((65536, 4096), b'B'), ((1, 255), b'max_n'), ((1, 0), b'max_n'), ((1, -4), b'max_n')):
        assert sb(*args) == -1
        assert word in lib.ss_last_error(), (args, lib.ss_last_error())


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def _bands(lo=None, hi=None):
    lo, hi = list(R.LO) if lo is None else lo, list(R.HI) if hi is None else hi
    return (C.c_int * len(lo))(*lo), (C.c_int * len(hi))(*hi)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_stoi_scratch_bytes(2, 4096)
    stoi = lambda **k: lib.ss_stoi(*[k.get(a, d) for a, d in (('x', PTR), ('y', PTR), ('n', None), ('B', 2), ('max_n', 4096), ('lo', LO),
                                                              ('hi', HI), ('n_bands', 15), ('extended', 0), ('out', PTR), ('scratch', PTR),
                                                              ('bytes', nb), ('stream', None))])
    comp = lambda **k: lib.ss_op_stoi_compact(*[k.get(a, d) for a, d in (('x', PTR), ('y', PTR), ('n', None), ('B', 2), ('max_n', 4096),
                                                                         ('from_map', 0), ('e', PTR), ('inv', PTR), ('k', PTR), ('xp', PTR),
                                                                         ('yp', PTR), ('stream', None))])
    band = lambda **k: lib.ss_op_stoi_bands(*[k.get(a, d) for a, d in (('sig', PTR), ('len', None), ('B', 2), ('max_len', 4096), ('lo', LO),
                                                                       ('hi', HI), ('n_bands', 15), ('env', PTR), ('stream', None))])
    # null required pointers
    for call, names in ((stoi, ('x', 'y', 'out', 'scratch')), (comp, ('x', 'y', 'e', 'inv', 'k', 'xp', 'yp')), (band, ('sig', 'env'))):
        for a in names:
            _refused(call(**{a: None}), a + '_dev')
    _refused(comp(from_map=1, e=None, inv=None), 'inv_dev')                               # e may be NULL with from_map, the map may not
    _refused(comp(from_map=1, e=None, k=None), 'k_dev')
    for call in (stoi, band):
        _refused(call(lo=None), 'band_lo')
        _refused(call(hi=None), 'band_hi')
    # shapes
    for call in (stoi, comp, band):
        for B in (0, -3, 65536):
            _refused(call(B=B), 'B outside')
    for n in (255, 0, -1):
        _refused(stoi(max_n=n), 'max_n')
        _refused(comp(max_n=n), 'max_n')
    for n in (256, 0, -1):
        _refused(band(max_len=n), 'max_len')
    for call in (stoi, band):
        for n in (0, -1, 33):
            _refused(call(n_bands=n), 'n_bands')
        lo, hi = _bands(lo=[-1] + list(R.LO[1:]))
        _refused(call(lo=lo, hi=hi), 'band_lo[0]')
        lo, hi = _bands(hi=list(R.HI[:-1]) + [258])
        _refused(call(lo=lo, hi=hi), 'band_hi[14]')
        for bad in (11, 12):                                                               # lo == hi, lo > hi
            lo, hi = _bands(lo=list(R.LO[:2]) + [bad] + list(R.LO[3:]), hi=list(R.HI[:2]) + [11] + list(R.HI[3:]))
            _refused(call(lo=lo, hi=hi), 'band_lo[2] is not below band_hi[2]')
    for v in (2, -1):
        _refused(stoi(extended=v), 'extended')
        _refused(comp(from_map=v), 'from_map')
    # scratch
    _refused(stoi(bytes=nb - 1), 'scratch_bytes')
    _refused(stoi(bytes=0), 'scratch_bytes')
    _refused(stoi(B=3), 'scratch_bytes')
    _refused(stoi(max_n=4096 + 128), 'scratch_bytes')
    _refused(stoi(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
    _refused(stoi(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')
    # the widest band table a call may pass is accepted up to the scratch check: bins 0 .. 257
    lo, hi = _bands(lo=[0] * 32, hi=[257] * 32)
    _refused(stoi(lo=lo, hi=hi, n_bands=32, bytes=0), 'scratch_bytes')


# ---------------------------------------------------------------------------------------------- host side of metrics.py / convert.py
def _fake_batch(calls):
    def run(x, y, n, extended, device):
        calls.append((x.copy(), y.copy(), list(n), extended))
        assert x.shape == y.shape and x.shape[1] >= 256 and x.shape[1] == max(max(n), 256)
        out = np.zeros((len(n), 3))
        for r, nr in enumerate(n):
            assert not x[r, nr:].any() and not y[r, nr:].any()                             # zeros behind every row's own samples
            ref = R.stoi(x[r, :nr], y[r, :nr], extended)
            out[r] = ref['score'], ref['S'], ref['K']
        return out
    return run


def _waves(seed, lengths):
    rng = np.random.RandomState(seed)
    t = np.arange(max(lengths) + 50)
    base = np.sin(2 * np.pi * 180.0 * t / 10000.0) * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t / 10000.0)) + 0.05 * rng.standard_normal(t.shape[0])
    return [base[:n].copy() for n in lengths], [base[:n + 7] + 0.3 * rng.standard_normal(n + 7) for n in lengths]


def test_stoi_cuts_pairs_and_batches_without_changing_results(monkeypatch):
    calls = []
    monkeypatch.setattr(metrics, 'stoi_batch', _fake_batch(calls))
    lengths = [5000, 300, 4400, 4096, 100, 4700]
    refs, degs = _waves(3, lengths)
    all_at_once = metrics.stoi(refs, degs, sr=10000, max_rows=16)
    assert len(calls) == 1 and calls[0][2] == sorted(lengths) and calls[0][0].shape == (6, 5000)
    one_by_one = metrics.stoi(refs, degs, sr=10000, max_rows=1)
    assert len(calls) == 1 + 6 and [c[0].shape[1] for c in calls[1:]] == [256, 300, 4096, 4400, 4700, 5000]
    pairs = metrics.stoi(refs, degs, sr=10000, max_rows=4)
    assert [c[2] for c in calls[7:]] == [[100, 300, 4096, 4400], [4700, 5000]]
    for got in (all_at_once, one_by_one, pairs):
        for i, n in enumerate(lengths):
            ref = R.stoi(refs[i], degs[i][:n])                                             # each pair cut to the shorter of the two
            assert set(got[i]) == {'stoi', 'segments', 'frames_kept', 'frames'}
            assert (got[i]['segments'], got[i]['frames_kept'], got[i]['frames']) == (ref['S'], ref['K'], ref['F'])
            assert got[i]['stoi'] == ref['score'] or (math.isnan(got[i]['stoi']) and math.isnan(ref['score']))
    assert math.isnan(all_at_once[1]['stoi']) and all_at_once[1]['frames'] == 1 and all_at_once[4]['frames'] == 0
    assert all_at_once[0]['segments'] >= 1
    # the cut works either way round, one pair in gives one dict out, extended is handed on
    a = metrics.stoi(degs[0], refs[0], sr=10000, extended=True)
    assert isinstance(a, dict) and calls[-1][3] is True and calls[-1][2] == [5000]
    assert metrics.stoi([], [], sr=10000) == []


def test_stoi_refuses_bad_input_by_name():
    for refs, degs, word in (([np.zeros(300)], [], 'one degraded waveform per reference'), ([np.zeros((2, 300))], [np.zeros(300)], 'pair 0'),
                             ([np.zeros(300), np.zeros(0)], [np.zeros(300), np.zeros(5)], 'pair 1')):
        with pytest.raises(ValueError, match=word):
            metrics.stoi(refs, degs, sr=10000)
    with pytest.raises(ValueError, match='max_rows'):
        metrics.stoi([np.zeros(300)], [np.zeros(300)], sr=10000, max_rows=0)


def test_stoi_resamples_both_sides_unless_already_at_10k(monkeypatch):
    from speechsplit_amd import features
    seen = []

    def fake_resample(xs, sr_in, sr_out=16000, max_rows=16, device='cuda'):
        seen.append((len(xs), sr_in, sr_out, [x.shape[0] for x in xs]))
        return [np.asarray(x[::2]) for x in xs]
    monkeypatch.setattr(features, 'resample', fake_resample)
    monkeypatch.setattr(metrics, 'stoi_batch', _fake_batch([]))
    refs, degs = _waves(5, [9000, 8000])
    got = metrics.stoi(refs, degs, sr=20000)
    assert seen == [(4, 20000, 10000, [9000, 8000, 9000, 8000])]                           # cut first, then one call for both sides
    assert got[0]['frames'] == R.n_frames(4500)
    metrics.stoi(refs, degs, sr=10000)
    assert len(seen) == 1


def test_conversion_stoi_keeps_names_and_nesting(monkeypatch):
    monkeypatch.setattr(metrics, 'stoi_batch', _fake_batch([]))
    refs, degs = _waves(9, [4500, 4200, 4800])
    flat = convert.conversion_stoi([('F', degs[0]), ('U', degs[1])], refs[:2], sr=10000)
    assert [n for n, _ in flat] == ['F', 'U'] and flat[0][1]['stoi'] == R.stoi(refs[0], degs[0][:4500])['score']
    nested = convert.conversion_stoi([[('F', degs[0])], [('U', degs[1]), ('FU', degs[2])]], [[refs[0]], [refs[1], refs[2]]], sr=10000,
                                     extended=True)
    assert [[n for n, _ in p] for p in nested] == [['F'], ['U', 'FU']]
    assert nested[1][1][1]['stoi'] == R.stoi(refs[2], degs[2][:4800], True)['score']
    for bad in ([refs[0]], [[refs[0]], [refs[1]]]):
        with pytest.raises(ValueError, match='references'):
            convert.conversion_stoi([[('F', degs[0])], [('U', degs[1]), ('FU', degs[2])]], bad, sr=10000)
    doc = re.sub(r'\s+', ' ', convert.conversion_stoi.__doc__)
    for phrase in ('``F``, ``U``, ``FU``', 'has no defined STOI', 'any vocoded mel against the recording the mel came from'):
        assert phrase in doc, phrase
