"""CPU-only checks of the conversion scores' interface: the C symbols and their header text, the scratch arithmetic, every refusal (each is
made before anything is enqueued, so a fake non-null pointer is enough and no device is needed), and the host side of metrics.py and
convert.conversion_scores with the device call replaced by the numpy restatement.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dtw_ref as R
from speechsplit_amd import _capi, convert, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    'ss_mel_cepstra': (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),                    # mel, len, B, max_t, n_mels, dct, n_ceps, out, stream
    'ss_dtw_scratch_bytes': (_l, [_i, _i, _i]),                                           # B, max_tx, max_ty
    # fx, tx, fy, ty, B, max_tx, max_ty, dim, scale, out, path, path_len, scratch, bytes, stream
    'ss_dtw': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _l, _vp]),
    'ss_path_f0_stats': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),                 # path, path_len, f0x, f0y, B, max_tx, max_ty, out, stream
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null, 256-byte aligned; never dereferenced
MAXF = 8192


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_declares_them_between_the_vocoder_and_collate():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))                 # comments out: declarations carry inline ones
    for decl in ('int ss_mel_cepstra(const float* mel_dev, const int* len_dev, int B, int max_t, int n_mels, const double* dct_dev, '
                 'int n_ceps, double* out_dev, void* stream);',
                 'long ss_dtw_scratch_bytes(int B, int max_tx, int max_ty);',
                 'int ss_dtw(const double* fx_dev, const int* tx_dev, const double* fy_dev, const int* ty_dev, int B, int max_tx, '
                 'int max_ty, int dim, double scale, double* out_dev , int* path_dev , int* path_len_dev , void* scratch_dev, '
                 'long scratch_bytes, void* stream);',
                 'int ss_path_f0_stats(const int* path_dev, const int* path_len_dev, const double* f0x_dev, const double* f0y_dev, int B, '
                 'int max_tx, int max_ty, double* out_dev , void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_istft(') < raw.index(' ss_mel_cepstra(') < raw.index('long ss_dtw_scratch_bytes(') < raw.index(' ss_dtw(') \
        < raw.index(' ss_path_f0_stats(') < raw.index('int ss_collate(')
    assert '#define SS_MAX_EVAL_FRAMES 8192' in raw
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('the diagonal wins', '50 sqrt(2)', '-1e10', 'strict <', 'no band and no slope constraint', 'one term at a time',
                   'sqrt(2 / n_mels) cos(pi d (m + 1/2) / n_mels)', 'what it gives alone'):
        assert phrase in whole, phrase


def test_scratch_bytes_arithmetic_and_monotonicity():
    """2-bit backpointers (so at least a quarter byte a cell, and never more than a byte), one boundary row of D a pair, and room for a
    path; every part rounded up to 256 bytes (two parts a pair) and every lattice row to a whole byte"""
    lib = _capi.lib()
    sb = lib.ss_dtw_scratch_bytes
    for B, tx, ty in ((1, 1, 1), (1, 49, 41), (3, 135, 105), (16, 800, 777), (2, 8192, 8192), (7, 64, 65), (5, 1, 8192), (5, 8192, 1)):
        got = sb(B, tx, ty)
        assert got % 256 == 0 and got * 4 >= B * tx * ty, (B, tx, ty, got)
        assert got <= B * (tx * ty + 8 * ty + 8 * (tx + ty - 1) + 2 * 255 + tx), (B, tx, ty, got)
    assert sb(2, 100, 100) > sb(1, 100, 100)
    assert sb(1, 300, 100) > sb(1, 100, 100) and sb(1, 100, 2000) > sb(1, 100, 100)
    for a in range(1, 40):                                                                 # never decreasing in any argument
        assert sb(a + 1, 37, 53) >= sb(a, 37, 53) and sb(3, a + 1, 53) >= sb(3, a, 53) and sb(3, 37, a + 1) >= sb(3, 37, a)
    assert sb(65535, MAXF, MAXF) > 2 ** 40                                                 # long arithmetic
    for args, word in (((0, 10, 10), b'B'), ((-1, 10, 10), b'B'), ((65536, 10, 10), b'B'), ((1, 0, 10), b'max_tx'),
                       ((1, MAXF + 1, 10), b'max_tx'), ((1, 10, 0), b'max_ty'), ((1, 10, MAXF + 1), b'max_ty'), ((1, -5, 10), b'max_tx')):
        assert sb(*args) == -1
        assert word in lib.ss_last_error(), (args, lib.ss_last_error())
    assert sb(1, 1, 1) > 0 and sb(65535, 1, 1) > 0


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_dtw_scratch_bytes(2, 50, 40)
    nan, inf = float('nan'), float('inf')
    cep = lambda **k: lib.ss_mel_cepstra(*[k.get(a, d) for a, d in (('mel', PTR), ('len', None), ('B', 2), ('max_t', 50), ('n_mels', 80),
                                                                    ('dct', PTR), ('n_ceps', 24), ('out', PTR), ('stream', None))])
    dtw = lambda **k: lib.ss_dtw(*[k.get(a, d) for a, d in (('fx', PTR), ('tx', None), ('fy', PTR), ('ty', None), ('B', 2), ('max_tx', 50),
                                                            ('max_ty', 40), ('dim', 24), ('scale', 1.0), ('out', PTR), ('path', PTR),
                                                            ('path_len', PTR), ('scratch', PTR), ('bytes', nb), ('stream', None))])
    f0 = lambda **k: lib.ss_path_f0_stats(*[k.get(a, d) for a, d in (('path', PTR), ('path_len', None), ('f0x', PTR), ('f0y', PTR), ('B', 2),
                                                                     ('max_tx', 50), ('max_ty', 40), ('out', PTR), ('stream', None))])
    # null required pointers
    _refused(cep(mel=None), 'mel_dev')
    _refused(cep(dct=None), 'dct_dev')
    _refused(cep(out=None), 'out_dev')
    _refused(dtw(fx=None), 'fx_dev')
    _refused(dtw(fy=None), 'fy_dev')
    _refused(dtw(out=None), 'out_dev')
    _refused(dtw(scratch=None), 'scratch_dev')
    _refused(f0(path=None), 'path_dev')
    _refused(f0(f0x=None), 'f0x_dev')
    _refused(f0(f0y=None), 'f0y_dev')
    _refused(f0(out=None), 'out_dev')
    # shapes
    for call in (cep, dtw, f0):
        for B in (0, -3, 65536):
            _refused(call(B=B), 'B outside')
    for T in (0, -1, MAXF + 1):
        _refused(cep(max_t=T), 'max_t')
        for call in (dtw, f0):
            _refused(call(max_tx=T), 'max_tx')
            _refused(call(max_ty=T), 'max_ty')
    for n in (0, -1, 129):
        _refused(cep(n_mels=n), 'n_mels')
    for n in (0, -1, 41):
        _refused(cep(n_ceps=n), 'n_ceps')
        _refused(dtw(dim=n), 'dim')
    for sc in (0.0, -1.0, nan, inf, -inf):
        _refused(dtw(scale=sc), 'scale')
    # the path and its length come together
    _refused(dtw(path=None), 'path_dev and path_len_dev')
    _refused(dtw(path_len=None), 'path_dev and path_len_dev')
    # scratch
    _refused(dtw(bytes=nb - 1), 'scratch_bytes')
    _refused(dtw(bytes=0), 'scratch_bytes')
    _refused(dtw(B=3), 'scratch_bytes')
    _refused(dtw(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
    _refused(dtw(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')


# ---------------------------------------------------------------------------------------------- host side of metrics.py
def test_dct_basis_is_the_references():
    for n_ceps, n_mels in ((24, 80), (1, 80), (40, 128), (13, 1)):
        b = metrics.dct_basis(n_ceps, n_mels)
        assert b.dtype == np.float64 and b.shape == (n_ceps, n_mels) and np.array_equal(b, R.dct_basis(n_ceps, n_mels))
    assert metrics.dct_basis().shape == (24, 80)
    assert metrics.SCALE == R.SCALE == 50.0 * 2.0 ** 0.5
    for bad in ((0, 80), (41, 80), (24, 0), (24, 129)):
        with pytest.raises(ValueError, match='n_ceps|n_mels'):
            metrics.dct_basis(*bad)


def _host_score_batch(seen, max_rows):
    """metrics.score_batch on the host: the numpy restatement, recording and checking what it was handed"""
    def fake(mel_x, tx, mel_y, ty, f0x, f0y, dct, device, want_path):
        B, Tx, Ty = len(tx), mel_x.shape[1], mel_y.shape[1]
        seen.append(list(zip(tx, ty)))
        assert mel_x.dtype == mel_y.dtype == np.float32 and dct.dtype == np.float64 and device == 'cpu'
        assert B <= max_rows and Tx == max(tx) and Ty == max(ty) and mel_x.shape[0] == mel_y.shape[0] == B
        lens = [max(a, b) for a, b in zip(tx, ty)]
        assert lens == sorted(lens)
        cap = Tx + Ty - 1
        out, stats = np.zeros((B, 3)), (np.zeros((B, 5)) if f0x is not None else None)
        path, plen = (np.full((B, cap, 2), -1, np.int32), np.zeros(B, np.int32)) if want_path else (None, None)
        for b in range(B):
            assert not mel_x[b, tx[b]:].any() and not mel_y[b, ty[b]:].any()               # zeros behind each row's own frames
            total, p, mcd = R.dtw(R.cepstra(mel_x[b, :tx[b]], dct), R.cepstra(mel_y[b, :ty[b]], dct))
            out[b] = total, len(p), mcd
            if f0x is not None:
                assert f0x.dtype == f0y.dtype == np.float64 and f0x.shape == (B, Tx) and f0y.shape == (B, Ty)
                assert np.all(f0x[b, tx[b]:] == -1e10) and np.all(f0y[b, ty[b]:] == -1e10)
                stats[b] = R.f0_stats(p, f0x[b], f0y[b])
            if want_path:
                path[b, :len(p)], plen[b] = p, len(p)
        return out, stats, path, plen
    return fake


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_mcd_dtw_batches_and_returns_input_order(monkeypatch, max_rows):
    """the batching of mcd_dtw with the device call replaced by a host stand-in that records what it was handed: plan_batches order on
    max(Tx, Ty), each row's own lengths, zeros (-1e10 for F0) behind them -- and the results back in input order whatever max_rows is"""
    rng = np.random.default_rng(7)
    shapes = [(9, 12), (3, 3), (20, 5), (1, 7), (12, 9)]
    xs = [rng.uniform(0, 1, (a, 80)).astype(np.float32) for a, _ in shapes]
    ys = [rng.uniform(0, 1, (b, 80)).astype(np.float32) for _, b in shapes]
    f0x = [np.where(rng.uniform(size=a) < 0.3, -1e10, rng.normal(5.0, 0.2, a)) for a, _ in shapes]
    f0y = [np.where(rng.uniform(size=b) < 0.3, -1e10, rng.normal(5.0, 0.2, b)) for _, b in shapes]
    seen = []
    monkeypatch.setattr(metrics, 'score_batch', _host_score_batch(seen, max_rows))
    out = metrics.mcd_dtw(xs, ys, f0x, f0y, max_rows=max_rows, device='cpu', return_paths=True)
    assert isinstance(out, list) and len(out) == len(shapes)
    for x, y, fx, fy, got in zip(xs, ys, f0x, f0y, out):
        want = R.score(x, y, 24, fx, fy)
        assert set(got) == {'mcd_db', 'total', 'path_len', 'f0_rmse_cents', 'f0_corr', 'vuv_error', 'n_voiced', 'path'}
        assert got['path'].dtype == np.int32 and np.array_equal(got['path'], want['path'])
        for k in ('mcd_db', 'total', 'path_len', 'f0_rmse_cents', 'f0_corr', 'vuv_error', 'n_voiced'):
            assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k
        assert isinstance(got['path_len'], int) and isinstance(got['n_voiced'], int) and isinstance(got['mcd_db'], float)
    lens = [max(s) for s in shapes]
    assert [max(p) for b in seen for p in b] == sorted(lens)
    assert [len(b) for b in seen] == [len(b) for b in convert.plan_batches(lens, max_rows)]
    # without F0 and without paths: the three keys; one pair in, one dict out
    plain = metrics.mcd_dtw(xs, ys, max_rows=max_rows, device='cpu')
    assert [set(r) for r in plain] == [{'mcd_db', 'total', 'path_len'}] * len(shapes)
    assert [r['total'] for r in plain] == [r['total'] for r in out]
    one = metrics.mcd_dtw(xs[2], ys[2], f0x[2], f0y[2], n_ceps=13, max_rows=max_rows, device='cpu')
    assert isinstance(one, dict) and one['total'] == R.score(xs[2], ys[2], 13)['total'] and 'f0_corr' in one and 'path' not in one
    assert metrics.mcd_dtw([], [], device='cpu') == []


def test_mcd_dtw_refuses_by_argument(monkeypatch):
    monkeypatch.setattr(metrics, 'score_batch', _host_score_batch([], 16))
    m = lambda t: np.full((t, 80), 0.5, np.float32)
    with pytest.raises(ValueError, match='xs'):
        metrics.mcd_dtw([m(3), m(0)], [m(3), m(3)], device='cpu')
    with pytest.raises(ValueError, match='ys'):
        metrics.mcd_dtw([m(3)], [np.zeros((0, 80), np.float32)], device='cpu')
    with pytest.raises(ValueError, match='ys'):
        metrics.mcd_dtw([m(3), m(4)], [m(3)], device='cpu')
    with pytest.raises(ValueError, match='ys'):
        metrics.mcd_dtw([m(3)], [np.zeros((3, 40), np.float32)], device='cpu')
    with pytest.raises(ValueError, match='xs'):
        metrics.mcd_dtw([np.zeros(5, np.float32)], [m(3)], device='cpu')
    with pytest.raises(ValueError, match='f0x'):
        metrics.mcd_dtw([m(3)], [m(4)], f0x=[np.zeros(4)], f0y=[np.zeros(4)], device='cpu')
    with pytest.raises(ValueError, match='f0y'):
        metrics.mcd_dtw([m(3)], [m(4)], f0x=[np.zeros(3)], f0y=[np.zeros(3)], device='cpu')
    with pytest.raises(ValueError, match='f0y'):
        metrics.mcd_dtw([m(3), m(3)], [m(4), m(4)], f0x=[np.zeros(3)] * 2, f0y=[np.zeros(4)], device='cpu')
    with pytest.raises(ValueError, match='f0x and f0y'):
        metrics.mcd_dtw([m(3)], [m(4)], f0x=[np.zeros(3)], device='cpu')
    with pytest.raises(ValueError, match='n_ceps'):
        metrics.mcd_dtw([m(3)], [m(4)], n_ceps=41, device='cpu')


def test_conversion_scores_keeps_the_nesting_and_calls_once(monkeypatch):
    rng = np.random.default_rng(11)
    mel = lambda t: rng.uniform(0, 1, (t, 80)).astype(np.float32)
    pairs = [[(f'p{p}_{c}', mel(5 + p + n)) for n, c in enumerate(('R', 'F', 'U'))] for p in range(2)]
    targets = [[mel(6 + n) for n in range(3)] for _ in range(2)]
    calls = []
    real = metrics.mcd_dtw
    monkeypatch.setattr(metrics, 'score_batch', _host_score_batch([], 4))
    monkeypatch.setattr(metrics, 'mcd_dtw', lambda *a, **k: calls.append(k) or real(*a, **k))
    nested = convert.conversion_scores(pairs, targets, max_rows=4, device='cpu')
    assert len(calls) == 1 and calls[0] == {'max_rows': 4, 'device': 'cpu'}
    assert [[n for n, _ in pair] for pair in nested] == [[n for n, _ in pair] for pair in pairs]
    for pair, tpair, got in zip(pairs, targets, nested):
        for (_, x), y, (_, s) in zip(pair, tpair, got):
            assert s['total'] == R.score(x, y)['total'] and s['path_len'] == R.score(x, y)['path_len']
    flat = convert.conversion_scores(pairs[1], targets[1], max_rows=4, device='cpu')
    assert len(calls) == 2 and [n for n, _ in flat] == [n for n, _ in pairs[1]]
    assert [s for _, s in flat] == [s for _, s in nested[1]]
    assert convert.conversion_scores([], [], device='cpu') == []
    with pytest.raises(ValueError, match='targets'):
        convert.conversion_scores(pairs, targets[:1], device='cpu')
    with pytest.raises(ValueError, match='targets'):
        convert.conversion_scores(pairs[0], targets[0][:2], device='cpu')
