"""CPU-only checks of the non-negative mel inversion's interface: the two C symbols and their header text, ss_mel_nnls_pack (host only) against
the packing restated in nnls_ref.py, every refusal of both calls by message (each is made before anything is enqueued, so a fake non-null
pointer is enough and no device is needed) and the Python `inversion=` argument.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from speechsplit_amd import _capi, features, vocoder
from tests import nnls_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    'ss_mel_nnls_pack': (_l, [_vp, _i, _vp, _l]),                                          # basis, n_mels, packed, cap
    # mel, inv_basis, packed, packed_doubles, frames, B, max_frames, n_mels, n_iter, step, floor, mag, stream
    'ss_mel_to_linear_nnls': (_i, [_vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _d, _d, _vp, _vp]),
}
PTR = C.c_void_p(1 << 20)                                                                  # fake, non-null; never dereferenced
MAX_PACKED = 3072


@pytest.fixture(scope='module')
def bank():
    return np.ascontiguousarray(features.mel_filter_bank().T, dtype=np.float64)


def _pack(basis, cap=None, write=True):
    """(return value, the buffer handed in or None)"""
    lib = _capi.lib()
    b = np.ascontiguousarray(basis, dtype=np.float64)
    if not write:
        return lib.ss_mel_nnls_pack(C.c_void_p(b.ctypes.data), b.shape[1], None, 0 if cap is None else cap), None
    cap = lib.ss_mel_nnls_pack(C.c_void_p(b.ctypes.data), b.shape[1], None, 0) if cap is None else cap
    buf = np.full(max(cap, 1), -7.0)
    return lib.ss_mel_nnls_pack(C.c_void_p(b.ctypes.data), b.shape[1], C.c_void_p(buf.ctypes.data), cap), buf


def _refused(rc, *words):
    msg = _capi.lib().ss_last_error()
    assert rc == -1 and all(w.encode() in msg for w in words), (words, msg)


def test_symbols_signatures_and_header():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2                                                       # additive: the version is unchanged
    text = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read())
    for decl in ('long ss_mel_nnls_pack(const double* basis_host /* [513][n_mels] */, int n_mels, double* packed_host, long cap_doubles);',
                 'int ss_mel_to_linear_nnls(const float* mel_dev, const double* inv_basis_dev, const double* packed_dev, long packed_doubles, '
                 'const int* frames_dev, int B, int max_frames, int n_mels, int n_iter, double step, double floor, double* mag_dev, '
                 'void* stream);'):
        assert decl in text, decl
    assert text.index('int ss_mel_to_linear(') < text.index('long ss_mel_nnls_pack(') < text.index('int ss_op_stft (')
    for phrase in ('tn = (1 + sqrt(1 + 4 t^2)) / 2', 'y = xn + ((t - 1) / tn) (xn - x)', 'packed[2 m + 1]', '3072 doubles'):
        assert phrase in text, phrase


def test_pack_of_the_projects_bank_is_the_restated_packing(bank):
    size, _ = _pack(bank, write=False)
    assert size == 2 * 80 + 941                                                            # the size query: NULL packed_host
    n, buf = _pack(bank)
    assert n == size and np.array_equal(buf, N.pack(bank))
    lo, ln, off, w = N.unpack(buf, 80)
    assert w.shape == (941,) and int(ln.max()) == 34 and (w > 0).all()
    # a cap that does not suffice: the size comes back and nothing is written; a larger one: only `size` doubles are
    n, buf = _pack(bank, cap=size - 1)
    assert n == size and (buf == -7.0).all()
    n, buf = _pack(bank, cap=size + 5)
    assert n == size and np.array_equal(buf[:size], N.pack(bank)) and (buf[size:] == -7.0).all()
    assert _pack(bank, cap=size + 5, write=False)[0] == size                               # NULL with a cap: still the query


def test_pack_other_supports(bank):
    """bands with no weight at all, one-bin bands, a band that is all 513 bins, runs that touch both ends"""
    b = np.zeros((513, 5))
    b[0, 0] = 0.25
    b[512, 1] = 0.5
    b[100:200, 3] = np.linspace(1e-300, 1.0, 100)
    b[:, 4] = 1.0
    n, buf = _pack(b)
    assert n == 10 + 1 + 1 + 100 + 513 and np.array_equal(buf, N.pack(b))
    assert buf[:10].tolist() == [0, 1, 512, 1, 0, 0, 100, 100, 0, 513]
    half = bank[:, ::2]
    n, buf = _pack(half)
    assert n == buf.shape[0] and np.array_equal(buf, N.pack(half))


def test_pack_refusals(bank):
    lib = _capi.lib()
    _refused(lib.ss_mel_nnls_pack(None, 80, None, 0), 'ss_mel_nnls_pack', 'basis_host')
    for n in (0, -1, 4097):
        _refused(lib.ss_mel_nnls_pack(PTR, n, None, 0), 'ss_mel_nnls_pack', 'n_mels outside 1 .. 4096')
    holes = bank.copy()
    holes[np.flatnonzero(bank[:, 40])[1], 40] = 0.0
    _refused(_pack(holes, write=False)[0], 'ss_mel_nnls_pack', 'band 40', 'contiguous')
    two = bank.copy()
    two[500, 2] = 0.1                                                                      # a second run far from the first
    _refused(_pack(two, write=False)[0], 'ss_mel_nnls_pack', 'band 2', 'contiguous')
    for bad in (-1e-300, -1.0, float('nan'), float('inf'), float('-inf')):
        neg = bank.copy()
        neg[17, 9] = bad
        _refused(_pack(neg, write=False)[0], 'ss_mel_nnls_pack', 'band 9, bin 17', 'negative or not finite')
    # sizes: the last that fits, the first that does not
    fits = np.zeros((513, 8))
    fits[:382, :] = 1.0                                                                    # 16 + 8 * 382 = 3072
    assert _pack(fits, write=False)[0] == MAX_PACKED
    fits[382, 0] = 1.0
    _refused(_pack(fits, write=False)[0], 'ss_mel_nnls_pack', '3073 doubles', '3072', 'LDS')
    _refused(_pack(np.ones((513, 80)), write=False)[0], 'ss_mel_nnls_pack', 'LDS')
    _refused(_pack(np.zeros((513, 1537)), write=False)[0], 'ss_mel_nnls_pack', 'LDS')     # 2 n_mels alone is beyond it


def test_every_refusal_of_the_device_call_names_its_argument():
    lib = _capi.lib()
    nan, inf = float('nan'), float('inf')
    call = lambda **k: lib.ss_mel_to_linear_nnls(*[k.get(a, d) for a, d in (
        ('mel', PTR), ('inv', PTR), ('packed', PTR), ('pd', 1101), ('frames', None), ('B', 2), ('F', 9), ('n_mels', 80), ('n_iter', 200),
        ('step', 555.0), ('floor', 1e-10), ('mag', PTR), ('stream', None))])

    def refused(rc, word):
        _refused(rc, 'ss_mel_to_linear_nnls', word)

    # ss_mel_to_linear's refusals
    refused(call(mel=None), 'mel_dev')
    refused(call(inv=None), 'inv_basis_dev')
    refused(call(mag=None), 'mag_dev')
    for B in (0, -3, 65536):
        refused(call(B=B), 'B outside')
    for F in (3, 8193):
        refused(call(F=F), 'max_frames')
    for n in (0, -1, 4097):
        refused(call(n_mels=n), 'n_mels outside 1 .. 4096')
    for f in (-1e-30, nan):
        refused(call(floor=f), 'floor')
    # its own
    refused(call(packed=None), 'packed_dev')
    for it in (-1, 100001):
        refused(call(n_iter=it), 'n_iter outside 0 .. 100000')
    for st in (0.0, -1.0, nan, inf, -inf):
        refused(call(step=st), 'step is not finite and positive')
    for pd in (159, 0, -5):                                                                # below the 2 n_mels of the bands' runs
        refused(call(pd=pd), 'packed_doubles disagrees with n_mels')
    refused(call(pd=1101, n_mels=2), 'packed_doubles disagrees with n_mels')               # above 2 n_mels + 513 n_mels
    refused(call(pd=3073), 'packed_doubles beyond the 3072')
    refused(call(pd=1 << 40), 'packed_doubles')


def test_inversion_argument():
    mel = np.zeros((9, 80), np.float32)
    for fn in (vocoder.mel_to_linear, vocoder.griffin_lim):
        for bad in ('NNLS', 'fista', '', None):
            with pytest.raises(ValueError, match="inversion is 'pinv' or 'nnls'"):
                fn(mel, inversion=bad, device='cpu')
    assert vocoder.INVERSIONS == ('pinv', 'nnls')


def test_python_packs_once_and_passes_the_step(monkeypatch, bank):
    """griffin_lim(inversion='nnls') with the device calls replaced by host stand-ins: the packed bank and 1 / lambda_max reach the call, the
    default path is not touched, and the project's own bank is packed once"""
    import torch
    seen = []

    def fake_nnls(mel_dev, inv_dev, packed_dev, frames_dev, n_iter, step, floor):
        seen.append((packed_dev.numpy().copy(), frames_dev.tolist(), n_iter, step, floor))
        return torch.zeros(mel_dev.shape[0], mel_dev.shape[1], 513, dtype=torch.float64)

    def no_pinv_path(*a):
        raise AssertionError('the pseudo-inverse call on the nnls path')

    monkeypatch.setattr(vocoder, '_mel_to_linear_nnls', fake_nnls)
    monkeypatch.setattr(vocoder, '_mel_to_linear', no_pinv_path)
    monkeypatch.setattr(vocoder, 'griffin_lim_mag', lambda mag, ph, fr, n, m: torch.zeros(mag.shape[0], 256 * (mag.shape[1] - 1), dtype=torch.float64))
    mels = [np.zeros((n, 80), np.float32) for n in (9, 4, 5)]
    out = vocoder.griffin_lim(mels, n_iter=1, max_rows=2, device='cpu', inversion='nnls', nnls_iter=37)
    assert [w.shape[0] for w in out] == [2048, 768, 1024] and len(seen) == 2
    for packed, frames, n_iter, step, floor in seen:
        assert np.array_equal(packed, N.pack(bank)) and n_iter == 37 and floor == 1e-10
        assert abs(step - N.step_of(bank)) <= 1e-12 * step and abs(1.0 / step - 1.7994e-3) < 1e-7
    assert vocoder._nnls_basis(None)[0] is vocoder._nnls_basis(None)[0]                    # cached the way _PINV is
    half = bank[:, ::2]
    p, st = vocoder._nnls_basis(half)
    assert np.array_equal(p, N.pack(half)) and abs(st - N.step_of(half)) <= 1e-12 * st
    with pytest.raises(ValueError, match='513'):
        vocoder._nnls_basis(bank.T)
    with pytest.raises(RuntimeError, match='contiguous'):
        vocoder._nnls_basis(np.eye(513)[:, :4] + np.eye(513)[:, 8:12])
