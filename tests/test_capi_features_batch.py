"""CPU-only checks of the batched feature extraction's interface: the C symbols and their header text, the scratch arithmetic, every refusal
(each is made before anything is enqueued, so a fake non-null device pointer is enough and no device is needed), and the host side of
features.extract_batch: the draw order, the odd-length fix, the packing, the lengths it refuses.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from speechsplit_amd import _capi, convert, features
from tests import filtfilt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    'ss_filtfilt_scratch_bytes': (_l, [_i, _i]),                                                       # B, max_n
    # x, n, B, max_n, b, a, zi, gain, dither, dither_scale, y, scratch, bytes, stream
    'ss_filtfilt': (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _d, _vp, _d, _vp, _vp, _l, _vp]),
    'ss_melspec_batch': (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),                                  # wav, n, B, max_n, mel_basis, n_mels, out, stream
    'ss_f0_normalize_batch': (_i, [_vp, _vp, _i, _i, _d, _vp, _vp]),                                  # f0, n, B, max_n, unvoiced, out, stream
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null, 256-byte aligned; never dereferenced
MAX_N = 256 * 8191                                                                        # ss_pitch_track's cap


def _host(v):
    a = np.ascontiguousarray(v, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_declares_them_between_the_pitch_tracker_and_the_vocoder():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('long ss_filtfilt_scratch_bytes(int B, int max_n);',
                 'int ss_filtfilt(const double* x_dev, const int* n_dev, int B, int max_n, const double* b, const double* a, const double* zi, '
                 'double gain, const double* dither_dev, double dither_scale, double* y_dev, void* scratch_dev, long scratch_bytes, void* stream);',
                 'int ss_melspec_batch(const double* wav_dev, const int* n_dev, int B, int max_n, const double* mel_basis_dev, int n_mels, '
                 'float* out_dev, void* stream);',
                 'int ss_f0_normalize_batch(const double* f0_dev, const int* n_dev, int B, int max_n, double unvoiced, float* out_dev, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_pitch_dp(') < raw.index('long ss_filtfilt_scratch_bytes(') < raw.index(' ss_f0_normalize_batch(const') \
        < raw.index(' ss_griffinlim_samples(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('ext[j] = 2 x[0] - x[-i]', 'ext[j] = 2 x[n-1] - x[2(n-1) - i]', 'y = b0*u + z0', 'z_i = (b_{i+1}*u + z_{i+1}) - a_{i+1}*y',
                   'z4 = b5*u - a5*y', 'z = zi * ext[0]', 'z = zi * v[n+35]', 'j descending', 'y[i] = w[i + 18]',
                   'out[i] = y[i]*gain + (r[i] - 0.5)*dither_scale', 'no fused multiply-add', 'a[0] must be exactly 1', 'HOST arrays',
                   '[B][max_n + 36] doubles', 'No other order is provided', 'in bin order', '(float)unvoiced'):
        assert phrase in whole, phrase


def test_scratch_bytes_arithmetic():
    lib = _capi.lib()
    sb = lib.ss_filtfilt_scratch_bytes
    for B, n in ((1, 513), (3, 2304), (16, 48000), (7, 12345)):
        need = B * (n + 36) * 8
        assert sb(B, n) == (need + 255) // 256 * 256, (B, n)
    assert sb(2, 513) > sb(1, 513) and sb(1, 600) > sb(1, 513)
    big = sb(65535, MAX_N)
    assert big == (65535 * (MAX_N + 36) * 8 + 255) // 256 * 256 and big > 2 ** 32                      # long arithmetic
    for args, word in (((0, 513), b'B'), ((-1, 513), b'B'), ((65536, 513), b'B'), ((1, 512), b'max_n'), ((1, MAX_N + 1), b'max_n')):
        assert sb(*args) == -1
        assert word in lib.ss_last_error(), (args, lib.ss_last_error())
    assert sb(1, MAX_N) > 0


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    b, a, zi = R.coefficients()
    keep = [_host(b), _host(a), _host(zi)]
    nb = lib.ss_filtfilt_scratch_bytes(2, 2304)
    nan, inf = float('nan'), float('inf')
    filt = lambda **k: lib.ss_filtfilt(*[k.get(n, d) for n, d in (('x', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('b', keep[0][1]),
                                                                  ('a', keep[1][1]), ('zi', keep[2][1]), ('gain', 0.96), ('dither', None),
                                                                  ('scale', 1e-6), ('y', PTR), ('scratch', PTR), ('bytes', nb),
                                                                  ('stream', None))])
    mel = lambda **k: lib.ss_melspec_batch(*[k.get(n, d) for n, d in (('wav', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('basis', PTR),
                                                                      ('n_mels', 80), ('out', PTR), ('stream', None))])
    f0n = lambda **k: lib.ss_f0_normalize_batch(*[k.get(n, d) for n, d in (('f0', PTR), ('n', None), ('B', 2), ('max_n', 2304),
                                                                           ('unvoiced', 0.0), ('out', PTR), ('stream', None))])
    # null required pointers
    _refused(filt(x=None), 'x_dev')
    _refused(filt(y=None), 'y_dev')
    _refused(filt(b=None), 'null pointer: b')
    _refused(filt(a=None), 'null pointer: a')
    _refused(filt(zi=None), 'null pointer: zi')
    _refused(filt(scratch=None), 'scratch_dev')
    _refused(mel(wav=None), 'wav_dev')
    _refused(mel(basis=None), 'mel_basis_dev')
    _refused(mel(out=None), 'out_dev')
    _refused(f0n(f0=None), 'f0_dev')
    _refused(f0n(out=None), 'out_dev')
    for call in (filt, mel, f0n):
        _refused(call(B=0), 'B')
        _refused(call(B=-3), 'B')
        _refused(call(max_n=512), 'max_n')
        _refused(call(max_n=0), 'max_n')
        _refused(call(max_n=MAX_N + 1), 'max_n')
    # the coefficients
    for k in range(3):
        name = ('b', 'a', 'zi')[k]
        for pos in (0, len(keep[k][0]) - 1):
            for bad in (nan, inf, -inf):
                v = keep[k][0].copy()
                v[pos] = bad
                _refused(filt(**{name: _host(v)[1]}), f'{name}[{pos}] is not finite')
    for a0 in (1.0 + 2.0 ** -52, 0.5, 0.0, -1.0):
        v = keep[1][0].copy()
        v[0] = a0
        _refused(filt(a=_host(v)[1]), 'a[0] is not exactly 1')
    for bad in (nan, inf, -inf):
        _refused(filt(gain=bad), 'gain')
        _refused(filt(scale=bad), 'dither_scale')
    # the scratch
    _refused(filt(bytes=nb - 1), 'scratch_bytes')
    _refused(filt(bytes=0), 'scratch_bytes')
    _refused(filt(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
    _refused(filt(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')
    _refused(filt(max_n=2400), 'scratch_bytes')                                            # a longer batch needs more scratch
    # the rest
    _refused(mel(n_mels=0), 'n_mels')
    _refused(mel(n_mels=-80), 'n_mels')
    _refused(f0n(unvoiced=nan), 'unvoiced')


def test_wrapper_refuses_other_orders_by_name():
    """only 6 coefficients (pad length 18) are provided; the lengths are checked before the library is touched with them"""
    b, a, zi = R.coefficients()
    x = np.zeros((1, 600))

    class FakeTensor:
        shape = x.shape
    for kw, word in ((dict(b=b[:5]), 'b must have 6'), (dict(a=np.r_[a, 0.0]), 'a must have 6'), (dict(zi=zi[:4]), 'zi must have 5')):
        args = dict(b=b, a=a, zi=zi)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            features.filtfilt_dev(FakeTensor(), None, args['b'], args['a'], args['zi'])


# ---------------------------------------------------------------------------------------------- host side of extract_batch
LENGTHS = [2304, 513, 5000, 1100, 512, 768]


def _recordings():
    rng = np.random.default_rng(11)
    return [rng.uniform(-1.0, 1.0, n) for n in LENGTHS]


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_staging_draws_in_input_order_whatever_max_rows_is(max_rows):
    xs = _recordings()
    prng = np.random.RandomState(226)
    flat, lens, batches = features.stage_batches(xs, prng, max_rows)
    fixed = [R.odd_length_fix(x) for x in xs]                                              # 2304, 512 and 768 grow by the 1e-6 sample
    assert [len(x) for x in fixed] == [2305, 513, 5000, 1100, 513, 769]
    ref = np.random.RandomState(226)
    draws = [ref.rand(len(x)) for x in fixed]                                              # input order, the reference's loop
    assert prng.rand() == ref.rand()                                                        # the generator is left where the loop leaves it
    assert [idx for idx, _, _, _ in batches] == convert.plan_batches([len(x) for x in fixed], max_rows)
    assert flat.dtype == np.float64 and lens.dtype == np.int32
    assert lens.tolist() == [len(fixed[i]) for idx, _, _, _ in batches for i in idx]
    off = 0
    for idx, o, B, max_n in batches:
        assert o == off and B == len(idx) <= max_rows and max_n == len(fixed[idx[-1]])
        xb, rb = flat[o:o + B * max_n].reshape(B, max_n), flat[o + B * max_n:o + 2 * B * max_n].reshape(B, max_n)
        for r, i in enumerate(idx):
            n = len(fixed[i])
            assert np.array_equal(xb[r, :n], fixed[i]) and not xb[r, n:].any()
            assert np.array_equal(rb[r, :n], draws[i]) and not rb[r, n:].any()
        off += 2 * B * max_n
    assert off == flat.shape[0]


def test_staging_refuses_short_recordings_by_position():
    xs = _recordings()
    with pytest.raises(ValueError, match='recording 1 has 511 samples.*n >= 513'):
        features.stage_batches([xs[0], xs[0][:511]], np.random.RandomState(1), 4)
    with pytest.raises(ValueError, match=r'recording 0 must be \[n\]'):
        features.stage_batches([np.zeros((2, 600))], np.random.RandomState(1), 4)
    with pytest.raises(ValueError, match='max_rows'):
        features.stage_batches(xs, np.random.RandomState(1), 0)
    features.stage_batches([xs[0][:512]], np.random.RandomState(1), 4)                     # 512 samples: 513 after the odd-length fix


def test_extract_batch_runs_the_four_calls_on_every_batch(monkeypatch):
    """the device calls replaced by host stand-ins that record what they were handed: the same lengths to every call, the coefficients of
    the reference's filter, 0.96 and 1e-06, the float32 round trip in front of the pitch tracker, results back in input order"""
    import torch
    xs = _recordings()
    seen = []
    b, a, zi = R.coefficients()

    def fake_filt(x, n, b_, a_, zi_, gain, dither, scale):
        assert np.array_equal(b_, b) and np.array_equal(a_, a) and np.array_equal(zi_, zi) and (gain, scale) == (0.96, 1e-06)
        assert x.dtype == torch.float64 and dither.shape == x.shape and n.dtype == torch.int32
        seen.append(n.tolist())
        return x + 0.1234567890123                                                          # not a float32 value

    def fake_mel(wav, n, mb):
        assert mb.shape == (513, 80) and mb.dtype == torch.float64
        return wav[:, :1, None].float().expand(wav.shape[0], wav.shape[1] // 256 + 1, 80).contiguous()

    def fake_pitch(wav, n, lo, hi):
        assert (lo, hi) == (100, 600) and torch.equal(wav, wav.float().double())
        return torch.zeros(wav.shape[0], wav.shape[1] // 256 + 1, dtype=torch.float64)

    def fake_norm(f0, n, max_n, unvoiced):
        assert f0.shape[1] == max_n // 256 + 1 and unvoiced == -1e10
        return n[:, None].float().expand(f0.shape).contiguous()

    monkeypatch.setattr(features, 'filtfilt_dev', fake_filt)
    monkeypatch.setattr(features, 'melspec_batch_dev', fake_mel)
    monkeypatch.setattr(features, 'pitch_track_dev', fake_pitch)
    monkeypatch.setattr(features, 'f0_normalize_batch_dev', fake_norm)
    out = features.extract_batch(xs, np.random.RandomState(3), 'F', max_rows=4, device='cpu', unvoiced=-1e10)
    fixed = [len(R.odd_length_fix(x)) for x in xs]
    assert [n for bt in seen for n in bt] == sorted(fixed) and [len(bt) for bt in seen] == [4, 2]
    for x, n, (S, f0n) in zip(xs, fixed, out):
        F = n // 256 + 1
        assert S.dtype == np.float32 and S.shape == (F, 80) and f0n.dtype == np.float32 and f0n.shape == (F,)
        assert np.all(S == np.float32(x[0] + 0.1234567890123)) and np.all(f0n == n)        # each row's own identity, in input order


def test_make_spect_f0_takes_max_rows_and_defaults_to_the_per_file_path():
    import inspect
    sig = inspect.signature(features.make_spect_f0)
    assert list(sig.parameters)[-1] == 'max_rows' and sig.parameters['max_rows'].default is None
    sig = inspect.signature(features.extract_batch)
    assert list(sig.parameters) == ['xs', 'prng', 'gender', 'max_rows', 'device', 'mel_basis', 'unvoiced']
    assert [sig.parameters[k].default for k in ('max_rows', 'device', 'mel_basis', 'unvoiced')] == [16, 'cuda', None, 0.0]
