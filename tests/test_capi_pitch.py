"""CPU-only checks of the pitch tracker's interface: the C symbols and their header text, the scratch arithmetic, every refusal (each is made
before anything is enqueued, so a fake non-null pointer is enough and no device is needed), and the host side of features.py: f0_range,
read_wav, the batching of pitch_track.  No kernel is launched here."""
import ctypes as C
import os
import re
import wave

import numpy as np
import pytest

from speechsplit_amd import _capi, convert, features, vocoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    'ss_pitch_scratch_bytes': (_l, [_i, _i, _d, _d]),                                     # B, max_n, lo_hz, hi_hz
    'ss_pitch_track': (_i, [_vp, _vp, _i, _i, _d, _d, _d, _vp, _vp, _l, _vp]),            # wav, n, B, max_n, scale, lo, hi, f0, scratch, bytes, stream
    'ss_op_nccf': (_i, [_vp, _vp, _i, _i, _d, _d, _d, _vp, _vp, _vp]),                    # wav, n, B, max_n, scale, lo, hi, phi, rms, stream
    'ss_op_pitch_dp': (_i, [_vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _l, _vp]),           # phi, rms, n, B, max_n, lo, hi, f0, scratch, bytes, stream
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null, 256-byte aligned; never dereferenced
MAX_N = 256 * 8191


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_declares_them_between_f0_normalize_and_the_vocoder():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))                 # comments out: two declarations carry inline ones
    for decl in ('long ss_pitch_scratch_bytes(int B, int max_n, double lo_hz, double hi_hz);',
                 'int ss_pitch_track(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double lo_hz, double hi_hz, '
                 'double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);',
                 'int ss_op_nccf(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double lo_hz, double hi_hz, '
                 'double* phi_dev , double* rms_dev , void* stream);',
                 'int ss_op_pitch_dp(const double* phi_dev, const double* rms_dev, const int* n_dev, int B, int max_n, double lo_hz, '
                 'double hi_hz, double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);'):
        assert decl in text, decl
    assert raw.index('ss_f0_normalize(') < raw.index('long ss_pitch_scratch_bytes(') < raw.index(' ss_op_pitch_dp(') \
        < raw.index(' ss_griffinlim_samples(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('NOT a port of SPTK', 'Talkin 1995', 'CAND_TR = 0.3', 'A_FACT = 10000', 'spectral-stationarity', 'two-rate search',
                   'the lowest b on a tie', 'the smaller lag first on equal v', '-1e10'):
        assert phrase in whole, phrase


def test_scratch_bytes_arithmetic_and_monotonicity():
    lib = _capi.lib()
    sb = lib.ss_pitch_scratch_bytes
    for B, n, lo, hi, K in ((1, 513, 50.0, 250.0, 257), (3, 2304, 100.0, 600.0, 135), (16, 48000, 40.0, 1000.0, 385)):
        F = n // 256 + 1
        assert lib.ss_melspec_frames(n) == F
        got = sb(B, n, lo, hi)
        # phi and rms, three doubles per state (cost, lag, its logarithm), a count and a row of backpointers per frame
        need = B * F * (8 * K + 8 + 3 * 20 * 8 + 4 + 20)
        assert got % 256 == 0 and need <= got <= need + B * F * 12 + 7 * 256, (B, n, got, need)
    assert sb(2, 513, 50.0, 250.0) > sb(1, 513, 50.0, 250.0)                               # more rows
    assert sb(1, 768, 50.0, 250.0) > sb(1, 767, 50.0, 250.0) == sb(1, 513, 50.0, 250.0)    # a new frame every 256 samples
    assert sb(1, 5000, 40.0, 250.0) > sb(1, 5000, 50.0, 250.0) > sb(1, 5000, 50.0, 200.0)  # more lags
    assert sb(65535, MAX_N, 40.0, 1000.0) > 2 ** 40                                        # long arithmetic
    nan = float('nan')
    for args, word in (((0, 513, 50.0, 250.0), b'B'), ((-1, 513, 50.0, 250.0), b'B'), ((65536, 513, 50.0, 250.0), b'B'),
                       ((1, 512, 50.0, 250.0), b'max_n'), ((1, MAX_N + 1, 50.0, 250.0), b'max_n'),
                       ((1, 513, nan, 250.0), b'lo_hz'), ((1, 513, 50.0, nan), b'hi_hz'), ((1, 513, 39.9, 250.0), b'lo_hz'),
                       ((1, 513, 50.0, 1000.5), b'hi_hz'), ((1, 513, 250.0, 50.0), b'lo_hz')):
        assert sb(*args) == -1
        assert word in lib.ss_last_error(), (args, lib.ss_last_error())
    assert sb(1, 513, 40.0, 1000.0) > 0 and sb(1, MAX_N, 50.0, 250.0) > 0                  # the corners are inside


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_pitch_scratch_bytes(2, 2304, 50.0, 250.0)
    nan, inf = float('nan'), float('inf')
    track = lambda **k: lib.ss_pitch_track(*[k.get(a, d) for a, d in (('wav', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('scale', 32768.0),
                                                                      ('lo', 50.0), ('hi', 250.0), ('f0', PTR), ('scratch', PTR), ('bytes', nb),
                                                                      ('stream', None))])
    nccf = lambda **k: lib.ss_op_nccf(*[k.get(a, d) for a, d in (('wav', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('scale', 32768.0),
                                                                 ('lo', 50.0), ('hi', 250.0), ('phi', PTR), ('rms', PTR), ('stream', None))])
    dp = lambda **k: lib.ss_op_pitch_dp(*[k.get(a, d) for a, d in (('phi', PTR), ('rms', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('lo', 50.0),
                                                                   ('hi', 250.0), ('f0', PTR), ('scratch', PTR), ('bytes', nb), ('stream', None))])
    # null required pointers
    _refused(track(wav=None), 'wav_dev')
    _refused(track(f0=None), 'f0_dev')
    _refused(track(scratch=None), 'scratch_dev')
    _refused(nccf(wav=None), 'wav_dev')
    _refused(nccf(phi=None), 'phi_dev')
    _refused(nccf(rms=None), 'rms_dev')
    _refused(dp(phi=None), 'phi_dev')
    _refused(dp(rms=None), 'rms_dev')
    _refused(dp(f0=None), 'f0_dev')
    _refused(dp(scratch=None), 'scratch_dev')
    for call in (track, nccf, dp):
        # shapes
        _refused(call(B=0), 'B')
        _refused(call(B=-3), 'B')
        _refused(call(max_n=512), 'max_n')
        _refused(call(max_n=0), 'max_n')
        _refused(call(max_n=MAX_N + 1), 'max_n')
        # the search range
        _refused(call(lo=nan), 'lo_hz')
        _refused(call(hi=nan), 'hi_hz')
        _refused(call(lo=0.0), 'lo_hz')
        _refused(call(lo=-50.0), 'lo_hz')
        _refused(call(hi=inf), 'hi_hz')
        _refused(call(lo=250.0, hi=250.0), 'lo_hz is not below hi_hz')
        _refused(call(lo=300.0, hi=250.0), 'lo_hz is not below hi_hz')
        _refused(call(hi=1000.1), 'hi_hz')                                                 # Lmin = 15
        _refused(call(lo=39.9), 'lo_hz')                                                   # Lmax = 402
        _refused(call(lo=999.0, hi=1000.0), 'fewer than 3 lags')                           # Lmin = 16, Lmax = 17
    for call in (track, nccf):
        for sc in (0.0, -1.0, nan, inf):
            _refused(call(scale=sc), 'scale')
    for call in (track, dp):
        _refused(call(bytes=nb - 1), 'scratch_bytes')
        _refused(call(bytes=0), 'scratch_bytes')
        _refused(call(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
        _refused(call(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')
        _refused(call(lo=40.0, hi=1000.0), 'scratch_bytes')                                # more lags need more scratch


# ---------------------------------------------------------------------------------------------- host side of features.py
def test_f0_range():
    assert features.f0_range('M') == (50, 250) and features.f0_range('F') == (100, 600)
    for bad in ('m', 'X', None, ''):
        with pytest.raises(ValueError, match="'M' or 'F'"):
            features.f0_range(bad)


def test_read_wav_round_trips_save_wav(tmp_path):
    x = np.concatenate([np.sin(2 * np.pi * 440 * np.arange(800) / 16000) * 0.5, [1.0, -1.0, 0.0, 0.25]])
    path = str(tmp_path / 'a.wav')
    vocoder.save_wav(path, x)
    got = features.read_wav(path)
    assert got.dtype == np.float64 and got.shape == x.shape
    assert np.array_equal(got * 32768.0, np.round(x * 32767.0))                            # the PCM values themselves, over 32768
    assert np.abs(got - x).max() <= 1.5 / 32768
    # other formats are refused by name
    vocoder.save_wav(path, x[:10], sr=22050)
    with pytest.raises(ValueError, match='sample rate 22050'):
        features.read_wav(path)
    for ch, width, word in ((2, 2, '2 channels'), (1, 1, '8-bit'), (1, 4, '32-bit')):
        with wave.open(path, 'wb') as f:
            f.setnchannels(ch)
            f.setsampwidth(width)
            f.setframerate(16000)
            f.writeframes(bytes(ch * width * 8))
        with pytest.raises(ValueError, match=word):
            features.read_wav(path)


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_pitch_track_batches_and_returns_input_order(monkeypatch, max_rows):
    """the batching of pitch_track with the device call replaced by a host stand-in that records what it was handed: plan_batches order, each
    row's own length, zeros behind it, samples rounded through float32 -- and the results back in input order whatever max_rows is"""
    import torch
    lengths = [2304, 513, 5000, 1100, 513]
    rng = np.random.default_rng(4)
    wavs = [rng.uniform(-1.0, 1.0, n) for n in lengths]
    seen = []

    def fake_track(wav_dev, n_dev, lo, hi, scale=32768.0):
        B, max_n = wav_dev.shape
        ns = n_dev.tolist()
        seen.append(ns)
        assert wav_dev.dtype == torch.float64 and n_dev.dtype == torch.int32 and (lo, hi, scale) == (50, 250, 32768.0)
        assert ns == sorted(ns) and ns[-1] == max_n and B <= max_rows
        f0 = torch.full((B, max_n // 256 + 1), -1e10, dtype=torch.float64)
        for b in range(B):
            assert not wav_dev[b, ns[b]:].any()
            assert torch.equal(wav_dev[b, :ns[b]], wav_dev[b, :ns[b]].float().double())     # float32 values
            f0[b, :ns[b] // 256 + 1] = wav_dev[b, 0]                                        # carries the row's identity through
        return f0

    monkeypatch.setattr(features, 'pitch_track_dev', fake_track)
    out = features.pitch_track(wavs, 50, 250, max_rows=max_rows, device='cpu')
    for n, w, f0 in zip(lengths, wavs, out):
        assert f0.dtype == np.float64 and f0.shape == (n // 256 + 1,) and np.all(f0 == np.float64(np.float32(w[0])))
    assert [n for b in seen for n in b] == sorted(lengths)
    assert [len(b) for b in seen] == [len(b) for b in convert.plan_batches(lengths, max_rows)]
    one = features.pitch_track(wavs[3], 50, 250, max_rows=max_rows, device='cpu')
    assert isinstance(one, np.ndarray) and one.shape == (5,)
    with pytest.raises(ValueError, match='n >= 513'):
        features.pitch_track([wavs[0], wavs[0][:512]], 50, 250, device='cpu')


def test_dropin_script_calls_the_directory_walk():
    text = open(os.path.join(ROOT, 'dropin', 'make_spect_f0.py')).read()
    assert 'from speechsplit_amd.features import make_spect_f0' in text
    for word in ("'assets/wavs'", "'assets/spmel'", "'assets/raptf0'", "'assets/spk2gen.pkl'"):
        assert word in text
