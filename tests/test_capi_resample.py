"""CPU-only checks of the resampler's interface: the C symbols and their header text, ss_resample_len against scipy's output lengths, every
refusal (each is made before anything is enqueued, so a fake non-null device pointer is enough and no device is needed), features.read_audio
at every sample width, and the host side of features.resample / extract_batch_sr / make_spect_f0(resample=...) with the device calls
replaced by host stand-ins: the grouping by rate, the plan_batches order, the draws on the resampled lengths in input order.  No kernel is
launched here."""
import ctypes as C
import inspect
import os
import re
import struct
import wave

import numpy as np
import pytest
from scipy import signal

from speechsplit_amd import _capi, convert, features
from tests import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
SIGNATURES = {
    'ss_resample_len': (_l, [_l, _i, _i]),                                                # n, up, down
    'ss_resample_scratch_bytes': (_l, [_i, _i]),                                          # up, n_taps
    # x, n, B, max_n, up, down, h, n_taps, y, scratch, bytes, stream
    'ss_resample': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _l, _vp]),
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null, 256-byte aligned; never dereferenced


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_declares_them_with_the_batched_feature_calls():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('long ss_resample_len(long n, int up, int down);', 'long ss_resample_scratch_bytes(int up, int n_taps);',
                 'int ss_resample(const double* x_dev, const int* n_dev, int B, int max_n, int up, int down, const double* h_dev, int n_taps, '
                 'double* y_dev, void* scratch_dev, long scratch_bytes, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_f0_normalize_batch(const') < raw.index('long ss_resample_len(') < raw.index(' ss_resample(const') \
        < raw.index(' ss_griffinlim_samples(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('half = (n_taps - 1) / 2', 'n_b = min(max(n[b], 1), max_n)', 'm_b = ceil(n_b up / down)', 'M = ceil(max_n up / down)',
                   'y[b][m] = 0.0 + sum over k of x[b][k] * h[m*down + half - k*up]', '0 <= k < n_b and 0 <= m*down + half - k*up < n_taps',
                   'k ascending', 'no fused multiply-add', 'columns m_b .. M - 1', 'NaN * 0 is NaN', "window=('kaiser', 5.0)) * up",
                   'ON THE DEVICE', 'in long', 'scratch_dev may then be NULL'):
        assert phrase in whole, phrase


def test_resample_len_is_scipys_output_length():
    lib = _capi.lib()
    for sr_in, sr_out in ((48000, 16000), (44100, 16000), (32000, 16000), (24000, 16000), (22050, 16000), (11025, 16000), (8000, 16000),
                          (16000, 48000), (16000, 44100)):
        up, down = R.ratio(sr_in, sr_out)
        for n in (1, 2, 5, 17, 255, 256, 257, 769, 1539):
            want = signal.resample_poly(np.zeros(n), sr_out, sr_in).shape[0]
            assert lib.ss_resample_len(n, up, down) == want == features.resample_len(n, up, down) == R.out_len(n, up, down), (sr_in, sr_out, n)
    assert lib.ss_resample_len(0, 1, 3) == 0
    assert lib.ss_resample_len(1 << 40, 1024, 1) == 1 << 50                                # long arithmetic
    for args, word in (((-1, 1, 3), b'n'), (((1 << 40) + 1, 1, 3), b'n'), ((5, 0, 3), b'up'), ((5, 1025, 3), b'up'), ((5, 1, 0), b'down'),
                       ((5, 1, -2), b'down'), ((5, 1, 1025), b'down')):
        assert lib.ss_resample_len(*args) == -1
        assert b'ss_resample_len: ' + word + b' ' in lib.ss_last_error(), (args, lib.ss_last_error())
    sb = lib.ss_resample_scratch_bytes
    assert sb(160, 8821) >= 0 and sb(1, 61) >= 0 and sb(1024, 1) >= 0
    for args, word in (((0, 61), b'up'), ((1025, 61), b'up'), ((1, 0), b'n_taps'), ((1, -3), b'n_taps'), ((1, 60), b'n_taps is even')):
        assert sb(*args) == -1
        assert word in lib.ss_last_error(), (args, lib.ss_last_error())


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_resample_scratch_bytes(160, 8821)
    call = lambda **k: lib.ss_resample(*[k.get(a, d) for a, d in (('x', PTR), ('n', None), ('B', 2), ('max_n', 3000), ('up', 160), ('down', 441),
                                                                  ('h', PTR), ('n_taps', 8821), ('y', PTR), ('scratch', PTR), ('bytes', nb),
                                                                  ('stream', None))])
    _refused(call(x=None), 'null pointer: x_dev')
    _refused(call(h=None), 'null pointer: h_dev')
    _refused(call(y=None), 'null pointer: y_dev')
    for B in (0, -3, 65536):
        _refused(call(B=B), 'B outside 1 .. 65535')
    for n in (0, -5):
        _refused(call(max_n=n), 'max_n below 1')
    for v in (0, -1, 1025):
        _refused(call(up=v), 'up outside 1 .. 1024')
        _refused(call(down=v), 'down outside 1 .. 1024')
    for t in (0, -61):
        _refused(call(n_taps=t), 'n_taps below 1')
    for t in (2, 8820):
        _refused(call(n_taps=t), 'n_taps is even')
    _refused(call(max_n=1 << 30, up=3, down=1), 'max_n: M = ceil(max_n up / down) does not fit an int')
    _refused(call(max_n=(1 << 31) - 1, up=1024, down=1023), 'does not fit an int')
    _refused(call(bytes=nb - 1), 'scratch_bytes below ss_resample_scratch_bytes')
    _refused(call(bytes=-256), 'scratch_bytes')
    _refused(call(scratch=C.c_void_p((1 << 20) + 128)), 'scratch_dev is not 256-byte aligned')
    _refused(call(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')
    if nb > 0:
        _refused(call(scratch=None), 'null pointer: scratch_dev')


def test_rate_ratio_reduces_and_refuses():
    assert features.rate_ratio(48000) == (1, 3) and features.rate_ratio(44100) == (160, 441) and features.rate_ratio(22050) == (320, 441)
    assert features.rate_ratio(11025) == (640, 441) and features.rate_ratio(16000, 48000) == (3, 1) and features.rate_ratio(16000) == (1, 1)
    for bad in ((16001, 16000), (0, 16000), (44100.5, 16000), (16000, -1)):
        with pytest.raises(ValueError, match='rate_ratio'):
            features.rate_ratio(*bad)
    for up, down in ((1, 3), (160, 441), (3, 1)):
        assert np.array_equal(features.resample_filter(up, down), R.design(up, down))


# ---------------------------------------------------------------------------------------------- read_audio
def _write(path, pcm, width, sr, channels=1):
    with wave.open(path, 'wb') as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(sr)
        if width == 1:
            f.writeframes((pcm + 128).astype(np.uint8).tobytes())
        elif width == 3:
            f.writeframes(b''.join(struct.pack('<i', int(v))[:3] for v in pcm))
        else:
            f.writeframes(pcm.astype('<i2' if width == 2 else '<i4').tobytes())


@pytest.mark.parametrize('width', [1, 2, 3, 4])
def test_read_audio_round_trips_every_width_at_several_rates(tmp_path, width):
    bits = 8 * width
    top = 1 << (bits - 1)
    rng = np.random.default_rng(width)
    pcm = np.concatenate([[-top, top - 1, 0, -1, 1], rng.integers(-top, top, 300)]).astype(np.int64)
    for sr in (8000, 16000, 22050, 44100, 48000):
        path = str(tmp_path / f'a{sr}.wav')
        _write(path, pcm, width, sr)
        x, got_sr = features.read_audio(path)
        assert got_sr == sr and x.dtype == np.float64 and x.shape == pcm.shape
        assert np.array_equal(x * top, pcm) and x.min() == -1.0 and x.max() == (top - 1) / top   # the PCM values over 2^(bits - 1)
    path = str(tmp_path / 'b.wav')
    _write(path, np.zeros(8, np.int64), width, 16000, channels=2)
    with pytest.raises(ValueError, match='2 channels; mono only'):
        features.read_audio(path)


def test_read_audio_agrees_with_read_wav_and_refuses_float_and_extensible_files(tmp_path):
    from speechsplit_amd import vocoder
    x = np.sin(2 * np.pi * 440 * np.arange(800) / 16000) * 0.5
    path = str(tmp_path / 'a.wav')
    vocoder.save_wav(path, x)
    got, sr = features.read_audio(path)
    assert sr == 16000 and np.array_equal(got, features.read_wav(path))
    for tag in (3, 0xFFFE):                                                                # IEEE float, WAVE_FORMAT_EXTENSIBLE
        fmt = struct.pack('<HHIIHH', tag, 1, 16000, 64000, 4, 32)
        data = struct.pack('<4f', 0.0, 0.5, -0.5, 0.25)
        body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'data' + struct.pack('<I', len(data)) + data
        with open(path, 'wb') as f:
            f.write(b'RIFF' + struct.pack('<I', len(body)) + body)
        with pytest.raises(ValueError, match=f'unknown format: {tag}; integer PCM WAV only'):
            features.read_audio(path)


# ---------------------------------------------------------------------------------------------- host side, the device calls replaced
LENGTHS = [2304, 1600, 5000, 1100, 1539, 3072]


def _recordings():
    rng = np.random.default_rng(12)
    return [rng.uniform(-1.0, 1.0, n) for n in LENGTHS]


def _fake_resample_dev(seen):
    """the device call on the host: the restatement on every row, zeros behind a row's own outputs; records (up, down, lengths)"""
    import torch

    def fake(x_dev, n_dev, up, down, h_dev):
        B, max_n = x_dev.shape
        ns = n_dev.tolist()
        assert x_dev.dtype == torch.float64 and n_dev.dtype == torch.int32 and h_dev.dtype == torch.float64
        assert ns == sorted(ns) and ns[-1] == max_n
        assert np.array_equal(h_dev.numpy(), R.design(up, down))
        seen.append((up, down, ns))
        y = torch.zeros(B, R.out_len(max_n, up, down), dtype=torch.float64)
        for b in range(B):
            assert not x_dev[b, ns[b]:].any()
            row = R.resample(x_dev[b].numpy(), up, down, h_dev.numpy(), n=ns[b])
            y[b, :row.shape[0]] = torch.from_numpy(row)
        return y
    return fake


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_resample_batches_and_returns_input_order(monkeypatch, max_rows):
    xs = _recordings()
    seen = []
    monkeypatch.setattr(features, 'resample_dev', _fake_resample_dev(seen))
    out = features.resample(xs, 44100, max_rows=max_rows, device='cpu')
    for x, y in zip(xs, out):
        assert R.same(y, signal.resample_poly(x, 16000, 44100))                            # input order, whatever max_rows is
    assert all((up, down) == (160, 441) for up, down, _ in seen)
    assert [ns for _, _, ns in seen] == [[LENGTHS[i] for i in b] for b in convert.plan_batches(LENGTHS, max_rows)]
    one = features.resample(xs[3], 48000, 16000, max_rows=max_rows, device='cpu')
    assert isinstance(one, np.ndarray) and R.same(one, signal.resample_poly(xs[3], 1, 3))
    up3 = features.resample(xs[3][:300], 16000, 48000, device='cpu')
    assert R.same(up3, signal.resample_poly(xs[3][:300], 3, 1))
    # the same rate: copies, as scipy returns, and no device call
    calls = len(seen)
    same = features.resample(xs[:2], 16000, device='cpu')
    assert len(seen) == calls and all(np.array_equal(a, b) and a is not b for a, b in zip(same, xs))
    with pytest.raises(ValueError, match=r'recording 1 must be \[n\]'):
        features.resample([xs[0], np.zeros((2, 5))], 48000, device='cpu')
    with pytest.raises(ValueError, match='recording 0'):
        features.resample([np.zeros(0)], 48000, device='cpu')


def _fake_chain(monkeypatch, log):
    """extract_batch's four device calls as host stand-ins that record the rows and draws they were handed"""
    import torch

    def fake_filt(x, n, b_, a_, zi_, gain, dither, scale):
        assert (gain, scale) == (0.96, 1e-06) and x.dtype == torch.float64 and dither.shape == x.shape and n.dtype == torch.int32
        log.append((n.tolist(), x.numpy().copy(), dither.numpy().copy()))
        return x + 0.1234567890123

    def fake_mel(wav, n, mb):
        return wav[:, :1, None].float().expand(wav.shape[0], wav.shape[1] // 256 + 1, 80).contiguous()

    def fake_pitch(wav, n, lo, hi):
        assert (lo, hi) == (100, 600) and torch.equal(wav, wav.float().double())
        return torch.zeros(wav.shape[0], wav.shape[1] // 256 + 1, dtype=torch.float64)

    def fake_norm(f0, n, max_n, unvoiced):
        return n[:, None].float().expand(f0.shape).contiguous()

    monkeypatch.setattr(features, 'filtfilt_dev', fake_filt)
    monkeypatch.setattr(features, 'melspec_batch_dev', fake_mel)
    monkeypatch.setattr(features, 'pitch_track_dev', fake_pitch)
    monkeypatch.setattr(features, 'f0_normalize_batch_dev', fake_norm)


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_extract_batch_sr_groups_by_rate_and_draws_on_the_resampled_lengths(monkeypatch, max_rows):
    xs = _recordings()
    srs = [48000, 44100, 48000, 16000, 44100, 48000]
    seen, log = [], []
    monkeypatch.setattr(features, 'resample_dev', _fake_resample_dev(seen))
    _fake_chain(monkeypatch, log)
    prng = np.random.RandomState(226)
    out = features.extract_batch_sr(xs, srs, prng, 'F', max_rows=max_rows, device='cpu', unvoiced=-1e10)
    # what the 16 kHz path is handed: scipy's resampling, then the odd-length fix on the RESAMPLED length (2304 and 3072 at 48 kHz: 768, 1024)
    at16 = [x.copy() if sr == 16000 else signal.resample_poly(x, 16000, sr) for x, sr in zip(xs, srs)]
    assert [len(y) for y in at16] == [768, 581, 1667, 1100, 559, 1024]
    fixed = [np.concatenate((y, [1e-06])) if len(y) % 256 == 0 else y for y in at16]
    assert [len(y) for y in fixed] == [769, 581, 1667, 1100, 559, 1025]
    ref = np.random.RandomState(226)
    draws = [ref.rand(len(y)) for y in fixed]                                              # input order, on the resampled lengths
    assert prng.rand() == ref.rand()                                                        # the generator is left where the loop leaves it
    # the resampler saw each rate's recordings together, each group in plan_batches order, 16 kHz recordings not at all
    for ratio, members in (((1, 3), [0, 2, 5]), ((160, 441), [1, 4])):
        got = [ns for up, down, ns in seen if (up, down) == ratio]
        lens = [LENGTHS[i] for i in members]
        assert got == [[lens[i] for i in b] for b in convert.plan_batches(lens, max_rows)], ratio
    assert {(up, down) for up, down, _ in seen} == {(1, 3), (160, 441)}
    # the chain saw the resampled recordings in plan_batches order of their fixed lengths, each row with its own draw
    plan = convert.plan_batches([len(y) for y in fixed], max_rows)
    assert [ns for ns, _, _ in log] == [[len(fixed[i]) for i in b] for b in plan]
    for b, (ns, x, r) in zip(plan, log):
        for k, i in enumerate(b):
            assert np.array_equal(x[k, :ns[k]], fixed[i]) and not x[k, ns[k]:].any(), i     # scipy's bits, the 1e-6 sample where it belongs
            assert np.array_equal(r[k, :ns[k]], draws[i]) and not r[k, ns[k]:].any(), i
    for y, (S, f0n) in zip(fixed, out):
        F = len(y) // 256 + 1
        assert S.dtype == np.float32 and S.shape == (F, 80) and f0n.dtype == np.float32 and f0n.shape == (F,)
        assert np.all(S == np.float32(y[0] + 0.1234567890123)) and np.all(f0n == len(y))   # each row's own identity, in input order
    # one rate for all
    log.clear()
    one = features.extract_batch_sr(xs[:2], 48000, np.random.RandomState(1), 'F', max_rows=max_rows, device='cpu')
    assert [S.shape[0] for S, _ in one] == [769 // 256 + 1, 534 // 256 + 1]
    with pytest.raises(ValueError, match='recording 1 has 367 samples at 16 kHz'):
        features.extract_batch_sr([xs[0], xs[3]], 48000, np.random.RandomState(1), 'F', device='cpu')
    with pytest.raises(ValueError, match='2 sample rates for 3 recordings'):
        features.extract_batch_sr(xs[:3], [48000, 16000], np.random.RandomState(1), 'F', device='cpu')


def test_at_16_khz_the_calls_made_are_todays(monkeypatch):
    xs = _recordings()
    handed = []

    def spy(*args):
        handed.append(args)
        return 'result'

    def never(*args):
        raise AssertionError('the resampler has nothing to do at 16 kHz')

    monkeypatch.setattr(features, 'extract_batch', spy)
    monkeypatch.setattr(features, 'resample_dev', never)
    prng = np.random.RandomState(5)
    for sr in (16000, [16000] * len(xs)):
        assert features.extract_batch_sr(xs, sr, prng, 'M', 4, 'cpu', None, -1e10) == 'result'
        got = handed.pop()
        assert all(np.array_equal(a, b) for a, b in zip(got[0], xs)) and got[1] is prng and got[2:] == ('M', 4, 'cpu', None, -1e10)
    # extract with the default rate does not touch the resampler either; signatures: the new arguments default to today's behaviour
    sig = inspect.signature(features.extract)
    assert list(sig.parameters)[-1] == 'sr' and sig.parameters['sr'].default == 16000
    sig = inspect.signature(features.make_spect_f0)
    assert list(sig.parameters)[-2:] == ['resample', 'max_rows'] and sig.parameters['resample'].default is False
    with pytest.raises(TypeError, match='resample must be True or False'):
        features.make_spect_f0('nowhere', 'a', 'b', {}, 'cpu', 4)
    sig = inspect.signature(features.resample)
    assert list(sig.parameters) == ['xs', 'sr_in', 'sr_out', 'max_rows', 'device']
    assert [sig.parameters[k].default for k in ('sr_out', 'max_rows', 'device')] == [16000, 16, 'cuda']
