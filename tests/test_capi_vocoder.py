"""CPU-only checks of the Griffin-Lim vocoder's interface: the C symbols and their header text, the sample / frame arithmetic, every refusal
(each is made before anything is enqueued, so a fake non-null pointer is enough and no device is needed), the host side of
vocoder.griffin_lim (ordering, draws, batching plan) and save_wav.  No kernel is launched here."""
import ctypes as C
import os
import re
import wave

import numpy as np
import pytest

from speechsplit_amd import _capi, convert, vocoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    'ss_griffinlim_samples': (_i, [_i]),                                                  # frames
    'ss_griffinlim_scratch_bytes': (_l, [_i, _i]),                                        # B, max_frames
    'ss_mel_to_linear': (_i, [_vp, _vp, _vp, _i, _i, _i, _d, _vp, _vp]),                  # mel, inv_basis, frames, B, max_frames, n_mels, floor, mag, stream
    'ss_griffinlim': (_i, [_vp, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _l, _vp]),            # mag, phase0, frames, B, max_frames, n_iter, momentum, wav, scratch, bytes, stream
    'ss_op_stft': (_i, [_vp, _vp, _i, _i, _vp, _vp]),                                     # wav, frames, B, max_frames, spec, stream
    'ss_op_istft': (_i, [_vp, _vp, _i, _i, _vp, _vp, _l, _vp]),                           # spec, frames, B, max_frames, wav, scratch, bytes, stream
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


def test_header_declares_them():
    text = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read())
    for decl in ('int ss_griffinlim_samples(int frames);',
                 'long ss_griffinlim_scratch_bytes(int B, int max_frames);',
                 'int ss_mel_to_linear(const float* mel_dev, const double* inv_basis_dev, const int* frames_dev, int B, int max_frames, '
                 'int n_mels, double floor, double* mag_dev, void* stream);',
                 'int ss_griffinlim(const double* mag_dev, const double* phase0_dev, const int* frames_dev, int B, int max_frames, int n_iter, '
                 'double momentum, double* wav_dev, void* scratch_dev, long scratch_bytes, void* stream);',
                 'int ss_op_stft (const double* wav_dev, const int* frames_dev, int B, int max_frames, double* spec_dev, void* stream);',
                 'int ss_op_istft(const double* spec_dev, const int* frames_dev, int B, int max_frames, double* wav_dev, '
                 'void* scratch_dev, long scratch_bytes, void* stream);'):
        assert decl in text, decl
    assert text.index('ss_f0_normalize(') < text.index('int ss_griffinlim_samples(') < text.index('int ss_collate(')


def test_samples_and_frames():
    lib = _capi.lib()
    assert [lib.ss_griffinlim_samples(F) for F in (0, 3, 4, 192)] == [0, 0, 768, 48896]
    assert lib.ss_griffinlim_samples(-7) == 0
    for F in (4, 5, 9, 41, 192, 8192):
        assert lib.ss_melspec_frames(lib.ss_griffinlim_samples(F)) == F


def test_scratch_bytes():
    lib = _capi.lib()
    small, big = lib.ss_griffinlim_scratch_bytes(1, 4), lib.ss_griffinlim_scratch_bytes(7, 192)
    # the windowed time frames and two complex spectra per frame
    assert small >= 4 * (1024 + 2 * 2 * 513) * 8 and small % 256 == 0
    assert big >= 7 * 192 * (1024 + 2 * 2 * 513) * 8 and big % 256 == 0
    assert lib.ss_griffinlim_scratch_bytes(65535, 8192) > 2 ** 32                          # long arithmetic
    for B, F, word in ((0, 9, b'B'), (-1, 9, b'B'), (1, 3, b'max_frames'), (1, 8193, b'max_frames')):
        assert lib.ss_griffinlim_scratch_bytes(B, F) == -1
        assert word in lib.ss_last_error(), (B, F, lib.ss_last_error())


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_griffinlim_scratch_bytes(2, 9)
    nan = float('nan')
    mel = lambda **k: lib.ss_mel_to_linear(*[k.get(a, d) for a, d in (('mel', PTR), ('inv', PTR), ('frames', None), ('B', 2), ('F', 9), ('n_mels', 80),
                                                                      ('floor', 1e-10), ('mag', PTR), ('stream', None))])
    gl = lambda **k: lib.ss_griffinlim(*[k.get(a, d) for a, d in (('mag', PTR), ('phase0', None), ('frames', None), ('B', 2), ('F', 9), ('n_iter', 4),
                                                                  ('momentum', 0.99), ('wav', PTR), ('scratch', PTR), ('bytes', nb), ('stream', None))])
    stft = lambda **k: lib.ss_op_stft(*[k.get(a, d) for a, d in (('wav', PTR), ('frames', None), ('B', 2), ('F', 9), ('spec', PTR), ('stream', None))])
    istft = lambda **k: lib.ss_op_istft(*[k.get(a, d) for a, d in (('spec', PTR), ('frames', None), ('B', 2), ('F', 9), ('wav', PTR), ('scratch', PTR),
                                                                   ('bytes', nb), ('stream', None))])
    # null required pointers
    _refused(mel(mel=None), 'mel_dev')
    _refused(mel(inv=None), 'inv_basis_dev')
    _refused(mel(mag=None), 'mag_dev')
    _refused(gl(mag=None), 'mag_dev')
    _refused(gl(wav=None), 'wav_dev')
    _refused(gl(scratch=None), 'scratch_dev')
    _refused(stft(wav=None), 'wav_dev')
    _refused(stft(spec=None), 'spec_dev')
    _refused(istft(spec=None), 'spec_dev')
    _refused(istft(wav=None), 'wav_dev')
    _refused(istft(scratch=None), 'scratch_dev')
    # shapes
    for call in (mel, gl, stft, istft):
        _refused(call(B=0), 'B')
        _refused(call(B=-3), 'B')
        _refused(call(F=3), 'max_frames')
        _refused(call(F=8193), 'max_frames')
    _refused(mel(n_mels=0), 'n_mels')
    # scalars
    _refused(gl(n_iter=-1), 'n_iter')
    _refused(gl(n_iter=1025), 'n_iter')
    for m in (-0.01, 1.0, 1.5, nan):
        _refused(gl(momentum=m), 'momentum')
    for f in (-1e-30, nan):
        _refused(mel(floor=f), 'floor')
    # scratch
    for call in (gl, istft):
        _refused(call(bytes=nb - 1), 'scratch_bytes')
        _refused(call(bytes=0), 'scratch_bytes')
        _refused(call(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
        _refused(call(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')


# ---------------------------------------------------------------------------------------------- host side of griffin_lim
def _mels(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 1.0, (n, 80)).astype(np.float32) for n in lengths]


def test_prepare_draws_per_utterance_in_input_order():
    lengths = [41, 4, 9, 5, 9]
    mels = _mels(lengths)
    single, ms, ps = vocoder.prepare(mels, None, np.random.default_rng(5))
    assert not single and [m.shape for m in ms] == [(n, 80) for n in lengths]
    gen = np.random.default_rng(5)
    for n, p in zip(lengths, ps):                                       # the same generator calls, in the order the utterances were given
        ref = gen.uniform(-np.pi, np.pi, (n, 513))
        assert p.dtype == np.float64 and np.array_equal(p, ref)
        assert p.min() >= -np.pi and p.max() < np.pi
    # the default generator is seeded: two calls draw the same phases
    assert all(np.array_equal(a, b) for a, b in zip(vocoder.prepare(mels)[2], vocoder.prepare(mels)[2]))
    # one array in, one array out; given phases are taken as they are; 'zero' hands the C call a null pointer
    single, ms, ps = vocoder.prepare(mels[0], ps[0])
    assert single and len(ms) == 1 and ps[0].shape == (41, 513)
    assert vocoder.prepare(mels, 'zero')[2] is None


def test_prepare_refuses_bad_inputs():
    with pytest.raises(ValueError, match='L >= 4'):
        vocoder.prepare(_mels([9, 3]))
    with pytest.raises(ValueError, match='n_mels'):
        vocoder.prepare([np.zeros((9, 80), np.float32), np.zeros((9, 40), np.float32)])
    with pytest.raises(ValueError, match='one \\[L, 513\\]'):
        vocoder.prepare(_mels([9, 5]), [np.zeros((9, 513))])
    with pytest.raises(ValueError, match='one \\[L, 513\\]'):
        vocoder.prepare(_mels([9]), [np.zeros((8, 513))])
    with pytest.raises(ValueError, match="'zero'"):
        vocoder.prepare(_mels([9]), 'random')


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_griffin_lim_batches_and_returns_input_order(monkeypatch, max_rows):
    """the batching of griffin_lim with the two device calls replaced by host stand-ins that record what they were handed: plan_batches order,
    each row's own frame count, padding behind it, the row's own draws -- and the results back in input order whatever max_rows is"""
    import torch
    lengths = [41, 4, 9, 5, 9]
    mels = _mels(lengths, 3)
    seen = []

    def fake_mel_to_linear(mel_dev, inv_dev, frames_dev, floor):
        assert mel_dev.dtype == torch.float32 and inv_dev.shape == (80, 513) and inv_dev.dtype == torch.float64
        mag = torch.zeros(mel_dev.shape[0], mel_dev.shape[1], 513, dtype=torch.float64)
        mag[:, :, 0] = mel_dev[:, :, 0].double()                          # carries the row's identity through
        return mag

    def fake_griffin_lim(mag, phase0, frames, n_iter, momentum):
        B, T = mag.shape[:2]
        fr = frames.tolist()
        seen.append(fr)
        assert fr == sorted(fr) and fr[-1] == T and B <= max_rows and (n_iter, momentum) == (7, 0.5)
        wav = torch.zeros(B, 256 * (T - 1), dtype=torch.float64)
        for b in range(B):
            assert float(mag[b, fr[b]:].abs().max() if fr[b] < T else 0.0) == 0.0 and float(phase0[b, fr[b]:].abs().max() if fr[b] < T else 0.0) == 0.0
            wav[b, :256 * (fr[b] - 1)] = mag[b, 0, 0] + phase0[b, 0, 0]
        return wav

    monkeypatch.setattr(vocoder, '_mel_to_linear', fake_mel_to_linear)
    monkeypatch.setattr(vocoder, 'griffin_lim_mag', fake_griffin_lim)
    out = vocoder.griffin_lim(mels, n_iter=7, momentum=0.5, generator=np.random.default_rng(9), max_rows=max_rows, device='cpu')
    gen = np.random.default_rng(9)
    for n, m, w in zip(lengths, mels, out):
        ph = gen.uniform(-np.pi, np.pi, (n, 513))
        assert w.dtype == np.float64 and w.shape == (256 * (n - 1),)
        assert np.all(w == float(m[0, 0]) + ph[0, 0])
    assert [i for b in seen for i in b] == sorted(lengths)
    assert [len(b) for b in seen] == [len(b) for b in convert.plan_batches(lengths, max_rows)]
    # one array in, one array out
    one = vocoder.griffin_lim(mels[2], n_iter=7, momentum=0.5, generator=np.random.default_rng(9), max_rows=max_rows, device='cpu')
    assert isinstance(one, np.ndarray) and one.shape == (256 * 8,)


def test_conversion_waveforms_keeps_names_and_order(monkeypatch):
    results = [('p1_p2_u_R', np.zeros((9, 80), np.float32)), ('p1_p2_u_F', np.zeros((5, 80), np.float32))]
    monkeypatch.setattr(vocoder, 'griffin_lim', lambda mels, **kw: [np.full(256 * (m.shape[0] - 1), kw['n_iter'], np.float64) for m in mels])
    out = convert.conversion_waveforms(results, n_iter=3)
    assert [n for n, _ in out] == ['p1_p2_u_R', 'p1_p2_u_F'] and [w.shape for _, w in out] == [(2048,), (1024,)]
    assert all(np.all(w == 3) for _, w in out)


def test_save_wav_round_trips_through_wave(tmp_path):
    x = np.concatenate([np.sin(2 * np.pi * 440 * np.arange(800) / 16000) * 0.5, [1.7, -1.7, 1.0, -1.0, 0.0]])
    path = str(tmp_path / 'a.wav')
    vocoder.save_wav(path, x)
    with wave.open(path, 'rb') as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 16000, x.shape[0])
        pcm = np.frombuffer(f.readframes(f.getnframes()), '<i2')
    assert np.array_equal(pcm, np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))
    assert pcm[-5:].tolist() == [32767, -32767, 32767, -32767, 0]                          # clipped, not wrapped
    assert np.abs(pcm / 32767.0 - np.clip(x, -1, 1)).max() <= 0.5 / 32767 + 1e-12
    vocoder.save_wav(path, x[:10], sr=22050)
    with wave.open(path, 'rb') as f:
        assert f.getframerate() == 22050 and f.getnframes() == 10


def test_dropin_reexports():
    import importlib.util
    for mod, names in (('vocoder', ('griffin_lim', 'mel_to_linear', 'save_wav')), ('convert', ('conversion_waveforms', 'demo_conversion'))):
        spec = importlib.util.spec_from_file_location('dropin_' + mod, os.path.join(ROOT, 'dropin', mod + '.py'))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        for n in names:
            assert getattr(m, n) is getattr(vocoder if mod == 'vocoder' else convert, n)
