"""CPU-only checks of the harmonic mel inversion's interface: the C symbols and their header text, every refusal by message (each is made
before anything is enqueued, so a fake non-null pointer is enough and no device is needed), the Python arguments, the ln-Hz -> Hz conversion
and features.f0_from_norm.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from speechsplit_amd import _capi, convert, features, vocoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    # mel, f0_hz, inv_basis, packed, packed_doubles, frames, B, max_frames, n_mels, f_top, n_iter, floor, mag, share, stream
    'ss_mel_to_linear_harmonic': (_i, [_vp, _vp, _vp, _vp, _l, _vp, _i, _i, _i, _d, _i, _d, _vp, _vp, _vp]),
    'ss_harmonic_phase_scratch_bytes': (_l, [_i, _i]),
    # f0_hz, share, rand_phase, frames, B, max_frames, f_top, phase0, scratch, scratch_bytes, stream
    'ss_harmonic_phase': (_i, [_vp, _vp, _vp, _vp, _i, _i, _d, _vp, _vp, _l, _vp]),
    'ss_op_harmonic_u': (_i, [_vp, _vp, _i, _i, _vp, _vp]),
}
PTR = C.c_void_p(1 << 20)                                                                  # fake, non-null, 256-byte aligned; never dereferenced
NAN, INF = float('nan'), float('inf')


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
    for decl in ('int ss_mel_to_linear_harmonic(const float* mel_dev, const double* f0_hz_dev, const double* inv_basis_dev, '
                 'const double* packed_dev, long packed_doubles, const int* frames_dev, int B, int max_frames, int n_mels, double f_top, '
                 'int n_iter, double floor, double* mag_dev /* in/out */, double* share_dev /* out */, void* stream);',
                 'long ss_harmonic_phase_scratch_bytes(int B, int max_frames);',
                 'int ss_harmonic_phase(const double* f0_hz_dev, const double* share_dev, const double* rand_phase_dev, '
                 'const int* frames_dev, int B, int max_frames, double f_top, double* phase0_dev /* out */, void* scratch_dev, '
                 'long scratch_bytes, void* stream);'):
        assert decl in text, decl
    assert text.index('int ss_mel_to_linear_nnls(') < text.index('int ss_mel_to_linear_harmonic(') < text.index('int ss_op_stft (')
    for phrase in ('H = min(floor(f_top / f), 190)', 'W(d) = 0.5 s(d) + 0.25 s(d - 1) + 0.25 s(d + 1)', 'u_i = frac(u_{i-1} + 0.008 (f_{i-1} + f_i))',
                   'h_k = min(max(rint(k / p_1), 1), H)', 'phi_h = 2 pi frac(h_k u_i + 0.5 (k mod 2))', '40 <= f <= 1000',
                   'The F0 has to BELONG to the mel'):
        assert phrase in text, phrase


def test_scratch_bytes():
    lib = _capi.lib()
    assert lib.ss_harmonic_phase_scratch_bytes(1, 4) == 256                                # 32 bytes of u, rounded up to 256
    assert lib.ss_harmonic_phase_scratch_bytes(7, 192) == 10752                            # 7 * 192 * 8, a multiple of 256 already
    assert lib.ss_harmonic_phase_scratch_bytes(3, 41) == 1024
    for B, F, word in ((0, 9, 'B outside'), (65536, 9, 'B outside'), (1, 3, 'max_frames'), (1, 8193, 'max_frames')):
        _refused(lib.ss_harmonic_phase_scratch_bytes(B, F), 'ss_harmonic_phase_scratch_bytes', word)


def test_every_refusal_of_the_fit_names_its_argument():
    lib = _capi.lib()
    call = lambda **k: lib.ss_mel_to_linear_harmonic(*[k.get(a, d) for a, d in (
        ('mel', PTR), ('f0', PTR), ('inv', PTR), ('packed', PTR), ('pd', 1101), ('frames', None), ('B', 2), ('F', 9), ('n_mels', 80),
        ('f_top', 7600.0), ('n_iter', 50), ('floor', 1e-10), ('mag', PTR), ('share', PTR), ('stream', None))])

    def refused(rc, word):
        _refused(rc, 'ss_mel_to_linear_harmonic', word)

    for arg, name in (('mel', 'mel_dev'), ('f0', 'f0_hz_dev'), ('inv', 'inv_basis_dev'), ('packed', 'packed_dev'), ('mag', 'mag_dev'),
                      ('share', 'share_dev')):
        refused(call(**{arg: None}), 'null pointer: ' + name)
    for B in (0, -3, 65536):
        refused(call(B=B), 'B outside')
    for F in (3, 8193):
        refused(call(F=F), 'max_frames')
    for n in (0, -1, 4097):
        refused(call(n_mels=n), 'n_mels outside 1 .. 4096')
    for pd in (159, 0, -5):
        refused(call(pd=pd), 'packed_doubles disagrees with n_mels')
    refused(call(pd=1101, n_mels=2), 'packed_doubles disagrees with n_mels')
    refused(call(pd=3073), 'packed_doubles beyond the 3072')
    refused(call(pd=1 << 40), 'packed_doubles')
    for ft in (999.9, 8000.1, 0.0, -7600.0, NAN, INF, -INF):
        refused(call(f_top=ft), 'f_top outside 1000 .. 8000')
    for it in (-1, 100001):
        refused(call(n_iter=it), 'n_iter outside 0 .. 100000')
    for f in (-1e-30, NAN):
        refused(call(floor=f), 'floor')


def test_every_refusal_of_the_phase_call_names_its_argument():
    lib = _capi.lib()
    call = lambda **k: lib.ss_harmonic_phase(*[k.get(a, d) for a, d in (
        ('f0', PTR), ('share', PTR), ('rand', PTR), ('frames', None), ('B', 2), ('F', 9), ('f_top', 7600.0), ('phase0', PTR),
        ('scratch', PTR), ('bytes', 256), ('stream', None))])

    def refused(rc, word):
        _refused(rc, 'ss_harmonic_phase', word)

    for arg, name in (('f0', 'f0_hz_dev'), ('share', 'share_dev'), ('phase0', 'phase0_dev'), ('scratch', 'scratch_dev')):
        refused(call(**{arg: None}), 'null pointer: ' + name)
    for B in (0, 65536):
        refused(call(B=B), 'B outside')
    for F in (3, 8193):
        refused(call(F=F), 'max_frames')
    for ft in (999.9, 8000.1, NAN, INF):
        refused(call(f_top=ft), 'f_top outside 1000 .. 8000')
    refused(call(scratch=C.c_void_p((1 << 20) + 8)), 'scratch_dev is not 256-byte aligned')
    for nb in (255, 0, -1):
        refused(call(bytes=nb), 'scratch_bytes below ss_harmonic_phase_scratch_bytes(B, max_frames)')
    hook = lambda **k: lib.ss_op_harmonic_u(*[k.get(a, d) for a, d in (('f0', PTR), ('frames', None), ('B', 2), ('F', 9), ('u', PTR),
                                                                         ('stream', None))])
    _refused(hook(f0=None), 'ss_op_harmonic_u', 'f0_hz_dev')
    _refused(hook(u=None), 'ss_op_harmonic_u', 'u_dev')
    _refused(hook(B=0), 'ss_op_harmonic_u', 'B outside')
    _refused(hook(F=3), 'ss_op_harmonic_u', 'max_frames')


def test_f0_hz_conversion():
    ln = np.array([np.log(100.0), -1e10, np.log(40.0), NAN, INF, -INF, 800.0, np.log(250.5)])
    hz = vocoder.f0_hz(ln)
    assert hz.dtype == np.float64 and np.array_equal(hz == 0.0, [False, True, False, True, True, True, True, False])
    assert np.array_equal(hz[[0, 2, 7]], np.exp(ln[[0, 2, 7]]))


def test_f0_from_norm_inverts_the_speaker_normalisation():
    """the reference's normalisation restated: (ln f0 - mean) / std / 4, clipped to [-1, 1], mapped to [0, 1]; 0 on unvoiced frames"""
    rng = np.random.default_rng(3)
    ln = np.where(rng.uniform(size=200) < 0.3, -1e10, rng.normal(np.log(180.0), 0.2, 200))
    v = ln != -1e10
    mean, std = ln[v].mean(), ln[v].std()
    norm = np.where(v, (np.clip((ln - mean) / std / 4.0, -1.0, 1.0) + 1.0) / 2.0, 0.0)
    back = features.f0_from_norm(norm, mean, std)
    assert back.dtype == np.float64 and np.array_equal(back == -1e10, ~v)
    assert np.abs(back[v] - ln[v]).max() <= 1e-12                                          # 0.2 / (4 * 0.2): nothing was clipped
    assert np.array_equal(vocoder.f0_hz(back) > 0.0, v)
    other = features.f0_from_norm(norm, np.log(110.0), 0.1)                                # another speaker's statistics: another register
    assert abs(np.exp(other[v]).mean() / 110.0 - 1.0) < 0.05
    assert np.array_equal(features.f0_from_norm(norm.astype(np.float32), mean, std) == -1e10, ~v)
    for bad in ((norm[None], mean, std), (norm, NAN, std), (norm, mean, 0.0), (norm, mean, -1.0), (norm, mean, INF)):
        with pytest.raises(ValueError, match='f0_from_norm'):
            features.f0_from_norm(*bad)


def test_python_argument_checks():
    mel = np.zeros((9, 80), np.float32)
    for fn in (vocoder.mel_to_linear, vocoder.griffin_lim):
        for bad in (np.zeros(8), np.zeros(10), np.zeros((9, 1)), [np.zeros(9), np.zeros(9)]):
            with pytest.raises(ValueError, match='f0 must hold one track per mel, each as long as its mel'):
                fn(mel, f0=bad, device='cpu')
    with pytest.raises(ValueError, match='one track per mel'):
        vocoder.griffin_lim([mel, mel], f0=[np.zeros(9)], device='cpu')
    with pytest.raises(ValueError, match='one track per mel'):
        vocoder.griffin_lim([mel, np.zeros((5, 80), np.float32)], f0=[np.zeros(5), np.zeros(9)], device='cpu')
    assert vocoder.INVERSIONS == ('pinv', 'nnls')                                          # the feature is switched on by f0, not by a name
    res = [('a', mel), ('b', mel)]
    with pytest.raises(ValueError, match='conversion_waveforms: f0s'):
        convert.conversion_waveforms(res, f0s=[np.zeros(9)], device='cpu')
    with pytest.raises(ValueError, match='conversion_waveforms: f0s'):
        convert.conversion_waveforms([res, res], f0s=[[np.zeros(9)] * 2, [np.zeros(9)]], device='cpu')


def _patch(monkeypatch, seen):
    import torch

    def route(tag):
        def fake(mel_dev, *a):
            seen.append((tag, mel_dev.shape[0]))
            return torch.full((mel_dev.shape[0], mel_dev.shape[1], 513), 3.0, dtype=torch.float64)
        return fake

    def fake_fit(mel_dev, f0hz_dev, inv_dev, packed_dev, frames_dev, n_iter, f_top, floor, mag_dev):
        seen.append(('fit', f0hz_dev.numpy().copy(), None if frames_dev is None else frames_dev.tolist(), n_iter, f_top, floor, float(mag_dev.min()), packed_dev.numel()))
        return torch.full(mag_dev.shape, 0.5, dtype=torch.float64)

    def fake_phase(f0hz_dev, share_dev, rand_dev, frames_dev, f_top):
        seen.append(('phase', float(share_dev.max()), None if rand_dev is None else rand_dev.numpy().copy(), None if frames_dev is None else frames_dev.tolist(), f_top))
        return torch.full(share_dev.shape, 0.25, dtype=torch.float64)

    def fake_gl(mag, ph, fr, n, m):
        seen.append(('gl', None if ph is None else float(ph.max())))
        return torch.zeros(mag.shape[0], 256 * (mag.shape[1] - 1), dtype=torch.float64)

    monkeypatch.setattr(vocoder, '_mel_to_linear', route('pinv'))
    monkeypatch.setattr(vocoder, '_mel_to_linear_nnls', route('nnls'))
    monkeypatch.setattr(vocoder, '_mel_to_linear_harmonic', fake_fit)
    monkeypatch.setattr(vocoder, '_harmonic_phase', fake_phase)
    monkeypatch.setattr(vocoder, 'griffin_lim_mag', fake_gl)


def test_without_f0_the_harmonic_calls_are_not_reached(monkeypatch):
    seen = []
    _patch(monkeypatch, seen)
    mels = [np.zeros((n, 80), np.float32) for n in (9, 4, 5)]
    for inv in ('pinv', 'nnls'):
        out = vocoder.griffin_lim(mels, n_iter=1, max_rows=2, device='cpu', inversion=inv)
        assert [w.shape[0] for w in out] == [2048, 768, 1024]
    tags = [s[0] for s in seen]
    assert 'fit' not in tags and 'phase' not in tags and tags.count('gl') == 4
    assert [s[1] for s in seen if s[0] == 'gl'] != [0.25] * 4                               # the drawn phases reach Griffin-Lim themselves


def test_with_f0_both_routes_feed_the_harmonic_calls(monkeypatch):
    seen = []
    _patch(monkeypatch, seen)
    mels = [np.zeros((n, 80), np.float32) for n in (9, 4, 5)]
    tracks = [np.full(9, np.log(100.0)), np.full(4, -1e10), np.array([np.log(50.0), -1e10, np.log(200.0), NAN, np.log(120.0)])]
    for inv in ('pinv', 'nnls'):
        del seen[:]
        vocoder.griffin_lim(mels, n_iter=1, max_rows=2, device='cpu', inversion=inv, f0=tracks, harmonic_iter=37, f_top=7000.0)
        tags = [s[0] for s in seen]
        assert tags == [inv, 'fit', 'phase', 'gl'] * 2, tags                                # two batches: rows [4, 5] and [9]
        fits = [s for s in seen if s[0] == 'fit']
        assert [f[2] for f in fits] == [[4, 5], [9]]
        hz = fits[0][1]
        assert hz.shape == (2, 5) and not hz[0].any()                                       # the unvoiced track, zero-padded to 5 frames
        assert np.allclose(hz[1], [50.0, 0.0, 200.0, 0.0, 120.0], rtol=1e-14) and np.allclose(fits[1][1], 100.0, rtol=1e-14)
        for f in fits:
            assert f[3:6] == (37, 7000.0, 1e-10) and f[6] == 3.0 and f[7] == 2 * 80 + 941   # the route's magnitude, the packed bank
        for p in (s for s in seen if s[0] == 'phase'):
            assert p[1] == 0.5 and p[2] is not None and p[4] == 7000.0                      # the fit's share and the drawn phases
        assert [s[1] for s in seen if s[0] == 'gl'] == [0.25, 0.25]                         # Griffin-Lim starts from the mixed phases
    del seen[:]
    vocoder.griffin_lim(mels[0], n_iter=1, device='cpu', f0=tracks[0], phases='zero')
    assert [s[0] for s in seen] == ['pinv', 'fit', 'phase', 'gl'] and seen[2][2] is None    # 'zero' plays phi_rand as NULL
    # mel_to_linear: the share comes back on request; conversion_waveforms hands nested tracks on flat
    mag, share = vocoder.mel_to_linear(mels[0], device='cpu', f0=tracks[0], return_share=True)
    assert mag.shape == share.shape == (9, 513) and float(share.max()) == 0.5
    mag, share = vocoder.mel_to_linear(mels[0], device='cpu', return_share=True)
    assert not share.any()
    del seen[:]
    res = [[('a', mels[0])], [('b', mels[1]), ('c', mels[2])]]
    out = convert.conversion_waveforms(res, f0s=[[tracks[0]], [tracks[1], tracks[2]]], n_iter=1, device='cpu', max_rows=4)
    assert [[n for n, _ in pair] for pair in out] == [['a'], ['b', 'c']] and [s[2] for s in seen if s[0] == 'fit'] == [[4, 5, 9]]
