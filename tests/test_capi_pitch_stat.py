"""CPU-only checks of the interface of the pitch tracker's spectral-stationarity term: the four C symbols and their header text, the scratch
arithmetic, every refusal (each is made before anything is enqueued, so a fake non-null pointer is enough and no device is needed), and the
`stationarity` option of features.py.  No kernel is launched here.

Where the option lives.  The argument lists of `extract`, `extract_batch`, `make_spect_f0` and `make_spect_f0_batched` are pinned by
earlier tests (test_capi_resample.py, test_capi_features_batch.py, test_capi_mtrand.py), so they cannot grow a keyword; they stay as they
are, and the option is taken by `pitch_track_dev`, `pitch_track`, `extract_batch_sr` and by two entry points that take every option by
keyword, `extract_opt` and `make_spect_f0_opt` (the drop-in script reaches the latter through `--stationarity`)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from speechsplit_amd import _capi, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d = C.c_void_p, C.c_int, C.c_long, C.c_double
SIGNATURES = {
    'ss_pitch_stat_scratch_bytes': (_l, [_i, _i, _d, _d]),                                # B, max_n, lo_hz, hi_hz
    'ss_pitch_track_stat': (_i, [_vp, _vp, _i, _i, _d, _d, _d, _vp, _vp, _l, _vp]),       # wav, n, B, max_n, scale, lo, hi, f0, scratch, bytes, stream
    'ss_op_pitch_stationarity': (_i, [_vp, _vp, _i, _i, _d, _vp, _vp]),                   # wav, n, B, max_n, scale, stat, stream
    'ss_op_pitch_dp_stat': (_i, [_vp, _vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _l, _vp]),  # phi, rms, stat, n, B, max_n, lo, hi, f0, scratch, bytes, stream
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


def test_header_states_the_term_and_declares_the_entry_points():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('long ss_pitch_stat_scratch_bytes(int B, int max_n, double lo_hz, double hi_hz);',
                 'int ss_pitch_track_stat(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double lo_hz, double hi_hz, '
                 'double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);',
                 'int ss_op_pitch_stationarity(const double* wav_dev, const int* n_dev, int B, int max_n, double scale, double* stat_dev , '
                 'void* stream);',
                 'int ss_op_pitch_dp_stat(const double* phi_dev, const double* rms_dev, const double* stat_dev, const int* n_dev, int B, int max_n, '
                 'double lo_hz, double hi_hz, double* f0_dev, void* scratch_dev, long scratch_bytes, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_op_pitch_dp(') < raw.index('long ss_pitch_stat_scratch_bytes(') < raw.index(' ss_op_pitch_dp_stat(') \
        < raw.index(' ss_griffinlim_samples(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('STAT_W = 480', 'STAT_GAP = 320', 'LPC_ORD = 18', 'PREEMP = 0.4', 'ff = 1 / (1 + 10^-3)', 'VTR_S_C = 0.5',
                   '256 i - 160', '256 i + 160', 'Levinson-Durbin', 'Itakura', 'min(0.2 / (max(d, 1) - 0.8), 1)', '24 chunks',
                   'in chunk order', 'optional and off by default', 'rr stays the ratio'):
        assert phrase in whole, phrase
    assert 'its two-rate search are left out' not in whole                                 # the old sentence is amended


def test_scratch_bytes_is_the_trackers_plus_one_aligned_track():
    lib = _capi.lib()
    for B, n, lo, hi in ((1, 513, 50.0, 250.0), (3, 2304, 100.0, 600.0), (16, 48000, 40.0, 1000.0), (4, 12345, 50.0, 250.0)):
        F = n // 256 + 1
        base, got = lib.ss_pitch_scratch_bytes(B, n, lo, hi), lib.ss_pitch_stat_scratch_bytes(B, n, lo, hi)
        assert got >= base and got % 256 == 0
        assert got - base == -(-B * F * 8 // 256) * 256, (B, n, got, base)
    assert lib.ss_pitch_stat_scratch_bytes(65535, MAX_N, 40.0, 1000.0) > 2 ** 40            # long arithmetic
    nan = float('nan')
    for args, word in (((0, 513, 50.0, 250.0), b'B'), ((65536, 513, 50.0, 250.0), b'B'), ((1, 512, 50.0, 250.0), b'max_n'),
                       ((1, MAX_N + 1, 50.0, 250.0), b'max_n'), ((1, 513, nan, 250.0), b'lo_hz'), ((1, 513, 50.0, nan), b'hi_hz'),
                       ((1, 513, 39.9, 250.0), b'lo_hz'), ((1, 513, 50.0, 1000.5), b'hi_hz'), ((1, 513, 250.0, 50.0), b'lo_hz')):
        assert lib.ss_pitch_stat_scratch_bytes(*args) == -1
        msg = lib.ss_last_error()
        assert word in msg and b'ss_pitch_stat_scratch_bytes' in msg, (args, msg)


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_pitch_scratch_bytes(2, 2304, 50.0, 250.0)
    nbs = lib.ss_pitch_stat_scratch_bytes(2, 2304, 50.0, 250.0)
    nan, inf = float('nan'), float('inf')
    track = lambda **k: lib.ss_pitch_track_stat(*[k.get(a, d) for a, d in (
        ('wav', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('scale', 32768.0), ('lo', 50.0), ('hi', 250.0), ('f0', PTR), ('scratch', PTR),
        ('bytes', nbs), ('stream', None))])
    stat = lambda **k: lib.ss_op_pitch_stationarity(*[k.get(a, d) for a, d in (
        ('wav', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('scale', 32768.0), ('stat', PTR), ('stream', None))])
    dp = lambda **k: lib.ss_op_pitch_dp_stat(*[k.get(a, d) for a, d in (
        ('phi', PTR), ('rms', PTR), ('stat', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('lo', 50.0), ('hi', 250.0), ('f0', PTR),
        ('scratch', PTR), ('bytes', nb), ('stream', None))])
    # null required pointers
    _refused(track(wav=None), 'wav_dev')
    _refused(track(f0=None), 'f0_dev')
    _refused(track(scratch=None), 'scratch_dev')
    _refused(stat(wav=None), 'wav_dev')
    _refused(stat(stat=None), 'stat_dev')
    _refused(dp(phi=None), 'phi_dev')
    _refused(dp(rms=None), 'rms_dev')
    _refused(dp(stat=None), 'stat_dev')
    _refused(dp(f0=None), 'f0_dev')
    _refused(dp(scratch=None), 'scratch_dev')
    for call, who in ((track, 'ss_pitch_track_stat'), (stat, 'ss_op_pitch_stationarity'), (dp, 'ss_op_pitch_dp_stat')):
        _refused(call(B=0), 'B')
        _refused(call(B=-3), 'B')
        _refused(call(B=65536), 'B')
        _refused(call(max_n=512), 'max_n')
        _refused(call(max_n=0), 'max_n')
        _refused(call(max_n=MAX_N + 1), 'max_n')
        _refused(call(B=0), who)                                                           # ... and says who refused
    for call in (track, dp):                                                               # the search range (the stationarity has none)
        _refused(call(lo=nan), 'lo_hz')
        _refused(call(hi=nan), 'hi_hz')
        _refused(call(lo=0.0), 'lo_hz')
        _refused(call(lo=-50.0), 'lo_hz')
        _refused(call(hi=inf), 'hi_hz')
        _refused(call(lo=250.0, hi=250.0), 'lo_hz is not below hi_hz')
        _refused(call(lo=300.0, hi=250.0), 'lo_hz is not below hi_hz')
        _refused(call(hi=1000.1), 'hi_hz')
        _refused(call(lo=39.9), 'lo_hz')
        _refused(call(lo=999.0, hi=1000.0), 'fewer than 3 lags')
        _refused(call(bytes=0), 'scratch_bytes')
        _refused(call(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
        _refused(call(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')
        _refused(call(lo=40.0, hi=1000.0), 'scratch_bytes')                                # more lags need more scratch
    for call in (track, stat):
        for sc in (0.0, -1.0, nan, inf):
            _refused(call(scale=sc), 'scale')
    _refused(track(bytes=nbs - 1), 'ss_pitch_stat_scratch_bytes')                          # the tracker's own scratch is one track short
    _refused(track(bytes=nb), 'ss_pitch_stat_scratch_bytes')
    _refused(dp(bytes=nb - 1), 'scratch_bytes')


# ---------------------------------------------------------------------------------------------- the Python option
TAKES_IT = ('pitch_track_dev', 'pitch_track', 'extract_batch_sr', 'extract_opt', 'make_spect_f0_opt')
PINNED = ('extract', 'extract_batch', 'make_spect_f0', 'make_spect_f0_batched')


def test_the_keyword_exists_is_keyword_only_and_defaults_to_off():
    for name in TAKES_IT:
        p = inspect.signature(getattr(features, name)).parameters['stationarity']
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in PINNED:                                                                    # the earlier tests' argument lists stand
        assert 'stationarity' not in inspect.signature(getattr(features, name)).parameters, name
    text = open(os.path.join(ROOT, 'dropin', 'make_spect_f0.py')).read()
    assert 'make_spect_f0_opt' in text and '--stationarity' in text and 'stationarity=True' in text


@pytest.mark.parametrize('bad', [None, 0, 1, 'yes', 1.0, np.bool_(True)])
def test_a_value_that_is_not_a_bool_is_refused_by_name(bad, tmp_path):
    x = np.zeros(600)
    prng = np.random.RandomState(0)
    calls = {'pitch_track_dev': lambda: features.pitch_track_dev(None, None, 50, 250, stationarity=bad),
             'pitch_track': lambda: features.pitch_track(x, 50, 250, device='cpu', stationarity=bad),
             'extract_batch_sr': lambda: features.extract_batch_sr([x], 16000, prng, 'M', device='cpu', stationarity=bad),
             'extract_opt': lambda: features.extract_opt(x, prng, 'M', device='cpu', stationarity=bad),
             'make_spect_f0_opt': lambda: features.make_spect_f0_opt(str(tmp_path), str(tmp_path / 'a'), str(tmp_path / 'b'), {},
                                                                     device='cpu', stationarity=bad)}
    for name, call in calls.items():
        with pytest.raises(TypeError, match=f'{name}: stationarity must be True or False'):
            call()
    assert prng.get_state()[2] == np.random.RandomState(0).get_state()[2]                  # refused before a draw is made


def test_off_makes_the_earlier_calls_and_on_is_handed_down(monkeypatch):
    """pitch_track_dev replaced by a host stand-in that records its keywords: off, every layer calls it exactly as before (no keyword at
    all, so the stand-ins of the earlier tests still fit); on, the keyword arrives from every entry point"""
    import torch
    seen = []

    def fake_track(wav_dev, n_dev, lo, hi, **kw):
        seen.append(kw)
        return torch.full((wav_dev.shape[0], wav_dev.shape[1] // 256 + 1), -1e10, dtype=torch.float64)

    monkeypatch.setattr(features, 'pitch_track_dev', fake_track)
    x = np.random.default_rng(2).uniform(-0.5, 0.5, 1100)
    features.pitch_track(x, 50, 250, device='cpu')
    features.pitch_track([x, x[:600]], 50, 250, device='cpu', stationarity=False)
    features.pitch_track(x, 50, 250, device='cpu', stationarity=True)
    assert seen == [{}, {}, {'stationarity': True}]
    del seen[:]
    monkeypatch.setattr(features, 'filtfilt_dev', lambda x_, n, b, a, zi, gain, dither, scale: x_)
    monkeypatch.setattr(features, 'melspec_batch_dev', lambda wav, n, mb: torch.zeros(wav.shape[0], wav.shape[1] // 256 + 1, 80))
    monkeypatch.setattr(features, 'f0_normalize_batch_dev', lambda f0, n, max_n, unvoiced: torch.zeros(f0.shape, dtype=torch.float32))
    for kw in ({}, {'stationarity': False}, {'stationarity': True}):
        out = features.extract_batch_sr([x, x[:700]], 16000, np.random.RandomState(1), 'M', device='cpu', **kw)
        assert [s.shape for s, _ in out] == [(5, 80), (3, 80)]
    assert seen == [{}, {}, {'stationarity': True}]
    del seen[:]
    handed = []
    monkeypatch.setattr(features, 'pitch_track', lambda wav, lo, hi, **kw: handed.append(kw) or np.full(wav.shape[0] // 256 + 1, -1e10))
    monkeypatch.setattr(features, 'melspectrogram', lambda wav, mb, device: torch.zeros(wav.shape[0] // 256 + 1, 80))
    monkeypatch.setattr(features, 'normalize_f0', lambda f0, device: torch.zeros(f0.shape[0]))
    features.extract(x, np.random.RandomState(1), 'M', 'cpu')
    features.extract_opt(x, np.random.RandomState(1), 'M', device='cpu')
    features.extract_opt(x, np.random.RandomState(1), 'M', device='cpu', stationarity=True)
    assert handed == [{'device': 'cpu'}, {'device': 'cpu'}, {'device': 'cpu', 'stationarity': True}]


def test_the_walk_hands_the_keyword_on_only_when_it_is_set(monkeypatch, tmp_path):
    seen, one = [], []
    feats = (np.zeros((3, 80), np.float32), np.zeros(3, np.float32))
    monkeypatch.setattr(features, 'extract_batch_sr', lambda *a, **k: seen.append(k) or [feats])
    monkeypatch.setattr(features, 'extract', lambda *a, **k: one.append(('extract', k)) or feats)
    monkeypatch.setattr(features, '_extract', lambda *a: one.append(('_extract', a[3:])) or feats)
    monkeypatch.setattr(features, 'read_wav', lambda path: np.zeros(600))
    root = tmp_path / 'wavs' / 'p226'
    os.makedirs(root)
    open(root / 'a.wav', 'wb').close()
    args = (str(tmp_path / 'wavs'), str(tmp_path / 's'), str(tmp_path / 'f'), {'p226': 'M'})
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2) == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2, stationarity=True) == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2, device_draws=True, stationarity=True) == [('p226', 'a')]
    assert seen == [{'unvoiced': -1e10}, {'unvoiced': -1e10, 'stationarity': True},
                    {'unvoiced': -1e10, 'device_draws': True, 'stationarity': True}]
    assert features.make_spect_f0_opt(*args, device='cpu') == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', stationarity=True) == [('p226', 'a')]
    assert one == [('extract', {'unvoiced': -1e10, 'sr': 16000}), ('_extract', ('cpu', None, -1e10, 16000, True))]
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match='max_rows must be None or a positive integer'):
            features.make_spect_f0_opt(*args, max_rows=bad)
    with pytest.raises(ValueError, match='device_draws needs the batched walk'):
        features.make_spect_f0_opt(*args, device_draws=True)
