"""CPU-only checks of the interface of silence removal: the four C symbols and their header text, the scratch arithmetic, every refusal
(each is made before anything is enqueued, so a fake non-null pointer is enough and no device is needed), `Silence`'s validation, the
`silence` keyword of features.py -- where it lives, that off makes exactly the earlier calls and that on is handed down -- and the drop-in
script's flags.  No kernel is launched here.

Where the option lives.  The argument lists of `extract`, `extract_batch`, `make_spect_f0` and `make_spect_f0_batched` are pinned by
earlier tests, so the option is taken by `extract_batch_sr`, `extract_opt` and `make_spect_f0_opt`, keyword-only, default None."""
import ctypes as C
import importlib.util
import inspect
import math
import os
import re

import numpy as np
import pytest

import silence_ref as R
from speechsplit_amd import _capi, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l, _d, _dp = C.c_void_p, C.c_int, C.c_long, C.c_double, C.POINTER(C.c_double)
SIGNATURES = {
    'ss_silence_scratch_bytes': (_l, [_i, _i]),                                                       # B, max_n
    # x, n, B, max_n, ratio, hang, edge, pause, g (host), y, m, inv, k, scratch, bytes, stream
    'ss_remove_silence': (_i, [_vp, _vp, _i, _i, _d, _i, _i, _i, _dp, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    'ss_op_silence_levels': (_i, [_vp, _vp, _i, _i, _vp, _vp]),                                       # x, n, B, max_n, e, stream
    'ss_op_silence_mask': (_i, [_vp, _vp, _i, _i, _d, _i, _i, _i, _vp, _vp, _vp]),                    # e, j, B, max_j, ratio, hang, edge, pause, inv, k, stream
    'ss_op_silence_gather': (_i, [_vp, _vp, _i, _i, _vp, _vp, _dp, _vp, _vp, _vp]),                   # x, n, B, max_n, inv, k, g (host), y, m, stream
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null, 256-byte aligned; never dereferenced
MAX_N = 256 * 8191
GAINS = features.silence_fade()


def _g(g=GAINS):
    return np.ascontiguousarray(g, np.float64).ctypes.data_as(_dp)


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_states_the_definition_and_declares_the_entry_points():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('long ss_silence_scratch_bytes(int B, int max_n);',
                 'int ss_remove_silence(const double* x_dev, const int* n_dev, int B, int max_n, double ratio, int hang, int edge, int pause, '
                 'const double* g , double* y_dev , int* m_dev , int* inv_dev , int* k_dev , void* scratch_dev, long scratch_bytes, void* stream);',
                 'int ss_op_silence_levels(const double* x_dev, const int* n_dev, int B, int max_n, double* e_dev , void* stream);',
                 'int ss_op_silence_mask(const double* e_dev, const int* j_dev, int B, int max_j, double ratio, int hang, int edge, int pause, '
                 'int* inv_dev , int* k_dev , void* stream);',
                 'int ss_op_silence_gather(const double* x_dev, const int* n_dev, int B, int max_n, const int* inv_dev, const int* k_dev, '
                 'const double* g , double* y_dev, int* m_dev, void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_resample(') < raw.index('long ss_silence_scratch_bytes(') < raw.index(' ss_op_silence_gather(') \
        < raw.index(' ss_mt19937_rand(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('no fused multiply-add', 'J = ceil(n_b / 256)', "the chain's mel hop", 'E_j = ((Q_{2j-1} + Q_{2j}) + Q_{2j+1}) + Q_{2j+2}',
                   'a plain SUM, not a mean', 'E_j > ratio * E_max, STRICTLY', 'no logarithm on the device', '|i - j| <= hang',
                   'keeps its last min(R, edge) blocks', 'keeps its first min(R, edge) blocks', 'first ceil(pause / 2) and its last floor(pause / 2)',
                   'm_b = 256 (K - 1)', 'y[256 c + r] = x[256 (a + 1) + r] * (1.0 - g[r]) + x[256 inv[c] + r] * g[r]',
                   'g[r] = 0.5 - 0.5 cos(pi (r + 0.5) / 128)', 'Exact zeros are written behind m_b', 'a corrupt map changes numbers, never addresses',
                   'spoils that row only', 'may hold NaN', 'No atomics', 'no absolute gate', 'librosa.effects.trim'):
        assert phrase in whole, phrase


def test_scratch_bytes():
    lib = _capi.lib()
    up = lambda v: -(-v // 256) * 256
    for B, n in ((1, 1), (3, 2304), (16, 64000), (7, 49152), (4, 12345)):
        J = -(-n // 256)
        assert lib.ss_silence_scratch_bytes(B, n) == up(B * J * 8) + up(B * J * 4) + up(B * 4), (B, n)
    assert lib.ss_silence_scratch_bytes(65535, MAX_N) > 2 ** 32                             # long arithmetic
    for args, word in (((0, 513), b'B'), ((65536, 513), b'B'), ((1, 0), b'max_n'), ((1, MAX_N + 1), b'max_n')):
        assert lib.ss_silence_scratch_bytes(*args) == -1
        msg = lib.ss_last_error()
        assert word in msg and b'ss_silence_scratch_bytes' in msg, (args, msg)


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    nb = lib.ss_silence_scratch_bytes(2, 2304)
    nan, inf = float('nan'), float('inf')
    whole = lambda **k: lib.ss_remove_silence(*[k.get(a, d) for a, d in (
        ('x', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('ratio', 1e-4), ('hang', 2), ('edge', 6), ('pause', -1), ('g', _g()), ('y', PTR),
        ('m', PTR), ('inv', None), ('k', None), ('scratch', PTR), ('bytes', nb), ('stream', None))])
    levels = lambda **k: lib.ss_op_silence_levels(*[k.get(a, d) for a, d in (
        ('x', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('e', PTR), ('stream', None))])
    mask = lambda **k: lib.ss_op_silence_mask(*[k.get(a, d) for a, d in (
        ('e', PTR), ('j', None), ('B', 2), ('max_j', 9), ('ratio', 1e-4), ('hang', 2), ('edge', 6), ('pause', -1), ('inv', PTR), ('k', PTR),
        ('stream', None))])
    gather = lambda **k: lib.ss_op_silence_gather(*[k.get(a, d) for a, d in (
        ('x', PTR), ('n', None), ('B', 2), ('max_n', 2304), ('inv', PTR), ('k', PTR), ('g', _g()), ('y', PTR), ('m', PTR), ('stream', None))])
    # null required pointers
    for call, names in ((whole, ('x', 'y', 'm', 'g', 'scratch')), (levels, ('x', 'e')), (mask, ('e', 'inv', 'k')),
                        (gather, ('x', 'inv', 'k', 'g', 'y', 'm'))):
        for name in names:
            _refused(call(**{name: None}), name if name == 'g' else name + '_dev')
    for call, who in ((whole, 'ss_remove_silence'), (levels, 'ss_op_silence_levels'), (mask, 'ss_op_silence_mask'),
                      (gather, 'ss_op_silence_gather')):
        for B in (0, -3, 65536):
            _refused(call(B=B), 'B')
        _refused(call(B=0), who)                                                           # ... and says who refused
    for call in (whole, levels, gather):
        for n in (0, -1, MAX_N + 1):
            _refused(call(max_n=n), 'max_n')
    for j in (0, -1, 8192):
        _refused(mask(max_j=j), 'max_j')
    for call in (whole, mask):
        for ratio in (0.0, 1.0, -0.5, 1.5, nan, inf):
            _refused(call(ratio=ratio), 'ratio')
        _refused(call(hang=-1), 'hang')
        _refused(call(edge=-1), 'edge')
        _refused(call(pause=-2), 'pause')
    for call in (whole, gather):
        for r, bad in ((0, nan), (77, inf), (127, -inf)):
            g = GAINS.copy()
            g[r] = bad
            _refused(call(g=_g(g)), f'g[{r}]')
    _refused(whole(bytes=nb - 1), 'scratch_bytes')
    _refused(whole(bytes=0), 'ss_silence_scratch_bytes')
    _refused(whole(scratch=C.c_void_p((1 << 20) + 128)), 'aligned')
    _refused(whole(scratch=C.c_void_p((1 << 20) + 8)), 'aligned')


# ---------------------------------------------------------------------------------------------- the Python layer
def test_silence_is_immutable_and_validated_by_name():
    s = features.Silence()
    assert (s.top_db, s.hang, s.edge, s.pause) == (40.0, 2, 6, None) and s.pause_blocks == -1
    assert s.ratio == 10.0 ** (-40.0 / 10.0) == R.ratio_of(40.0)
    t = features.Silence(30, 0, 0, 8)
    assert (t.top_db, t.pause, t.pause_blocks) == (30.0, 8, 8) and isinstance(t.top_db, float)
    assert t == features.Silence(30.0, 0, 0, 8) and t != s and hash(t) == hash(features.Silence(30.0, 0, 0, 8))
    assert 'top_db=30.0' in repr(t) and 'pause=8' in repr(t)
    with pytest.raises(AttributeError):
        s.hang = 3
    with pytest.raises(AttributeError):
        del s.hang
    for bad in (0, 0.0, -3.0, float('nan'), float('inf'), '40', None, True, 1e6):
        with pytest.raises(ValueError, match='Silence: top_db'):
            features.Silence(top_db=bad)
    for name in ('hang', 'edge'):
        for bad in (-1, 1.0, True, None, '2', 2 ** 31):
            with pytest.raises(ValueError, match=f'Silence: {name}'):
                features.Silence(**{name: bad})
    for bad in (-1, 2.0, False, '8', 2 ** 31):
        with pytest.raises(ValueError, match='Silence: pause'):
            features.Silence(pause=bad)
    g = features.silence_fade()
    assert g.shape == (128,) and g.dtype == np.float64 and np.array_equal(g, R.fade_gains())
    assert g[0] == 0.5 - 0.5 * math.cos(math.pi * 0.5 / 128.0) and np.all(np.diff(g) > 0) and 0 < g[0] and g[-1] < 1
    assert np.allclose(g + g[::-1], 1.0, atol=1e-15)                                       # the two sides of the fade add up to one


TAKES_IT = ('extract_batch_sr', 'extract_opt', 'make_spect_f0_opt')
PINNED = ('extract', 'extract_batch', 'make_spect_f0', 'make_spect_f0_batched')


def test_the_keyword_exists_is_keyword_only_and_defaults_to_none():
    for name in TAKES_IT:
        p = inspect.signature(getattr(features, name)).parameters['silence']
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in PINNED:                                                                    # the earlier tests' argument lists stand
        assert 'silence' not in inspect.signature(getattr(features, name)).parameters, name
    sig = inspect.signature(features.remove_silence)
    assert list(sig.parameters) == ['xs', 'opts', 'max_rows', 'device', 'return_maps']
    assert sig.parameters['opts'].default == features.Silence() and sig.parameters['max_rows'].default == 16
    assert sig.parameters['return_maps'].default is False
    assert list(inspect.signature(features.remove_silence_dev).parameters) == ['x_dev', 'n_dev', 'opts']


@pytest.mark.parametrize('bad', [True, 40.0, 'on', (40, 2, 6), {'top_db': 40}])
def test_a_value_that_is_not_a_silence_is_refused_by_name(bad, tmp_path):
    x = np.zeros(600)
    prng = np.random.RandomState(0)
    calls = {'extract_batch_sr': lambda: features.extract_batch_sr([x], 16000, prng, 'M', device='cpu', silence=bad),
             'extract_opt': lambda: features.extract_opt(x, prng, 'M', device='cpu', silence=bad),
             'make_spect_f0_opt': lambda: features.make_spect_f0_opt(str(tmp_path), str(tmp_path / 'a'), str(tmp_path / 'b'), {},
                                                                     device='cpu', silence=bad),
             'remove_silence': lambda: features.remove_silence([x], bad, device='cpu'),
             'remove_silence_dev': lambda: features.remove_silence_dev(None, None, bad)}
    for name, call in calls.items():
        with pytest.raises(TypeError, match=f'{name}: silence must be a Silence'):
            call()
    assert prng.get_state()[2] == np.random.RandomState(0).get_state()[2]                  # refused before a draw is made


def _fake_remove(seen):
    """remove_silence_dev on the host through the restatement: records its options, returns what the device call returns"""
    import torch

    def fake(x_dev, n_dev, opts):
        seen.append(opts)
        B, max_n = x_dev.shape
        y = torch.zeros(B, max_n, dtype=torch.float64)
        inv = torch.full((B, -(-max_n // 256)), -1, dtype=torch.int32)
        m, k = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            r = R.remove_silence(x_dev[b, :int(n_dev[b])].numpy(), opts.ratio, opts.hang, opts.edge, opts.pause_blocks)
            y[b, :r['m']] = torch.from_numpy(r['y'])
            inv[b, :r['K']] = torch.from_numpy(r['inv'])
            m[b], k[b] = r['m'], r['K']
        return y, m, inv, k
    return fake


def test_off_makes_the_earlier_calls_and_on_trims_in_front_of_the_fix_and_the_draws(monkeypatch):
    import torch
    seen, chain_lens = [], []
    monkeypatch.setattr(features, 'remove_silence_dev', _fake_remove(seen))
    monkeypatch.setattr(features, 'filtfilt_dev', lambda x_, n, b, a, zi, gain, dither, scale: chain_lens.append(n.tolist()) or x_)
    monkeypatch.setattr(features, 'melspec_batch_dev', lambda wav, n, mb: torch.zeros(wav.shape[0], wav.shape[1] // 256 + 1, 80))
    monkeypatch.setattr(features, 'pitch_track_dev', lambda wav, n, lo, hi, **kw: torch.full((wav.shape[0], wav.shape[1] // 256 + 1), -1e10,
                                                                                            dtype=torch.float64))
    monkeypatch.setattr(features, 'f0_normalize_batch_dev', lambda f0, n, max_n, unvoiced: torch.zeros(f0.shape, dtype=torch.float32))
    quiet = lambda n, seed: np.random.default_rng(seed).uniform(-1, 1, n) * 1e-4
    loud = lambda n, seed: np.random.default_rng(seed).uniform(-1, 1, n)
    xs = [np.concatenate((quiet(2048, 1), loud(1024, 2), quiet(2048, 3))), np.concatenate((loud(900, 4), quiet(1500, 5)))]
    # off: the earlier calls, the earlier lengths, and nothing of silence.hip's
    prng = np.random.RandomState(3)
    out = features.extract_batch_sr(xs, 16000, prng, 'M', device='cpu')
    assert seen == [] and [s.shape[0] for s, _ in out] == [5120 // 256 + 1, 2400 // 256 + 1]
    ref = np.random.RandomState(3)
    ref.rand(5121 + 2400)                                                                  # 5120 gets the odd-length fix
    assert np.array_equal(prng.get_state()[1], ref.get_state()[1]) and prng.get_state()[2] == ref.get_state()[2]
    # on: each recording is trimmed first; the fix, the draws and the chain see the new lengths
    opts = features.Silence(40.0, 0, 1, None)
    want = [R.remove_silence(x, opts.ratio, 0, 1, -1)['m'] for x in xs]
    assert want[0] < 5120 and want[1] < 2400 and want[0] % 256 == 0
    fixed = [m + 1 if m % 256 == 0 else m for m in want]
    for more in ({}, {'max_rows': 1}):
        del seen[:], chain_lens[:]
        a, b = np.random.RandomState(3), np.random.RandomState(3)
        out = features.extract_batch_sr(xs, 16000, a, 'M', device='cpu', silence=opts, **more)
        assert seen and all(o is opts for o in seen)
        assert [s.shape[0] for s, _ in out] == [n // 256 + 1 for n in fixed]
        assert sorted(n for batch in chain_lens for n in batch) == sorted(fixed)
        b.rand(sum(fixed))                                                                 # the draws: the new lengths, in input order
        assert np.array_equal(a.get_state()[1], b.get_state()[1]) and a.get_state()[2] == b.get_state()[2]
    # a recording that ends below the minimum is refused by its index, with its new length, before a draw is made
    short = np.concatenate((loud(100, 6), quiet(1900, 7)))
    prng = np.random.RandomState(5)
    with pytest.raises(ValueError, match='recording 1 has 256 samples after silence removal'):
        features.extract_batch_sr([xs[0], short], 16000, prng, 'M', device='cpu', silence=features.Silence(40.0, 0, 0, None))
    assert prng.get_state()[2] == np.random.RandomState(5).get_state()[2]
    # the per-file path: extract_opt trims in front of preprocess_wav; off hands nothing new down
    handed = []
    monkeypatch.setattr(features, 'pitch_track', lambda wav, lo, hi, **kw: handed.append((wav.shape[0], kw)) or np.full(wav.shape[0] // 256 + 1, -1e10))
    monkeypatch.setattr(features, 'melspectrogram', lambda wav, mb, device: torch.zeros(wav.shape[0] // 256 + 1, 80))
    monkeypatch.setattr(features, 'normalize_f0', lambda f0, device: torch.zeros(f0.shape[0]))
    del seen[:]
    features.extract_opt(xs[0], np.random.RandomState(1), 'M', device='cpu')
    assert seen == [] and handed == [(5121, {'device': 'cpu'})]
    features.extract_opt(xs[0], np.random.RandomState(1), 'M', device='cpu', silence=opts)
    assert seen == [opts] and handed[1] == (fixed[0], {'device': 'cpu'})
    with pytest.raises(ValueError, match='recording 0 has 256 samples after silence removal'):
        features.extract_opt(short, np.random.RandomState(1), 'M', device='cpu', silence=features.Silence(40.0, 0, 0, None))


def test_remove_silence_batches_and_returns_maps(monkeypatch):
    seen = []
    monkeypatch.setattr(features, 'remove_silence_dev', _fake_remove(seen))
    x, o = R.INPUTS['pause_odd']
    opts = features.Silence(40.0, 0, 0, 3)
    xs = [x, x[:1000], x[:1]]
    refs = [R.remove_silence(v, opts.ratio, 0, 0, 3) for v in xs]
    for max_rows, calls in ((16, 1), (1, 3)):
        del seen[:]
        ys, invs = features.remove_silence(xs, opts, max_rows=max_rows, device='cpu', return_maps=True)
        assert len(seen) == calls
        for y, inv, ref in zip(ys, invs, refs):
            assert np.array_equal(y, ref['y']) and np.array_equal(inv, ref['inv']) and y.dtype == np.float64
    assert [len(y) for y in features.remove_silence(xs, opts, device='cpu')] == [r['m'] for r in refs]
    with pytest.raises(ValueError, match='remove_silence: recording 1 must be'):
        features.remove_silence([x, np.zeros(0)], opts, device='cpu')


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
    opts = features.Silence(35.0, 1, 2, 4)
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2) == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2, silence=None) == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2, silence=opts) == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', max_rows=2, device_draws=True, stationarity=True, silence=opts) == [('p226', 'a')]
    assert seen == [{'unvoiced': -1e10}, {'unvoiced': -1e10}, {'unvoiced': -1e10, 'silence': opts},
                    {'unvoiced': -1e10, 'device_draws': True, 'stationarity': True, 'silence': opts}]
    assert features.make_spect_f0_opt(*args, device='cpu') == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', silence=opts) == [('p226', 'a')]
    assert features.make_spect_f0_opt(*args, device='cpu', stationarity=True, silence=opts) == [('p226', 'a')]
    assert one == [('extract', {'unvoiced': -1e10, 'sr': 16000}), ('_extract', ('cpu', None, -1e10, 16000, False, opts)),
                   ('_extract', ('cpu', None, -1e10, 16000, True, opts))]


def test_the_drop_in_script_has_the_flags():
    path = os.path.join(ROOT, 'dropin', 'make_spect_f0.py')
    text = open(path).read()
    for flag in ('--trim-db', '--trim-hang', '--trim-edge', '--max-pause', '--stationarity', 'make_spect_f0_opt'):
        assert flag in text, flag
    spec = importlib.util.spec_from_file_location('dropin_make_spect_f0', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                                            # nothing runs on import
    assert mod.parse([]) == (False, None)                                                   # no flag: the reference's walk
    assert mod.parse(['--stationarity']) == (True, None)
    assert mod.parse(['--trim-db', '35']) == (False, features.Silence(35.0))
    assert mod.parse(['--max-pause', '8']) == (False, features.Silence(pause=8))
    assert mod.parse(['--trim-hang', '1', '--trim-edge', '3', '--stationarity']) == (True, features.Silence(40.0, 1, 3))
    with pytest.raises(ValueError, match='Silence: hang'):
        mod.parse(['--trim-hang', '-1'])
