"""CPU-only checks of the device generator's interface: the C symbols and their header text, every refusal (each is made before anything is
enqueued, so a fake non-null device pointer is enough and no device is needed), features.rand_dev's type checks, and the host side of
extract_batch_sr / make_spect_f0_batched with device_draws -- the draw made once for the sum of the fixed-up lengths in input order,
the prefix-sum offsets in the batches' row order, the upload half as long, the default making today's calls -- with the device calls replaced
by host stand-ins.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from speechsplit_amd import _capi, convert, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
SIGNATURES = {
    'ss_mt19937_rand': (_i, [_vp, _l, _vp, _vp]),                                          # state, count, out, stream
    'ss_dither_rows': (_i, [_vp, _l, _vp, _vp, _i, _i, _vp, _vp]),                         # draws, count, first, n, B, max_n, out, stream
}
PTR = C.c_void_p(1 << 20)                                                                 # fake, non-null; never dereferenced


def test_symbols_and_signatures():
    lib = _capi.lib()
    for name, (res, args) in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        assert _capi.SYMBOLS[name][0] is res and list(_capi.SYMBOLS[name][1]) == args, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.ss_abi_version() == 2


def test_header_declares_them_and_states_the_definition():
    raw = open(os.path.join(ROOT, 'include', 'speechsplit_amd.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', raw, flags=re.S))
    for decl in ('int ss_mt19937_rand(unsigned* state_dev , long count, double* out_dev , void* stream);',
                 'int ss_dither_rows(const double* draws_dev, long count, const long* first_dev, const int* n_dev, int B, int max_n, '
                 'double* out_dev , void* stream);'):
        assert decl in text, decl
    assert raw.index(' ss_resample(const') < raw.index(' ss_mt19937_rand(unsigned') < raw.index(' ss_dither_rows(const') \
        < raw.index(' ss_griffinlim_samples(')
    whole = re.sub(r'\s+', ' ', raw)
    for phrase in ('N = 624, M = 397, A = 0x9908b0df', 'y = (x[n] & 0x80000000) | (x[n+1] & 0x7fffffff)',
                   'x[n+624] = x[n+397] ^ (y >> 1) ^ ((y & 1) ? A : 0)', 'y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680; y ^= (y << 15) & 0xefc60000; y ^= y >> 18',
                   'w[j] = temper(x[pos + j])', 'out[i] = ((w[2i] >> 5) * 67108864.0 + (w[2i+1] >> 6)) / 9007199254740992.0',
                   'exact in double', 'k = (tot - 1) / 624', "key' = x[624k .. 624k + 623] and pos' = tot - 624k", 'the kernel treats it as 624',
                   'the state is unchanged, nothing is written', '227 consecutive words are independent', 'ONE workgroup',
                   'out[b][i] = draws[first[b] + i] for i < n_b', 'n_b = min(max(n[b], 0), max_n)', 'exact zeros behind n_b',
                   'spoils that row only', 'nothing outside draws[0 .. count) is read', 'count outside 0 .. 2^40'):
        assert phrase in whole, phrase


def _refused(rc, word):
    msg = _capi.lib().ss_last_error()
    assert rc != 0 and word.encode() in msg, (word, msg)


def test_every_refusal_names_its_argument():
    lib = _capi.lib()
    rand = lambda **k: lib.ss_mt19937_rand(*[k.get(a, d) for a, d in (('state', PTR), ('count', 100), ('out', PTR), ('stream', None))])
    _refused(rand(state=None), 'ss_mt19937_rand: null pointer: state_dev')
    _refused(rand(state=None, count=0, out=None), 'null pointer: state_dev')
    _refused(rand(out=None), 'ss_mt19937_rand: null pointer: out_dev')
    _refused(rand(out=None, count=1), 'null pointer: out_dev')
    for c in (-1, -(1 << 40), (1 << 40) + 1, 1 << 62):
        _refused(rand(count=c), 'ss_mt19937_rand: count outside 0 .. 2^40')
        _refused(rand(count=c, out=None), 'count outside 0 .. 2^40')
    rows = lambda **k: lib.ss_dither_rows(*[k.get(a, d) for a, d in (('draws', PTR), ('count', 5000), ('first', PTR), ('n', PTR), ('B', 3),
                                                                      ('max_n', 600), ('out', PTR), ('stream', None))])
    for arg in ('draws', 'first', 'n', 'out'):
        _refused(rows(**{arg: None}), f'ss_dither_rows: null pointer: {arg}_dev')
    for c in (-1, (1 << 40) + 1):
        _refused(rows(count=c), 'ss_dither_rows: count outside 0 .. 2^40')
    for B in (0, -3, 65536):
        _refused(rows(B=B), 'ss_dither_rows: B outside 1 .. 65535')
    for m in (0, -600):
        _refused(rows(max_n=m), 'ss_dither_rows: max_n below 1')


def test_rand_dev_takes_a_randomstate_on_mt19937_only():
    for bad in (np.random.default_rng(1), np.random.RandomState(np.random.PCG64(1)), np.random.MT19937(1), 7, None):
        with pytest.raises(TypeError, match='rand_dev'):
            features.rand_dev(bad, 10, 'cpu')
    with pytest.raises(ValueError, match='count'):
        features.rand_dev(np.random.RandomState(1), -1, 'cpu')
    prng = np.random.RandomState(3)
    before = prng.get_state()
    out = features.rand_dev(prng, 0, 'cpu')                                                # nothing to draw: no call, the generator as it was
    after = prng.get_state()
    assert out.shape == (0,) and str(out.dtype) == 'torch.float64'
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


# ---------------------------------------------------------------------------------------------- host side, the device calls replaced
LENGTHS = [2304, 513, 5000, 1100, 512, 768]
FIXED = [2305, 513, 5000, 1100, 513, 769]                                                  # 2304, 512 and 768 grow by the 1e-6 sample


def _recordings():
    rng = np.random.default_rng(11)
    return [rng.uniform(-1.0, 1.0, n) for n in LENGTHS]


def _stand_ins(monkeypatch, log):
    """rand_dev and dither_rows_dev on the host (numpy's own draws, numpy slicing) and the chain's four calls as recorders"""
    import torch

    def fake_rand(prng, count, device='cuda'):
        log['rand'].append(count)
        return torch.from_numpy(prng.rand(count))

    def fake_rows(draws, first, n, max_n):
        assert draws.dtype == torch.float64 and first.dtype == torch.int64 and n.dtype == torch.int32 and first.shape == n.shape
        out = torch.zeros(first.shape[0], max_n, dtype=torch.float64)
        for b, (f, k) in enumerate(zip(first.tolist(), n.tolist())):
            out[b, :k] = draws[f:f + k]
        log['rows'].append((first.tolist(), n.tolist(), max_n))
        return out

    def fake_filt(x, n, b_, a_, zi_, gain, dither, scale):
        assert (gain, scale) == (0.96, 1e-06) and dither.shape == x.shape and dither.dtype == torch.float64
        log['filt'].append((n.tolist(), x.numpy().copy(), dither.numpy().copy()))
        return x + 0.1234567890123

    monkeypatch.setattr(features, 'rand_dev', fake_rand)
    monkeypatch.setattr(features, 'dither_rows_dev', fake_rows)
    monkeypatch.setattr(features, 'filtfilt_dev', fake_filt)
    monkeypatch.setattr(features, 'melspec_batch_dev',
                        lambda wav, n, mb: wav[:, :1, None].float().expand(wav.shape[0], wav.shape[1] // 256 + 1, 80).contiguous())
    monkeypatch.setattr(features, 'pitch_track_dev', lambda wav, n, lo, hi: torch.zeros(wav.shape[0], wav.shape[1] // 256 + 1, dtype=torch.float64))
    monkeypatch.setattr(features, 'f0_normalize_batch_dev', lambda f0, n, max_n, unvoiced: n[:, None].float().expand(f0.shape).contiguous())


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_device_draws_is_one_draw_in_input_order_and_a_gather_per_batch(monkeypatch, max_rows):
    xs = _recordings()
    log = {'rand': [], 'rows': [], 'filt': []}
    _stand_ins(monkeypatch, log)
    prng = np.random.RandomState(226)
    out = features.extract_batch_sr(xs, 16000, prng, 'F', max_rows=max_rows, device='cpu', unvoiced=-1e10, device_draws=True)
    ref = np.random.RandomState(226)
    draws = [ref.rand(n) for n in FIXED]                                                   # input order, the reference's loop
    assert prng.rand() == ref.rand()                                                        # the generator is left where the loop leaves it
    plan = convert.plan_batches(FIXED, max_rows)
    start = np.concatenate(([0], np.cumsum(FIXED)[:-1])).tolist()
    assert log['rand'] == [sum(FIXED)]                                                      # ONE draw, whatever max_rows is
    assert log['rows'] == [([start[i] for i in b], [FIXED[i] for i in b], FIXED[b[-1]]) for b in plan]
    assert [ns for ns, _, _ in log['filt']] == [[FIXED[i] for i in b] for b in plan]
    for b, (ns, x, r) in zip(plan, log['filt']):
        for k, i in enumerate(b):
            assert np.array_equal(r[k, :ns[k]], draws[i]) and not r[k, ns[k]:].any(), i     # each row its own draws, zeros behind
            assert np.array_equal(x[k, :LENGTHS[i]], xs[i]) and not x[k, ns[k]:].any(), i
    assert len(out) == len(xs) and all(np.all(f0n == n) for n, (_, f0n) in zip(FIXED, out))
    # the host path, same stand-ins: no device draw, the same rows handed to the filter
    host = {'rand': [], 'rows': [], 'filt': []}
    _stand_ins(monkeypatch, host)
    features.extract_batch(xs, np.random.RandomState(226), 'F', max_rows=max_rows, device='cpu', unvoiced=-1e10)
    assert host['rand'] == [] and host['rows'] == [] and len(host['filt']) == len(log['filt'])
    for (ns, x, r), (ns2, x2, r2) in zip(log['filt'], host['filt']):
        assert ns == ns2 and np.array_equal(x, x2) and np.array_equal(r, r2)


def test_the_upload_carries_the_recordings_only():
    xs = _recordings()
    prng = np.random.RandomState(5)
    before = prng.get_state()
    flat, lens, batches = features.stage_batches(xs, prng, 4, host_draws=False)
    assert np.array_equal(before[1], prng.get_state()[1]) and before[2] == prng.get_state()[2]     # no draw was made
    both, lens2, batches2 = features.stage_batches(xs, np.random.RandomState(5), 4)
    assert 2 * flat.shape[0] == both.shape[0] and np.array_equal(lens, lens2)
    assert [b[0] for b in batches] == [b[0] for b in batches2]
    for (idx, o, B, max_n), (_, o2, _, _) in zip(batches, batches2):
        assert 2 * o == o2 and np.array_equal(flat[o:o + B * max_n], both[o2:o2 + B * max_n])


def test_extract_batch_sr_draws_once_on_the_resampled_lengths(monkeypatch):
    import torch
    from scipy import signal
    xs = _recordings()
    srs = [48000, 16000, 48000, 16000, 48000, 48000]
    log = {'rand': [], 'rows': [], 'filt': []}
    _stand_ins(monkeypatch, log)
    monkeypatch.setattr(features, '_resample_group', lambda ws, up, down, max_rows, device:
                        [torch.from_numpy(signal.resample_poly(w, up, down)) for w in ws])
    at16 = [x if sr == 16000 else signal.resample_poly(x, 16000, sr) for x, sr in zip(xs[:4], srs[:4])]
    fixed = [len(y) + 1 if len(y) % 256 == 0 else len(y) for y in at16]
    assert fixed == [769, 513, 1667, 1100]
    prng = np.random.RandomState(231)
    features.extract_batch_sr(xs[:4], srs[:4], prng, 'F', max_rows=2, device='cpu', device_draws=True)
    ref = np.random.RandomState(231)
    draws = [ref.rand(n) for n in fixed]
    assert prng.rand() == ref.rand() and log['rand'] == [sum(fixed)]
    plan = convert.plan_batches(fixed, 2)
    start = np.concatenate(([0], np.cumsum(fixed)[:-1])).tolist()
    assert log['rows'] == [([start[i] for i in b], [fixed[i] for i in b], fixed[b[-1]]) for b in plan]
    for b, (ns, x, r) in zip(plan, log['filt']):
        for k, i in enumerate(b):
            assert np.array_equal(r[k, :ns[k]], draws[i]) and not r[k, ns[k]:].any(), i


def test_the_keyword_defaults_to_off_and_off_makes_todays_calls(monkeypatch, tmp_path):
    for fn in (features.extract_batch_sr, features.make_spect_f0_batched):
        p = inspect.signature(fn).parameters['device_draws']
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    # extract_batch and make_spect_f0 keep the argument lists the existing tests pin; the batched walk takes its options by keyword
    assert 'device_draws' not in inspect.signature(features.extract_batch).parameters
    assert 'device_draws' not in inspect.signature(features.make_spect_f0).parameters
    assert list(inspect.signature(features.make_spect_f0_batched).parameters) == [
        'root_dir', 'target_dir', 'target_dir_f0', 'spk2gen', 'max_rows', 'device', 'resample', 'device_draws']
    handed = []
    monkeypatch.setattr(features, 'extract_batch', lambda *a, **k: handed.append((a, k)) or 'result')
    monkeypatch.setattr(features, '_extract_batch', lambda *a: handed.append((a, 'device')) or 'on the device')
    monkeypatch.setattr(features, 'rand_dev', lambda *a, **k: pytest.fail('the default draws on the host'))
    xs = _recordings()
    prng = np.random.RandomState(5)
    assert features.extract_batch_sr(xs, 16000, prng, 'M', 4, 'cpu', None, -1e10) == 'result'
    got = handed.pop()
    assert got[0][1:] == (prng, 'M', 4, 'cpu', None, -1e10) and got[1] == {}               # today's call: no keyword at all
    assert features.extract_batch_sr(xs, 16000, prng, 'M', 4, 'cpu', None, -1e10, device_draws=True) == 'on the device'
    got = handed.pop()
    assert got[0][1:] == (prng, 'M', 4, 'cpu', None, -1e10, True) and got[1] == 'device'
    # the walk hands the keyword on only when it is set
    seen = []
    monkeypatch.setattr(features, 'extract_batch_sr', lambda *a, **k: seen.append(k) or [(np.zeros((3, 80), np.float32), np.zeros(3, np.float32))])
    monkeypatch.setattr(features, 'read_wav', lambda path: np.zeros(600))
    root = tmp_path / 'wavs' / 'p226'
    os.makedirs(root)
    open(root / 'a.wav', 'wb').close()
    args = (str(tmp_path / 'wavs'), str(tmp_path / 's'), str(tmp_path / 'f'), {'p226': 'M'})
    assert features.make_spect_f0(*args, device='cpu', max_rows=2) == [('p226', 'a')]
    assert features.make_spect_f0_batched(*args, 2, device='cpu') == [('p226', 'a')]
    assert features.make_spect_f0_batched(*args, max_rows=2, device='cpu', device_draws=True) == [('p226', 'a')]
    assert seen == [{'unvoiced': -1e10}, {'unvoiced': -1e10}, {'unvoiced': -1e10, 'device_draws': True}]
    for bad in (None, 0, True, 2.0):
        with pytest.raises(ValueError, match='max_rows must be a positive integer'):
            features.make_spect_f0_batched(*args, max_rows=bad)
    with pytest.raises(TypeError, match='device_draws must be True or False'):
        features.make_spect_f0_batched(*args, device_draws=1)
