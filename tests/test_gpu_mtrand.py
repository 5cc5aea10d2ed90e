"""numpy's MT19937 stream on the GPU (csrc/mtrand.hip through the C ABI): pytest -m gpu.  Seconds in total.

ss_mt19937_rand against numpy.random.RandomState itself, to the bit, in every draw and in the state left behind: seeds 0, 1, 225, 2^32 - 1,
start positions 0, 1, 2, 623, 624 and counts 0, 1, 2, 311, 312, 313, 624, 625, 5000 (test_mtrand_ref_selftest.py's grid: an odd position makes
a double straddle a regeneration, 312 / 313 draws end on / cross a block from position 0 and 624, 113 / 114 draws a 227-word step), one run of
200 001 draws (about 1 760 steps, the ring wrapped 390 times), two chained calls against one, count 0, and containment on guarded buffers.
ss_dither_rows against numpy slicing; features.rand_dev against prng.rand; extract_batch_sr (at 16 kHz, where it is extract_batch, and at
48 kHz) and make_spect_f0_batched with device_draws=True against extract_batch, extract_batch_sr and make_spect_f0 with the host's draws --
array equality throughout: the draws are the same numbers, so everything behind them is."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import mtrand_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
NAN = float('nan')
SEEDS = [0, 1, 225, 2 ** 32 - 1]
POSITIONS = [0, 1, 2, 623, 624]
COUNTS = [0, 1, 2, 311, 312, 313, 624, 625, 5000]


@pytest.fixture(scope='module')
def lib():
    from speechsplit_amd import _capi
    return _capi.lib()


@functools.lru_cache(maxsize=None)
def gold():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def numpy_says(seed, pos, count):
    """(state words uint32 [625] before, draws, state words after) of numpy's own generator"""
    prng = R.generator_at(seed, pos)
    before = words_of(prng)
    draws = prng.rand(count)
    after = words_of(prng)
    for a in (before, draws, after):
        a.setflags(write=False)
    return before, draws, after


def words_of(prng):
    s = prng.get_state()
    return np.concatenate((s[1], [s[2]])).astype(np.uint32)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.ss_last_error()


def _state_dev(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32)).to(DEV)


def _words(state_dev):
    return state_dev.cpu().numpy().view(np.uint32)


def gpu_rand(lib, words, count, room=0):
    """-> (draws numpy [count], what lies behind them [room], state words after); the output starts as NaN"""
    st = _state_dev(words)
    out = torch.full((count + room,), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_mt19937_rand(_p(st), count, _p(out), _s()))
    got = out.cpu().numpy()
    return got[:count], got[count:], _words(st)


# ---------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize('seed', SEEDS)
def test_the_grid_equals_numpy_in_every_draw_and_in_the_end_state(lib, seed):
    for pos in POSITIONS:
        for count in COUNTS:
            before, want, after = numpy_says(seed, pos, count)
            got, behind, state = gpu_rand(lib, before, count, room=3)
            assert R.same(got, want), (seed, pos, count, int((got != want).sum()))
            assert np.array_equal(state, after), (seed, pos, count, int(state[624]), int(after[624]))
            assert np.isnan(behind).all(), (seed, pos, count)


def test_200001_draws_equal_numpy(lib):
    before, want, after = numpy_says(225, 623, 200001)
    got, _, state = gpu_rand(lib, before, 200001)
    assert R.same(got, want), int((got != want).sum())
    assert np.array_equal(state, after)


def test_two_chained_calls_equal_one(lib):
    before, want, after = numpy_says(1, 2, 5000)
    st = _state_dev(before)
    out = torch.full((5000,), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_mt19937_rand(_p(st), 313, _p(out), _s()))
    _check(lib, lib.ss_mt19937_rand(_p(st), 4687, _p(out[313:]), _s()))
    assert R.same(out.cpu().numpy(), want) and np.array_equal(_words(st), after)


def test_count_0_leaves_the_state_and_the_output_untouched(lib):
    before, _, _ = numpy_says(225, 623, 0)
    got, behind, state = gpu_rand(lib, before, 0, room=8)
    assert got.shape == (0,) and np.isnan(behind).all() and np.array_equal(state, before)
    st = _state_dev(before)
    _check(lib, lib.ss_mt19937_rand(_p(st), 0, None, _s()))                                 # out_dev may be NULL when count is 0
    assert np.array_equal(_words(st), before)


def test_a_pos_above_624_reads_as_624(lib):
    before, want, after = numpy_says(0, 624, 625)
    bent = before.copy()
    bent[624] = 0xffffffff
    got, _, state = gpu_rand(lib, bent, 625)
    assert R.same(got, want) and np.array_equal(state, after)


@pytest.mark.parametrize('pos,count', [(623, 1), (1, 313), (624, 5000)])
def test_containment_rand(lib, pos, count):
    before, want, after = numpy_says(2 ** 32 - 1, pos, count)
    gs = G.out((625,), DEV, dtype=torch.int32, fill=torch.from_numpy(before.view(np.int32).copy()), name='state')
    go = G.out((count,), DEV, dtype=torch.float64, name='out')
    _check(lib, lib.ss_mt19937_rand(_p(gs.t), count, _p(go.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gs, go])                                                                   # nothing outside out[0 .. count) or state[0 .. 625)
    assert R.same(go.t.cpu().numpy(), want) and np.array_equal(_words(gs.t.contiguous()), after)


# ---------------------------------------------------------------------------------------------- the gather
LENS, MAX_N = [513, 600, 12345], 12345


@functools.lru_cache(maxsize=None)
def stream():
    d = np.random.RandomState(7).rand(sum(LENS) + 100)
    d.setflags(write=False)
    return d


def gpu_rows(lib, draws, first, n, max_n, count=None):
    out = torch.full((len(first), max_n), NAN, dtype=torch.float64, device=DEV)
    f_dev, n_dev = torch.tensor(first, dtype=torch.int64, device=DEV), torch.tensor(n, dtype=torch.int32, device=DEV)
    _check(lib, lib.ss_dither_rows(_p(draws), draws.numel() if count is None else count, _p(f_dev), _p(n_dev), len(first), max_n, _p(out), _s()))
    return out.cpu().numpy()                                                                # (f_dev and n_dev live until the copy has waited)


def _zeros_behind(row, k):
    return not row[k:].any() and not np.signbit(row[k:]).any()


def test_ragged_rows_equal_numpy_slicing_in_any_order(lib):
    d = stream()
    draws = torch.tensor(d).to(DEV)
    first = [0, 513, 1113]                                                                  # the prefix sums of the lengths
    got = gpu_rows(lib, draws, first, LENS, MAX_N)
    for b, (f, k) in enumerate(zip(first, LENS)):
        assert R.same(got[b, :k], d[f:f + k]) and _zeros_behind(got[b], k), b
    perm = [2, 0, 1]
    again = gpu_rows(lib, draws, [first[i] for i in perm], [LENS[i] for i in perm], MAX_N)
    for b, i in enumerate(perm):
        assert np.array_equal(again[b].view(np.int64), got[i].view(np.int64)), i
    # lengths are clamped into [0, max_n]; a max_n that is no multiple of the launcher's tile, and a single column
    odd = gpu_rows(lib, draws, [5, 7, 9, 11], [-3, 0, 1 << 30, 1030], 1031)
    assert _zeros_behind(odd[0], 0) and _zeros_behind(odd[1], 0) and R.same(odd[2], d[9:9 + 1031])
    assert R.same(odd[3, :1030], d[11:11 + 1030]) and _zeros_behind(odd[3], 1030)
    assert R.same(gpu_rows(lib, draws, [40], [1], 1)[0], d[40:41])


def test_an_out_of_range_first_spoils_its_row_only_and_reads_nothing_outside_draws(lib):
    d = stream()
    count = sum(LENS)                                                                       # the 100 draws behind it are not part of the call
    gd = G.inp(d[:count].copy(), DEV, name='draws')
    first = [-5, 513, count - 100, 1 << 40]
    n = [513, 600, 600, 513]
    gf = G.inp(torch.tensor(first, dtype=torch.int64), DEV, name='first')
    gn = G.inp(torch.tensor(n, dtype=torch.int32), DEV, name='n')
    go = G.out((4, 700), DEV, dtype=torch.float64, name='out')
    _check(lib, lib.ss_dither_rows(_p(gd.t), count, _p(gf.t), _p(gn.t), 4, 700, _p(go.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gd, gf, gn, go])
    got = go.t.cpu().numpy()                                                                # a read outside draws would have brought a NaN
    assert R.same(got[1, :600], d[513:1113]) and _zeros_behind(got[1], 600)                 # the row between them is what it should be
    for b, f in ((0, 0), (2, count - 600), (3, count - 513)):                               # clamped into [0, count - n_b]
        assert R.same(got[b, :n[b]], d[f:f + n[b]]) and _zeros_behind(got[b], n[b]), b
    # more draws asked for than there are: the columns whose draw would lie at or beyond count are zero
    short = gpu_rows(lib, gd.t, [3], [600], 700, count=500)
    assert R.same(short[0, :500], d[:500]) and _zeros_behind(short[0], 500)
    gd.check()


# ---------------------------------------------------------------------------------------------- the Python layer
def test_rand_dev_is_prng_rand_and_leaves_the_generator_where_rand_does():
    from speechsplit_amd import features
    prng, ref = np.random.RandomState(226), np.random.RandomState(226)
    ref.normal()
    prng.normal()                                                                           # a cached gaussian is carried over
    for count in (5, 12345, 0, 313):
        got = features.rand_dev(prng, count, DEV)
        assert got.dtype == torch.float64 and got.device.type == 'cuda'
        assert R.same(got.cpu().numpy(), ref.rand(count)), count
    a, b = prng.get_state(), ref.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:] and a[3] == 1
    assert R.same(prng.rand(5), ref.rand(5)) and prng.normal() == ref.normal()
    for bad in (np.random.default_rng(1), np.random.RandomState(np.random.PCG64(1))):
        with pytest.raises(TypeError, match='rand_dev'):
            features.rand_dev(bad, 10, DEV)


def _same_features(got, want):
    assert len(got) == len(want)
    for k, ((S, f0), (Sw, fw)) in enumerate(zip(got, want)):
        assert S.dtype == np.float32 and f0.dtype == np.float32 and S.shape == Sw.shape and f0.shape == fw.shape, k
        assert np.array_equal(S.view(np.int32), Sw.view(np.int32)) and np.array_equal(f0.view(np.int32), fw.view(np.int32)), k


def _same_generator(a, b):
    sa, sb = a.get_state(), b.get_state()
    return np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize('max_rows', [1, 2, 16])
def test_extract_batch_with_device_draws_equals_the_hosts(max_rows):
    from speechsplit_amd import features
    g = gold()
    xs = [np.ascontiguousarray(g[k], np.float64) for k in ('u0_x', 'u1_x')]
    seed = int(g['u0_spk'])
    host, dev = np.random.RandomState(seed), np.random.RandomState(seed)
    want = features.extract_batch(xs, host, 'M', max_rows=max_rows, mel_basis=g['mel_basis'])
    got = features.extract_batch_sr(xs, 16000, dev, 'M', max_rows=max_rows, mel_basis=g['mel_basis'], device_draws=True)
    _same_features(got, want)
    assert _same_generator(dev, host)
    assert sum(int((f > 0).sum()) for _, f in want) >= 6                                    # voiced frames were compared


def test_extract_batch_sr_with_device_draws_equals_the_hosts():
    from scipy import signal
    from speechsplit_amd import features
    g = gold()
    hi = [signal.resample_poly(np.ascontiguousarray(g[k], np.float64), 3, 1) for k in ('u0_x', 'u1_x')]       # 48 kHz
    seed = int(g['u1_spk'])
    host, dev = np.random.RandomState(seed), np.random.RandomState(seed)
    want = features.extract_batch_sr(hi, 48000, host, 'M', max_rows=2, mel_basis=g['mel_basis'])
    got = features.extract_batch_sr(hi, 48000, dev, 'M', max_rows=2, mel_basis=g['mel_basis'], device_draws=True)
    _same_features(got, want)
    assert _same_generator(dev, host)


def test_make_spect_f0_with_device_draws_writes_the_same_bytes(tmp_path):
    from speechsplit_amd import features, vocoder
    from tests import pitch_ref as P
    root = tmp_path / 'wavs'
    files = {('p226', 'b.wav'): 2304, ('p226', 'a.wav'): 1500, ('p231', 'c.wav'): 3000, ('p231', 'd.wav'): 777}    # 2304 = 9 * 256
    for (spk, name), n in files.items():
        os.makedirs(root / spk, exist_ok=True)
        vocoder.save_wav(str(root / spk / name), P.tone(110.0 if spk == 'p226' else 220.0, n))
    gen = {'p226': 'M', 'p231': 'F'}
    one = features.make_spect_f0(str(root), str(tmp_path / 's1'), str(tmp_path / 'f1'), gen, max_rows=2)
    two = features.make_spect_f0_batched(str(root), str(tmp_path / 's2'), str(tmp_path / 'f2'), gen, max_rows=2, device_draws=True)
    assert one == two == [('p226', 'a'), ('p226', 'b'), ('p231', 'c'), ('p231', 'd')]
    for spk, name in one:
        for a, b in (('s1', 's2'), ('f1', 'f2')):
            want = open(tmp_path / a / spk / (name + '.npy'), 'rb').read()
            assert len(want) > 128 and open(tmp_path / b / spk / (name + '.npy'), 'rb').read() == want, (spk, name, a)
