"""The resampler on the GPU (csrc/resample.hip through the C ABI): pytest -m gpu.  Seconds in total.

ss_resample against its restatement (resample_ref.py, which test_resample_ref_selftest.py shows to BE scipy.signal.resample_poly to the bit
and to report seven wrong stand-ins) and against resample_poly itself: the bar is array equality -- summing the same taps in the other order
already differs in the last place, so no tolerance above 0 means anything.

One ragged batch per rate pair: 1/3, 160/441, 320/441, 2/3, 2/1, 640/441 and 3/1 (48, 44.1, 22.05, 24, 8, 11.025 kHz to 16 kHz, and 16 to 48
kHz), which take the kernel that stages a tile's input span in LDS, and 1/16, whose span of 4402 samples outgrows the LDS array and takes the
kernel that reads x from global memory.  Rows: 1, 5 and 17 samples (shorter than the filter), the three lengths whose output counts sit around
the launcher's tile of 256 outputs -- 255, 256 and 257 where the ratio reaches them, else the nearest count it does reach on that side (2/1:
254 and 258; 3/1: 255, 768, 258; 640/441: 254) -- and features.npz's u0_x whole (12345 samples: 772 .. 37035 outputs, 4 .. 145 tiles).
max_n = 12400, NaN behind every row.

Then the batch properties (rows alone, two runs, NaN or zeros behind a row, clamped lengths, no lengths), containment on guarded buffers
(guarded.py: input, lengths, taps, output, scratch) and the Python layer end to end: features.resample, extract(sr=...), extract_batch_sr
against extract_batch on scipy-resampled recordings, make_spect_f0(resample=True) on a tree of 48 kHz files."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
from scipy import signal

from tests import guarded as G
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
NAN = float('nan')
TILE = 256
MAX_N = 12400
PAIRS = [(1, 3), (160, 441), (320, 441), (2, 3), (2, 1), (640, 441), (3, 1), (1, 16)]
IDS = [f'{u}-{d}' for u, d in PAIRS]


# ---------------------------------------------------------------------------------------------- inputs and references, computed once
@functools.lru_cache(maxsize=None)
def gold():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def source():
    x = np.ascontiguousarray(gold()['u0_x'], np.float64)
    assert x.shape == (12345,)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def lengths(up, down):
    """1, 5, 17; the longest input whose outputs stay inside one tile, one that fills whole tiles exactly, the shortest that needs one output
    of the next tile; all of u0_x"""
    ns = range(1, 3 * TILE * down // up + 2)
    below = max(n for n in ns if R.out_len(n, up, down) < TILE)
    exact = min(n for n in ns if R.out_len(n, up, down) % TILE == 0)
    above = min(n for n in ns if R.out_len(n, up, down) > TILE)
    return (1, 5, 17, below, exact, above, 12345)


@functools.lru_cache(maxsize=None)
def taps(up, down):
    h = R.design(up, down)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def ref(up, down, n):
    y = R.resample(source()[:n], up, down, taps(up, down))
    y.setflags(write=False)
    return y


@pytest.fixture(scope='module')
def lib():
    from speechsplit_amd import _capi
    return _capi.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a)).to(device=DEV, dtype=dtype)          # a copy: the references are read-only


def _ints(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _check(lib, rc):
    assert rc == 0, lib.ss_last_error()


def _rows(ns, max_n, fill):
    out = np.full((len(ns), max_n), fill)
    for b, n in enumerate(ns):
        out[b, :n] = source()[:n]
    return out


def bits(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def gpu_resample(lib, x, n, up, down):
    """x [B, max_n] (tensor), n int32 [B] or None -> numpy [B, M]; the output starts as NaN"""
    B, max_n = x.shape
    M = lib.ss_resample_len(max_n, up, down)
    h = _dev(taps(up, down))
    nb = lib.ss_resample_scratch_bytes(up, h.numel())
    assert M == R.out_len(max_n, up, down) and nb >= 0, lib.ss_last_error()
    sc = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    y = torch.full((B, M), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_resample(_p(x), _p(n), B, max_n, up, down, _p(h), h.numel(), _p(y), _p(sc), nb, _s()))
    return y.cpu().numpy()


def _zeros_behind(row, k):
    return not row[k:].any() and not np.signbit(row[k:]).any()


# ---------------------------------------------------------------------------------------------- a ragged batch per rate pair
def test_the_rows_sit_around_the_tile_edges():
    counts = {p: [R.out_len(n, *p) for n in lengths(*p)[3:6]] for p in PAIRS}
    for p in ((1, 3), (160, 441), (320, 441), (2, 3), (1, 16)):
        assert counts[p] == [255, 256, 257], p
    assert counts[(2, 1)] == [254, 256, 258] and counts[(3, 1)] == [255, 768, 258] and counts[(640, 441)] == [254, 256, 257]
    # which kernel the launcher takes: the span of a tile, ((256 - 1) down + n_taps - 1) / up + 2 input samples, against 2048
    span = {p: (255 * p[1] + 20 * max(p)) // p[0] + 2 for p in PAIRS}
    assert [p for p in PAIRS if span[p] > 2048] == [(1, 16)] and span[(1, 3)] == 827 and span[(160, 441)] == 759 and span[(1, 16)] == 4402


@pytest.mark.parametrize('up,down', PAIRS, ids=IDS)
def test_ragged_batch_equals_the_restatement_and_scipy(lib, up, down):
    ns = lengths(up, down)
    got = gpu_resample(lib, _dev(_rows(ns, MAX_N, NAN)), _ints(ns), up, down)       # NaN behind every row's end: nothing there is read
    assert got.shape == (len(ns), R.out_len(MAX_N, up, down))
    for b, n in enumerate(ns):
        want = ref(up, down, n)
        k = want.shape[0]
        sci = signal.resample_poly(source()[:n], up, down)
        d_ref, d_sci = float(np.abs(got[b, :k] - want).max()), float(np.abs(got[b, :k] - sci).max())
        print(f'ss_resample {up}/{down}, {n} samples -> {k}: max |difference| {d_ref:.3g} (restatement), {d_sci:.3g} (resample_poly)')
        assert R.same(got[b, :k], want) and R.same(got[b, :k], sci), (n, d_ref, d_sci)
        assert _zeros_behind(got[b], k), n                                          # exact zeros behind the row's own outputs


@pytest.mark.parametrize('up,down', PAIRS, ids=IDS)
def test_rows_alone_give_the_batchs_bits_two_runs_agree_and_nothing_behind_a_row_is_read(lib, up, down):
    ns = lengths(up, down)
    x, n = _dev(_rows(ns, MAX_N, NAN)), _ints(ns)
    got = gpu_resample(lib, x, n, up, down)
    assert np.array_equal(bits(got), bits(gpu_resample(lib, x, n, up, down)))
    assert np.array_equal(bits(got), bits(gpu_resample(lib, _dev(_rows(ns, MAX_N, 0.0)), n, up, down)))
    for b, k in enumerate(ns):
        alone = gpu_resample(lib, _dev(source()[:k])[None], None, up, down)
        assert alone.shape == (1, R.out_len(k, up, down)) and np.array_equal(bits(alone[0]), bits(got[b, :alone.shape[1]])), k


@pytest.mark.parametrize('up,down', [(160, 441), (1, 16)], ids=['160-441', '1-16'])
def test_lengths_outside_the_contract_are_clamped_and_spoil_only_their_row(lib, up, down):
    """n[b] is clamped into [1, max_n]: 0 and -7 read as 1, 2^30 as max_n, and the row between them is untouched by either"""
    max_n = 4500
    x = _rows([max_n] * 4, max_n, NAN)
    x[0, 1:] = NAN
    x[3, 1:] = NAN
    got = gpu_resample(lib, _dev(x), _ints([0, 4200, 1 << 30, -7]), up, down)
    one = ref(up, down, 1)
    for b in (0, 3):
        assert R.same(got[b, :one.shape[0]], one) and _zeros_behind(got[b], one.shape[0])
    k = R.out_len(4200, up, down)
    assert R.same(got[1, :k], ref(up, down, 4200)) and _zeros_behind(got[1], k)
    assert R.same(got[2], ref(up, down, max_n))


@pytest.mark.parametrize('up,down', [(1, 3), (3, 1), (1, 16)], ids=['1-3', '3-1', '1-16'])
def test_without_lengths_every_row_has_max_n(lib, up, down):
    max_n = 4100
    x = np.stack([source()[:max_n], source()[100:100 + max_n]])
    got = gpu_resample(lib, _dev(x), None, up, down)
    assert R.same(got[0], ref(up, down, max_n)) and R.same(got[1], R.resample(x[1], up, down, taps(up, down)))


# ---------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize('up,down', [(160, 441), (3, 1), (1, 16)], ids=['160-441', '3-1', '1-16'])
def test_containment_resample(lib, up, down):
    ns = list(lengths(up, down)[2:6])
    max_n = max(ns) + 3
    gx = G.inp(_rows(ns, max_n, NAN), DEV, name='x')
    gn = G.inp(torch.tensor(ns, dtype=torch.int32), DEV, name='n')
    gh = G.inp(taps(up, down).copy(), DEV, name='h')                                 # a copy: the references are read-only
    M = R.out_len(max_n, up, down)
    gy = G.out((len(ns), M), DEV, dtype=torch.float64, name='y')
    nb = lib.ss_resample_scratch_bytes(up, taps(up, down).shape[0])
    gsc = G.out((max(nb, 2048) // 8,), DEV, dtype=torch.float64, offset=32, fill=0.0, name='scratch')
    assert gsc.t.data_ptr() % 256 == 0
    _check(lib, lib.ss_resample(_p(gx.t), _p(gn.t), len(ns), max_n, up, down, _p(gh.t), gh.t.numel(), _p(gy.t), _p(gsc.t), max(nb, 2048), _s()))
    torch.cuda.synchronize()
    G.check_all([gx, gn, gh, gy, gsc])
    got = gy.t.cpu().numpy()
    for b, n in enumerate(ns):
        k = R.out_len(n, up, down)
        assert R.same(got[b, :k], ref(up, down, n)) and _zeros_behind(got[b], k), n


# ---------------------------------------------------------------------------------------------- the Python layer
@functools.lru_cache(maxsize=None)
def recordings_at(sr):
    """u0_x and u1_x brought up to sr on the host, and what scipy makes of them on the way back down"""
    g = gold()
    hi = [signal.resample_poly(np.ascontiguousarray(g[k], np.float64), sr, 16000) for k in ('u0_x', 'u1_x')]
    return hi, [signal.resample_poly(x, 16000, sr) for x in hi]


def test_resample_is_resample_poly_whatever_max_rows_is():
    from speechsplit_amd import features
    xs = [source()[:n] for n in (5000, 17, 12345, 769)]
    for sr_in, sr_out in ((44100, 16000), (16000, 48000)):
        want = [signal.resample_poly(x, sr_out, sr_in) for x in xs]
        for max_rows in (1, 2, 16):
            got = features.resample(xs, sr_in, sr_out, max_rows=max_rows)
            assert all(R.same(a, b) for a, b in zip(got, want)), (sr_in, sr_out, max_rows)
    assert R.same(features.resample(xs[0], 48000), signal.resample_poly(xs[0], 1, 3))


def _same_features(got, want):
    assert len(got) == len(want)
    for k, ((S, f0), (Sw, fw)) in enumerate(zip(got, want)):
        assert S.dtype == np.float32 and f0.dtype == np.float32 and S.shape == Sw.shape and f0.shape == fw.shape, k
        assert np.array_equal(bits(f0), bits(fw)), k                                       # F0 to the bit
        assert float(np.abs(S.astype(np.float64) - Sw.astype(np.float64)).max()) == 0.0, k


@pytest.mark.parametrize('sr', [48000, 44100])
def test_extract_batch_sr_is_extract_batch_on_scipys_resampling(sr):
    from speechsplit_amd import features
    g = gold()
    hi, at16 = recordings_at(sr)
    assert at16[1].shape[0] % 256 == 0                                                      # the odd-length fix applies to the RESAMPLED length
    want = features.extract_batch(at16, np.random.RandomState(226), 'M', mel_basis=g['mel_basis'])
    for max_rows in (1, 2, 16):
        got = features.extract_batch_sr(hi, sr, np.random.RandomState(226), 'M', max_rows=max_rows, mel_basis=g['mel_basis'])
        _same_features(got, want)
    assert sum(int((f > 0).sum()) for _, f in want) >= 6                                    # voiced frames were compared


def test_extract_batch_sr_takes_a_rate_per_recording_and_extract_takes_one():
    from speechsplit_amd import features
    g = gold()
    (hi48, at48), (hi44, at44) = recordings_at(48000), recordings_at(44100)
    low = np.ascontiguousarray(g['u1_x'][:5000], np.float64)
    xs, srs, at16 = [hi48[0], hi44[1], low, hi48[1]], [48000, 44100, 16000, 48000], [at48[0], at44[1], low, at48[1]]
    want = features.extract_batch(at16, np.random.RandomState(231), 'F', max_rows=2, mel_basis=g['mel_basis'], unvoiced=-1e10)
    got = features.extract_batch_sr(xs, srs, np.random.RandomState(231), 'F', max_rows=2, mel_basis=g['mel_basis'], unvoiced=-1e10)
    _same_features(got, want)
    one = features.extract(hi44[1][:14000], np.random.RandomState(3), 'M', mel_basis=g['mel_basis'], sr=44100)
    ref_one = features.extract(signal.resample_poly(hi44[1][:14000], 16000, 44100), np.random.RandomState(3), 'M', mel_basis=g['mel_basis'])
    _same_features([one], [ref_one])


def test_make_spect_f0_resamples_a_tree_of_48_khz_files(tmp_path):
    from speechsplit_amd import features, vocoder
    from tests import pitch_ref as P
    root = tmp_path / 'wavs'
    files = {('p226', 'b.wav'): 2304, ('p226', 'a.wav'): 1500, ('p231', 'c.wav'): 3000}    # samples at 16 kHz; 2304 = 9 * 256
    for (spk, name), n in files.items():
        os.makedirs(root / spk, exist_ok=True)
        vocoder.save_wav(str(root / spk / name), signal.resample_poly(P.tone(110.0 if spk == 'p226' else 220.0, n), 3, 1), sr=48000)
    gen = {'p226': 'M', 'p231': 'F'}
    with pytest.raises(ValueError, match='sample rate 48000'):
        features.make_spect_f0(str(root), str(tmp_path / 's0'), str(tmp_path / 'f0'), gen)            # the default still refuses them
    one = features.make_spect_f0(str(root), str(tmp_path / 's1'), str(tmp_path / 'f1'), gen, resample=True)
    two = features.make_spect_f0(str(root), str(tmp_path / 's2'), str(tmp_path / 'f2'), gen, resample=True, max_rows=2)
    assert one == two == [('p226', 'a'), ('p226', 'b'), ('p231', 'c')]
    for spk in ('p226', 'p231'):
        names = sorted(name for s, name in files if s == spk)
        at16 = []
        for name in names:
            x, sr = features.read_audio(str(root / spk / name))
            assert sr == 48000 and x.shape[0] == 3 * files[(spk, name)]
            at16.append(signal.resample_poly(x, 16000, 48000))
        prng = np.random.RandomState(int(spk[1:]))
        per_file = [features.extract(y, prng, gen[spk], unvoiced=-1e10) for y in at16]
        batched = features.extract_batch(at16, np.random.RandomState(int(spk[1:])), gen[spk], 2, unvoiced=-1e10)
        for name, w1, w2 in zip(names, per_file, batched):
            for d_s, d_f, want in (('s1', 'f1', w1), ('s2', 'f2', w2)):
                S = np.load(tmp_path / d_s / spk / (name[:-4] + '.npy'))
                f0 = np.load(tmp_path / d_f / spk / (name[:-4] + '.npy'))
                _same_features([(S, f0)], [want])
            assert (w1[1] != np.float32(-1e10)).sum() >= 2
