"""Batched feature extraction on the GPU (csrc/filtfilt.hip and csrc/features.hip through the C ABI): pytest -m gpu.  Seconds in total.

ss_filtfilt against its restatement (filtfilt_ref.py, which test_filtfilt_ref_selftest.py shows to BE scipy.signal.filtfilt to the bit and to
report seven wrong stand-ins): the bar is array equality, because the reference's filter is ill-conditioned in scipy's direct form and any
other arrangement of the arithmetic lands ~3e-7 away -- no tolerance between 0 and that means anything.  One ragged batch of 513, 600, 1100 and
2305 samples (cuts of features.npz's u1_x), 10241 (u1_x with its appended sample) and 12345 (u0_x), max_n = 12400, NaN behind every row.

ss_melspec_batch at 3, 5, 10, 41 and 49 frames (u1_wav cut to 513, 1100 and 2304 = 9 * 256 samples, the last frame centred on the end; u1_wav;
u0_wav) and 80, 7 and 1 mel bands, each within 1e-6 -- the project's bar for a spectrogram, test_gpu_pitch.py's against the fixture -- of the
float64 numpy restatement (griffinlim_ref.melspec), of ss_melspec on the same row and of the fixture's u0_S / u1_S.  Measured, printed by the
tests: see DESIGN.md section 8.

ss_f0_normalize_batch: voiced frames with the bits of ss_f0_normalize on the row alone, the fill at 0 and at -1e10.  All three calls on guarded
buffers (guarded.py), scratch included.  extract_batch against extract, make_spect_f0(max_rows=2) against make_spect_f0()."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import filtfilt_ref as R
from tests import griffinlim_ref as GL
from tests import guarded as G

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
NAN = float('nan')
UNVOICED = -1e10
MEL_BAR = 1e-6

# ---------------------------------------------------------------------------------------------- inputs and references, computed once
FILT_ROWS = ('513', '600', '1100', '2305', 'u1', 'u0')
FILT_MAX_N = 12400
MEL_ROWS = (('513', 3), ('1100', 5), ('2304', 10), ('u1', 41), ('u0', 49))


@functools.lru_cache(maxsize=None)
def gold():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def recordings():
    g = gold()
    u1 = np.ascontiguousarray(g['u1_x'], np.float64)
    out = {'513': u1[:513].copy(), '600': u1[:600].copy(), '1100': u1[:1100].copy(), '2305': u1[:2305].copy(), 'u1': R.odd_length_fix(u1),
           'u0': np.ascontiguousarray(g['u0_x'], np.float64)}
    assert [out[k].shape[0] for k in FILT_ROWS] == [513, 600, 1100, 2305, 10241, 12345]
    return out


@functools.lru_cache(maxsize=None)
def draws(name):
    """prng.rand for this recording as its speaker's first (the fixture's speakers for u0 / u1)"""
    g = gold()
    seed = {'u0': int(g['u0_spk']), 'u1': int(g['u1_spk'])}.get(name, 7)
    r = np.random.RandomState(seed).rand(recordings()[name].shape[0])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def filt_ref(name, dithered=False, cut=None):
    b, a, zi = R.coefficients()
    x = recordings()[name][:cut]
    y = R.filtfilt(x, b, a, zi, R.GAIN, draws(name)[:cut], R.DITHER_SCALE) if dithered else R.filtfilt(x, b, a, zi)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def waves():
    g = gold()
    u1 = np.ascontiguousarray(g['u1_wav'], np.float64)
    return {'513': u1[:513].copy(), '1100': u1[:1100].copy(), '2304': u1[:2304].copy(), 'u1': u1, 'u0': np.ascontiguousarray(g['u0_wav'], np.float64)}


@functools.lru_cache(maxsize=None)
def basis(n_mels):
    mb = gold()['mel_basis']
    return np.ascontiguousarray({80: mb, 7: mb[:, 10:80:10], 1: mb[:, 40:41]}[n_mels], np.float64)


@functools.lru_cache(maxsize=None)
def mel_ref(name, n_mels):
    S = GL.melspec(waves()[name], basis(n_mels))
    S.setflags(write=False)
    return S


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


def _host(v):
    a = np.ascontiguousarray(v, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


def _rows(sigs, max_n, fill):
    """[len(sigs), max_n] with each signal at the head of its row and `fill` behind it"""
    out = np.full((len(sigs), max_n), fill)
    for b, x in enumerate(sigs):
        out[b, :x.shape[0]] = x
    return out


def gpu_filtfilt(lib, x, n, gain=1.0, dither=None, scale=0.0):
    """x [B, max_n] (tensor), n int32 [B] or None -> numpy [B, max_n]; the output starts as NaN"""
    B, max_n = x.shape
    (b, pb), (a, pa), (zi, pz) = (_host(v) for v in R.coefficients())
    nb = lib.ss_filtfilt_scratch_bytes(B, max_n)
    assert nb > 0, lib.ss_last_error()
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    y = torch.full((B, max_n), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_filtfilt(_p(x), _p(n), B, max_n, pb, pa, pz, gain, _p(dither), scale, _p(y), _p(sc), nb, _s()))
    return y.cpu().numpy()


def gpu_mel(lib, wav, n, mb):
    """wav [B, max_n], mb [513, n_mels] (tensors) -> numpy float32 [B, F, n_mels]; the output starts as NaN"""
    B, max_n = wav.shape
    out = torch.full((B, max_n // 256 + 1, mb.shape[1]), NAN, dtype=torch.float32, device=DEV)
    _check(lib, lib.ss_melspec_batch(_p(wav), _p(n), B, max_n, _p(mb), mb.shape[1], _p(out), _s()))
    return out.cpu().numpy()


def gpu_mel_single(lib, x, mb):
    out = torch.full((x.shape[0] // 256 + 1, mb.shape[1]), NAN, dtype=torch.float32, device=DEV)
    _check(lib, lib.ss_melspec(_p(x), x.shape[0], _p(mb), mb.shape[1], _p(out), _s()))
    return out.cpu().numpy()


def gpu_f0n(lib, f0, n, max_n, unvoiced):
    B, F = f0.shape
    out = torch.full((B, F), NAN, dtype=torch.float32, device=DEV)
    _check(lib, lib.ss_f0_normalize_batch(_p(f0), _p(n), B, max_n, unvoiced, _p(out), _s()))
    return out.cpu().numpy()


def gpu_f0n_single(lib, f0):
    out = torch.full((f0.shape[0],), NAN, dtype=torch.float32, device=DEV)
    _check(lib, lib.ss_f0_normalize(_p(f0), f0.shape[0], _p(out), _s()))
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------- the filter
def _filt_batch(fill):
    sigs = [recordings()[k] for k in FILT_ROWS]
    return _dev(_rows(sigs, FILT_MAX_N, fill)), _ints([s.shape[0] for s in sigs])


def test_filtfilt_ragged_batch_equals_the_restatement(lib):
    x, n = _filt_batch(NAN)                                              # NaN behind every row's end: nothing there is read
    got = gpu_filtfilt(lib, x, n)
    for b, name in enumerate(FILT_ROWS):
        want = filt_ref(name)
        k = want.shape[0]
        worst = float(np.abs(got[b, :k] - want).max())
        print(f'ss_filtfilt {name} ({k} samples): max |difference| {worst:.3g}, max |y| {float(np.abs(want).max()):.3g}')
        assert R.same(got[b, :k], want), (name, worst)
        assert not got[b, k:].any() and not np.signbit(got[b, k:]).any(), name             # exact zeros behind the row


def test_filtfilt_with_gain_and_dither_is_the_fixtures_waveform(lib):
    x, n = _filt_batch(NAN)
    r = _dev(_rows([draws(k) for k in FILT_ROWS], FILT_MAX_N, NAN))
    got = gpu_filtfilt(lib, x, n, R.GAIN, r, R.DITHER_SCALE)
    for b, name in enumerate(FILT_ROWS):
        want = filt_ref(name, True)
        assert R.same(got[b, :want.shape[0]], want), name
        assert not got[b, want.shape[0]:].any(), name
    g = gold()
    assert R.same(got[4, :10241], np.ascontiguousarray(g['u1_wav'], np.float64))
    assert R.same(got[5, :12345], np.ascontiguousarray(g['u0_wav'], np.float64))
    # gain alone, no dither input
    plain = gpu_filtfilt(lib, x, n, R.GAIN)
    assert R.same(plain[1, :600], np.asarray(filt_ref('600')) * R.GAIN)


def test_filtfilt_rows_alone_give_the_batchs_bits_and_two_runs_agree(lib):
    x, n = _filt_batch(NAN)
    r = _dev(_rows([draws(k) for k in FILT_ROWS], FILT_MAX_N, NAN))
    got = gpu_filtfilt(lib, x, n, R.GAIN, r, R.DITHER_SCALE)
    again = gpu_filtfilt(lib, x, n, R.GAIN, r, R.DITHER_SCALE)
    assert np.array_equal(bits(got), bits(again))
    for b, name in enumerate(FILT_ROWS):
        k = recordings()[name].shape[0]
        alone = gpu_filtfilt(lib, _dev(recordings()[name])[None], None, R.GAIN, _dev(draws(name))[None], R.DITHER_SCALE)
        assert np.array_equal(bits(alone[0]), bits(got[b, :k])), name


def test_filtfilt_without_lengths_every_row_has_max_n(lib):
    g = gold()
    sigs = [recordings()['600'], np.ascontiguousarray(g['u0_x'][:600], np.float64)]
    got = gpu_filtfilt(lib, _dev(np.stack(sigs)), None)
    b, a, zi = R.coefficients()
    assert R.same(got[0], filt_ref('600')) and R.same(got[1], R.filtfilt(sigs[1], b, a, zi))


def test_filtfilt_lengths_outside_the_contract_are_clamped(lib):
    """every kernel clamps n[b] into [513, max_n]: 0 reads as 513, 2^30 as max_n, and the row between them is untouched by either"""
    x = np.stack([recordings()['600']] * 3)
    x[0, 513:] = NAN
    got = gpu_filtfilt(lib, _dev(x), _ints([0, 600, 1 << 30]))
    assert R.same(got[0, :513], filt_ref('600', False, 513)) and not got[0, 513:].any()
    assert R.same(got[1], filt_ref('600')) and R.same(got[2], filt_ref('600'))
    assert R.same(filt_ref('600', False, 513), filt_ref('513'))                             # the same cut of u1_x


# ---------------------------------------------------------------------------------------------- the mel spectrogram
def _mel_batch(fill):
    sigs = [waves()[k] for k, _ in MEL_ROWS]
    return _dev(_rows(sigs, 12345, fill)), _ints([s.shape[0] for s in sigs])


@pytest.mark.parametrize('n_mels', [80, 7, 1])
def test_melspec_batch_against_the_restatement_the_single_call_and_the_fixture(lib, n_mels):
    wav, n = _mel_batch(NAN)
    mb = _dev(basis(n_mels))
    got = gpu_mel(lib, wav, n, mb)
    assert got.shape == (5, 49, n_mels) and got.dtype == np.float32
    for b, (name, F) in enumerate(MEL_ROWS):
        want = mel_ref(name, n_mels)
        assert want.shape == (F, n_mels)
        single = gpu_mel_single(lib, _dev(waves()[name]), mb)
        d_ref = float(np.abs(got[b, :F].astype(np.float64) - want).max())
        d_one = float(np.abs(got[b, :F].astype(np.float64) - single.astype(np.float64)).max())
        print(f'ss_melspec_batch {name} ({F} frames, {n_mels} bands): against numpy {d_ref:.3g}, against ss_melspec {d_one:.3g}')
        assert np.isfinite(got[b, :F]).all() and d_ref <= MEL_BAR and d_one <= MEL_BAR, (name, d_ref, d_one)
        assert not got[b, F:].any(), name                                                   # zeros behind the row's own frames
        if n_mels == 80 and name in ('u0', 'u1'):
            d_fix = float(np.abs(got[b, :F].astype(np.float64) - gold()[name + '_S'].astype(np.float64)).max())
            print(f'ss_melspec_batch {name}: against the fixture {d_fix:.3g}')
            assert d_fix <= MEL_BAR


def test_melspec_batch_rows_alone_give_the_batchs_bits(lib):
    wav, n = _mel_batch(NAN)
    mb = _dev(basis(80))
    got = gpu_mel(lib, wav, n, mb)
    assert np.array_equal(bits(got), bits(gpu_mel(lib, _mel_batch(0.0)[0], n, mb)))          # and what lies behind a row is not read
    assert np.array_equal(bits(got), bits(gpu_mel(lib, wav, n, mb)))
    for b, (name, F) in enumerate(MEL_ROWS):
        alone = gpu_mel(lib, _dev(waves()[name])[None], None, mb)
        assert alone.shape == (1, F, 80) and np.array_equal(bits(alone[0]), bits(got[b, :F])), name
    # lengths outside the contract: 0 reads as 513, 2^30 as max_n
    x = _dev(np.stack([waves()['1100']] * 2))
    odd = gpu_mel(lib, x, _ints([0, 1 << 30]), mb)
    assert np.array_equal(bits(odd[0, :3]), bits(got[0, :3])) and not odd[0, 3:].any() and np.array_equal(bits(odd[1]), bits(got[1, :5]))


# ---------------------------------------------------------------------------------------------- the F0 normalisation
def _tracks(F, lens, seed):
    """ln-F0 tracks [len(lens), F]: voiced values in ln(80) .. ln(300) with unvoiced stretches, NaN behind each row's own frames"""
    rng = np.random.default_rng(seed)
    f0 = np.full((len(lens), F), NAN)
    for b, n in enumerate(lens):
        Fb = n // 256 + 1
        row = np.log(rng.uniform(80.0, 300.0, Fb))
        row[rng.uniform(size=Fb) < 0.35] = UNVOICED
        row[:2] = np.log([120.0, 190.0])                                                     # at least two distinct voiced values
        f0[b, :Fb] = row
    return f0


@pytest.mark.parametrize('unvoiced', [0.0, UNVOICED])
@pytest.mark.parametrize('max_n,lens', [(12345, [12345, 2304, 513, 1100]), (76800, [66000, 76800])], ids=['49-frames', '301-frames'])
def test_f0_normalize_batch_is_the_single_call_on_every_row(lib, max_n, lens, unvoiced):
    F = max_n // 256 + 1
    f0 = _tracks(F, lens, 5)
    if len(lens) == 4:
        f0[2, :3] = UNVOICED                                                                 # an all-unvoiced row
    got = gpu_f0n(lib, _dev(f0), _ints(lens), max_n, unvoiced)
    fill = np.float32(unvoiced)
    for b, n in enumerate(lens):
        Fb = n // 256 + 1
        row = f0[b, :Fb]
        v = row != UNVOICED
        assert np.all(got[b, Fb:] == fill) and np.all(got[b, :Fb][~v] == fill), b
        if v.any():
            single = gpu_f0n_single(lib, _dev(row))
            assert np.array_equal(bits(got[b, :Fb][v]), bits(single[v])), b                   # bit for bit
            assert got[b, :Fb][v].min() >= 0.0 and got[b, :Fb][v].max() <= 1.0
            want = (np.clip((row[v] - row[v].mean()) / row[v].std() / 4.0, -1.0, 1.0) + 1.0) / 2.0
            assert np.abs(got[b, :Fb][v] - want).max() <= 1e-6
    if len(lens) == 4:
        assert np.all(got[2] == fill)
    assert np.array_equal(bits(got), bits(gpu_f0n(lib, _dev(f0), _ints(lens), max_n, unvoiced)))
    # without lengths every row has F frames
    full = np.nan_to_num(f0, nan=UNVOICED)
    whole = gpu_f0n(lib, _dev(full), None, max_n, unvoiced)
    assert np.array_equal(bits(whole[-1 if len(lens) == 2 else 0]), bits(got[-1 if len(lens) == 2 else 0]))


# ---------------------------------------------------------------------------------------------- containment
CB, CN, CLEN = 3, 2304, [2304, 513, 1300]
CF = CN // 256 + 1


def test_containment_filtfilt(lib):
    x = _rows([recordings()['2305'][:n] for n in CLEN], CN, NAN)
    r = _rows([draws('2305')[:n] for n in CLEN], CN, NAN)
    gx, gr = G.inp(x, DEV, name='x'), G.inp(r, DEV, name='dither')
    gn = G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')
    gy = G.out((CB, CN), DEV, dtype=torch.float64, name='y')
    nb = lib.ss_filtfilt_scratch_bytes(CB, CN)
    gsc = G.out((nb // 8,), DEV, dtype=torch.float64, offset=32, fill=0.0, name='scratch')
    assert gsc.t.data_ptr() % 256 == 0
    (b, pb), (a, pa), (zi, pz) = (_host(v) for v in R.coefficients())
    _check(lib, lib.ss_filtfilt(_p(gx.t), _p(gn.t), CB, CN, pb, pa, pz, R.GAIN, _p(gr.t), R.DITHER_SCALE, _p(gy.t), _p(gsc.t), nb, _s()))
    torch.cuda.synchronize()
    G.check_all([gx, gr, gn, gy, gsc])
    got = gy.t.cpu().numpy()
    for k, n in enumerate(CLEN):
        assert R.same(got[k, :n], filt_ref('2305', True, n)) and not got[k, n:].any()


def test_containment_melspec_batch(lib):
    gw = G.inp(_rows([waves()['2304'][:n] for n in CLEN], CN, NAN), DEV, name='wav')
    gn = G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')
    gmb = G.inp(basis(7), DEV, name='mel_basis')
    go = G.out((CB, CF, 7), DEV, dtype=torch.float32, name='out')
    _check(lib, lib.ss_melspec_batch(_p(gw.t), _p(gn.t), CB, CN, _p(gmb.t), 7, _p(go.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gw, gn, gmb, go])
    got = go.t.cpu().numpy()
    for k, n in enumerate(CLEN):
        F = n // 256 + 1
        assert np.abs(got[k, :F] - GL.melspec(waves()['2304'][:n], basis(7))).max() <= MEL_BAR and not got[k, F:].any()


def test_containment_f0_normalize_batch(lib):
    f0 = _tracks(CF, CLEN, 9)
    gf = G.inp(f0, DEV, name='f0')
    gn = G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')
    go = G.out((CB, CF), DEV, dtype=torch.float32, name='out')
    _check(lib, lib.ss_f0_normalize_batch(_p(gf.t), _p(gn.t), CB, CN, 0.0, _p(go.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gf, gn, go])
    got = go.t.cpu().numpy()
    for k, n in enumerate(CLEN):
        F = n // 256 + 1
        v = f0[k, :F] != UNVOICED
        assert np.array_equal(bits(got[k, :F][v]), bits(gpu_f0n_single(lib, _dev(f0[k, :F]))[v]))
        assert not got[k, :F][~v].any() and not got[k, F:].any()


# ---------------------------------------------------------------------------------------------- the Python layer
def test_extract_batch_is_extract_on_every_recording():
    from speechsplit_amd import features
    g = gold()
    xs = [g['u0_x'], g['u1_x'], g['u1_x'][:5000]]
    prng = np.random.RandomState(226)
    want = [features.extract(x, prng, 'M', mel_basis=g['mel_basis']) for x in xs]          # one speaker stream, the reference's order
    runs = [features.extract_batch(xs, np.random.RandomState(226), 'M', max_rows=r, mel_basis=g['mel_basis']) for r in (1, 2, 16)]
    for other in runs[1:]:
        for (S0, f0), (S1, f1) in zip(runs[0], other):
            assert np.array_equal(bits(S0), bits(S1)) and np.array_equal(bits(f0), bits(f1))
    for k, ((S, f0n), (Sw, fw)) in enumerate(zip(runs[0], want)):
        d = float(np.abs(S.astype(np.float64) - Sw.astype(np.float64)).max())
        print(f'extract_batch recording {k}: S within {d:.3g} of extract, {int((f0n > 0).sum())} of {f0n.shape[0]} frames voiced')
        assert S.dtype == np.float32 and f0n.dtype == np.float32 and S.shape == Sw.shape and f0n.shape == fw.shape
        assert np.array_equal(bits(f0n), bits(fw)), k                                       # extract's bits
        assert d <= MEL_BAR, (k, d)
    # the marker the reference's files carry, as make_spect_f0 asks for it
    prng = np.random.RandomState(226)
    want_kept = [features.extract(x, prng, 'M', mel_basis=g['mel_basis'], unvoiced=-1e10)[1] for x in xs]
    kept = features.extract_batch(xs, np.random.RandomState(226), 'M', mel_basis=g['mel_basis'], unvoiced=-1e10)
    for k, ((_, fk), fw) in enumerate(zip(kept, want_kept)):
        assert np.array_equal(bits(fk), bits(fw)), k
    assert sum(int((f != np.float32(UNVOICED)).sum()) for f in want_kept) >= 6              # voiced frames were compared
    assert any((f == np.float32(UNVOICED)).any() for f in want_kept)                        # and unvoiced ones
    S_d, f_d = features.extract_batch(xs[2:], np.random.RandomState(4), 'F')[0]             # the default basis, the other range
    assert S_d.shape == (20, 80) and np.isfinite(S_d).all() and f_d.shape == (20,)


def test_make_spect_f0_batched_writes_the_per_file_paths_files(tmp_path):
    from speechsplit_amd import features, vocoder
    from tests import pitch_ref as P
    root = tmp_path / 'wavs'
    lengths = {('p226', 'b.wav'): 2048, ('p226', 'a.wav'): 1500, ('p231', 'c.wav'): 3000}
    for (spk, name), n in lengths.items():
        os.makedirs(root / spk, exist_ok=True)
        vocoder.save_wav(str(root / spk / name), P.tone(110.0 if spk == 'p226' else 220.0, n))
    gen = {'p226': 'M', 'p231': 'F'}
    one = features.make_spect_f0(str(root), str(tmp_path / 'spmel'), str(tmp_path / 'raptf0'), gen)
    two = features.make_spect_f0(str(root), str(tmp_path / 'spmel2'), str(tmp_path / 'raptf02'), gen, max_rows=2)
    assert one == two == [('p226', 'a'), ('p226', 'b'), ('p231', 'c')]
    for (spk, name), n in lengths.items():
        S1, S2 = (np.load(tmp_path / d / spk / (name[:-4] + '.npy')) for d in ('spmel', 'spmel2'))
        f1, f2 = (np.load(tmp_path / d / spk / (name[:-4] + '.npy')) for d in ('raptf0', 'raptf02'))
        F = (n + 1 if n % 256 == 0 else n) // 256 + 1
        assert S2.dtype == np.float32 and S2.shape == S1.shape == (F, 80) and f2.dtype == np.float32 and f2.shape == (F,)
        assert np.array_equal(bits(f1), bits(f2)), (spk, name)                              # identical F0 files
        assert (f2 != np.float32(UNVOICED)).sum() >= 2
        assert float(np.abs(S1.astype(np.float64) - S2.astype(np.float64)).max()) <= MEL_BAR, (spk, name)
