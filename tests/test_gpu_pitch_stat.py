"""The pitch tracker's spectral-stationarity term on the GPU (csrc/pitch.hip: stat_kernel, dp_kernel<true>, through the C ABI) against its
float64 numpy restatement (pitch_stat_ref.py, proven on wrong stand-ins by test_pitch_stat_ref_selftest.py): pytest -m gpu.  The largest
input has 58 frames: seconds in total.

Inputs: test_gpu_pitch.py's six signals -- features.npz's u1_wav cut to 513 (3 frames: the windows of its first and last frame hang over
both ends), 1100 (5) and 2304 samples (10), the whole u1_wav (41) and u0_wav (49), and the composite (58) -- in (50, 250) and (100, 600).

Conditions on the inputs (asserted on the CPU reference when a case is set up; not measurements): with the term on, the best path's margin
(pitch_stat_ref.margins_stat) and the candidate-rule gap are >= 1e-6 for every (input, range), so no rounding difference can flip a decision
and NO frame is left out of a comparison.  Found when this was written: margin >= 1.06e-3 (u0 in (50, 250)).

Bounds.  ss_op_pitch_stationarity: per input, 100 x the disagreement of the reference's own S under two summation orders (numpy's reductions
against term-by-term sums) -- one factor of ten for a third order, one for fused multiply-adds -- capped at 1e-9; S is O(1), the bound is
absolute.  ss_op_pitch_dp_stat on the reference's own phi / rms / S: the reference's track to the bit.  ss_pitch_track_stat end to end: the
same voiced / unvoiced pattern, voiced values within 1e-10 relative (test_gpu_pitch.py's VALUE_TOL).

Measured (MI355X; the two-orders column on the host the tests were written on):

    input      two orders  bound      GPU S
    513        7.42e-14    7.42e-12   2.38e-14
    1100       2.67e-13    2.67e-11   1.61e-13
    2304       9.25e-13    9.25e-11   1.78e-13
    u1         9.55e-13    9.55e-11   6.17e-13
    u0         1.56e-12    1.56e-10   6.88e-13
    composite  2.19e-12    2.19e-10   2.86e-12

ss_op_pitch_dp_stat: the reference's track to the bit on the twelve cases; ss_pitch_track_stat: the same pattern, voiced values within
2.6e-15 relative (u0 in (50, 250); 7e-16 or less elsewhere).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import pitch_ref as R
from tests import pitch_stat_ref as Q

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
NAN = float('nan')
SCALE = 32768.0
M, W_ = (50.0, 250.0), (100.0, 600.0)
NAMES = ('513', '1100', '2304', 'u1', 'u0', 'composite')
CASES = [(name, rng) for name in NAMES for rng in (M, W_)]
IDS = [f'{name}-{int(lo)}-{int(hi)}' for name, (lo, hi) in CASES]
MARGIN_FLOOR = 1e-6
VALUE_TOL = 1e-10


@functools.lru_cache(maxsize=None)
def signals():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    u1 = np.ascontiguousarray(f['u1_wav'], dtype=np.float64)
    return {'513': u1[:513].copy(), '1100': u1[:1100].copy(), '2304': u1[:2304].copy(), 'u1': u1,
            'u0': np.ascontiguousarray(f['u0_wav'], dtype=np.float64), 'composite': R.composite()}


@functools.lru_cache(maxsize=None)
def ref_s(name):
    """the reference's S of one input and its bound, computed once and never modified"""
    x = signals()[name]
    S = Q.stationarity(x, None, SCALE)
    div = Q.divergence_stat(x, SCALE)
    S.setflags(write=False)
    return dict(x=x, S=S, div=div, bound=min(1e-9, 100.0 * div))


@functools.lru_cache(maxsize=None)
def ref(name, rng):
    """the reference's phi, rms and track with the term on; the input conditions are asserted here"""
    r = ref_s(name)
    phi, rms = R.nccf(r['x'], *rng, SCALE)
    f0 = Q.dp_stat(phi, rms, r['S'], *rng)
    margin, gap = Q.margins_stat(phi, rms, r['S'], *rng), R.margins_phi(phi, rms, *rng)[1]
    assert margin >= MARGIN_FLOOR and gap >= MARGIN_FLOOR, (name, rng, margin, gap)
    for a in (phi, rms, f0):
        a.setflags(write=False)
    return dict(x=r['x'], S=r['S'], phi=phi, rms=rms, f0=f0, margin=margin)


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


def _scratch(lib, B, max_n, rng, stat=False):
    nb = (lib.ss_pitch_stat_scratch_bytes if stat else lib.ss_pitch_scratch_bytes)(B, max_n, *rng)
    assert nb > 0, lib.ss_last_error()
    return torch.empty(nb, dtype=torch.uint8, device=DEV)


def gpu_stat(lib, wav, n):
    """wav [B, max_n] (tensor), n int32 [B] or None -> numpy S [B, F]"""
    B, max_n = wav.shape
    S = torch.full((B, max_n // 256 + 1), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_pitch_stationarity(_p(wav), _p(n), B, max_n, SCALE, _p(S), _s()))
    return S.cpu().numpy()


def gpu_dp_stat(lib, phi, rms, S, n, max_n, rng):
    """phi [B, F, K], rms, S [B, F] (tensors) -> numpy f0 [B, F]"""
    B, F = rms.shape
    f0 = torch.full((B, F), NAN, dtype=torch.float64, device=DEV)
    sc = _scratch(lib, B, max_n, rng)
    _check(lib, lib.ss_op_pitch_dp_stat(_p(phi), _p(rms), _p(S), _p(n), B, max_n, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    return f0.cpu().numpy()


def gpu_dp(lib, phi, rms, n, max_n, rng):
    B, F = rms.shape
    f0 = torch.full((B, F), NAN, dtype=torch.float64, device=DEV)
    sc = _scratch(lib, B, max_n, rng)
    _check(lib, lib.ss_op_pitch_dp(_p(phi), _p(rms), _p(n), B, max_n, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    return f0.cpu().numpy()


def gpu_track(lib, wav, n, rng, stat=True):
    """wav [B, max_n] (tensor) -> numpy f0 [B, F]"""
    B, max_n = wav.shape
    f0 = torch.full((B, max_n // 256 + 1), NAN, dtype=torch.float64, device=DEV)
    sc = _scratch(lib, B, max_n, rng, stat)
    fn = lib.ss_pitch_track_stat if stat else lib.ss_pitch_track
    _check(lib, fn(_p(wav), _p(n), B, max_n, SCALE, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    return f0.cpu().numpy()


def assert_same_track(got, want, what):
    """the voiced / unvoiced pattern exactly, voiced values within 1e-10 relative; returns the worst relative difference"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    v = R.voiced(want)
    assert np.array_equal(R.voiced(got), v), (what, np.nonzero(R.voiced(got) != v)[0])
    assert np.all(got[~v] == R.UNVOICED)
    worst = float(np.abs(got[v] / want[v] - 1.0).max()) if v.any() else 0.0
    assert worst <= VALUE_TOL, (what, worst)
    return worst


# ---------------------------------------------------------------------------------------------- the halves alone, and end to end
@pytest.mark.parametrize('name', NAMES)
def test_stationarity_matches_the_reference(lib, name):
    r = ref_s(name)
    S = gpu_stat(lib, _dev(r['x'])[None], None)[0]
    assert S.shape == r['S'].shape and np.isfinite(S).all()
    assert S[0] == 0.0 and not np.signbit(S[0]) and np.all(S[1:] > 0.0) and np.all(S <= 1.0)
    worst = float(np.abs(S - r['S']).max())
    print(f'ss_op_pitch_stationarity {name}: two orders {r["div"]:.3g}, bound {r["bound"]:.3g}, S {worst:.3g}; S spans '
          f'{S[1:].min():.3g} .. {S[1:].max():.3g}')
    assert worst <= r['bound']


def test_silence_is_stationary_to_the_bit(lib):
    """r_0 == 0 in both windows: rho = a = (1, 0, ..), E = 1, d = 1, and the cap cuts 0.2 / (1 - 0.8) = 1 + 2^-52 off"""
    S = gpu_stat(lib, torch.zeros(1, 1100, dtype=torch.float64, device=DEV), None)[0]
    assert np.array_equal(S, [0.0, 1.0, 1.0, 1.0, 1.0])


@pytest.mark.parametrize('name,rng', CASES, ids=IDS)
def test_dp_stat_on_the_references_own_operands(lib, name, rng):
    r = ref(name, rng)
    got = gpu_dp_stat(lib, _dev(r['phi'])[None], _dev(r['rms'])[None], _dev(r['S'])[None], None, r['x'].shape[0], rng)[0]
    assert np.array_equal(got.view(np.int64), r['f0'].view(np.int64)), (name, rng, np.nonzero(got != r['f0'])[0])
    print(f'ss_op_pitch_dp_stat {name} {rng}: {int(R.voiced(got).sum())} of {got.shape[0]} frames voiced, margin {r["margin"]:.3g}')


@pytest.mark.parametrize('name,rng', CASES, ids=IDS)
def test_dp_stat_with_a_zero_track_is_dp(lib, name, rng):
    r = ref(name, rng)
    phi, rms = _dev(r['phi'])[None], _dev(r['rms'])[None]
    a = gpu_dp_stat(lib, phi, rms, torch.zeros_like(rms), None, r['x'].shape[0], rng)
    b = gpu_dp(lib, phi, rms, None, r['x'].shape[0], rng)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize('name,rng', CASES, ids=IDS)
def test_track_stat_end_to_end(lib, name, rng):
    r = ref(name, rng)
    got = gpu_track(lib, _dev(r['x'])[None], None, rng)[0]
    worst = assert_same_track(got, r['f0'], (name, rng))
    print(f'ss_pitch_track_stat {name} {rng}: {int(R.voiced(got).sum())} of {got.shape[0]} frames voiced, values within {worst:.3g}')


@pytest.mark.parametrize('key', list(Q.STAT_CASE_TRACKS))
def test_dp_stat_on_the_crafted_lattice(lib, key):
    """the test that shows the term doing what it is for (pitch_stat_ref.stat_case): a two-frame dip inside strong frames is cut out
    without the term (margin 5.2e-2), stays voiced where the spectrum stands still (S = 1: 0.95), is cut out again where the spectrum
    changes at its edges (S = 0.05 there: 2.3e-3), and stays voiced at S = 0.08 only if the term enters both transitions (2.8e-2)"""
    phi, rms = Q.stat_case()
    S = Q.STAT_CASE_TRACKS[key]
    assert Q.margins_stat(phi, rms, S, *M) >= MARGIN_FLOOR
    want = Q.dp_stat(phi, rms, S, *M)
    dip = np.array([1, 1, 1, 0, 0, 1, 1, 1], bool)
    assert np.array_equal(R.voiced(want), {'zeros': dip, 'ones': np.ones(8, bool), 'edges': dip, 'low': np.ones(8, bool)}[key])
    got = gpu_dp_stat(lib, _dev(phi)[None], _dev(rms)[None], _dev(S)[None], None, 7 * 256, M)[0]
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (key, got)


# ---------------------------------------------------------------------------------------------- ragged batches, determinism
RAGGED = [('2304', 2304), ('513', 513), ('u0', 12345), ('1100', 1100)]


def _ragged(fill):
    wav = np.full((len(RAGGED), 12345), fill)
    for b, (name, n) in enumerate(RAGGED):
        wav[b, :n] = signals()[name]
    return _dev(wav), _ints([n for _, n in RAGGED])


def test_ragged_batch_rows_are_the_utterances_alone(lib):
    wav, n = _ragged(NAN)                                                # NaN behind every row's end
    got = gpu_track(lib, wav, n, M)
    S = gpu_stat(lib, wav, n)
    assert np.array_equal(got.view(np.int64), gpu_track(lib, _ragged(0.0)[0], n, M).view(np.int64))
    phi, rms = np.zeros((4, 49, 257)), np.zeros((4, 49))
    for b, (name, cnt) in enumerate(RAGGED):
        F = cnt // 256 + 1
        x = _dev(signals()[name])[None]
        assert np.array_equal(got[b, :F], gpu_track(lib, x, None, M)[0]), name               # bit for bit
        assert np.all(got[b, F:] == R.UNVOICED), name
        assert_same_track(got[b, :F], ref(name, M)['f0'], name)
        assert np.array_equal(S[b, :F], gpu_stat(lib, x, None)[0]), name
        assert not S[b, F:].any() and not np.signbit(S[b, F:]).any(), name                   # exact zeros behind the row's frames
        phi[b, :F], rms[b, :F] = ref(name, M)['phi'], ref(name, M)['rms']
    # the hook never reads phi / rms / stat behind a row's own frames
    pn, rn, sn = phi.copy(), rms.copy(), S.copy()
    for b, (_, cnt) in enumerate(RAGGED):
        pn[b, cnt // 256 + 1:] = NAN
        rn[b, cnt // 256 + 1:] = NAN
        sn[b, cnt // 256 + 1:] = NAN
    a = gpu_dp_stat(lib, _dev(pn), _dev(rn), _dev(sn), n, 12345, M)
    assert np.array_equal(a.view(np.int64), gpu_dp_stat(lib, _dev(phi), _dev(rms), _dev(S), n, 12345, M).view(np.int64))
    for b, (name, cnt) in enumerate(RAGGED):
        assert_same_track(a[b, :cnt // 256 + 1], ref(name, M)['f0'], name)
        assert np.all(a[b, cnt // 256 + 1:] == R.UNVOICED)


def test_lengths_outside_the_contract_spoil_their_row_only(lib):
    """every kernel clamps n[b] into [513, max_n]: rows 1 and 2 come out as they would alone whatever rows 0 and 3 claim"""
    x = signals()['2304']
    wav, n = _dev(np.stack([x] * 4)), _ints([-3, 2304, 1100, 1 << 30])
    got, S = gpu_track(lib, wav, n, M), gpu_stat(lib, wav, n)
    full, sfull = gpu_track(lib, _dev(x)[None], None, M)[0], gpu_stat(lib, _dev(x)[None], None)[0]
    assert np.array_equal(got[1], full) and np.array_equal(got[3], full)                     # above max_n: max_n
    assert np.array_equal(S[1], sfull) and np.array_equal(S[3], sfull)
    assert np.array_equal(got[2, :5], gpu_track(lib, _dev(x[:1100])[None], None, M)[0]) and np.all(got[2, 5:] == R.UNVOICED)
    assert np.array_equal(S[2, :5], gpu_stat(lib, _dev(x[:1100])[None], None)[0]) and not S[2, 5:].any()
    assert np.array_equal(got[0, :3], gpu_track(lib, _dev(x[:513])[None], None, M)[0]) and np.all(got[0, 3:] == R.UNVOICED)   # below 513: 513
    assert np.array_equal(S[0, :3], gpu_stat(lib, _dev(x[:513])[None], None)[0]) and not S[0, 3:].any()


def test_two_runs_give_the_same_bits(lib):
    wav, n = _ragged(NAN)
    a, b = gpu_track(lib, wav, n, W_), gpu_track(lib, wav, n, W_)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    sa, sb = gpu_stat(lib, wav, n), gpu_stat(lib, wav, n)
    assert np.array_equal(sa.view(np.int64), sb.view(np.int64))


# ---------------------------------------------------------------------------------------------- containment
CB, CN, CLEN = 3, 2304, [2304, 513, 1300]
CF, CK = CN // 256 + 1, 257


def _guarded_wav():
    wav = np.full((CB, CN), NAN)
    for b, n in enumerate(CLEN):
        wav[b, :n] = signals()['2304'][:n]
    return G.inp(wav, DEV, name='wav'), G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')


def _guarded_scratch(lib, stat):
    nb = (lib.ss_pitch_stat_scratch_bytes if stat else lib.ss_pitch_scratch_bytes)(CB, CN, *M)
    g = G.out((nb // 8,), DEV, dtype=torch.float64, offset=32, fill=0.0, name='scratch')
    assert g.t.data_ptr() % 256 == 0
    return g


@functools.lru_cache(maxsize=None)
def _contained_refs():
    out = []
    for n in CLEN:
        x = signals()['2304'][:n]
        phi, rms = R.nccf(x, *M, SCALE)
        S = Q.stationarity(x, None, SCALE)
        assert Q.margins_stat(phi, rms, S, *M) >= MARGIN_FLOOR
        out.append((phi, rms, S, Q.dp_stat(phi, rms, S, *M)))
    return out


def test_containment_stationarity(lib):
    gw, gn = _guarded_wav()
    gs = G.out((CB, CF), DEV, dtype=torch.float64, name='stat')
    _check(lib, lib.ss_op_pitch_stationarity(_p(gw.t), _p(gn.t), CB, CN, SCALE, _p(gs.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gw, gn, gs])
    S = gs.t.cpu().numpy()
    for b, (n, (_, _, rS, _)) in enumerate(zip(CLEN, _contained_refs())):
        F = n // 256 + 1
        assert np.abs(S[b, :F] - rS).max() <= 1e-9 and not S[b, F:].any()


def test_containment_pitch_dp_stat(lib):
    phi, rms, S = np.full((CB, CF, CK), NAN), np.full((CB, CF), NAN), np.full((CB, CF), NAN)
    for b, (n, (rphi, rrms, rS, _)) in enumerate(zip(CLEN, _contained_refs())):
        phi[b, :n // 256 + 1], rms[b, :n // 256 + 1], S[b, :n // 256 + 1] = rphi, rrms, rS
    gp, gr, gs = G.inp(phi, DEV, name='phi'), G.inp(rms, DEV, name='rms'), G.inp(S, DEV, name='stat')
    gn = G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')
    gf, gsc = G.out((CB, CF), DEV, dtype=torch.float64, name='f0'), _guarded_scratch(lib, False)
    _check(lib, lib.ss_op_pitch_dp_stat(_p(gp.t), _p(gr.t), _p(gs.t), _p(gn.t), CB, CN, *M, _p(gf.t), _p(gsc.t), gsc.t.numel() * 8, _s()))
    torch.cuda.synchronize()
    G.check_all([gp, gr, gs, gn, gf, gsc])
    got = gf.t.cpu().numpy()
    for b, (n, (_, _, _, rf0)) in enumerate(zip(CLEN, _contained_refs())):
        assert_same_track(got[b, :n // 256 + 1], rf0, b)
        assert np.all(got[b, n // 256 + 1:] == R.UNVOICED)


def test_containment_pitch_track_stat(lib):
    gw, gn = _guarded_wav()
    gf, gsc = G.out((CB, CF), DEV, dtype=torch.float64, name='f0'), _guarded_scratch(lib, True)
    _check(lib, lib.ss_pitch_track_stat(_p(gw.t), _p(gn.t), CB, CN, SCALE, *M, _p(gf.t), _p(gsc.t), gsc.t.numel() * 8, _s()))
    torch.cuda.synchronize()
    G.check_all([gw, gn, gf, gsc])
    got = gf.t.cpu().numpy()
    for b, (n, (_, _, _, rf0)) in enumerate(zip(CLEN, _contained_refs())):
        assert_same_track(got[b, :n // 256 + 1], rf0, b)
        assert np.all(got[b, n // 256 + 1:] == R.UNVOICED)


# ---------------------------------------------------------------------------------------------- the Python layer
def test_pitch_track_off_is_ss_pitch_track_to_the_bit_and_on_is_the_reference(lib):
    from speechsplit_amd import features
    names = ['2304', '513', 'u1', '1100']
    wavs = [signals()[k] for k in names]
    off = features.pitch_track(wavs, *M, stationarity=False)
    on = features.pitch_track(wavs, *M, max_rows=3, stationarity=True)
    for k, w, a, b, c in zip(names, wavs, off, on, features.pitch_track(wavs, *M)):
        w32 = w.astype(np.float32).astype(np.float64)
        assert np.array_equal(a.view(np.int64), gpu_track(lib, _dev(w32)[None], None, M, stat=False)[0].view(np.int64)), k
        assert np.array_equal(a.view(np.int64), c.view(np.int64)), k
        assert np.array_equal(b.view(np.int64), gpu_track(lib, _dev(w32)[None], None, M, stat=True)[0].view(np.int64)), k
        assert_same_track(b, Q.track_stat(w32, *M), k)


def test_extract_carries_the_new_track_through_normalisation():
    """`extract` itself keeps its pinned argument list; `extract_opt` is `extract` with the option, and `extract_batch_sr` takes it too"""
    from speechsplit_amd import features
    f = np.load(os.path.join(GOLD, 'features.npz'))
    S0, base = features.extract(f['u1_x'], np.random.RandomState(231), 'M', mel_basis=f['mel_basis'])
    S1, off = features.extract_opt(f['u1_x'], np.random.RandomState(231), 'M', mel_basis=f['mel_basis'])
    assert np.array_equal(S0, S1) and np.array_equal(base, off)                              # off: extract, to the bit
    S2, f0n = features.extract_opt(f['u1_x'], np.random.RandomState(231), 'M', mel_basis=f['mel_basis'], stationarity=True)
    assert np.array_equal(S2, S0) and f0n.dtype == np.float32 and f0n.shape == (41,)
    track = features.pitch_track(f['u1_wav'], *M, stationarity=True)
    v = R.voiced(track)
    want = np.where(v, (np.clip((track - track[v].mean()) / track[v].std() / 4.0, -1.0, 1.0) + 1.0) / 2.0, 0.0)
    assert v.sum() >= 2 and np.abs(f0n - want).max() <= 1e-6 and np.all(f0n[~v] == 0.0)
    (S3, f0b), = features.extract_batch_sr([f['u1_x']], 16000, np.random.RandomState(231), 'M', mel_basis=f['mel_basis'], stationarity=True)
    assert np.array_equal(f0b, f0n) and np.abs(S3 - S0).max() <= 1e-6
