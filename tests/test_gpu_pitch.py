"""The pitch tracker on the GPU (csrc/pitch.hip through the C ABI) against its float64 numpy restatement (pitch_ref.py, proven on wrong
stand-ins by test_pitch_ref_selftest.py) and against tones of known F0: pytest -m gpu.  Seconds in total.

Inputs: features.npz's u1_wav cut to 513 (3 frames), 1100 (5) and 2304 = 9 * 256 samples (10 frames, the last centred on the end), the whole
u1_wav (10241, 41 frames) and u0_wav (12345, 49 frames), and a composite (quiet noise, a glide, louder noise, the glide reversed, zeros) whose
glide frames have more than 19 qualifying peaks.  Ranges (50, 250): 257 lags; (100, 600): 135; (40, 1000): 385, on the 1100-sample input.

Conditions on the inputs (asserted on the CPU reference when the module is set up; not measurements): the best path's margin and the
candidate-rule gap are both >= 1e-6 for every (input, range), so no rounding difference can flip a decision and NO frame is left out of a
comparison.  Found when this was written: margin >= 1.06e-3, gap >= 4.86e-5.

Bounds.  ss_op_nccf: per input, 100 x the disagreement of the reference's own NCCF under two summation orders (numpy's reductions against
term-by-term sums) -- one factor of ten for a third order, one for fused multiply-adds -- capped at 1e-9; phi is O(1), rms the same bound,
relative.  ss_op_pitch_dp on the reference's own phi / rms, and ss_pitch_track end to end: the same voiced / unvoiced pattern, voiced values
within 1e-10 relative.  Measured (MI355X; the two-orders column on the host the tests were written on):

    input      range      two orders  bound      GPU phi    GPU rms (relative)
    513        50-250     6.12e-15    6.12e-13   1.44e-15   1.61e-16
    513        100-600    1.67e-15    1.67e-13   1.28e-15   0
    1100       50-250     4.09e-15    4.09e-13   1.44e-15   1.98e-16
    1100       100-600    1.55e-15    1.55e-13   1.55e-15   1.38e-16
    2304       50-250     1.25e-15    1.25e-13   1.44e-15   1.98e-16
    2304       100-600    1.55e-15    1.55e-13   1.28e-15   1.92e-16
    u1         50-250     4.59e-15    4.59e-13   1.67e-15   2.61e-16
    u1         100-600    1.92e-15    1.92e-13   1.67e-15   1.38e-16
    u0         50-250     1.95e-15    1.95e-13   1.33e-15   1.32e-16
    u0         100-600    3.07e-15    3.07e-13   1.39e-15   1.95e-16
    composite  50-250     1.22e-15    1.22e-13   1.44e-15   2.18e-16
    composite  100-600    1.33e-15    1.33e-13   1.11e-15   2.15e-16
    1100       40-1000    2.76e-15    2.76e-13   1.44e-15   1.9e-16

ss_op_pitch_dp on the reference's phi / rms: the reference's track to the bit on every input; ss_pitch_track end to end: the same pattern,
voiced values within 2.6e-15 relative (u0 in (50, 250); 7e-16 or less elsewhere).  Tones: 100 Hz 2.4e-4, 550 Hz 3.7e-4 (bound 2e-3).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import pitch_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
NAN = float('nan')
SCALE = 32768.0
M, W_, WIDE = (50.0, 250.0), (100.0, 600.0), (40.0, 1000.0)
CASES = [(name, rng) for name in ('513', '1100', '2304', 'u1', 'u0', 'composite') for rng in (M, W_)] + [('1100', WIDE)]
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
def ref(name, rng):
    """the reference's phi, rms and track of one (input, range), computed once and never modified; the input conditions are asserted here"""
    x = signals()[name]
    phi, rms = R.nccf(x, *rng, SCALE)
    f0 = R.dp(phi, rms, *rng)
    div = R.divergence(x, *rng, SCALE)
    margin, gap = R.margins(x, *rng, SCALE)
    assert margin >= MARGIN_FLOOR and gap >= MARGIN_FLOOR, (name, rng, margin, gap)
    for a in (phi, rms, f0):
        a.setflags(write=False)
    return dict(x=x, phi=phi, rms=rms, f0=f0, div=div, bound=min(1e-9, 100.0 * div), margin=margin, gap=gap)


def test_input_conditions():
    worst_margin = min(ref(n, r)['margin'] for n, r in CASES)
    worst_gap = min(ref(n, r)['gap'] for n, r in CASES)
    peaks = R.most_peaks(signals()['composite'], *M, SCALE)
    print(f'path margin >= {worst_margin:.3g}, candidate-rule gap >= {worst_gap:.3g}; composite: up to {peaks} qualifying peaks in a frame')
    assert worst_margin >= MARGIN_FLOOR and worst_gap >= MARGIN_FLOOR
    assert peaks > R.N_CANDS - 1                                        # the cap is exercised
    assert sum(int(R.voiced(ref(n, r)['f0']).sum()) for n, r in CASES) > 100 and any((~R.voiced(ref(n, r)['f0'])).any() for n, r in CASES)


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


def _scratch(lib, B, max_n, rng):
    nb = lib.ss_pitch_scratch_bytes(B, max_n, *rng)
    assert nb > 0, lib.ss_last_error()
    return torch.empty(nb, dtype=torch.uint8, device=DEV)


def gpu_nccf(lib, wav, n, rng):
    """wav [B, max_n] (tensor), n int32 [B] or None -> numpy phi [B, F, K], rms [B, F]"""
    B, max_n = wav.shape
    F, K = max_n // 256 + 1, R.lag_range(*rng)[2]
    phi = torch.full((B, F, K), NAN, dtype=torch.float64, device=DEV)
    rms = torch.full((B, F), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_nccf(_p(wav), _p(n), B, max_n, SCALE, *rng, _p(phi), _p(rms), _s()))
    return phi.cpu().numpy(), rms.cpu().numpy()


def gpu_dp(lib, phi, rms, n, max_n, rng):
    """phi [B, F, K], rms [B, F] (tensors) -> numpy f0 [B, F]"""
    B, F = rms.shape
    f0 = torch.full((B, F), NAN, dtype=torch.float64, device=DEV)
    sc = _scratch(lib, B, max_n, rng)
    _check(lib, lib.ss_op_pitch_dp(_p(phi), _p(rms), _p(n), B, max_n, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    return f0.cpu().numpy()


def gpu_track(lib, wav, n, rng):
    """wav [B, max_n] (tensor) -> numpy f0 [B, F]"""
    B, max_n = wav.shape
    f0 = torch.full((B, max_n // 256 + 1), NAN, dtype=torch.float64, device=DEV)
    sc = _scratch(lib, B, max_n, rng)
    _check(lib, lib.ss_pitch_track(_p(wav), _p(n), B, max_n, SCALE, *rng, _p(f0), _p(sc), sc.numel(), _s()))
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


# ---------------------------------------------------------------------------------------------- the two halves alone, and end to end
@pytest.mark.parametrize('name,rng', CASES, ids=IDS)
def test_nccf_matches_the_reference(lib, name, rng):
    r = ref(name, rng)
    phi, rms = gpu_nccf(lib, _dev(r['x'])[None], None, rng)
    assert phi.shape[1:] == r['phi'].shape and np.isfinite(phi).all() and np.isfinite(rms).all()
    dphi = float(np.abs(phi[0] - r['phi']).max())
    drms = float((np.abs(rms[0] - r['rms']) / r['rms']).max())
    print(f'ss_op_nccf {name} {rng}: two orders {r["div"]:.3g}, bound {r["bound"]:.3g}, phi {dphi:.3g}, rms {drms:.3g} (relative)')
    assert dphi <= r['bound'] and drms <= r['bound']


@pytest.mark.parametrize('name,rng', CASES, ids=IDS)
def test_dp_on_the_references_own_nccf(lib, name, rng):
    r = ref(name, rng)
    got = gpu_dp(lib, _dev(r['phi'])[None], _dev(r['rms'])[None], None, r['x'].shape[0], rng)[0]
    worst = assert_same_track(got, r['f0'], (name, rng))
    print(f'ss_op_pitch_dp {name} {rng}: {int(R.voiced(got).sum())} of {got.shape[0]} frames voiced, values within {worst:.3g}')


@pytest.mark.parametrize('name,rng', CASES, ids=IDS)
def test_track_end_to_end(lib, name, rng):
    r = ref(name, rng)
    got = gpu_track(lib, _dev(r['x'])[None], None, rng)[0]
    worst = assert_same_track(got, r['f0'], (name, rng))
    print(f'ss_pitch_track {name} {rng}: {int(R.voiced(got).sum())} of {got.shape[0]} frames voiced, values within {worst:.3g}')


@pytest.mark.parametrize('case', ['tie', 'cap', 'doubling'])
def test_dp_on_crafted_lattices(lib, case):
    """decisions the waveforms do not force (pitch_ref.tie_case / cap_case / doubling_case; the self-test shows that the matching wrong
    variant changes each): two paths whose costs are equal to the bit -- the lowest state wins; a frame whose cheapest state is its twentieth
    candidate -- the cap drops it; an octave jump that only the doubling term makes worthwhile"""
    phi, rms = {'tie': lambda: R.tie_case(*M, frames=3)[:2], 'cap': R.cap_case, 'doubling': R.doubling_case}[case]()
    if case != 'tie':
        assert min(R.margins_phi(phi, rms, *M)) >= MARGIN_FLOOR
    got = gpu_dp(lib, _dev(phi)[None], _dev(rms)[None], None, 513, M)[0]
    assert_same_track(got, R.dp(phi, rms, *M), case)
    assert R.voiced(got).all()


@pytest.mark.parametrize('f0_true,rng', [(100.0, M), (550.0, W_)])
def test_harmonic_tones_come_out_at_their_frequency(lib, f0_true, rng):
    """ground truth that neither implementation defines: frames 2 .. F - 3 voiced, |exp(f0) / f0_true - 1| <= 2e-3.
    Measured: 100 Hz 2.38e-4, 550 Hz 3.74e-4, the reference's own figures"""
    got = gpu_track(lib, _dev(R.tone(f0_true))[None], None, rng)[0]
    inner = got[2:-2]
    assert got.shape == (63,) and R.voiced(inner).all()
    err = float(np.abs(np.exp(inner) / f0_true - 1.0).max())
    print(f'tone {f0_true} Hz in {rng}: worst relative error {err:.3g}')
    assert err <= 2e-3


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
    assert np.array_equal(got.view(np.int64), gpu_track(lib, _ragged(0.0)[0], n, M).view(np.int64))
    phi, rms = gpu_nccf(lib, wav, n, M)
    for b, (name, cnt) in enumerate(RAGGED):
        F = cnt // 256 + 1
        x = _dev(signals()[name])[None]
        assert np.array_equal(got[b, :F], gpu_track(lib, x, None, M)[0]), name               # bit for bit
        assert np.all(got[b, F:] == R.UNVOICED), name
        assert_same_track(got[b, :F], ref(name, M)['f0'], name)
        p1, r1 = gpu_nccf(lib, x, None, M)
        assert np.array_equal(phi[b, :F], p1[0]) and np.array_equal(rms[b, :F], r1[0]), name
        assert not phi[b, F:].any() and not rms[b, F:].any() and not np.signbit(phi[b, F:]).any(), name
    # the hook never reads phi / rms behind a row's own frames
    pn, rn = phi.copy(), rms.copy()
    for b, (_, cnt) in enumerate(RAGGED):
        pn[b, cnt // 256 + 1:] = NAN
        rn[b, cnt // 256 + 1:] = NAN
    assert np.array_equal(gpu_dp(lib, _dev(pn), _dev(rn), n, 12345, M), got)


def test_lengths_outside_the_contract_spoil_their_row_only(lib):
    """every kernel clamps n[b] into [513, max_n]: rows 1 and 2 come out as they would alone whatever rows 0 and 3 claim"""
    x = signals()['2304']
    got = gpu_track(lib, _dev(np.stack([x] * 4)), _ints([-3, 2304, 1100, 1 << 30]), M)
    full = gpu_track(lib, _dev(x)[None], None, M)[0]
    assert np.array_equal(got[1], full) and np.array_equal(got[3], full)                     # above max_n: max_n
    assert np.array_equal(got[2, :5], gpu_track(lib, _dev(x[:1100])[None], None, M)[0]) and np.all(got[2, 5:] == R.UNVOICED)
    assert np.array_equal(got[0, :3], gpu_track(lib, _dev(x[:513])[None], None, M)[0]) and np.all(got[0, 3:] == R.UNVOICED)   # below 513: 513


def test_two_runs_give_the_same_bits(lib):
    wav, n = _ragged(NAN)
    a, b = gpu_track(lib, wav, n, W_), gpu_track(lib, wav, n, W_)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    (pa, ra), (pb, rb) = gpu_nccf(lib, wav, n, W_), gpu_nccf(lib, wav, n, W_)
    assert np.array_equal(pa.view(np.int64), pb.view(np.int64)) and np.array_equal(ra.view(np.int64), rb.view(np.int64))


# ---------------------------------------------------------------------------------------------- containment
CB, CN, CLEN = 3, 2304, [2304, 513, 1300]
CF, CK = CN // 256 + 1, 257


def _guarded_wav():
    wav = np.full((CB, CN), NAN)
    for b, n in enumerate(CLEN):
        wav[b, :n] = signals()['2304'][:n]
    return G.inp(wav, DEV, name='wav'), G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')


def _guarded_scratch(lib):
    g = G.out((lib.ss_pitch_scratch_bytes(CB, CN, *M) // 8,), DEV, dtype=torch.float64, offset=32, fill=0.0, name='scratch')
    assert g.t.data_ptr() % 256 == 0
    return g


@functools.lru_cache(maxsize=None)
def _contained_refs():
    out = []
    for n in CLEN:
        phi, rms = R.nccf(signals()['2304'][:n], *M, SCALE)
        out.append((phi, rms, R.dp(phi, rms, *M)))
    return out


def test_containment_nccf(lib):
    gw, gn = _guarded_wav()
    gp, gr = G.out((CB, CF, CK), DEV, dtype=torch.float64, name='phi'), G.out((CB, CF), DEV, dtype=torch.float64, name='rms')
    _check(lib, lib.ss_op_nccf(_p(gw.t), _p(gn.t), CB, CN, SCALE, *M, _p(gp.t), _p(gr.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gw, gn, gp, gr])
    phi, rms = gp.t.cpu().numpy(), gr.t.cpu().numpy()
    for b, (n, (rphi, rrms, _)) in enumerate(zip(CLEN, _contained_refs())):
        F = n // 256 + 1
        assert np.abs(phi[b, :F] - rphi).max() <= 1e-9 and np.abs(rms[b, :F] / rrms - 1.0).max() <= 1e-9
        assert not phi[b, F:].any() and not rms[b, F:].any()


def test_containment_pitch_dp(lib):
    phi, rms = np.full((CB, CF, CK), NAN), np.full((CB, CF), NAN)
    for b, (n, (rphi, rrms, _)) in enumerate(zip(CLEN, _contained_refs())):
        phi[b, :n // 256 + 1], rms[b, :n // 256 + 1] = rphi, rrms
    gp, gr = G.inp(phi, DEV, name='phi'), G.inp(rms, DEV, name='rms')
    gn = G.inp(torch.tensor(CLEN, dtype=torch.int32), DEV, name='n')
    gf, gsc = G.out((CB, CF), DEV, dtype=torch.float64, name='f0'), _guarded_scratch(lib)
    _check(lib, lib.ss_op_pitch_dp(_p(gp.t), _p(gr.t), _p(gn.t), CB, CN, *M, _p(gf.t), _p(gsc.t), gsc.t.numel() * 8, _s()))
    torch.cuda.synchronize()
    G.check_all([gp, gr, gn, gf, gsc])
    got = gf.t.cpu().numpy()
    for b, (n, (_, _, rf0)) in enumerate(zip(CLEN, _contained_refs())):
        assert_same_track(got[b, :n // 256 + 1], rf0, b)
        assert np.all(got[b, n // 256 + 1:] == R.UNVOICED)


def test_containment_pitch_track(lib):
    gw, gn = _guarded_wav()
    gf, gsc = G.out((CB, CF), DEV, dtype=torch.float64, name='f0'), _guarded_scratch(lib)
    _check(lib, lib.ss_pitch_track(_p(gw.t), _p(gn.t), CB, CN, SCALE, *M, _p(gf.t), _p(gsc.t), gsc.t.numel() * 8, _s()))
    torch.cuda.synchronize()
    G.check_all([gw, gn, gf, gsc])
    got = gf.t.cpu().numpy()
    for b, (n, (_, _, rf0)) in enumerate(zip(CLEN, _contained_refs())):
        assert_same_track(got[b, :n // 256 + 1], rf0, b)
        assert np.all(got[b, n // 256 + 1:] == R.UNVOICED)


# ---------------------------------------------------------------------------------------------- the Python layer
def test_pitch_track_rounds_through_float32_and_ignores_max_rows():
    from speechsplit_amd import features
    names = ['2304', '513', 'u1', '1100']
    wavs = [signals()[k] for k in names]
    runs = [features.pitch_track(wavs, *M, max_rows=r) for r in (1, 3, 16)]
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))
    for k, w, got in zip(names, wavs, runs[0]):
        assert got.dtype == np.float64 and got.shape == (w.shape[0] // 256 + 1,)
        assert_same_track(got, R.track(w.astype(np.float32).astype(np.float64), *M), k)
    one = features.pitch_track(wavs[3], *M)
    assert isinstance(one, np.ndarray) and np.array_equal(one, runs[0][3])


def test_extract_is_the_references_loop_body():
    """S is compared through the fixture's own mel_basis: features.npz was generated with a synthetic basis, not with the filter bank that
    `mel_filter_bank` restates, so extract's default basis cannot reproduce u1_S; the default is exercised for shape and range."""
    from speechsplit_amd import features
    f = np.load(os.path.join(GOLD, 'features.npz'))
    S, f0n = features.extract(f['u1_x'], np.random.RandomState(231), 'M', mel_basis=f['mel_basis'])
    assert S.dtype == np.float32 and S.shape == (41, 80) and float(np.abs(S - f['u1_S']).max()) <= 1e-6
    assert f0n.dtype == np.float32 and f0n.shape == (41,) and f0n.min() >= 0.0 and f0n.max() <= 1.0
    track = features.pitch_track(f['u1_wav'], *M)
    assert np.all(f0n[~R.voiced(track)] == 0.0) and R.voiced(track).sum() >= 2 and (f0n[R.voiced(track)] > 0.0).any()
    # the normalisation of the reference on the same track (utils.py:35-42)
    v = R.voiced(track)
    want = np.where(v, (np.clip((track - track[v].mean()) / track[v].std() / 4.0, -1.0, 1.0) + 1.0) / 2.0, 0.0)
    assert np.abs(f0n - want).max() <= 1e-6
    kept = features.extract(f['u1_x'], np.random.RandomState(231), 'M', mel_basis=f['mel_basis'], unvoiced=-1e10)[1]
    assert np.array_equal(kept[v], f0n[v]) and np.all(kept[~v] == np.float32(-1e10))       # what make_spect_f0 writes
    S2, f0n2 = features.extract(f['u1_x'], np.random.RandomState(231), 'M')
    assert S2.shape == (41, 80) and S2.dtype == np.float32 and np.isfinite(S2).all() and np.array_equal(f0n2, f0n)


def test_make_spect_f0_writes_the_references_files(tmp_path):
    from speechsplit_amd import features, vocoder
    root = tmp_path / 'wavs'
    lengths = {('p226', 'b.wav'): 2048, ('p226', 'a.wav'): 1500, ('p231', 'c.wav'): 3000}
    for (spk, name), n in lengths.items():
        os.makedirs(root / spk, exist_ok=True)
        vocoder.save_wav(str(root / spk / name), R.tone(110.0 if spk == 'p226' else 220.0, n))
    done = features.make_spect_f0(str(root), str(tmp_path / 'spmel'), str(tmp_path / 'raptf0'), {'p226': 'M', 'p231': 'F'})
    assert done == [('p226', 'a'), ('p226', 'b'), ('p231', 'c')]
    for (spk, name), n in lengths.items():
        S = np.load(tmp_path / 'spmel' / spk / (name[:-4] + '.npy'))
        f0 = np.load(tmp_path / 'raptf0' / spk / (name[:-4] + '.npy'))
        F = (n + 1 if n % 256 == 0 else n) // 256 + 1                                          # make_spect_f0.py:52-53
        assert S.dtype == np.float32 and S.shape == (F, 80) and f0.dtype == np.float32 and f0.shape == (F,) and len(S) == len(f0)
        v = f0 != np.float32(R.UNVOICED)                                                        # the reference's files keep its marker
        assert v.sum() >= 2 and f0[v].min() >= 0.0 and f0[v].max() <= 1.0
    with pytest.raises(ValueError, match="'M' or 'F'"):
        features.make_spect_f0(str(root), str(tmp_path / 'x'), str(tmp_path / 'y'), {'p226': 'M', 'p231': '?'})
