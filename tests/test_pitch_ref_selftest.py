"""The numpy restatement of the pitch tracker (pitch_ref.py) checked against itself, against tones of known F0, and on wrong stand-ins.
CPU only.

Measured when this was written.  Tones (worst |exp(f0) / f0_true - 1| over frames 2 .. F - 3, all of them voiced): 60 Hz 6.2e-5, 100 Hz
2.4e-4, 240 Hz 2.9e-4 in (50, 250); 120 Hz 1.9e-4, 550 Hz 3.7e-4 in (100, 600) -- the bound is 2e-3.  0.1 x randn(8192): 0 voiced frames of
33 (at most 2 allowed).  The reference's two summation orders differ by at most 1.1e-14 in phi on the inputs used here.  Every wrong
stand-in moves phi by more than 1e-3 or the track by more than 1e-4 (most change the voiced / unvoiced pattern or a lag outright)."""
import math
import os

import numpy as np
import pytest

from tests import pitch_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
M, W_ = (50.0, 250.0), (100.0, 600.0)
PARITY_CAP = 1e-9                       # the largest bound any GPU comparison of phi uses
VALUE_TOL = 1e-10                       # the bound on voiced values


@pytest.fixture(scope='module')
def inputs():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    return {'u1': np.ascontiguousarray(f['u1_wav'], dtype=np.float64), 'u0': np.ascontiguousarray(f['u0_wav'], dtype=np.float64),
            'composite': R.composite()}


def track_diff(a, b):
    """inf when the voiced / unvoiced patterns differ, else the largest relative difference of a voiced value"""
    va, vb = R.voiced(a), R.voiced(b)
    if not np.array_equal(va, vb):
        return math.inf
    return float(np.abs(a[va] / b[va] - 1.0).max()) if va.any() else 0.0


def test_lag_ranges_and_frames():
    assert R.lag_range(50, 250) == (64, 320, 257) and R.lag_range(100, 600) == (26, 160, 135) and R.lag_range(40, 1000) == (16, 400, 385)
    assert [R.frames_of(n) for n in (513, 1100, 2304, 10241, 12345)] == [3, 5, 10, 41, 49]


@pytest.mark.parametrize('rng', [M, W_])
def test_the_two_summation_orders_agree(inputs, rng):
    for name, x in inputs.items():
        d = R.divergence(x, *rng)
        pa, ra = R.nccf(x, *rng, order='dot')
        pb, rb = R.nccf(x, *rng, order='seq')
        same = track_diff(R.dp(pa, ra, *rng), R.dp(pb, rb, *rng))
        print(f'{name} {rng}: two orders {d:.3g}; tracks differ by {same:.3g}')
        assert d <= 1e-12 and same <= VALUE_TOL
        assert np.abs(pa).max() <= 1.0 + 1e-12 and rb.min() >= 1.0


def test_margins_are_large_on_the_parity_inputs(inputs):
    for name, x in inputs.items():
        for rng in (M, W_):
            margin, gap = R.margins(x, *rng)
            print(f'{name} {rng}: path margin {margin:.3g}, candidate-rule gap {gap:.3g}')
            assert margin >= 1e-6 and gap >= 1e-6
    assert R.most_peaks(inputs['composite'], *M) > R.N_CANDS - 1


def test_crafted_lattices_do_what_they_are_for():
    """the cap drops lag 70 in the middle frame; the doubling term takes the octave jump -- both with a margin rounding cannot touch"""
    for phi, rms in (R.cap_case(), R.doubling_case()):
        margin, gap = R.margins_phi(phi, rms, *M)
        assert margin >= 1e-4 and gap >= 1e-4, (margin, gap)
    f0 = np.exp(R.dp(*R.cap_case(), *M))
    assert abs(f0[0] - 16000 / 70) < 1e-9 and abs(f0[2] - 16000 / 70) < 1e-9 and f0[1] < 16000 / 249
    assert np.allclose(np.exp(R.dp(*R.cap_case(), *M, variant='no_cap')), 16000 / 70)
    assert np.allclose(np.exp(R.dp(*R.doubling_case(), *M)), [160.0, 160.0, 80.0])
    assert np.allclose(np.exp(R.dp(*R.doubling_case(), *M, variant='no_doubling')), [160.0, 160.0, 16000 / 130])


def test_margin_is_zero_on_a_tie():
    phi, rms, want = R.tie_case()
    assert np.array_equal(R.dp(phi, rms, *M), [want] * 3)
    # the same lattice through margins' two passes: the runner-up path costs exactly as much
    lmin, lmax, _ = R.lag_range(*M)
    Ls, ds = R._lattice(phi, lmin, lmax)
    assert len(Ls[0]) == 3 and ds[0][1] == ds[0][2] < ds[0][0] and Ls[0][1] > Ls[0][2]


@pytest.mark.parametrize('variant', R.WRONG)
def test_wrong_variants_are_reported(inputs, variant):
    """every fault a kernel could plausibly have moves phi or the track by far more than any bound in use, on the inputs the GPU tests use
    (the waveforms, and the three crafted lattices the DP hook is run on)"""
    dphi, dtrack = 0.0, 0.0
    for name, x in inputs.items():
        good_phi, good_rms = R.nccf(x, *M)
        phi, rms = R.nccf(x, *M, variant=variant)
        dphi = max(dphi, float(np.abs(phi - good_phi).max()))
        dtrack = max(dtrack, track_diff(R.dp(phi, rms, *M, variant=variant), R.dp(good_phi, good_rms, *M)))
    for phi, rms in (R.tie_case()[:2], R.cap_case(), R.doubling_case()):
        dtrack = max(dtrack, track_diff(R.dp(phi, rms, *M, variant=variant), R.dp(phi, rms, *M)))
    print(f'{variant}: phi moves by {dphi:.3g}, the track by {dtrack:.3g}')
    assert dphi > 1e3 * PARITY_CAP or dtrack > 1e3 * VALUE_TOL


@pytest.mark.parametrize('f0,rng', [(60.0, M), (100.0, M), (240.0, M), (120.0, W_), (550.0, W_)])
def test_harmonic_tones_come_out_at_their_frequency(f0, rng):
    """ground truth that neither implementation defines.  Measured: 6.2e-5, 2.4e-4, 2.9e-4, 1.9e-4, 3.7e-4 (bound 2e-3)"""
    got = R.track(R.tone(f0), *rng)
    inner = got[2:-2]
    assert got.shape == (63,) and R.voiced(inner).all()
    err = float(np.abs(np.exp(inner) / f0 - 1.0).max())
    print(f'tone {f0} Hz in {rng}: worst relative error {err:.3g}')
    assert err <= 2e-3


def test_silence_and_noise_are_unvoiced():
    assert not R.voiced(R.track(np.zeros(4096), *M)).any()
    noise = R.track(0.1 * np.random.RandomState(0).randn(8192), *M)
    print(f'noise: {int(R.voiced(noise).sum())} voiced frames of {noise.shape[0]}')
    assert noise.shape == (33,) and R.voiced(noise).sum() <= 2


def test_candidates_order_cap_and_refinement():
    lmin, lmax, K = R.lag_range(*M)
    phi = np.zeros(K)
    for i, v in ((10, 0.5), (30, 0.9), (50, 0.5), (70, 0.2)):              # 0.2 < 0.3 x 0.9: below the threshold
        phi[i] = v
    phi[31] = 0.3                                                          # pulls the 0.9 peak's refined lag up
    cand, phimax = R.candidates(phi, lmin, lmax)
    assert phimax == 0.9 and [round(L) for L, _ in cand] == [lmin + 30, lmin + 10, lmin + 50]      # by v, the smaller lag first on equal v
    assert lmin + 30 < cand[0][0] < lmin + 30.5 and cand[0][1] > 0.9 and cand[1] == (lmin + 10.0, 0.5)
    many = np.zeros(K)
    many[1:121:4] = np.linspace(0.5, 1.0, 30)
    kept, _ = R.candidates(many, lmin, lmax)
    assert len(kept) == R.N_CANDS - 1 and [v for _, v in kept] == sorted(np.linspace(0.5, 1.0, 30), reverse=True)[:19]
    assert len(R.candidates(many, lmin, lmax, 'no_cap')[0]) == 30
