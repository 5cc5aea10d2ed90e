"""The numpy restatement of the pitch tracker's spectral-stationarity term (pitch_stat_ref.py) checked against itself, against signals whose
answer neither implementation defines, and on wrong stand-ins.  CPU only.

Measured when this was written.  Two summation orders (numpy's reductions against term-by-term sums), max |S_dot - S_seq|: 513 7.4e-14,
1100 2.7e-13, 2304 9.2e-13, u1 9.6e-13, u0 1.6e-12, composite 2.2e-12 -- the GPU bound is min(1e-9, 100 x that) per input.  d >= 1 to the
bit on every input.  S spans 0.062 .. 0.924 on the speech inputs and 0.0018 .. 0.996 on the composite.  Ground truth: interior frames of a
steady five-harmonic 120 Hz tone 0.99999 (and silence exactly 1), the frame at an abrupt noise-to-tone change 0.135, white noise 0.44 ..
0.80.  Path margins with the term on, the twelve (input, range) cases: >= 1.06e-3 (u0 in (50, 250)).  The crafted lattice: margins 5.2e-2,
0.95 and 2.3e-3 for the issue's three S tracks, and 2.8e-2 for a fourth (0.08 everywhere) that only a term on BOTH transitions keeps voiced:
the wrong variant with the term on `up` alone changes no other track."""
import functools
import os

import numpy as np
import pytest

from tests import pitch_ref as R
from tests import pitch_stat_ref as Q

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
M, W_ = (50.0, 250.0), (100.0, 600.0)
NAMES = ('513', '1100', '2304', 'u1', 'u0', 'composite')
MARGIN_FLOOR = 1e-6                      # test_gpu_pitch.py's
S_MOVED = 1e-3                           # a wrong variant is reported when it moves S by more than this, or changes the lattice's track


@functools.lru_cache(maxsize=None)
def signals():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    u1 = np.ascontiguousarray(f['u1_wav'], dtype=np.float64)
    return {'513': u1[:513].copy(), '1100': u1[:1100].copy(), '2304': u1[:2304].copy(), 'u1': u1,
            'u0': np.ascontiguousarray(f['u0_wav'], dtype=np.float64), 'composite': R.composite()}


@functools.lru_cache(maxsize=None)
def good(name):
    S, d = Q.stationarity(signals()[name], with_d=True)
    S.setflags(write=False)
    d.setflags(write=False)
    return S, d


@functools.lru_cache(maxsize=None)
def noise_to_tone():
    """2560 samples (10 hops) of white noise, then a five-harmonic 120 Hz tone: frame 10 is centred on the change"""
    return np.concatenate([0.05 * np.random.RandomState(1).randn(2560), R.tone(120.0, 2560)])


def test_constants():
    assert (Q.STAT_W, Q.STAT_GAP, Q.LPC_ORD, Q.PREEMP, Q.VTR_S_C) == (480, 320, 18, 0.4, 0.5) and Q.FF == 1.0 / 1.001
    assert len(Q.WRONG) >= 10 and len(set(Q.WRONG)) == len(Q.WRONG)


def test_the_two_summation_orders_agree():
    for name in NAMES:
        div = Q.divergence_stat(signals()[name])
        print(f'{name}: two orders {div:.3g}, GPU bound {min(1e-9, 100.0 * div):.3g}')
        assert 0.0 < div <= 1e-10                                           # S is O(1); a bound of 100 x this stays far below any variant


def test_d_is_at_least_one_and_s_in_range():
    inputs = [signals()[k] for k in NAMES] + [noise_to_tone(), np.zeros(4096), R.tone(120.0, 8192), 0.1 * np.random.RandomState(0).randn(8192)]
    for x in inputs:
        for order in ('dot', 'seq'):
            S, d = Q.stationarity(x, order=order, with_d=True)
            assert S.shape == (R.frames_of(x.shape[0]),) and S[0] == 0.0
            assert d.min() >= 1.0 - 1e-12, d.min()
            assert np.all(S[1:] > 0.0) and np.all(S <= 1.0), (S.min(), S.max())
    speech = np.concatenate([good(k)[0][1:] for k in NAMES[:-1]])
    comp = good('composite')[0][1:]
    print(f'S on speech {speech.min():.3g} .. {speech.max():.3g}, on the composite {comp.min():.3g} .. {comp.max():.3g}')
    assert speech.min() < 0.1 and speech.max() > 0.9 and comp.min() < 0.01 and comp.max() > 0.99     # the whole range is exercised


def test_dp_stat_with_a_zero_track_is_the_tracker_without_the_term():
    for name in NAMES:
        for rng in (M, W_):
            phi, rms = R.nccf(signals()[name], *rng)
            a, b = Q.dp_stat(phi, rms, np.zeros(phi.shape[0]), *rng), R.dp(phi, rms, *rng)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (name, rng)
    for phi, rms in (R.tie_case()[:2], R.cap_case(), R.doubling_case(), Q.stat_case()):
        assert np.array_equal(Q.dp_stat(phi, rms, np.zeros(phi.shape[0]), *M), R.dp(phi, rms, *M))


def test_ground_truth_steady_signals_are_stationary_and_a_change_is_not():
    """Neither implementation defines these.  Bounds from the restatement's own values with the margin stated: a steady tone gives
    0.99999 and silence exactly 1 -- the bound 0.99 leaves a thousand times the tone's distance from 1; the frame on the change gives
    0.135 -- the bound 0.27 is twice that; the frames inside the noise give 0.55 or more and are held above 0.4, three times the change's
    value and a quarter below their own smallest."""
    tone = Q.stationarity(R.tone(120.0, 8192))[2:-2]
    silence = Q.stationarity(np.zeros(4096))[1:]
    S = Q.stationarity(noise_to_tone())
    print(f'tone {tone.min():.6g}, silence {silence.min():.6g}, change {S[10]:.3g}, inside the noise >= {S[2:9].min():.3g}, '
          f'inside the tone >= {S[12:19].min():.6g}')
    assert tone.min() >= 0.99 and np.all(silence == 1.0)
    assert S[10] <= 0.27 and S[2:9].min() >= 0.4 and S[12:19].min() >= 0.99


def test_the_crafted_lattice_does_what_it_is_for():
    phi, rms = Q.stat_case()
    dip = np.array([1, 1, 1, 0, 0, 1, 1, 1], bool)
    want = {'zeros': (dip, 5.2e-2), 'ones': (np.ones(8, bool), 0.95), 'edges': (dip, 2.3e-3), 'low': (np.ones(8, bool), 2.8e-2)}
    for key, S in Q.STAT_CASE_TRACKS.items():
        f0 = Q.dp_stat(phi, rms, S, *M)
        margin = Q.margins_stat(phi, rms, S, *M)
        print(f'{key}: voiced {R.voiced(f0).astype(int)}, margin {margin:.3g}')
        assert np.array_equal(R.voiced(f0), want[key][0]) and margin >= MARGIN_FLOOR
        assert abs(margin / want[key][1] - 1.0) <= 0.05                     # the figures the lattice was built to
        assert np.allclose(np.exp(f0[R.voiced(f0)]), 16000.0 / 133.0, rtol=1e-3)


@pytest.mark.parametrize('variant', Q.WRONG)
def test_wrong_variants_are_reported(variant):
    moved, track = 0.0, False
    if variant in Q.WRONG_S:
        for name in ('u1', 'composite'):
            moved = max(moved, float(np.abs(Q.stationarity(signals()[name], variant=variant) - good(name)[0]).max()))
    phi, rms = Q.stat_case()
    for S in Q.STAT_CASE_TRACKS.values():
        track = track or not np.array_equal(Q.dp_stat(phi, rms, S, *M, variant=variant if variant in Q.WRONG_DP else None), Q.dp_stat(phi, rms, S, *M))
    if variant in Q.WRONG_S:                                                # ... and end to end, on the speech
        a, b = Q.track_stat(signals()['u1'], *M, variant=variant), Q.track_stat(signals()['u1'], *M)
        print(f'{variant}: S moves by {moved:.3g}; u1 track {"changes" if not np.array_equal(a, b) else "stays"}')
    else:
        print(f'{variant}: the crafted lattice changes: {track}')
    assert moved > S_MOVED or track


def test_input_conditions_with_the_term_on():
    worst = np.inf
    for name in NAMES:
        for rng in (M, W_):
            phi, rms = R.nccf(signals()[name], *rng)
            margin = Q.margins_stat(phi, rms, good(name)[0], *rng)
            gap = R.margins_phi(phi, rms, *rng)[1]                          # the candidate rule does not see S
            print(f'{name} {rng}: path margin {margin:.3g}')
            assert margin >= MARGIN_FLOOR and gap >= MARGIN_FLOOR, (name, rng, margin, gap)
            worst = min(worst, margin)
    print(f'worst path margin {worst:.3g}')
