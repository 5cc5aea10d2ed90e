"""The numpy restatement of STOI / ESTOI (tests/stoi_ref.py) checked on its own, on the CPU: its two summation orders (term-by-term sums
around an explicit DFT matrix; numpy's reductions around numpy.fft.rfft) agree, a signal against itself scores 1, noise lowers the score
monotonically, and every deliberately wrong variant lies far from the definition.

Bars.  The two orders must agree below BAR = 1e-11.  A wrong variant must lie at least 100 BAR = 1e-9 from the definition on both
recordings, in the mode it bears on (clipping, beta and alpha exist in STOI only, the column step in ESTOI only); one that does not is
dropped with a note, never kept with a looser bar -- none had to be.  Measured (u0 / u1, the GPU tests' gated-plus-noise pairs at 10 kHz):
the two orders differ by at most 2.8e-16 in the score; 52 of 59 and 43 of 49 frames are kept, giving 22 and 13 segments; white noise at
20 / 10 / 0 / -10 dB SNR gives STOI 0.287 / 0.174 / 0.105 / 0.033 on u0 and 0.395 / 0.272 / 0.201 / 0.128 on u1; the variants' distances
(STOI, ESTOI where it applies):
    upper_edge_inclusive 4.8e-4 .. 1.1e-3     range_30db 1.6e-3 .. 0.034       last_frame_included 6.6e-4 .. 2.7e-3     n_29 4.7e-3 .. 6.6e-3
    no_clipping 0.024 .. 0.035 (STOI)         beta_minus_5 0.077 .. 0.081 (STOI)   no_alpha 0.57 .. 0.61 (STOI)         no_mean_removal 0.62 .. 0.75
    own_mask_for_y 2.9e-3 .. 0.071            window_twice 8.9e-3 .. 0.048     estoi_without_columns 0.083 .. 0.15 (ESTOI)
"""
import math
import os

import numpy as np
import pytest
from scipy import signal

import stoi_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BAR = 1e-11
STOI_ONLY = ('no_clipping', 'beta_minus_5', 'no_alpha')
ESTOI_ONLY = ('estoi_without_columns',)


def _load():
    f = np.load(os.path.join(GOLDEN, 'features.npz'))
    return {k: signal.resample_poly(f[k + '_wav'].astype(np.float64), 5, 8) for k in ('u0', 'u1')}


U = _load()
PAIRS = {'u0': R.make_pair(U['u0'], 1), 'u1': R.make_pair(U['u1'], 2)}
BASE = {(k, e): R.stoi(*PAIRS[k], e) for k in PAIRS for e in (False, True)}       # computed once, never changed


def test_constants_and_band_table():
    assert R.EPS == 2.0 ** -52 and (R.FRAME, R.HOP, R.NFFT, R.J, R.N) == (256, 128, 512, 15, 30)
    assert R.bands() == (list(R.LO), list(R.HI))
    assert R.LO[1:] == R.HI[:-1]                                                  # third-octave bands tile the axis
    w = R.window()
    assert np.abs(w - np.hanning(258)[1:-1]).max() < 1e-15 and w.shape == (256,)
    assert 1.0 + 10.0 ** (15 / 20) == 1.0 + 10.0 ** (-R.BETA / 20.0)
    assert [R.n_frames(n) for n in (255, 256, 383, 384, 4096, 3968)] == [0, 1, 1, 2, 31, 30]
    assert [R.frames_below(n) for n in (256, 257, 384, 385, 4096)] == [0, 1, 1, 2, 30]


@pytest.mark.parametrize('name', list(PAIRS))
@pytest.mark.parametrize('extended', (False, True))
def test_the_two_orders_agree(name, extended):
    x, y = PAIRS[name]
    a, b = BASE[name, extended], R.stoi(x, y, extended, 'numpy')
    assert a['K'] == b['K'] and a['S'] == b['S'] >= 2 and np.array_equal(a['inv'], b['inv'])
    assert a['K'] < a['F']                                                         # the mask removes frames on these inputs
    print(name, extended, a['score'], abs(a['score'] - b['score']), a['S'], a['K'], a['F'])
    assert abs(a['score'] - b['score']) < BAR
    assert np.abs(a['X'] - b['X']).max() < BAR * np.abs(a['X']).max()
    assert np.array_equal(a['xp'], b['xp'])                                        # two products and an add have one order


@pytest.mark.parametrize('name', list(PAIRS))
def test_a_signal_against_itself_scores_one(name):
    x = PAIRS[name][0]
    for order in ('loop', 'numpy'):
        assert abs(R.stoi(x, x, False, order)['score'] - 1.0) < 1e-12
        assert abs(R.stoi(x, x, True, order)['score'] - 1.0) < 1e-12


@pytest.mark.parametrize('name', list(U))
@pytest.mark.parametrize('extended', (False, True))
def test_the_score_falls_with_the_noise(name, extended):
    u = U[name]
    nz = np.random.RandomState(5).standard_normal(u.shape[0])
    nz *= math.sqrt(np.mean(u * u) / np.mean(nz * nz))
    scores = [R.stoi(u, u + nz * 10.0 ** (-snr / 20.0), extended)['score'] for snr in (20, 10, 0, -10)]
    print(name, extended, scores)
    assert all(a > b for a, b in zip(scores, scores[1:])), scores
    assert scores[0] < 1.0


def test_short_inputs_have_no_score():
    x, y = PAIRS['u0']
    for n, F in ((4096 - 128, 30), (256, 1), (255, 0), (1, 0)):
        r = R.stoi(x[:n], y[:n])
        assert math.isnan(r['score']) and r['S'] == 0 and r['F'] == F
    r = R.stoi(x[:4096], y[:4096])
    assert (r['F'], r['K'], r['S']) == (31, 31, 1) and 0.0 < r['score'] < 1.0


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_a_wrong_variant_lies_far_from_the_definition(variant):
    modes = (False,) if variant in STOI_ONLY else (True,) if variant in ESTOI_ONLY else (False, True)
    for name, (x, y) in PAIRS.items():
        for extended in modes:
            d = abs(R.stoi(x, y, extended, variant=variant)['score'] - BASE[name, extended]['score'])
            print(variant, name, extended, d)
            assert d >= 100 * BAR, (variant, name, extended, d)
