"""nnls_ref.py proven before test_gpu_mel_nnls.py relies on it (CPU only): its two summation orders agree, zero iterations are the
pseudo-inverse path, the iteration reaches a mel-consistent non-negative magnitude (scipy's NNLS confirms one exists), and every wrong variant
of the algorithm is far from it.  Inputs: griffinlim_ref.PARITY_SLICES of features.npz's u1_wav (4, 5, 9 and 41 frames), the mel through the
project's own filter bank, cast to float32.  The 4-frame slice is near silence (its pseudo-inverse residual is 1.2e-5 already): the edge of
the domain, not a test of the iteration.

Measured (numpy, float64): dense against band order, relative to max |x|

    frames   n_iter 1    50          200
    4        4.8e-17     1.2e-14     6.1e-14
    5        1.1e-16     2.1e-15     3.0e-14
    9        1.0e-16     3.9e-15     2.8e-14
    41       2.0e-16     8.6e-15     3.7e-14

residual || x B - amp || / || amp || at 200 iterations 9.8e-13 / 6.0e-13 / 1.3e-9 (5 / 9 / 41 frames) against the floored pseudo-inverse's
2.4e-2 / 5.6e-2 / 6.6e-2; the wrong variants lie between 6.6e-4 (half the step, 9 frames, 50 iterations) and 11 from the definition."""
import os

import numpy as np
import pytest

from speechsplit_amd import features
from tests import griffinlim_ref as R
from tests import nnls_ref as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FRAMES = (4, 5, 9, 41)
ITERATED = (5, 9, 41)                                                   # the inputs on which the iteration has something to do
GPU_BAR_FACTOR = 100.0                                                  # test_gpu_mel_nnls.py: 100 x the disagreement


@pytest.fixture(scope='module')
def S():
    """the basis, its pseudo-inverse and step, and per frame count the mel and the dense result at every iteration count"""
    B = features.mel_filter_bank().T.astype(np.float64)
    u1 = np.load(os.path.join(GOLD, 'features.npz'))['u1_wav']
    s = dict(B=B, P=np.linalg.pinv(B), step=N.step_of(B), mel={F: N.parity_mel(u1, F, B) for F in FRAMES})
    s['dense'] = {(F, it): N.mel_to_linear_nnls(s['mel'][F], B, it, s['step'], inv_basis=s['P']) for F in FRAMES for it in (50, 200)}
    return s


def test_the_bank_and_its_step(S):
    lam = 1.0 / S['step']
    assert S['B'].shape == (513, 80) and abs(lam - 1.7994e-3) < 1e-7
    assert int((S['B'].sum(axis=1) == 0).sum()) == 32                   # bins no band covers


def test_two_orders_agree(S):
    worst = 0.0
    for F in FRAMES:
        for it in N.ITERS:
            _, d = N.disagreement(S['mel'][F], S['B'], it, S['P'], S['step'])
            print(f'{F} frames, n_iter {it}: dense vs band order {d:.3g} of max |x|')
            worst = max(worst, d)
            assert d <= N.DISAGREEMENT_CAP
            assert GPU_BAR_FACTOR * d * 100.0 <= N.SMALLEST_WRONG       # the GPU bar stays 100 x under the smallest fault
    print(f'worst {worst:.3g}, cap {N.DISAGREEMENT_CAP:g}')
    assert N.DISAGREEMENT_CAP <= 1e-11


@pytest.mark.parametrize('order', ['dense', 'band'])
def test_zero_iterations_are_the_floored_pseudo_inverse(S, order):
    for F in FRAMES:
        got = N.mel_to_linear_nnls(S['mel'][F], S['B'], 0, S['step'], order=order, inv_basis=S['P'])
        assert np.array_equal(got, R.mel_to_linear(S['mel'][F], S['P']))
        assert np.array_equal(N.mel_to_linear_nnls(S['mel'][F], S['B'], 0, S['step'], floor=0.5, order=order, inv_basis=S['P']),
                              R.mel_to_linear(S['mel'][F], S['P'], 0.5))


def test_residual_falls_a_thousandfold_and_nothing_is_below_the_floor(S):
    for F in ITERATED:
        mel = S['mel'][F]
        for order in ('dense', 'band'):
            x = S['dense'][F, 200] if order == 'dense' else N.mel_to_linear_nnls(mel, S['B'], 200, S['step'], order='band', inv_basis=S['P'])
            res, res0 = N.residual(x, mel, S['B']), N.residual(R.mel_to_linear(mel, S['P']), mel, S['B'])
            print(f'{F} frames, {order}: residual {res:.3g} against the floored pseudo-inverse\'s {res0:.3g}')
            assert res * 1000.0 <= res0
            assert x.min() >= 1e-10 and np.isfinite(x).all()


def test_uncovered_bins_keep_their_start(S):
    dead = S['B'].sum(axis=1) == 0
    for F in ITERATED:
        assert np.array_equal(S['dense'][F, 200][:, dead], R.mel_to_linear(S['mel'][F], S['P'])[:, dead])
        band = N.mel_to_linear_nnls(S['mel'][F], S['B'], 50, S['step'], order='band', inv_basis=S['P'])
        assert np.array_equal(band[:, dead], R.mel_to_linear(S['mel'][F], S['P'])[:, dead])


def test_scipy_nnls_confirms_a_consistent_non_negative_solution_exists(S):
    from scipy.optimize import nnls
    mel = S['mel'][41]
    amp = N.amplitudes(mel)
    for f in (0, 7, 20, 40):
        x, rnorm = nnls(S['B'].T, amp[f], maxiter=20000)
        rel = rnorm / np.linalg.norm(amp[f])
        ours = np.linalg.norm(S['dense'][41, 200][f] @ S['B'] - amp[f]) / np.linalg.norm(amp[f])
        print(f'frame {f}: scipy residual {rel:.3g}, 200 iterations {ours:.3g}')
        assert x.min() >= 0.0 and rel <= 1e-12                          # the residual, not the solution: it is not unique
        assert ours <= 1e-7


def test_every_wrong_variant_is_reported(S):
    smallest = np.inf
    for F in ITERATED:
        for it in (50, 200):
            for v in N.WRONG:
                d = N.rel_diff(N.mel_to_linear_nnls(S['mel'][F], S['B'], it, S['step'], inv_basis=S['P'], variant=v), S['dense'][F, it])
                print(f'{F} frames, n_iter {it}, {v}: {d:.3g}')
                smallest = min(smallest, d)
    print(f'smallest distance {smallest:.3g}')
    assert smallest >= N.SMALLEST_WRONG                                 # 6.62e-4: half the step, 9 frames, 50 iterations
    assert GPU_BAR_FACTOR * N.DISAGREEMENT_CAP * 100.0 <= N.SMALLEST_WRONG


def test_pack_restated(S):
    p = N.pack(S['B'])
    lo, ln, off, w = N.unpack(p, 80)
    assert p.shape == (2 * 80 + 941,) and w.shape == (941,) and int(ln.max()) == 34
    dense = np.zeros_like(S['B'])
    for m in range(80):
        dense[lo[m]:lo[m] + ln[m], m] = w[off[m]:off[m + 1]]
    assert np.array_equal(dense, S['B'])
    holes = S['B'].copy()
    holes[lo[40] + 1, 40] = 0.0
    with pytest.raises(ValueError, match='contiguous'):
        N.pack(holes)
    neg = S['B'].copy()
    neg[3, 3] = -1e-9
    with pytest.raises(ValueError, match='negative'):
        N.pack(neg)
