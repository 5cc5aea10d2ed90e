"""The numpy restatement of the conversion scores (dtw_ref.py) checked against a brute-force enumeration of all monotone paths, against
itself with x and y swapped, and on wrong stand-ins: every variant in dtw_ref.WRONG must be reported, with the distance it is off by
(printed; run with -s).  CPU only."""
import math
import os

import numpy as np
import pytest

import dtw_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def mels():
    z = np.load(os.path.join(GOLDEN, 'features.npz'))
    return z['u0_S'], z['u1_S']


def _f0_tracks(Tx, Ty, seed=5):
    """ln-Hz tracks with voiced and unvoiced runs"""
    rng = np.random.default_rng(seed)
    out = []
    for T in (Tx, Ty):
        f = math.log(120.0) + 0.2 * np.sin(np.arange(T) / 5.0) + rng.normal(0.0, 0.02, T)
        f[rng.uniform(size=T) < 0.3] = R.UNVOICED
        out.append(f)
    return out


@pytest.mark.parametrize('shape', [(1, 1), (1, 4), (4, 1), (2, 2), (3, 3), (3, 5), (4, 5), (5, 4)])
@pytest.mark.parametrize('kind', ['real', 'integer'])
def test_against_all_monotone_paths(shape, kind):
    """total equal to the bit (the running cost of a path is the recurrence's own sum) and the reported path among the optimal ones; on
    integer distances, where ties abound, it is the one the tie order dictates: walking back, the diagonal wherever it is optimal, else
    (i-1, j) wherever that is"""
    rng = np.random.default_rng(shape[0] * 16 + shape[1])
    d = rng.uniform(0.1, 2.0, shape) if kind == 'real' else rng.integers(1, 3, shape).astype(np.float64)
    D, code, _ = R.dtw_matrix(d)
    path = R.backtrack(code)
    total, best = R.brute_force(d)
    assert D[-1, -1] == total
    assert tuple(map(tuple, path.tolist())) in best
    assert max(shape) <= len(path) <= shape[0] + shape[1] - 1
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (shape[0] - 1, shape[1] - 1)
    # the tie order, restated on the brute force's D: D of a cell is the cheapest path to it
    i, j = shape[0] - 1, shape[1] - 1
    want = [(i, j)]
    while i or j:
        pred = [(i - 1, j - 1), (i - 1, j), (i, j - 1)]
        costs = [R.brute_force(d[:a + 1, :b + 1])[0] if a >= 0 and b >= 0 else np.inf for a, b in pred]
        i, j = pred[int(np.argmin(costs))]                               # argmin takes the first of equals: diagonal, then (i-1, j)
        want.append((i, j))
    assert want[::-1] == list(map(tuple, path.tolist()))


def test_swapping_x_and_y_transposes_the_path(mels):
    dct = R.dct_basis(24, 80)
    fx, fy = R.cepstra(mels[0], dct), R.cepstra(mels[1], dct)
    assert R.path_margin(fx, fy) > 0.0                                   # no ties: the path is unique
    t1, p1, m1 = R.dtw(fx, fy)
    t2, p2, m2 = R.dtw(fy, fx)
    assert t1 == t2 and m1 == m2 and np.array_equal(p1, p2[:, ::-1])


def test_the_two_summation_orders_agree(mels):
    dct = R.dct_basis(24, 80)
    fx, fy = R.cepstra(mels[0], dct), R.cepstra(mels[1], dct)
    e = R.two_orders(fx, fy)
    c = np.abs(R.cepstra(mels[0], dct, 'numpy') - fx).max() / np.abs(fx).max()
    print(f'two orders: total {e:.3g}, cepstra {c:.3g}')
    assert e < 1e-13 and c < 1e-14
    assert np.array_equal(R.dtw(fx, fy, order='numpy')[1], R.dtw(fx, fy)[1])


def test_margin_is_zero_on_a_tie_and_the_diagonal_wins():
    x = np.zeros((3, 1))
    assert R.path_margin(x, x, 1.0) == 0.0                               # the constant lattice: every interior cell ties three ways
    total, path, mcd = R.dtw(x + 1.0, x, 1.0)
    assert total == 3.0 and mcd == 1.0 and path.tolist() == [[0, 0], [1, 1], [2, 2]]
    total, path, _ = R.dtw(np.ones((2, 1)), np.zeros((4, 1)), 1.0)
    assert path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3]]             # walking back the diagonal comes first, the row's rest is forced


def test_dct_basis_is_orthonormal_without_the_level():
    b = R.dct_basis(40, 80)
    assert np.abs(b @ b.T - np.eye(40)).max() < 1e-14
    assert np.abs(b.sum(1)).max() < 1e-13                                # every row is orthogonal to the constant: the level is left out


def test_f0_stats_by_hand():
    u = R.UNVOICED
    path = np.array([[0, 0], [1, 1], [2, 1], [3, 2], [3, 3]], np.int32)
    f0x = np.log([100.0, 200.0, 100.0, 1.0]); f0x[3] = u
    f0y = np.log([200.0, 200.0, 1.0, 1.0]); f0y[2] = u; f0y[3] = float('nan')
    n_vv, n_vu, rmse, corr, vuv = R.f0_stats(path, f0x, f0y)
    assert (n_vv, n_vu, vuv) == (3, 0, 0.0)                              # (3,2) and (3,3): neither voiced (NaN is not voiced)
    assert abs(rmse - 1200.0 * math.sqrt(2.0 / 3.0)) < 1e-9             # an octave twice, unison once
    assert math.isnan(R.f0_stats(path[:2], f0x, f0y)[3])                 # ly is constant over these two steps: its centred sum is 0
    assert math.isnan(R.f0_stats(path[:1], f0x, f0y)[3])
    assert math.isnan(R.f0_stats(path[3:], f0x, f0y)[2])                 # no voiced step at all
    f0y[0] = u
    assert R.f0_stats(path, f0x, f0y)[:2] == (2, 1) and R.f0_stats(path, f0x, f0y)[4] == 0.2


@pytest.mark.parametrize('variant', R.WRONG)
def test_wrong_variants_are_reported(mels, variant):
    """each wrong stand-in moves a result the GPU test compares -- the path, the total, the distortion or an F0 statistic -- by far more than
    that test's bound, on the golden pair or on a crafted lattice made for it"""
    f0x, f0y = _f0_tracks(49, 41)
    good = R.score(mels[0], mels[1], 24, f0x, f0y)
    bad = R.score(mels[0], mels[1], 24, f0x, f0y, variant)
    moved = {k: abs(bad[k] - good[k]) / abs(good[k]) for k in ('total', 'mcd_db', 'f0_rmse_cents', 'f0_corr', 'vuv_error')}
    path_differs = bad['path'].shape != good['path'].shape or not np.array_equal(bad['path'], good['path'])
    if variant in ('tie_swapped', 'le_for_lt'):                          # speech has no ties: these show on integer distances only
        for seed in range(200):
            d = np.random.default_rng(seed).integers(0, 4, (4, 5)).astype(np.float64)
            (D, code, _), (Db, codeb, _) = R.dtw_matrix(d), R.dtw_matrix(d, variant)
            g, b = R.backtrack(code), R.backtrack(codeb)
            assert np.array_equal(D, Db)                                 # a tie order changes no cost
            if not np.array_equal(g, b):
                break
        print(f'{variant}: integer lattice of seed {seed}: same total {D[-1, -1]}, path {g.tolist()} becomes {b.tolist()}')
        assert not np.array_equal(g, b)
        return
    if variant in ('first_row_not_accumulated', 'first_col_not_accumulated'):   # the golden pair's path leaves the edge at once
        x, y = np.array([[5.0], [5.0]]), np.array([[0.0], [0.0], [5.0]])
        if variant == 'first_col_not_accumulated':
            x, y = y, x
        g, b = R.dtw(x, y, 1.0), R.dtw(x, y, 1.0, variant=variant)
        print(f'{variant}: crafted lattice: total {g[0]} becomes {b[0]}')
        assert g[0] == 10.0 and b[0] == 0.0
        return
    worst = max(moved.values())
    print(f'{variant}: path differs: {path_differs}; ' + ', '.join(f'{k} moves by {v:.3g}' for k, v in moved.items()))
    assert worst > 1e-6 or path_differs, moved
    if variant in ('voiced_if_either', 'corr_no_mean', 'cents_ln10'):
        assert not path_differs and moved['total'] == 0.0 and max(moved['f0_rmse_cents'], moved['f0_corr']) > 1e-3
    else:
        assert max(moved['total'], moved['mcd_db']) > 1e-3


def test_warped_is_a_float32_mel_of_the_asked_length(mels):
    y = R.warped(mels[0], 60, 3)
    assert y.dtype == np.float32 and y.shape == (60, 80) and y.min() >= 0.0 and y.max() <= 1.0
    assert np.array_equal(y, R.warped(mels[0], 60, 3)) and not np.array_equal(y, R.warped(mels[0], 60, 4))
