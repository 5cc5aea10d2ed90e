"""The conversion scores on the GPU (csrc/dtw.hip: ss_mel_cepstra, ss_dtw, ss_path_f0_stats) against the float64 numpy restatement
tests/dtw_ref.py, which tests/test_dtw_ref_selftest.py checks on its own.

Bounds.  The path and its length must be the reference's exactly; that is a fair demand only where the reference's own path is safe from
rounding, so the module asserts on the CPU, before anything runs, that every input's smallest on-path gap between the best and the
second-best predecessor (dtw_ref.path_margin) is at least 1e-6 -- ten orders above the rounding of D.  The total is held to
min(1e-9, 100 x two_orders) relative, two_orders being the reference's own disagreement between numpy's reductions and term-by-term sums
(one factor of ten for a third order of summation, one for fused multiply-adds); the cepstra to the same kind of bound on the max norm.
Where the two orders agree to the bit that bound is 0: the kernel must then give the term-by-term sum exactly, which it is built to do
(no fused multiply-adds, correctly rounded root and division).  F0 statistics are computed on the reference's own path: counts exact,
values within 1e-10 relative, NaN where the definition says NaN.

Measured on an MI355X, worst over all cases: cepstra 0 (the reference's two orders disagree by up to 4.9e-15), total 0 (two orders: 0
on fifteen of the twenty inputs, up to 1.8e-16 on the rest), F0 statistics 0; every path, length and crafted tie as the reference has
it; smallest on-path margin 1.3e-5 (out_F / out_RFU), 1.4e-2 or more on the warped copies.  The whole file runs in 3 s.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import dtw_ref as R
import guarded as G
from speechsplit_amd import _capi, convert, metrics

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NT = 64                                                # the kernel's strip height (kernels.h: DTW_STRIP); its fy ring holds 2 NT columns
MARGIN = 1e-6


def _golden():
    f, d = np.load(os.path.join(GOLDEN, 'features.npz')), np.load(os.path.join(GOLDEN, 'demo_conversion.npz'))
    return {'u0': f['u0_S'], 'u1': f['u1_S'], **{k: d[k] for k in d.files if k.startswith('out_')}}


GOLD = _golden()
# 180 frames that change from one to the next, to cut warped pairs from (the demo's converted mels are too even in time to pin a warp)
BASE = np.concatenate([GOLD['u0'], GOLD['u1'], GOLD['u0'][::-1], GOLD['u1'][::-1]]).astype(np.float32)


def _warped_pair(Tx, Ty, seed):
    x = np.ascontiguousarray(BASE[:Tx])
    return x, R.warped(x, Ty, seed)


# name -> (mel_x, mel_y, n_ceps); `WARPED` names the warped copies
CASES = {f'features_u0_u1_c{c}': (GOLD['u0'], GOLD['u1'], c) for c in (1, 13, 24, 40)}
CASES['demo_R_F'] = (GOLD['out_R'], GOLD['out_F'], 24)
CASES['demo_F_RFU'] = (GOLD['out_F'], GOLD['out_RFU'], 24)
WARPED = {}
for n, (tx, ty) in enumerate([(1, 1), (1, 5), (5, 1), (2, 2),                               # degenerate lattices
                              (NT - 1, 70), (NT, 70), (NT + 1, 70),                         # a strip: one row below, at, above
                              (70, NT - 1), (70, NT), (70, NT + 1),                         # a ring refill of NT columns
                              (120, 2 * NT - 1), (120, 2 * NT), (120, 2 * NT + 1),          # the ring of 2 NT columns wraps
                              (150, 170)]):                                                 # three strips, three refills
    WARPED[f'warped_{tx}x{ty}'] = (tx, ty)
    CASES[f'warped_{tx}x{ty}'] = (*_warped_pair(tx, ty, 100 + n), 24)

REF = {}                                               # name -> dict(cx, cy, total, path, mcd, two_orders, cep_orders); computed once, never changed


def _reference(name):
    if name not in REF:
        x, y, c = CASES[name]
        dct = R.dct_basis(c, x.shape[1])
        cx, cy = R.cepstra(x, dct), R.cepstra(y, dct)
        total, path, mcd = R.dtw(cx, cy)
        cep = max(np.abs(R.cepstra(m, dct, 'numpy') - f).max() / np.abs(f).max() for m, f in ((x, cx), (y, cy)))
        REF[name] = dict(dct=dct, cx=cx, cy=cy, total=total, path=path, mcd=mcd, two_orders=R.two_orders(cx, cy), cep_orders=cep,
                         margin=R.path_margin(cx, cy))
    return REF[name]


def test_conditions_hold_on_the_cpu_reference():
    """not measurements: what makes 'the path, exactly' a fair demand, and what makes the warped cases exercise both one-sided steps"""
    assert len(CASES) == 6 + 14
    for name in CASES:
        r = _reference(name)
        assert r['margin'] >= MARGIN, (name, r['margin'])
        if name in WARPED and min(WARPED[name]) >= 8:                                      # a lattice with an interior to speak of
            p, (tx, ty) = r['path'], WARPED[name]
            step = np.diff(p, axis=0)
            inner = (p[1:, 0] > 0) & (p[1:, 0] < tx - 1) & (p[1:, 1] > 0) & (p[1:, 1] < ty - 1)
            vertical = int(((step[:, 0] == 1) & (step[:, 1] == 0) & inner).sum())
            horizontal = int(((step[:, 0] == 0) & (step[:, 1] == 1) & inner).sum())
            assert vertical >= 2 and horizontal >= 2, (name, vertical, horizontal)
    print('smallest margin:', min((REF[n]['margin'], n) for n in CASES))


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _run(mel_x, mel_y, dct, scale=R.SCALE):
    """one pair alone through the three C calls -> (cx, cy, out[3], path [P, 2])"""
    d = _t(dct)
    cx, cy = metrics.cepstra_dev(_t(mel_x)[None], None, d), metrics.cepstra_dev(_t(mel_y)[None], None, d)
    out, path, plen = metrics.dtw_dev(cx, None, cy, None, scale)
    torch.cuda.synchronize()
    P = int(plen[0])
    assert bool((path[0, P:] == -1).all())
    return cx[0].cpu().numpy(), cy[0].cpu().numpy(), out[0].cpu().numpy(), path[0, :P].cpu().numpy()


@pytest.mark.parametrize('name', list(CASES))
def test_path_total_and_cepstra_against_the_reference(name):
    r = _reference(name)
    x, y, _ = CASES[name]
    cx, cy, out, path = _run(x, y, r['dct'])
    e_cep = max(np.abs(cx - r['cx']).max() / np.abs(r['cx']).max(), np.abs(cy - r['cy']).max() / np.abs(r['cy']).max())
    e_tot = abs(out[0] - r['total']) / r['total']
    print(f'{name}: cepstra {e_cep:.3g} (two orders {r["cep_orders"]:.3g}), total {e_tot:.3g} (two orders {r["two_orders"]:.3g}), '
          f'P {int(out[1])}, mcd {out[2]:.6f} dB, margin {r["margin"]:.3g}')
    assert path.shape == r['path'].shape and np.array_equal(path, r['path'])
    assert out[1] == len(r['path']) and max(len(x), len(y)) <= out[1] <= len(x) + len(y) - 1
    assert e_cep <= min(1e-9, 100 * r['cep_orders'])
    assert e_tot <= min(1e-9, 100 * r['two_orders'])
    assert out[2] == out[0] / out[1]


def _f0_tracks(Tx, Ty, seed, p_unvoiced=0.3):
    rng = np.random.default_rng(seed)
    out = []
    for T in (Tx, Ty):
        f = math.log(120.0) + 0.2 * np.sin(np.arange(T) / 5.0) + rng.normal(0.0, 0.02, T)
        f[rng.uniform(size=T) < p_unvoiced] = R.UNVOICED
        out.append(f)
    return out


def _stats_close(got, want, what):
    assert got[0] == want[0] and got[1] == want[1], (what, got, want)
    worst = 0.0
    for g, w in zip(got[2:], want[2:]):
        if math.isnan(w):
            assert math.isnan(g), (what, got, want)
        else:
            worst = max(worst, abs(g - w) / abs(w) if w else abs(g))
            assert abs(g - w) <= 1e-10 * abs(w), (what, got, want)
    return worst


def test_f0_statistics_on_the_references_own_path():
    worst = 0.0
    for name in ('features_u0_u1_c24', 'demo_R_F', 'warped_150x170', 'warped_1x5', 'warped_1x1'):
        path = _reference(name)['path']
        Tx, Ty = len(CASES[name][0]), len(CASES[name][1])
        tracks = {'speech': _f0_tracks(Tx, Ty, 3), 'all_unvoiced': [np.full(Tx, R.UNVOICED), np.full(Ty, R.UNVOICED)],
                  'x_unvoiced': [np.full(Tx, R.UNVOICED), _f0_tracks(Tx, Ty, 4, 0.0)[1]],
                  'y_constant': [_f0_tracks(Tx, Ty, 5, 0.0)[0], np.full(Ty, 5.0)],          # 5.0: its sums and its mean are exact
                  'nan_and_inf': [np.where(np.arange(Tx) % 3 == 0, np.nan, _f0_tracks(Tx, Ty, 6)[0]),
                                  np.where(np.arange(Ty) % 4 == 0, np.inf, _f0_tracks(Tx, Ty, 6)[1])]}
        full = np.full((1, Tx + Ty - 1, 2), -1, np.int32)
        full[0, :len(path)] = path
        for kind, (f0x, f0y) in tracks.items():
            got = metrics.path_f0_stats_dev(_t(full), _t([len(path)], torch.int32), _t(f0x)[None], _t(f0y)[None])[0].cpu().tolist()
            want = R.f0_stats(path, f0x, f0y)
            assert got[4] == want[4]                                                       # n_vu / P: one division
            worst = max(worst, _stats_close(got, want, (name, kind)))
            if kind == 'all_unvoiced':
                assert got[0] == 0 and math.isnan(got[2]) and math.isnan(got[3]) and got[4] == 0.0
            if kind == 'x_unvoiced':
                assert got[0] == 0 and got[1] == len(path) and got[4] == 1.0
            if kind == 'y_constant' and len(path) > 1:
                assert got[0] == len(path) and math.isnan(got[3]) and not math.isnan(got[2])
    print(f'F0 statistics: worst relative difference {worst:.3g}')


ONE = np.ones((1, 1))
TIES = {   # integer "mels" with n_mels = n_ceps = 1, dct = [[1]], scale = 1: every distance is an exact integer
    'constant_5x8': (np.full(5, 3.0), np.full(8, 1.0), [[0, 0], [0, 1], [0, 2], [0, 3], [1, 4], [2, 5], [3, 6], [4, 7]]),
    'constant_8x5': (np.full(8, 3.0), np.full(5, 1.0), [[0, 0], [1, 0], [2, 0], [3, 0], [4, 1], [5, 2], [6, 3], [7, 4]]),
    'constant_70x131': (np.full(70, 2.0), np.full(131, 7.0), [[0, j] for j in range(62)] + [[i, 61 + i] for i in range(1, 70)]),
    'constant_131x70': (np.full(131, 2.0), np.full(70, 7.0), [[i, 0] for i in range(62)] + [[61 + j, j] for j in range(1, 70)]),
    'with_itself': (np.array([1.0, 1, 2, 2, 2, 5, 3, 3, 0, 0]), np.array([1.0, 1, 2, 2, 2, 5, 3, 3, 0, 0]), [[i, i] for i in range(10)]),
    'with_itself_200': (np.arange(200.0) // 3 % 5, np.arange(200.0) // 3 % 5, [[i, i] for i in range(200)]),
    # one two-way tie on the path, at the cell named: the diagonal against (i-1, j); the diagonal against (i, j-1); (i-1, j) against (i, j-1)
    'diag_or_up_at_2_2': (np.array([1.0, 2, 2, 4, 5, 0]), np.array([5.0, 3, 2, 4, 3]), [[0, 0], [1, 1], [2, 2], [3, 3], [4, 3], [5, 4]]),
    'diag_or_left_at_3_4': (np.array([3.0, 3, 5, 1, 4, 4]), np.array([0.0, 2, 5, 3, 0, 4]),
                            [[0, 0], [1, 1], [2, 2], [2, 3], [3, 4], [4, 5], [5, 5]]),
    'up_or_left_at_3_4': (np.array([2.0, 5, 2, 5]), np.array([5.0, 0, 5, 5, 2]), [[0, 0], [0, 1], [1, 2], [1, 3], [2, 4], [3, 4]]),
}


@pytest.mark.parametrize('name', list(TIES))
def test_crafted_exact_ties_follow_the_tie_order(name):
    x, y, want = TIES[name]
    total, ref_path, mcd = R.dtw(x[:, None], y[:, None], 1.0)
    assert ref_path.tolist() == want                                                       # the tie order, written out by hand above
    assert R.path_margin(x[:, None], y[:, None], 1.0) == 0.0                               # and it is a tie
    if '_or_' in name:                                                                     # which another order would have resolved otherwise
        assert any(R.dtw(x[:, None], y[:, None], 1.0, variant=v)[1].tolist() != want for v in ('tie_swapped', 'le_for_lt'))
    cx, cy, out, path = _run(x[:, None].astype(np.float32), y[:, None].astype(np.float32), ONE, 1.0)
    assert np.array_equal(cx[:, 0], x) and np.array_equal(cy[:, 0], y)
    assert path.tolist() == want
    assert out[0] == total and out[1] == len(want) and out[2] == mcd                        # integers: to the bit


RAGGED = ['features_u0_u1_c24', 'warped_1x5', 'warped_65x70', 'warped_150x170', 'warped_70x63']


def _ragged_batch(names, nan=True):
    tx, ty = [len(CASES[n][0]) for n in names], [len(CASES[n][1]) for n in names]
    fill = np.nan if nan else 0.0
    mx, my = np.full((len(names), max(tx), 80), fill, np.float32), np.full((len(names), max(ty), 80), fill, np.float32)
    for b, n in enumerate(names):
        mx[b, :tx[b]], my[b, :ty[b]] = CASES[n][0], CASES[n][1]
    return mx, tx, my, ty


def _run_batch(mx, tx, my, ty, f0x=None, f0y=None, poison=True):
    dct = _t(R.dct_basis(24, 80))
    txd, tyd = _t(tx, torch.int32), _t(ty, torch.int32)
    cx, cy = metrics.cepstra_dev(_t(mx), txd, dct), metrics.cepstra_dev(_t(my), tyd, dct)
    zeros = (cx.clone(), cy.clone())
    if poison:                                                                             # ss_dtw must not read behind a row's length either
        for c, lens in ((cx, tx), (cy, ty)):
            for b, n in enumerate(lens):
                c[b, max(1, min(n, c.shape[1])):] = float('nan')
    out, path, plen = metrics.dtw_dev(cx, txd, cy, tyd)
    stats = metrics.path_f0_stats_dev(path, plen, _t(f0x), _t(f0y)) if f0x is not None else None
    torch.cuda.synchronize()
    return zeros, out.cpu().numpy(), path.cpu().numpy(), plen.cpu().numpy(), (stats.cpu().numpy() if stats is not None else None)


def test_ragged_batch_rows_equal_the_pairs_alone():
    mx, tx, my, ty = _ragged_batch(RAGGED)
    assert 1 in tx and len(RAGGED) == 5
    f0 = [_f0_tracks(a, b, 20 + n) for n, (a, b) in enumerate(zip(tx, ty))]
    f0x, f0y = np.full((5, max(tx)), np.nan), np.full((5, max(ty)), np.nan)
    for b in range(5):
        f0x[b, :tx[b]], f0y[b, :ty[b]] = f0[b]
    (cx, cy), out, path, plen, stats = _run_batch(mx, tx, my, ty, f0x, f0y)
    for b, name in enumerate(RAGGED):
        r = _reference(name)
        acx, acy, aout, apath = _run(CASES[name][0], CASES[name][1], r['dct'])
        assert np.array_equal(cx[b, :tx[b]].cpu().numpy(), acx) and not bool(cx[b, tx[b]:].any())   # exact zeros behind the length
        assert np.array_equal(cy[b, :ty[b]].cpu().numpy(), acy) and not bool(cy[b, ty[b]:].any())
        assert np.array_equal(out[b], aout), (name, out[b], aout)                                   # bit for bit
        assert plen[b] == len(apath) and np.array_equal(path[b, :plen[b]], apath) and (path[b, plen[b]:] == -1).all()
        full = np.full((1, tx[b] + ty[b] - 1, 2), -1, np.int32)
        full[0, :len(apath)] = apath
        alone = metrics.path_f0_stats_dev(_t(full), _t([len(apath)], torch.int32), _t(f0[b][0])[None], _t(f0[b][1])[None])[0].cpu().numpy()
        assert np.array_equal(stats[b], alone, equal_nan=True), (name, stats[b], alone)
        _stats_close(stats[b].tolist(), R.f0_stats(r['path'], *f0[b]), name)


def test_out_of_contract_lengths_spoil_their_own_row_only():
    names = ['features_u0_u1_c24', 'warped_65x70', 'demo_R_F', 'warped_70x63']
    mx, tx, my, ty = _ragged_batch(names, nan=False)
    good = _run_batch(mx, tx, my, ty, poison=False)
    bad_tx, bad_ty = [tx[0], 0, 100000, tx[3]], [ty[0], -7, ty[2], ty[3]]
    bad = _run_batch(mx, bad_tx, my, bad_ty, poison=False)
    for b in (0, 3):
        assert np.array_equal(good[1][b], bad[1][b]) and np.array_equal(good[2][b], bad[2][b]) and good[3][b] == bad[3][b]
    assert bad[3][1] == 1 and bad[2][1, 0].tolist() == [0, 0] and (bad[2][1, 1:] == -1).all()        # clamped to one frame each
    Tx = mx.shape[1]                                                                       # clamped to max_tx: the row's zero padding joins in
    assert max(Tx, ty[2]) <= bad[3][2] <= Tx + ty[2] - 1 and bad[2][2, bad[3][2] - 1].tolist() == [Tx - 1, ty[2] - 1]
    assert np.isfinite(bad[1]).all()


def test_two_runs_give_the_same_bits():
    mx, tx, my, ty = _ragged_batch(RAGGED)
    f0x, f0y = _f0_tracks(max(tx), max(ty), 9)
    a = _run_batch(mx, tx, my, ty, np.tile(f0x, (5, 1)), np.tile(f0y, (5, 1)))
    b = _run_batch(mx, tx, my, ty, np.tile(f0x, (5, 1)), np.tile(f0y, (5, 1)))
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1])
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v, equal_nan=True)


def test_containment_of_all_three_calls():
    """outputs, path and scratch sit between bands of guard memory that must come back unchanged; inputs sit between NaN guards that must not
    reach a result; every output element must have been written"""
    lib = _capi.lib()
    ptr = lambda g: C.c_void_p(g.t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    names = ['warped_65x70', 'features_u0_u1_c24', 'warped_1x5']
    mx, tx, my, ty = _ragged_batch(names)
    B, Tx, Ty, nc = len(names), mx.shape[1], my.shape[1], 24
    dct = G.inp(R.dct_basis(nc, 80), DEV, name='dct')
    gmx, gmy = G.inp(mx, DEV, name='mel_x'), G.inp(my, DEV, name='mel_y')
    gtx, gty = G.inp(np.array(tx, np.int32), DEV, name='tx'), G.inp(np.array(ty, np.int32), DEV, name='ty')
    gcx = G.out((B, Tx, nc), DEV, dtype=torch.float64, name='cepstra_x')
    gcy = G.out((B, Ty, nc), DEV, dtype=torch.float64, name='cepstra_y')
    _capi.check(lib.ss_mel_cepstra(ptr(gmx), ptr(gtx), B, Tx, 80, ptr(dct), nc, ptr(gcx), stream))
    _capi.check(lib.ss_mel_cepstra(ptr(gmy), ptr(gty), B, Ty, 80, ptr(dct), nc, ptr(gcy), stream))
    torch.cuda.synchronize()
    G.check_all([dct, gmx, gmy, gtx, gty, gcx, gcy])
    # the DTW reads guarded copies of the cepstra with NaN behind every length
    cx, cy = gcx.t.clone(), gcy.t.clone()
    for b in range(B):
        cx[b, tx[b]:], cy[b, ty[b]:] = float('nan'), float('nan')
    gfx, gfy = G.inp(cx, DEV, name='fx'), G.inp(cy, DEV, name='fy')
    nbytes = lib.ss_dtw_scratch_bytes(B, Tx, Ty)
    gout = G.out((B, 3), DEV, dtype=torch.float64, name='dtw_out')
    gpath = G.out((B, Tx + Ty - 1, 2), DEV, dtype=torch.int32, name='path')
    gplen = G.out((B,), DEV, dtype=torch.int32, name='path_len')
    gscr = G.out((nbytes,), DEV, dtype=torch.uint8, offset=256, name='scratch')
    assert gscr.t.data_ptr() % 256 == 0
    _capi.check(lib.ss_dtw(ptr(gfx), ptr(gtx), ptr(gfy), ptr(gty), B, Tx, Ty, nc, R.SCALE, ptr(gout), ptr(gpath), ptr(gplen), ptr(gscr),
                           nbytes, stream))
    torch.cuda.synchronize()
    G.check_all([gfx, gfy, gtx, gty, gout, gpath, gplen])
    gscr.check(written=False)                                                              # bytes: the bands only
    for b, n in enumerate(names):
        r = _reference(n)
        P = int(gplen.t[b])
        assert P == len(r['path']) and np.array_equal(gpath.t[b, :P].cpu().numpy(), r['path'])
        assert abs(float(gout.t[b, 0]) - r['total']) <= min(1e-9, 100 * r['two_orders']) * r['total']
    # totals only: no path, no length
    gout2 = G.out((B, 3), DEV, dtype=torch.float64, name='dtw_out_no_path')
    _capi.check(lib.ss_dtw(ptr(gfx), ptr(gtx), ptr(gfy), ptr(gty), B, Tx, Ty, nc, R.SCALE, ptr(gout2), None, None, ptr(gscr), nbytes, stream))
    torch.cuda.synchronize()
    G.check_all([gout2, gpath, gplen])
    gscr.check(written=False)
    assert torch.equal(gout2.t, gout.t)
    # F0 statistics along the stored path
    f0x, f0y = np.full((B, Tx), np.nan), np.full((B, Ty), np.nan)
    for b in range(B):
        f0x[b, :tx[b]], f0y[b, :ty[b]] = _f0_tracks(tx[b], ty[b], 30 + b)
    gf0x, gf0y = G.inp(f0x, DEV, name='f0x'), G.inp(f0y, DEV, name='f0y')
    gpin, gplin = G.inp(gpath.t.clone(), DEV, name='path_in'), G.inp(gplen.t.clone(), DEV, name='path_len_in')
    gst = G.out((B, 5), DEV, dtype=torch.float64, name='stats')
    _capi.check(lib.ss_path_f0_stats(ptr(gpin), ptr(gplin), ptr(gf0x), ptr(gf0y), B, Tx, Ty, ptr(gst), stream))
    torch.cuda.synchronize()
    G.check_all([gf0x, gf0y, gpin, gplin])
    gst.check(written=False)                                                               # a statistic may rightly be NaN; the bands must hold
    for b, n in enumerate(names):
        _stats_close(gst.t[b].cpu().tolist(), R.f0_stats(_reference(n)['path'], f0x[b, :tx[b]], f0y[b, :ty[b]]), n)


def test_mcd_dtw_end_to_end_whatever_max_rows():
    names = ['features_u0_u1_c24', 'warped_150x170', 'demo_R_F', 'warped_1x5', 'warped_64x70', 'demo_F_RFU']
    xs, ys = [CASES[n][0] for n in names], [CASES[n][1] for n in names]
    f0 = [_f0_tracks(len(x), len(y), 40 + n) for n, (x, y) in enumerate(zip(xs, ys))]
    runs = [metrics.mcd_dtw(xs, ys, [f[0] for f in f0], [f[1] for f in f0], max_rows=m, device=DEV, return_paths=True) for m in (1, 4, 16)]
    for n, name in enumerate(names):
        r, got = _reference(name), runs[0][n]
        for other in runs[1:]:                                                             # bit for bit, whatever the batching
            assert all(np.array_equal(other[n][k], got[k], equal_nan=True) for k in got), name
        assert np.array_equal(got['path'], r['path']) and got['path_len'] == len(r['path'])
        assert abs(got['total'] - r['total']) <= min(1e-9, 100 * r['two_orders']) * r['total']
        assert got['mcd_db'] == got['total'] / got['path_len']
        want = R.f0_stats(r['path'], *f0[n])
        _stats_close([got['n_voiced'], want[1], got['f0_rmse_cents'], got['f0_corr'], got['vuv_error']], want, name)
    one = metrics.mcd_dtw(xs[0], ys[0], device=DEV)
    assert isinstance(one, dict) and one == {k: runs[0][0][k] for k in ('mcd_db', 'total', 'path_len')}


def test_conversion_scores_on_the_demo_conversion():
    """every condition of the golden conversion against the pitch-converted mel of the source's rhythm: five lattices of 135 x 135 (one of
    them out_F with itself: distortion 0 along the diagonal) and none of 105 x 135 is left out"""
    results = [('p_' + c, GOLD['out_' + c]) for c in convert.CONDITIONS]
    targets = [GOLD['out_F']] * len(results)
    dct = R.dct_basis(24, 80)
    got = convert.conversion_scores(results, targets, device=DEV, return_paths=True)
    assert [n for n, _ in got] == [n for n, _ in results]
    for (name, mel), (_, s) in zip(results, got):
        cx, cy = R.cepstra(mel, dct), R.cepstra(GOLD['out_F'], dct)
        total, path, mcd = R.dtw(cx, cy)
        assert R.path_margin(cx, cy) >= MARGIN, name
        print(f'{name}: mcd {s["mcd_db"]:.4f} dB over {s["path_len"]} steps (reference {mcd:.4f})')
        assert np.array_equal(s['path'], path) and s['path_len'] == len(path)
        assert abs(s['total'] - total) <= min(1e-9, 100 * R.two_orders(cx, cy)) * max(total, 1e-300)
    assert dict(got)['p_F']['total'] == 0.0 and dict(got)['p_F']['path_len'] == 135
    nested = convert.conversion_scores([results[:3], results[3:]], [targets[:3], targets[3:]], device=DEV, max_rows=2)
    assert [[n for n, _ in p] for p in nested] == [[n for n, _ in results[:3]], [n for n, _ in results[3:]]]
    assert [s['total'] for p in nested for _, s in p] == [s['total'] for _, s in got]
