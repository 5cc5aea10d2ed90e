"""The waveform scores on the GPU (csrc/stoi.hip: ss_stoi and its two test hooks) against the float64 numpy restatement tests/stoi_ref.py,
which tests/test_stoi_ref_selftest.py checks on its own.

Inputs.  features.npz's two recordings brought to 10 kHz (scipy's resample_poly, which the device resampler equals to the bit), two
stretches behind sample 4096 scaled by 1e-3 and 3e-3 so that the mask removes frames, y = x gated plus noise (stoi_ref.make_pair); and the
smallest cases: their first 4096 samples (31 frames, all kept, ONE segment), 3968 (30 frames: no segment, NaN) and 256 (one frame).

Bounds.  The mask is a threshold: the inverse map and K must be the reference's exactly, which is a fair demand only where the reference's
own min_f |e_f - (max - 40)| is far from rounding -- asserted on the CPU first, at 1e-6 dB.  x' and y' are two products and one add:
within 4 ulp, the ulp taken at the larger product (stoi_ref.overlap_scale).  Envelopes (max norm, relative) and scores (absolute; they are
of order one) are held to min(1e-9, 100 x the reference's own disagreement between its two summation orders on that input), a
disagreement below 2^-52 counting as 2^-52.  S, K and NaN-ness are exact.  A row in a ragged batch must have the bits it has alone.

Measured on an MI355X, worst over all cases (every run prints the figures): frame levels, inverse map, K, x' and y' equal to the
reference's to the bit (0 ulp, 0 dB); envelopes 1.14e-15 of the largest (the reference's two orders: 7.1e-16 .. 1.14e-15, so bounds of
7.1e-14 .. 1.14e-13); scores 3.6e-16 from the reference's (two orders 5.6e-17 .. 2.8e-16, bounds 2.2e-14 .. 2.8e-14); mask margins
0.47 dB (u0), 3.6 .. 3.7 dB (the rest), 0.064 dB or more on the end-to-end pairs.  The whole file runs in 4 s.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from scipy import signal

import guarded as G
import stoi_ref as R
from speechsplit_amd import _capi, convert, metrics

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MARGIN_DB = 1e-6
NAN = float('nan')


def _recordings():
    f = np.load(os.path.join(GOLDEN, 'features.npz'))
    return {k: f[k + '_wav'].astype(np.float64) for k in ('u0', 'u1')}


WAV16 = _recordings()
PAIRS = {}
for _k, _seed in (('u0', 1), ('u1', 2)):
    _x, _y = R.make_pair(signal.resample_poly(WAV16[_k], 5, 8), _seed)
    PAIRS[_k] = (_x, _y)
    PAIRS[_k + '_4096'] = (_x[:4096].copy(), _y[:4096].copy())
PAIRS['u0_3968'] = (PAIRS['u0'][0][:3968].copy(), PAIRS['u0'][1][:3968].copy())
PAIRS['u1_256'] = (PAIRS['u1'][0][:256].copy(), PAIRS['u1'][1][:256].copy())
SCORED = ('u0', 'u1', 'u0_4096', 'u1_4096')
REF = {}                                               # name -> reference; computed once, never changed


def _reference(name):
    if name not in REF:
        x, y = PAIRS[name]
        a, b = R.both_modes(x, y, 'loop'), R.both_modes(x, y, 'numpy')
        assert a['K'] == b['K'] and np.array_equal(a['inv'], b['inv'])
        env = max((float(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()) for k in ('X', 'Y')), default=0.0) if a['X'].size else 0.0
        a['env_orders'] = env
        a['score_orders'] = {e: (abs(a['score'][e] - b['score'][e]) if a['S'] >= 1 else 0.0) for e in (False, True)}
        a['margin'] = R.mask_margin(x)
        REF[name] = a
    return REF[name]


def _bound(two_orders):
    return min(1e-9, 100.0 * max(two_orders, 2.0 ** -52))


def test_conditions_hold_on_the_cpu_reference():
    """not measurements: what makes 'the mask, exactly' a fair demand, and that the cases are the cases the module says they are"""
    for name in PAIRS:
        r = _reference(name)
        assert r['margin'] > MARGIN_DB, (name, r['margin'])
    for name in ('u0', 'u1'):
        r = _reference(name)
        assert r['K'] < r['F'] - 3 and r['S'] >= 2, (name, r['K'], r['F'], r['S'])       # the mask removes frames, several segments
    for name in ('u0_4096', 'u1_4096'):
        r = _reference(name)
        assert (r['F'], r['K'], r['S']) == (31, 31, 1), name
    r = _reference('u0_3968')
    assert (r['F'], r['K'], r['S']) == (30, 30, 0) and math.isnan(r['score'][False]) and math.isnan(r['score'][True])
    r = _reference('u1_256')
    assert (r['F'], r['K'], r['S']) == (1, 1, 0)
    assert metrics.stoi_bands() == (list(R.LO), list(R.HI))
    print('margins (dB):', {n: round(REF[n]['margin'], 3) for n in PAIRS})
    print('two orders, score:', {n: REF[n]['score_orders'] for n in SCORED}, 'envelopes:', {n: REF[n]['env_orders'] for n in SCORED})


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _alone(name, extended):
    x, y = PAIRS[name]
    out = metrics.stoi_dev(_t(x)[None], _t(y)[None], None, extended)
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


@pytest.mark.parametrize('name', list(PAIRS))
def test_mask_and_compaction_against_the_reference(name):
    x, y = PAIRS[name]
    r = _reference(name)
    e, inv, k, xp, yp = metrics.stoi_compact_dev(_t(x)[None], _t(y)[None], None)
    torch.cuda.synchronize()
    e, inv, K = e[0].cpu().numpy(), inv[0].cpu().numpy(), int(k[0])
    assert e.shape == (r['F'],) and float(np.abs(e - r['e']).max()) < 1e-9                 # dB; the decision has MARGIN_DB to spare
    assert K == r['K'] and np.array_equal(inv[:K], r['inv']) and bool((inv[K:] == -1).all())
    L = 128 * (K - 1) + 256
    worst = 0.0
    for got, key, src in ((xp, 'xp', x), (yp, 'yp', y)):
        got = got[0].cpu().numpy()
        assert got.shape == (128 * (r['F'] - 1) + 256,) and bool((got[L:] == 0.0).all())
        ulp = np.spacing(np.maximum(R.overlap_scale(src, r['inv']), np.finfo(np.float64).tiny))
        err = np.abs(got[:L] - r[key]) / ulp
        worst = max(worst, float(err.max()))
    print(f'{name}: x\' / y\' worst error {worst:.2f} ulp, levels {float(np.abs(e - r["e"]).max()):.2e} dB')
    assert worst <= 4.0, (name, worst)


@pytest.mark.parametrize('name', SCORED + ('u0_3968',))
def test_envelopes_against_the_reference(name):
    """the transform stage alone, on the REFERENCE's x' and y' as a ragged batch of two with NaN behind both"""
    r = _reference(name)
    L = r['xp'].shape[0]
    sig = np.full((2, L + 130), NAN)
    sig[0, :L], sig[1, :L] = r['xp'], r['yp']
    env = metrics.stoi_envelopes_dev(_t(sig), _t([L, L], torch.int32)).cpu().numpy()
    M = r['X'].shape[1]
    assert env.shape == (2, 15, M + 1 + 1) and bool((env[:, :, M:] == 0.0).all())
    bound = _bound(r['env_orders'])
    for row, key in ((0, 'X'), (1, 'Y')):
        err = float(np.abs(env[row, :, :M] - r[key]).max() / np.abs(r[key]).max())
        print(f'{name} {key}: envelopes {err:.3e} (bound {bound:.3e}, the reference\'s two orders {r["env_orders"]:.3e})')
        assert err <= bound, (name, key, err, bound)


@pytest.mark.parametrize('extended', (False, True))
@pytest.mark.parametrize('name', list(PAIRS))
def test_score_against_the_reference(name, extended):
    r = _reference(name)
    out = _alone(name, extended)
    assert int(out[1]) == r['S'] and int(out[2]) == r['K'], (name, out, r['S'], r['K'])
    if r['S'] < 1:
        assert math.isnan(out[0])
        return
    bound = _bound(r['score_orders'][extended])
    err = abs(float(out[0]) - r['score'][extended])
    print(f'{name} extended={extended}: score {out[0]:.15f}, error {err:.3e} (bound {bound:.3e}, two orders {r["score_orders"][extended]:.3e})')
    assert err <= bound, (name, extended, err, bound)


def _ragged(names, fill=NAN):
    n = [PAIRS[k][0].shape[0] for k in names]
    bx, by = np.full((len(names), max(n)), fill), np.full((len(names), max(n)), fill)
    for r, k in enumerate(names):
        bx[r, :n[r]], by[r, :n[r]] = PAIRS[k]
    return bx, by, n


@pytest.mark.parametrize('extended', (False, True))
def test_a_ragged_batch_gives_each_pair_alone_to_the_bit_twice(extended):
    """every length above in one batch, NaN behind every row; run twice"""
    names = list(PAIRS)
    bx, by, n = _ragged(names)
    runs = []
    for _ in range(2):
        out = metrics.stoi_dev(_t(bx), _t(by), _t(n, torch.int32), extended)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    for r, k in enumerate(names):
        alone = _alone(k, extended)
        assert np.array_equal(np.isnan(runs[0][r]), np.isnan(alone)), k
        keep = ~np.isnan(alone)
        assert np.array_equal(_bits(runs[0][r][keep]), _bits(alone[keep])), (k, runs[0][r], alone)


def test_a_length_outside_the_contract_spoils_its_row_only():
    names = ['u1', 'u0_4096', 'u0']
    bx, by, n = _ragged(names)
    good = metrics.stoi_dev(_t(bx), _t(by), _t(n, torch.int32)).cpu().numpy()
    for bad in (0, -7, 2 ** 31 - 1):
        out = metrics.stoi_dev(_t(np.nan_to_num(bx)), _t(np.nan_to_num(by)), _t([n[0], bad, n[2]], torch.int32)).cpu().numpy()
        assert np.array_equal(_bits(out[[0, 2]]), _bits(good[[0, 2]])), bad
    assert math.isnan(metrics.stoi_dev(_t(np.nan_to_num(bx)), _t(np.nan_to_num(by)), _t([n[0], 0, n[2]], torch.int32)).cpu().numpy()[1, 0])


def test_guarded_slabs_with_nan_behind_every_row():
    """inputs in guarded slabs (NaN around them, in the row gaps and behind every row's own samples), outputs and scratch guarded too"""
    lib = _capi.lib()
    names = list(PAIRS)
    bx, by, n = _ragged(names)
    B, max_n = bx.shape
    gn = G.inp(torch.tensor(n, dtype=torch.int32), DEV, name='n')
    nbytes = lib.ss_stoi_scratch_bytes(B, max_n)
    gs = G.out((nbytes // 8,), DEV, dtype=torch.float64, name='scratch')
    lo, hi = metrics.stoi_bands()
    ilo, ihi = (C.c_int * 15)(*lo), (C.c_int * 15)(*hi)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ext in (0, 1):
        cx, cy = G.inp(bx, DEV, name='x'), G.inp(by, DEV, name='y')
        go = G.out((B, 3), DEV, dtype=torch.float64, name='out')
        assert gs.t.data_ptr() % 256 == 0
        _capi.check(lib.ss_stoi(C.c_void_p(cx.t.data_ptr()), C.c_void_p(cy.t.data_ptr()), C.c_void_p(gn.t.data_ptr()), B, max_n, ilo, ihi, 15,
                                ext, C.c_void_p(go.t.data_ptr()), C.c_void_p(gs.t.data_ptr()), nbytes, stream))
        torch.cuda.synchronize()
        G.check_all([cx, cy, gn])
        gs.check(written=False)
        out = go.t.cpu().numpy()
        for r, k in enumerate(names):
            alone = _alone(k, bool(ext))
            keep = ~np.isnan(alone)
            assert np.array_equal(np.isnan(out[r]), np.isnan(alone)) and np.array_equal(_bits(out[r][keep]), _bits(alone[keep])), k
        go.check()                                                                         # a NaN score is not the guard's NaN
    # the hooks' outputs
    F = metrics.stoi_frames(max_n)
    L = 128 * (F - 1) + 256
    cx, cy = G.inp(bx, DEV, name='x'), G.inp(by, DEV, name='y')
    ge, gi, gk = G.out((B, F), DEV, dtype=torch.float64, name='e'), G.out((B, F), DEV, dtype=torch.int32, name='inv'), \
        G.out((B,), DEV, dtype=torch.int32, name='k')
    gxp, gyp = G.out((B, L), DEV, dtype=torch.float64, name='xp'), G.out((B, L), DEV, dtype=torch.float64, name='yp')
    _capi.check(lib.ss_op_stoi_compact(C.c_void_p(cx.t.data_ptr()), C.c_void_p(cy.t.data_ptr()), C.c_void_p(gn.t.data_ptr()), B, max_n, 0,
                                       *[C.c_void_p(g.t.data_ptr()) for g in (ge, gi, gk, gxp, gyp)], stream))
    torch.cuda.synchronize()
    G.check_all([cx, cy, gn, ge, gi, gk, gxp, gyp])
    lens = (128 * (gk.t.cpu().numpy() - 1) + 256).astype(np.int32)
    M = -(-(L - 256) // 128)
    gl = G.inp(torch.from_numpy(lens), DEV, name='len')
    sig = gxp.t.clone()
    for r in range(B):
        sig[r, int(lens[r]):] = NAN
    gsig = G.inp(sig, DEV, name='sig')
    genv = G.out((B, 15, M), DEV, dtype=torch.float64, name='env')
    _capi.check(lib.ss_op_stoi_bands(C.c_void_p(gsig.t.data_ptr()), C.c_void_p(gl.t.data_ptr()), B, L, ilo, ihi, 15,
                                     C.c_void_p(genv.t.data_ptr()), stream))
    torch.cuda.synchronize()
    G.check_all([gsig, gl, genv])
    assert bool(torch.isfinite(genv.t).all())


def test_a_corrupt_map_changes_numbers_never_addresses():
    """the gather through a map and a K that hold garbage: every index is clamped into the row's own frames, so the inputs' guards (and the
    NaN behind every row) are never read, the outputs' guards never written, and the result is the gather through the clamped map"""
    lib = _capi.lib()
    names = ['u0', 'u1_256', 'u1']
    bx, by, n = _ragged(names)
    B, max_n = bx.shape
    F = metrics.stoi_frames(max_n)
    L = 128 * (F - 1) + 256
    rng = np.random.RandomState(7)
    inv = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(B, F)).astype(np.int32)
    inv[:, ::3] = rng.randint(0, 80, size=inv[:, ::3].shape)
    ks = np.array([2 ** 31 - 1, -5, 17], dtype=np.int32)
    cx, cy = G.inp(bx, DEV, name='x'), G.inp(by, DEV, name='y')
    gn, gi, gk = G.inp(torch.tensor(n, dtype=torch.int32), DEV, name='n'), G.inp(torch.from_numpy(inv), DEV, name='inv'), \
        G.inp(torch.from_numpy(ks), DEV, name='k')
    gxp, gyp = G.out((B, L), DEV, dtype=torch.float64, name='xp'), G.out((B, L), DEV, dtype=torch.float64, name='yp')
    _capi.check(lib.ss_op_stoi_compact(C.c_void_p(cx.t.data_ptr()), C.c_void_p(cy.t.data_ptr()), C.c_void_p(gn.t.data_ptr()), B, max_n, 1, None,
                                       C.c_void_p(gi.t.data_ptr()), C.c_void_p(gk.t.data_ptr()), C.c_void_p(gxp.t.data_ptr()),
                                       C.c_void_p(gyp.t.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    G.check_all([cx, cy, gn, gi, gk, gxp, gyp])
    for r, k in enumerate(names):
        Fr = R.n_frames(n[r])
        K = int(np.clip(ks[r], 0, Fr))
        m = np.clip(inv[r, :K].astype(np.int64), 0, Fr - 1)
        for got, src in ((gxp.t[r].cpu().numpy(), PAIRS[k][0]), (gyp.t[r].cpu().numpy(), PAIRS[k][1])):
            want = R.overlap_add(src, m)
            assert bool(np.isfinite(got).all()) and bool((got[want.shape[0]:] == 0.0).all())
            if not want.size:
                continue
            ulp = np.spacing(np.maximum(R.overlap_scale(src, m), np.finfo(np.float64).tiny))
            assert float((np.abs(got[:want.shape[0]] - want) / ulp).max()) <= 4.0, k


def _pipeline(ref16, deg16, extended):
    n = min(len(ref16), len(deg16))
    x, y = signal.resample_poly(ref16[:n], 5, 8), signal.resample_poly(deg16[:n], 5, 8)
    a, b = R.stoi(x, y, extended, 'loop'), R.stoi(x, y, extended, 'numpy')
    return a, (abs(a['score'] - b['score']) if a['S'] >= 1 else 0.0), R.mask_margin(x)


def test_metrics_stoi_and_conversion_stoi_end_to_end():
    """16 kHz in: cutting to the shorter, the device resampler, ragged batches -- against scipy's resampler and the numpy restatement"""
    refs, degs = [], []
    for k, seed in (('u0', 11), ('u1', 12)):
        x, y = R.make_pair(WAV16[k], seed)
        refs.append(x)
        degs.append(y)
    refs.append(refs[0][:9000])                                                           # a pair of unequal lengths
    degs.append(degs[0][:8000])
    refs.append(refs[1][:300])                                                            # too short for a frame at 10 kHz
    degs.append(degs[1][:300])
    for extended in (False, True):
        got = metrics.stoi(refs, degs, sr=16000, extended=extended, max_rows=16, device=DEV)
        one = metrics.stoi(refs, degs, sr=16000, extended=extended, max_rows=1, device=DEV)
        assert [(_bits(g['stoi']).tolist(), g['segments'], g['frames_kept'], g['frames']) for g in got] == \
            [(_bits(g['stoi']).tolist(), g['segments'], g['frames_kept'], g['frames']) for g in one]
        for i, g in enumerate(got):
            ref, orders, margin = _pipeline(refs[i], degs[i], extended)
            assert margin > MARGIN_DB
            assert (g['segments'], g['frames_kept'], g['frames']) == (ref['S'], ref['K'], ref['F']), (i, g)
            if ref['S'] < 1:
                assert math.isnan(g['stoi'])
                continue
            err = abs(g['stoi'] - ref['score'])
            print(f'pair {i} extended={extended}: {g["stoi"]:.15f}, error {err:.3e} (bound {_bound(orders):.3e})')
            assert err <= _bound(orders), (i, extended, err)
        assert _bits(metrics.stoi(refs[0], degs[0], extended=extended, device=DEV)['stoi']) == _bits(got[0]['stoi'])
        waves = [[('F', degs[0]), ('U', degs[2])], [('FU', degs[1])]]
        nested = convert.conversion_stoi(waves, [[refs[0], refs[2]], [refs[1]]], extended=extended, device=DEV)
        assert [[name for name, _ in p] for p in nested] == [['F', 'U'], ['FU']]
        assert [_bits(s['stoi']).tolist() for p in nested for _, s in p] == [_bits(got[i]['stoi']).tolist() for i in (0, 2, 1)]
    at10k = metrics.stoi(PAIRS['u0'][0], PAIRS['u0'][1], sr=10000, device=DEV)
    assert _bits(at10k['stoi']) == _bits(_alone('u0', False)[0])
