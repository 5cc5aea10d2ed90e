"""The audio kernels at utterance length, past their first chunk: pytest -m gpu.  The per-kernel files (test_gpu_harmonic.py, test_gpu_stoi.py,
test_gpu_pitch.py, test_gpu_pitch_stat.py, test_gpu_features_batch.py, test_gpu_vocoder.py) feed rows of at most 49 frames, so every loop
below made one trip there and every frame index stayed under 49.  The inputs are long_inputs.py's; test_long_inputs_selftest.py asserts
their conditions on the CPU and shows that each carried-state mistake named below changes the result on them and on none of the short ones.
References, bars and the shape of every assertion are the per-kernel files' own: nothing here has a tolerance of its own.

What is driven past its first chunk, by which input:

    harmonic_u_kernel (vocoder.hip)   `for i0 = 0; i0 < max_frames; i0 += 64` and `carry` across it.  Crafted tracks of 63, 64, 65, 127,
                                      128, 129, 200 and 1000 frames: a glide voiced throughout (the carry crosses frames 63 -> 64, 127 -> 128,
                                      ..), the glide with frame 62, 63, 64 or 65 unvoiced (a reset before, on and after the edge), alternating
                                      and all-unvoiced tracks; a ragged batch with frames = 64, 65, 128, 200 of max_frames = 200; long16's
                                      own track (177 frames, a voiced run across frame 64, one starting at 128).  u to the bit.
    mel_harmonic_kernel, harmonic_phase_kernel   frame indices 49 .. 176 (`fr * NBIN`): long16's mel and track at 0 and 2 fit rounds.
    energy_kernel (stoi.hip)          blockIdx.x >= 1 (frames from 256 on): the 257-, 258- and 681-frame pairs of long10.
    mask_kernel                       `for f0 = 0; f0 < F; f0 += 256` and `base` across it: one chunk exactly (f256), one frame and two
                                      frames into the second (f257, f258: both dropped, the second chunk writes nothing; k257, k258: both
                                      kept, it writes one and two slots behind `base`), three chunks with frames dropped in each (whole:
                                      109 + 109 + 18 kept of 681).  The max loop `for f = tid; f < F; f += 256` makes its second and third
                                      trip on the same inputs.
    compact_kernel, bands_kernel, segment_kernel   sample, frame and segment indices to 30 336, 235 and 206.
    final_kernel                      blockIdx.x == 1 (rows 64 .. 71): a batch of 72 rows, every row from 64 on with one segment.
    nccf_kernel, cand_kernel, stat_kernel   frame indices 49 .. 176 (`fr * K`, `fr * NST`): long16 in (50, 250) and (100, 600).
    dp_kernel                         recurrence and backtrack over 177 frames; the fill `for i = F + lane; i < max_frames; i += 64` makes
                                      three trips behind the 513-sample row of a 45 172-sample batch (174 frames to fill).
    filtfilt_kernel (filtfilt.hip)    blocks of CH = 256 steps over N = n + 36, groups of FG = 8 with a read-ahead, and the tail loop:
                                      N = 767, 768, 769, 775, 776, 777, 1024 (last blocks of 255, 256, 1, 7, 8, 9 and 256 steps; 768 and 1024
                                      end a pass on a block edge with an odd and an even block count) and 45 206 (177 blocks).
    stft_kernel, irfft_kernel, ola_kernel, gl_init_kernel and the Griffin-Lim loop   frame indices 49 .. 176: long16's first 45 056 samples.

Bars, each the per-kernel file's: u, the filter, the STOI levels' decisions, inverse map and K, and a row alone against the row in a batch are
equal to the bit; NCCF, stationarity, STOI envelopes and scores, the harmonic fit and Griffin-Lim are held to min(1e-9, 100 x the
reference's own two-order disagreement on that input); STFT / ISTFT to 1e-12 of the largest element; tracks to the same voiced pattern and
1e-10 relative; STOI's x' / y' to 4 ulp.

Measured on an MI355X in one run (profiles/r05/long_audio/test_figures.txt; figures, not bars):
    harmonic u       numpy's bits on the 56 crafted tracks (63 .. 1000 frames, up to 16 trips), the ragged batch and long16's track
    harmonic fit     long16, 177 frames, 171 voiced.  n_iter 0: S 3.0e-16 of max |S| (two orders 5.9e-16), share 0, phase0 5.6e-16;
                     n_iter 2: S 5.0e-16 (3.3e-16), share 3.4e-14 (2.8e-14), phase0 on one share 4.4e-15 (two orders 1.6e-12)
    STOI             pair    F / K / S         kept a chunk     mask margin   envelopes (two orders)   score error, worst of both modes
                     f256    256 / 100 / 70    100              9.9 dB        1.08e-15 (1.08e-15)      1.7e-16
                     f257    257 / 101 / 71    101, 0           9.9 dB        1.22e-15 (1.22e-15)      1.8e-16
                     f258    258 / 102 / 72    102, 0           9.9 dB        1.22e-15 (1.22e-15)      1.5e-16
                     whole   681 / 236 / 206   109, 109, 18     0.81 dB       1.22e-15 (1.22e-15)      8.3e-17
                     k257    257 / 119 / 89    118, 1           3.2 dB        8.1e-16 (8.1e-16)        2.5e-16
                     k258    258 / 122 / 92    120, 2           4.4 dB        8.1e-16 (8.1e-16)        2.2e-16
                     levels within 1.4e-14 dB, map and K exact, x' / y' 0 ulp; the ragged batch of six and all 72 rows their runs alone
    pitch            range       NCCF phi (two orders)   path margin   gap       voiced     track, relative
                     (50, 250)   3.7e-15 (4.1e-15)       4.97e-4       7.8e-4    171 / 177  2.6e-15; the hooks 2.2e-16: frame 141, one ulp of log
                     (100, 600)  1.8e-15 (1.8e-15)       8.4e-4        1.16e-3   169 / 177  6.7e-16; the hooks to the bit
                     stationarity 1.05e-12 (two orders 1.56e-12); 174, 112 and 59 frames filled behind the ragged rows
    filter           to the bit on N = 767, 768, 769, 775, 776, 777, 1024 and 45 206 (177 blocks), plain and with gain and dither
    vocoder          177 frames: STFT 3.9e-16, ISTFT 5.4e-16, istft(stft(x)) - x 4.3e-16; Griffin-Lim 1.1e-15 (0 rounds), 5.6e-14 (1),
                     2.9e-13 (8) against a bound of 1.67e-10 (fft against dft at 8 rounds 1.67e-12)
    wall time        56 tests in 4.9 s; the slowest 0.36 s (the first NCCF: it computes the references), nine more above 0.1 s

Every test prints its figures before it asserts."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import filtfilt_ref as FR
from tests import griffinlim_ref as GL
from tests import harmonic_ref as H
from tests import long_inputs as L
from tests import nnls_ref as NN
from tests import pitch_ref as P
from tests import pitch_stat_ref as Q
from tests import stoi_ref as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
M, W_ = L.M_RANGE, L.W_RANGE
RANGES = [M, W_]
RANGE_IDS = ['50-250', '100-600']
SCALE = L.SCALE
MARGIN_FLOOR = 1e-6                                                     # test_gpu_pitch.py's and test_gpu_stoi.py's
VALUE_TOL = 1e-10                                                       # test_gpu_pitch.py's
HOOK_TOL = 1e-12                                                        # test_gpu_vocoder.py's
FLOOR, F_TOP = 1e-10, 7600.0                                            # test_gpu_harmonic.py's
FIT_ROUNDS = (0, 2)                                                     # a few rounds: the numpy side of 171 voiced frames stays short
GL_ROUNDS = (0, 1, 8)


@pytest.fixture(scope='module')
def lib():
    from speechsplit_amd import _capi
    return _capi.lib()


@pytest.fixture(scope='module')
def V():
    from speechsplit_amd import vocoder
    return vocoder


@pytest.fixture(scope='module')
def metrics():
    from speechsplit_amd import metrics
    return metrics


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a)).to(device=DEV, dtype=dtype)         # a copy: the references are read-only


def _ints(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _check(lib, rc):
    assert rc == 0, lib.ss_last_error()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rows(sigs, width, fill, dtype=np.float64):
    """[len(sigs), width, ...] with each array at the head of its row and `fill` behind it"""
    out = np.full((len(sigs), width) + sigs[0].shape[1:], fill, dtype)
    for b, x in enumerate(sigs):
        out[b, :x.shape[0]] = x
    return out


def _plus_zeros(a):
    return not a.any() and not np.signbit(a).any()


def _bound(two_orders):
    return min(1e-9, 100.0 * max(two_orders, 2.0 ** -52))                   # test_gpu_stoi.py's and harmonic_ref.gpu_bound's rule


# ============================================================================================== 1. the harmonic phase u, fit and start phases
def u_of(lib, hz, frames=None):
    B, T = hz.shape
    u = torch.full((B, T), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_harmonic_u(_p(hz), _p(frames), B, T, _p(u), _s()))
    return u.cpu().numpy()


@pytest.mark.parametrize('F', L.U_FRAMES)
def test_u_on_crafted_tracks_is_numpys_to_the_bit(lib, F):
    for kind in L.U_KINDS:
        hz = L.u_track(kind, F)
        want = H.phase_u(hz)
        got = u_of(lib, _dev(hz)[None])[0]
        bad = np.flatnonzero(_bits(got) != _bits(want))
        print(f'u, {kind}, {F} frames: {int(H.voiced(hz).sum())} voiced, {int((want != 0.0).sum())} non-zero u, trips of the 64-frame loop '
              f'{-(-F // 64)}, frames that differ {bad[:5].tolist()}')
        assert bad.size == 0, (kind, F, bad[:5])
        if kind == 'glide' and F > 64:
            assert want[64] != 0.0 and want[F - 1] != 0.0                # the carry is in use on the far side of the edge
        if kind in ('alternating', 'unvoiced'):
            assert _plus_zeros(got)


def test_u_ragged_batch_rows_are_the_tracks_alone(lib):
    """frames = 64, 65, 128, 200 in rows of max_frames = 200; behind a row's own frames a VOICED value (a kernel that read it would chain on
    it), then NaN: the rows are the tracks alone either way, with zeros of positive sign behind them"""
    lens = [F for F, _ in L.U_RAGGED]
    assert lens == [64, 65, 128, 200]
    tracks = [L.u_track(kind, F) for F, kind in L.U_RAGGED]
    for fill in (100.0, NAN):
        got = u_of(lib, _dev(_rows(tracks, 200, fill)), _ints(lens))
        for b, (hz, F) in enumerate(zip(tracks, lens)):
            alone = u_of(lib, _dev(hz)[None])[0]
            assert np.array_equal(_bits(got[b, :F]), _bits(alone)) and np.array_equal(_bits(alone), _bits(H.phase_u(hz))), (fill, b)
            assert _plus_zeros(got[b, F:]), (fill, b)
    print(f'u, ragged: frames {lens} of 200, every row its run alone, zeros behind')


class Basis:
    def __init__(self, B):
        self.B = np.ascontiguousarray(B, dtype=np.float64)
        self.P = np.linalg.pinv(self.B)
        self.packed = NN.pack(self.B)
        self.P_dev, self.packed_dev = _dev(self.P), _dev(self.packed)


@pytest.fixture(scope='module')
def bank():
    return Basis(L.feats()['mel_basis'])


@functools.lru_cache(maxsize=None)
def harmonic_reference():
    """test_gpu_harmonic.py's _reference on long16: per round count the kernel-order (S, share, phase0), the two-order disagreement, the bound"""
    mel, hz = L.long16_mel(), L.long16_track()
    H.conditions(hz)
    B = np.ascontiguousarray(L.feats()['mel_basis'], np.float64)
    Pinv = np.linalg.pinv(B)
    rand = np.random.default_rng(177).uniform(-np.pi, np.pi, (mel.shape[0], 513))
    ref = {}
    for it in FIT_ROUNDS:
        (S, w, ph), d = H.disagreement(mel, hz, B, Pinv, rand, it)
        assert d[0] <= H.DISAGREEMENT_CAP and d[1] <= H.DISAGREEMENT_CAP
        ref[it] = dict(S=S, share=w, phase0=ph, div=d, bound=tuple(H.gpu_bound(x) for x in d))
    return dict(mel=mel, hz=hz, rand=rand, ref=ref, u=H.phase_u(hz))


def fit(lib, basis, mel, hz, n_iter, frames=None):
    """mel float32 [B, T, 80], hz float64 [B, T] on the device -> (mag, share) numpy [B, T, 513], on the pseudo-inverse route's magnitude"""
    B, T, n = mel.shape
    mag = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_mel_to_linear(_p(mel), _p(basis.P_dev), _p(frames), B, T, n, FLOOR, _p(mag), _s()))
    share = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_mel_to_linear_harmonic(_p(mel), _p(hz), _p(basis.P_dev), _p(basis.packed_dev), basis.packed_dev.numel(), _p(frames),
                                              B, T, n, F_TOP, n_iter, FLOOR, _p(mag), _p(share), _s()))
    return mag.cpu().numpy(), share.cpu().numpy()


def phase(lib, hz, share, rand, frames=None):
    B, T = hz.shape
    nb = lib.ss_harmonic_phase_scratch_bytes(B, T)
    assert nb >= B * T * 8
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((B, T, 513), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_harmonic_phase(_p(hz), _p(share), _p(rand), _p(frames), B, T, F_TOP, _p(out), _p(scratch), nb, _s()))
    return out.cpu().numpy()


def test_harmonic_u_fit_and_phases_on_long16(lib, bank):
    """test_gpu_harmonic.py's _check at 177 frames: u to the bit; S, share and phase0 (on one and the same share) within the bound of
    this input's own two-order disagreement at every round count"""
    inp = harmonic_reference()
    v = H.voiced(inp['hz'])
    assert L.voiced_runs(v) == [(2, 47), (50, 77), (128, 47)]
    mel, hz, rand = _dev(inp['mel'], torch.float32)[None], _dev(inp['hz'])[None], _dev(inp['rand'])[None]
    got_u = u_of(lib, hz)[0]
    assert np.array_equal(_bits(got_u), _bits(inp['u'])), np.flatnonzero(got_u != inp['u'])[:5]
    assert inp['u'][64] != 0.0 and inp['u'][127] == 0.0 and inp['u'][128] == 0.0 and inp['u'][129] != 0.0
    for it in FIT_ROUNDS:
        ref = inp['ref'][it]
        S, w = fit(lib, bank, mel, hz, it)
        assert np.isfinite(S).all() and np.isfinite(w).all() and w.min() >= 0.0 and w.max() <= 1.0 and S.min() >= FLOOR
        dS, dw = H.rel_diff(S[0], ref['S']), H.abs_diff(w[0], ref['share'])
        on_ref = H.phase_diff(phase(lib, hz, _dev(ref['share'])[None], rand)[0], ref['phase0'])
        on_own = H.phase_diff(phase(lib, hz, _dev(w), rand)[0], H.harmonic_phase(inp['hz'], w[0], inp['rand']))
        print(f'long16 (177 frames, {int(v.sum())} voiced), n_iter {it}: S {dS:.3g} of max |S| (two orders {ref["div"][0]:.3g}, bound '
              f'{ref["bound"][0]:.3g}); share {dw:.3g} ({ref["div"][1]:.3g}, {ref["bound"][1]:.3g}); phase0 on the reference\'s share '
              f'{on_ref:.3g}, on its own {on_own:.3g} ({ref["div"][2]:.3g}, {ref["bound"][2]:.3g})')
        assert dS <= ref['bound'][0]
        assert dw <= ref['bound'][1]
        assert on_ref <= ref['bound'][2] and on_own <= ref['bound'][2]
        assert _plus_zeros(w[0, ~v])                                         # unvoiced frames, beyond frame 48 too: share 0


# ============================================================================================== 2. STOI
STOI_NAMES = tuple(L.STOI_CUTS)
STOI_REF = {}                                                            # name -> reference; computed once, never changed


def stoi_reference(name):
    """test_gpu_stoi.py's _reference on a pair of long10"""
    if name not in STOI_REF:
        x, y = L.stoi_pairs()[name]
        a, b = SR.both_modes(x, y, 'loop'), SR.both_modes(x, y, 'numpy')
        assert a['K'] == b['K'] and np.array_equal(a['inv'], b['inv'])
        a['env_orders'] = max(float(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()) for k in ('X', 'Y'))
        a['score_orders'] = {e: abs(a['score'][e] - b['score'][e]) for e in (False, True)}
        a['margin'] = SR.mask_margin(x)
        assert a['margin'] > MARGIN_FLOOR and (a['F'], a['K'], a['S']) == L.STOI_FKS[name], (name, a['margin'], a['F'], a['K'], a['S'])
        STOI_REF[name] = a
    return STOI_REF[name]


def _stoi_alone(metrics, x, y, extended):
    out = metrics.stoi_dev(_dev(x)[None], _dev(y)[None], None, extended)
    torch.cuda.synchronize()
    return out[0].cpu().numpy()


@pytest.mark.parametrize('name', STOI_NAMES)
def test_stoi_levels_map_and_compaction(metrics, name):
    x, y = L.stoi_pairs()[name]
    r = stoi_reference(name)
    e, inv, k, xp, yp = metrics.stoi_compact_dev(_dev(x)[None], _dev(y)[None], None)
    torch.cuda.synchronize()
    e, inv, K = e[0].cpu().numpy(), inv[0].cpu().numpy(), int(k[0])
    levels = float(np.abs(e - r['e']).max())
    assert e.shape == (r['F'],) and levels < 1e-9                            # dB; the decision has the margin to spare
    chunks = [int(r['keep'][c:c + 256].sum()) for c in range(0, r['F'], 256)]
    assert K == r['K'] and np.array_equal(inv[:K], r['inv']) and bool((inv[K:] == -1).all()), (name, K, r['K'])
    Ln = 128 * (K - 1) + 256
    worst = 0.0
    for got, key, src in ((xp, 'xp', x), (yp, 'yp', y)):
        got = got[0].cpu().numpy()
        assert got.shape == (128 * (r['F'] - 1) + 256,) and bool((got[Ln:] == 0.0).all())
        ulp = np.spacing(np.maximum(SR.overlap_scale(src, r['inv']), np.finfo(np.float64).tiny))
        worst = max(worst, float((np.abs(got[:Ln] - r[key]) / ulp).max()))
    print(f'{name}: F {r["F"]} K {K} S {r["S"]}, kept a chunk of 256 {chunks}, mask margin {r["margin"]:.3g} dB, levels {levels:.2e} dB, '
          f'x\' / y\' worst error {worst:.2f} ulp')
    assert worst <= 4.0, (name, worst)


@pytest.mark.parametrize('name', STOI_NAMES)
def test_stoi_envelopes(metrics, name):
    """the transform stage alone, on the REFERENCE's x' and y' as a ragged batch of two with NaN behind both"""
    r = stoi_reference(name)
    Ln = r['xp'].shape[0]
    sig = np.full((2, Ln + 130), NAN)
    sig[0, :Ln], sig[1, :Ln] = r['xp'], r['yp']
    env = metrics.stoi_envelopes_dev(_dev(sig), _ints([Ln, Ln])).cpu().numpy()
    Mf = r['X'].shape[1]
    assert Mf == r['K'] - 1 and env.shape == (2, 15, Mf + 1 + 1) and bool((env[:, :, Mf:] == 0.0).all())
    bound = _bound(r['env_orders'])
    for row, key in ((0, 'X'), (1, 'Y')):
        err = float(np.abs(env[row, :, :Mf] - r[key]).max() / np.abs(r[key]).max())
        print(f'{name} {key} ({Mf} frames): envelopes {err:.3e} (bound {bound:.3e}, the reference\'s two orders {r["env_orders"]:.3e})')
        assert err <= bound, (name, key, err, bound)


@pytest.mark.parametrize('extended', (False, True))
@pytest.mark.parametrize('name', STOI_NAMES)
def test_stoi_scores(metrics, name, extended):
    r = stoi_reference(name)
    out = _stoi_alone(metrics, *L.stoi_pairs()[name], extended)
    assert int(out[1]) == r['S'] and int(out[2]) == r['K'], (name, out, r['S'], r['K'])
    bound = _bound(r['score_orders'][extended])
    err = abs(float(out[0]) - r['score'][extended])
    print(f'{name} extended={extended}: score {out[0]:.15f} over {r["S"]} segments, error {err:.3e} (bound {bound:.3e}, two orders '
          f'{r["score_orders"][extended]:.3e})')
    assert err <= bound, (name, extended, err, bound)


@pytest.mark.parametrize('extended', (False, True))
def test_stoi_ragged_batch_gives_each_pair_alone_to_the_bit_twice(metrics, extended):
    """the six pairs (256, 257, 258, 681, 257 and 258 frames) in one batch, NaN behind every row; run twice"""
    pairs = [L.stoi_pairs()[k] for k in STOI_NAMES]
    n = [p[0].shape[0] for p in pairs]
    bx, by = _dev(_rows([p[0] for p in pairs], max(n) + 77, NAN)), _dev(_rows([p[1] for p in pairs], max(n) + 77, NAN))
    runs = []
    for _ in range(2):
        out = metrics.stoi_dev(bx, by, _ints(n), extended)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    assert np.isfinite(runs[0]).all() and np.array_equal(_bits(runs[0]), _bits(runs[1]))
    for r, k in enumerate(STOI_NAMES):
        assert np.array_equal(_bits(runs[0][r]), _bits(_stoi_alone(metrics, *pairs[r], extended))), (k, runs[0][r])
        assert (int(runs[0][r][1]), int(runs[0][r][2])) == L.STOI_FKS[k][:0:-1], k


@pytest.mark.parametrize('extended', (False, True))
def test_stoi_batch_of_72_rows_reaches_final_kernels_second_block(metrics, extended):
    """70 cuts of 4096 samples (31 frames, all kept, one segment) and two rows too short for a segment, NaN behind the short ones:
    every row -- rows 64 .. 71 are final_kernel's second block -- is its run alone"""
    rows = L.stoi_many_rows()
    n = [x.shape[0] for x, _ in rows]
    assert len(rows) == L.MANY_ROWS >= 70 and all(n[r] == L.MANY_CUT for r in range(64, L.MANY_ROWS))
    out = metrics.stoi_dev(_dev(_rows([x for x, _ in rows], L.MANY_CUT, NAN)), _dev(_rows([y for _, y in rows], L.MANY_CUT, NAN)), _ints(n),
                           extended)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for r, (x, y) in enumerate(rows):
        alone = _stoi_alone(metrics, x, y, extended)
        if r in L.MANY_SHORT:
            assert math.isnan(out[r, 0]) and math.isnan(alone[0]) and out[r, 1] == 0.0 and np.array_equal(out[r, 1:], alone[1:]), r
        else:
            assert np.array_equal(_bits(out[r]), _bits(alone)) and (out[r, 1], out[r, 2]) == (1.0, 31.0), (r, out[r], alone)
    print(f'{L.MANY_ROWS} rows, extended={extended}: every row its run alone; rows 64 .. {L.MANY_ROWS - 1} score '
          f'{out[64:, 0].min():.4f} .. {out[64:, 0].max():.4f}')


# ============================================================================================== 3. pitch
@functools.lru_cache(maxsize=None)
def pitch_stat():
    x = L.long16()
    S = Q.stationarity(x, None, SCALE)
    div = Q.divergence_stat(x, SCALE)
    S.setflags(write=False)
    return dict(S=S, div=div, bound=min(1e-9, 100.0 * div))


@functools.lru_cache(maxsize=None)
def pitch_ref(rng):
    """the two per-kernel files' ref() on long16: phi, rms, both tracks, the bound and the input conditions"""
    x = L.long16()
    phi, rms = P.nccf(x, *rng, SCALE)
    S = pitch_stat()['S']
    f0, f0s = P.dp(phi, rms, *rng), Q.dp_stat(phi, rms, S, *rng)
    div = P.divergence(x, *rng, SCALE)
    margin, gap = P.margins_phi(phi, rms, *rng)
    margin_s = Q.margins_stat(phi, rms, S, *rng)
    assert margin >= MARGIN_FLOOR and gap >= MARGIN_FLOOR and margin_s >= MARGIN_FLOOR, (rng, margin, gap, margin_s)
    for a in (phi, rms, f0, f0s):
        a.setflags(write=False)
    return dict(x=x, phi=phi, rms=rms, f0=f0, f0s=f0s, S=S, div=div, bound=min(1e-9, 100.0 * div), margin=margin, gap=gap, margin_s=margin_s)


def _pitch_scratch(lib, B, max_n, rng, stat=False):
    nb = (lib.ss_pitch_stat_scratch_bytes if stat else lib.ss_pitch_scratch_bytes)(B, max_n, *rng)
    assert nb > 0, lib.ss_last_error()
    return torch.empty(nb, dtype=torch.uint8, device=DEV)


def gpu_nccf(lib, wav, n, rng):
    B, max_n = wav.shape
    F, K = max_n // 256 + 1, P.lag_range(*rng)[2]
    phi = torch.full((B, F, K), NAN, dtype=torch.float64, device=DEV)
    rms = torch.full((B, F), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_nccf(_p(wav), _p(n), B, max_n, SCALE, *rng, _p(phi), _p(rms), _s()))
    return phi.cpu().numpy(), rms.cpu().numpy()


def gpu_stat(lib, wav, n):
    B, max_n = wav.shape
    S = torch.full((B, max_n // 256 + 1), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_pitch_stationarity(_p(wav), _p(n), B, max_n, SCALE, _p(S), _s()))
    return S.cpu().numpy()


def gpu_dp(lib, phi, rms, S, n, max_n, rng):
    """phi [B, F, K], rms [B, F], S [B, F] or None (tensors) -> numpy f0 [B, F]"""
    B, F = rms.shape
    f0 = torch.full((B, F), NAN, dtype=torch.float64, device=DEV)
    sc = _pitch_scratch(lib, B, max_n, rng)
    if S is None:
        _check(lib, lib.ss_op_pitch_dp(_p(phi), _p(rms), _p(n), B, max_n, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    else:
        _check(lib, lib.ss_op_pitch_dp_stat(_p(phi), _p(rms), _p(S), _p(n), B, max_n, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    return f0.cpu().numpy()


def gpu_track(lib, wav, n, rng, stat):
    B, max_n = wav.shape
    f0 = torch.full((B, max_n // 256 + 1), NAN, dtype=torch.float64, device=DEV)
    sc = _pitch_scratch(lib, B, max_n, rng, stat)
    fn = lib.ss_pitch_track_stat if stat else lib.ss_pitch_track
    _check(lib, fn(_p(wav), _p(n), B, max_n, SCALE, *rng, _p(f0), _p(sc), sc.numel(), _s()))
    return f0.cpu().numpy()


def assert_same_track(got, want, what):
    """the voiced / unvoiced pattern exactly, voiced values within 1e-10 relative; returns the worst relative difference"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    v = P.voiced(want)
    assert np.array_equal(P.voiced(got), v), (what, np.nonzero(P.voiced(got) != v)[0])
    assert np.all(got[~v] == P.UNVOICED)
    worst = float(np.abs(got[v] / want[v] - 1.0).max()) if v.any() else 0.0
    assert worst <= VALUE_TOL, (what, worst)
    return worst


@pytest.mark.parametrize('rng', RANGES, ids=RANGE_IDS)
def test_pitch_nccf(lib, rng):
    r = pitch_ref(rng)
    phi, rms = gpu_nccf(lib, _dev(r['x'])[None], None, rng)
    assert phi.shape[1:] == r['phi'].shape == (L.LONG16_FRAMES, P.lag_range(*rng)[2]) and np.isfinite(phi).all() and np.isfinite(rms).all()
    err = np.abs(phi[0] - r['phi']).max(axis=1)
    dphi, drms = float(err.max()), float((np.abs(rms[0] - r['rms']) / r['rms']).max())
    print(f'ss_op_nccf long16 {rng}: two orders {r["div"]:.3g}, bound {r["bound"]:.3g}, phi {dphi:.3g} (frames 49 on: {float(err[49:].max()):.3g}), '
          f'rms {drms:.3g} (relative); path margin {r["margin"]:.3g}, candidate-rule gap {r["gap"]:.3g}')
    assert dphi <= r['bound'] and drms <= r['bound']


@pytest.mark.parametrize('rng', RANGES, ids=RANGE_IDS)
def test_pitch_dp_on_the_references_own_nccf(lib, rng):
    r = pitch_ref(rng)
    got = gpu_dp(lib, _dev(r['phi'])[None], _dev(r['rms'])[None], None, None, r['x'].shape[0], rng)[0]
    worst = assert_same_track(got, r['f0'], rng)
    print(f'ss_op_pitch_dp long16 {rng}: {int(P.voiced(got).sum())} of {got.shape[0]} frames voiced, runs {L.voiced_runs(P.voiced(got))}, '
          f'values within {worst:.3g}, frames whose bits differ {np.flatnonzero(got != r["f0"]).tolist()}')


@pytest.mark.parametrize('rng', RANGES, ids=RANGE_IDS)
def test_pitch_track_end_to_end(lib, rng):
    r = pitch_ref(rng)
    got = gpu_track(lib, _dev(r['x'])[None], None, rng, False)[0]
    worst = assert_same_track(got, r['f0'], rng)
    print(f'ss_pitch_track long16 {rng}: {int(P.voiced(got).sum())} of {got.shape[0]} frames voiced, values within {worst:.3g}')


def test_pitch_stationarity(lib):
    r = pitch_stat()
    S = gpu_stat(lib, _dev(L.long16())[None], None)[0]
    assert S.shape == r['S'].shape == (L.LONG16_FRAMES,) and np.isfinite(S).all()
    assert S[0] == 0.0 and not np.signbit(S[0]) and np.all(S[1:] > 0.0) and np.all(S <= 1.0)
    err = np.abs(S - r['S'])
    print(f'ss_op_pitch_stationarity long16: two orders {r["div"]:.3g}, bound {r["bound"]:.3g}, S {float(err.max()):.3g} (frames 49 on: '
          f'{float(err[49:].max()):.3g}); S spans {S[1:].min():.3g} .. {S[1:].max():.3g}')
    assert float(err.max()) <= r['bound']


@pytest.mark.parametrize('rng', RANGES, ids=RANGE_IDS)
def test_pitch_dp_stat_on_the_references_own_operands(lib, rng):
    """Held to the bar for tracks, the same voiced pattern and 1e-10 relative, as ss_op_pitch_dp is.  test_gpu_pitch_stat.py asks its twelve
    short cases for the reference's bits and gets them; the header promises f0 = ln(16000 / L) and no bits, and on long16 in (50, 250) ONE
    of the 171 voiced values, frame 141, is the neighbouring double of numpy's (2.2e-16 relative: the device's log against the C
    library's on the same L) -- in ss_op_pitch_dp's track as in this one.  Every decision is the reference's: the differing frames are
    printed."""
    r = pitch_ref(rng)
    got = gpu_dp(lib, _dev(r['phi'])[None], _dev(r['rms'])[None], _dev(r['S'])[None], None, r['x'].shape[0], rng)[0]
    worst = assert_same_track(got, r['f0s'], rng)
    print(f'ss_op_pitch_dp_stat long16 {rng}: {int(P.voiced(got).sum())} of {got.shape[0]} frames voiced, margin {r["margin_s"]:.3g}, '
          f'values within {worst:.3g}, frames whose bits differ {np.flatnonzero(got != r["f0s"]).tolist()}')


@pytest.mark.parametrize('rng', RANGES, ids=RANGE_IDS)
def test_pitch_track_stat_end_to_end(lib, rng):
    r = pitch_ref(rng)
    got = gpu_track(lib, _dev(r['x'])[None], None, rng, True)[0]
    worst = assert_same_track(got, r['f0s'], rng)
    print(f'ss_pitch_track_stat long16 {rng}: {int(P.voiced(got).sum())} of {got.shape[0]} frames voiced, values within {worst:.3g}')


def test_pitch_ragged_batch_rows_are_the_utterances_alone(lib):
    """45 172, 513, 16 400 and 30 000 samples of long16 in rows of 45 172 with NaN behind every row: each row is its run alone to the bit;
    f0 behind a row's frames is -1e10 (174 frames behind the 513-sample row: three trips of dp_kernel's fill), phi, rms and S exact zeros"""
    x = L.long16()
    lens = list(L.PITCH_RAGGED)
    wav, n = _dev(_rows([x[:k] for k in lens], L.LONG16_SAMPLES, NAN)), _ints(lens)
    assert L.LONG16_FRAMES - (513 // 256 + 1) == 174
    tracks = {stat: gpu_track(lib, wav, n, M, stat) for stat in (False, True)}
    phi, rms = gpu_nccf(lib, wav, n, M)
    S = gpu_stat(lib, wav, n)
    for b, k in enumerate(lens):
        F = k // 256 + 1
        one = _dev(x[:k])[None]
        for stat in (False, True):
            got = tracks[stat]
            assert np.array_equal(_bits(got[b, :F]), _bits(gpu_track(lib, one, None, M, stat)[0])), (k, stat)
            assert got[b, F:].shape == (L.LONG16_FRAMES - F,) and np.all(got[b, F:] == P.UNVOICED), (k, stat)
        p1, r1 = gpu_nccf(lib, one, None, M)
        assert np.array_equal(_bits(phi[b, :F]), _bits(p1[0])) and np.array_equal(_bits(rms[b, :F]), _bits(r1[0])), k
        assert np.array_equal(_bits(S[b, :F]), _bits(gpu_stat(lib, one, None)[0])), k
        assert _plus_zeros(phi[b, F:]) and _plus_zeros(rms[b, F:]) and _plus_zeros(S[b, F:]), k
    assert_same_track(tracks[False][0], pitch_ref(M)['f0'], 'row 0')
    assert_same_track(tracks[True][0], pitch_ref(M)['f0s'], 'row 0, stat')
    # the hooks never read phi / rms / S behind a row's own frames
    pn, rn, sn = phi.copy(), rms.copy(), S.copy()
    for b, k in enumerate(lens):
        pn[b, k // 256 + 1:], rn[b, k // 256 + 1:], sn[b, k // 256 + 1:] = NAN, NAN, NAN
    assert np.array_equal(_bits(gpu_dp(lib, _dev(pn), _dev(rn), None, n, L.LONG16_SAMPLES, M)), _bits(tracks[False]))
    assert np.array_equal(_bits(gpu_dp(lib, _dev(pn), _dev(rn), _dev(sn), n, L.LONG16_SAMPLES, M)), _bits(tracks[True]))
    print(f'pitch, ragged: samples {lens} of {L.LONG16_SAMPLES}, frames filled behind the rows {[L.LONG16_FRAMES - k // 256 - 1 for k in lens]}')


# ============================================================================================== 4. the filter
FILT_NAMES = tuple(str(k) for k in L.FILTER_N) + ('long',)
FILT_MAX_N = L.LONG16_X_SAMPLES + 30                                     # NaN behind the longest row too


@functools.lru_cache(maxsize=None)
def filt_ref(name, dithered):
    b, a, zi = FR.coefficients()
    x = L.filter_rows()[name]
    y = FR.filtfilt(x, b, a, zi, FR.GAIN, L.filter_draws(name), FR.DITHER_SCALE) if dithered else FR.filtfilt(x, b, a, zi)
    y.setflags(write=False)
    return y


def gpu_filtfilt(lib, x, n, gain=1.0, dither=None, scale=0.0):
    """x [B, max_n] (tensor), n int32 [B] or None -> numpy [B, max_n]; the output starts as NaN"""
    B, max_n = x.shape
    hosts = [np.ascontiguousarray(v, dtype=np.float64) for v in FR.coefficients()]
    pb, pa, pz = (h.ctypes.data_as(C.c_void_p) for h in hosts)
    nb = lib.ss_filtfilt_scratch_bytes(B, max_n)
    assert nb > 0, lib.ss_last_error()
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    y = torch.full((B, max_n), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_filtfilt(_p(x), _p(n), B, max_n, pb, pa, pz, gain, _p(dither), scale, _p(y), _p(sc), nb, _s()))
    return y.cpu().numpy()


def _filt_batch():
    sigs = [L.filter_rows()[k] for k in FILT_NAMES]
    return (_dev(_rows(sigs, FILT_MAX_N, NAN)), _ints([s.shape[0] for s in sigs]),
            _dev(_rows([L.filter_draws(k) for k in FILT_NAMES], FILT_MAX_N, NAN)))


@pytest.mark.parametrize('dithered', (False, True), ids=['plain', 'gain-and-dither'])
def test_filtfilt_ragged_batch_equals_the_restatement(lib, dithered):
    x, n, r = _filt_batch()                                              # NaN behind every row's end: nothing there is read
    got = gpu_filtfilt(lib, x, n, FR.GAIN, r, FR.DITHER_SCALE) if dithered else gpu_filtfilt(lib, x, n)
    for b, name in enumerate(FILT_NAMES):
        want = filt_ref(name, dithered)
        k = want.shape[0]
        N = k + 36
        bad = np.flatnonzero(got[b, :k] != want)
        worst = float(np.abs(got[b, :k] - want).max())
        print(f'ss_filtfilt {name} ({k} samples, N = {N}: {-(-N // 256)} blocks, the last of {(N - 1) % 256 + 1} steps), '
              f'{"gain and dither" if dithered else "plain"}: max |difference| {worst:.3g}, samples that differ {bad.size}')
        assert FR.same(got[b, :k], want), (name, worst, bad[:5])
        assert _plus_zeros(got[b, k:]), name                                 # exact zeros behind the row


def test_filtfilt_rows_alone_give_the_batchs_bits_and_two_runs_agree(lib):
    x, n, r = _filt_batch()
    got = gpu_filtfilt(lib, x, n, FR.GAIN, r, FR.DITHER_SCALE)
    assert np.array_equal(_bits(got), _bits(gpu_filtfilt(lib, x, n, FR.GAIN, r, FR.DITHER_SCALE)))
    for b, name in enumerate(FILT_NAMES):
        row = L.filter_rows()[name]
        alone = gpu_filtfilt(lib, _dev(row)[None], None, FR.GAIN, _dev(L.filter_draws(name))[None], FR.DITHER_SCALE)
        assert np.array_equal(_bits(alone[0]), _bits(got[b, :row.shape[0]])), name


# ============================================================================================== 5. STFT, ISTFT, Griffin-Lim
VOC_FRAMES = (177, 65)                                                   # the ragged pair; 177 alone everywhere else


@functools.lru_cache(maxsize=None)
def voc_input(F):
    """test_gpu_vocoder.py's inputs[F] on long16: x cut to 256 (F - 1) samples, S = |stft(x)|, seeded phases"""
    x = np.ascontiguousarray(L.long16()[:256 * (F - 1)])
    S = np.abs(GL.stft(x))
    assert S.shape == (F, 513)
    ph = np.random.default_rng(100 + F).uniform(-np.pi, np.pi, S.shape)
    return dict(x=x, S=S, ph=ph)


@functools.lru_cache(maxsize=None)
def voc_bound():
    """100 x the fft / dft divergence of Griffin-Lim on THIS input at the largest round count run here, capped at 1e-9 of max |x|"""
    inp = voc_input(177)
    div = GL.divergence(inp['S'], inp['ph'], max(GL_ROUNDS))
    assert div <= GL.DIVERGENCE_CAP
    return div, min(1e-9, 100.0 * div)


def _voc_scratch(lib, B, T):
    return torch.empty(lib.ss_griffinlim_scratch_bytes(B, T), dtype=torch.uint8, device=DEV)


def gpu_stft(lib, wav, frames, T):
    spec = torch.full((wav.shape[0], T, 513, 2), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_stft(_p(wav), _p(frames), wav.shape[0], T, _p(spec), _s()))
    s = spec.cpu().numpy()
    return s[..., 0] + 1j * s[..., 1]


def gpu_istft(lib, spec, frames, T):
    B = spec.shape[0]
    wav = torch.full((B, 256 * (T - 1)), NAN, dtype=torch.float64, device=DEV)
    sc = _voc_scratch(lib, B, T)
    _check(lib, lib.ss_op_istft(_p(spec), _p(frames), B, T, _p(wav), _p(sc), sc.numel(), _s()))
    return wav.cpu().numpy()


def _ri(z):
    return np.stack([z.real, z.imag], -1)


def test_stft_and_istft_at_177_frames(lib):
    x = voc_input(177)['x']
    ref = GL.stft(x)
    got = gpu_stft(lib, _dev(x)[None], None, 177)[0]
    per_frame = np.abs(got - ref).max(axis=1) / np.abs(ref).max()
    err = GL.rel_diff(got, ref)
    scale = np.abs(x).max()
    back_ref = gpu_istft(lib, _dev(_ri(ref))[None], None, 177)[0]
    ierr = float(np.abs(back_ref - GL.istft(ref)).max() / scale)
    back = gpu_istft(lib, _dev(_ri(got))[None], None, 177)[0]
    rt = float(np.abs(back - x).max() / scale)
    print(f'ss_op_stft, 177 frames: {err:.3g} of max |spec| (frames 49 on: {float(per_frame[49:].max()):.3g}); ss_op_istft: {ierr:.3g} of max |x|; '
          f'istft(stft(x)) - x: {rt:.3g}')
    assert err <= HOOK_TOL and ierr <= HOOK_TOL and rt <= HOOK_TOL


def test_griffinlim_parity_at_177_frames(V):
    inp = voc_input(177)
    div, bound = voc_bound()
    mag, ph = _dev(inp['S'])[None], _dev(inp['ph'])[None]
    worst = 0.0
    for n_iter in GL_ROUNDS:
        for momentum in GL.MOMENTA:
            for seeded in (False, True):
                got = V.griffin_lim_mag(mag, ph if seeded else None, None, n_iter, momentum)[0].cpu().numpy()
                ref = GL.griffin_lim(inp['S'], n_iter, momentum, inp['ph'] if seeded else None)
                assert got.shape == ref.shape == (256 * 176,) and np.isfinite(got).all()
                d = GL.rel_diff(got, ref)
                worst = max(worst, d)
                print(f'177 frames, n_iter {n_iter}, momentum {momentum}, {"seeded" if seeded else "zero"} phases: {d:.3g} (bound {bound:.3g})')
                assert d <= bound
    print(f'177 frames: fft vs dft at {max(GL_ROUNDS)} rounds {div:.3g}, bound {bound:.3g}, worst GPU difference {worst:.3g}')


def test_vocoder_ragged_pair_rows_are_the_utterances_alone(lib, V):
    """177 and 65 frames in rows of 177, NaN in every frame a row does not own: Griffin-Lim and both hooks give the rows alone, bit for bit"""
    T, fr = 177, _ints(list(VOC_FRAMES))
    ins = [voc_input(F) for F in VOC_FRAMES]
    mag, ph = _dev(_rows([i['S'] for i in ins], T, NAN)), _dev(_rows([i['ph'] for i in ins], T, NAN))
    got = V.griffin_lim_mag(mag, ph, fr, 4, 0.99).cpu().numpy()
    wav = _dev(_rows([i['x'] for i in ins], 256 * (T - 1), NAN))
    spec = gpu_stft(lib, wav, fr, T)
    back = gpu_istft(lib, _dev(_rows([_ri(GL.stft(i['x'])) for i in ins], T, NAN)), fr, T)
    for b, (F, i) in enumerate(zip(VOC_FRAMES, ins)):
        k = 256 * (F - 1)
        alone = V.griffin_lim_mag(_dev(i['S'])[None], _dev(i['ph'])[None], None, 4, 0.99)[0].cpu().numpy()
        assert np.array_equal(_bits(got[b, :k]), _bits(alone)) and _plus_zeros(got[b, k:]), F
        assert np.array_equal(spec[b, :F], gpu_stft(lib, _dev(i['x'])[None], None, F)[0]) and not spec[b, F:].any(), F
        assert np.array_equal(_bits(back[b, :k]), _bits(gpu_istft(lib, _dev(_ri(GL.stft(i['x'])))[None], None, F)[0])) and _plus_zeros(back[b, k:]), F
    print(f'vocoder, ragged: frames {list(VOC_FRAMES)} of {T}, every row its run alone')
