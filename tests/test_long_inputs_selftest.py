"""long_inputs.py on the CPU: the conditions test_gpu_long_audio.py relies on, as assertions and not as measurements -- if a fixture or a
restatement changes, this file fails rather than the GPU tests going quiet -- and the proof that the inputs are worth their time: for every
carried-state mistake they are there for, a numpy emulation of the mistake differs from the restatement on at least one of them and equals
it on every input of the per-kernel files, i.e. the short inputs could not have told.

    u with the carry dropped at every multiple of 64 frames           long_inputs.u_carry_dropped
    the STOI map with `base` not carried across a 256-frame chunk     long_inputs.stoi_map('base_not_carried')
    the STOI levels from frame 256 on at -inf                         long_inputs.stoi_map('second_block_missing')
    a pitch fill that makes one trip of 64 frames                     long_inputs.pitch_fill('one_trip')
    a filter that loses a last block of one step (N = 1 mod 256)      long_inputs.filtfilt_blocks('single_step_lost')
    a filter that restarts its state at a block edge                  'restart_at_closing_edge', 'restart_at_every_edge'
    a filter that skips a last block shorter than one group of 8      'short_tail_skipped'

A restart at EVERY block edge is told by the short inputs already (each has 3 to 49 blocks; asserted below), so the variant held to "the short
inputs agree" is the restart at an edge that closes the pass, N = 0 mod 256, which no earlier length reaches."""
import functools

import numpy as np
import pytest
from scipy import signal

from tests import filtfilt_ref as FR
from tests import griffinlim_ref as GL
from tests import harmonic_ref as H
from tests import long_inputs as L
from tests import pitch_ref as P
from tests import pitch_stat_ref as Q
from tests import stoi_ref as SR

MARGIN_FLOOR = 1e-6


# ---------------------------------------------------------------------------------------------- long16
@functools.lru_cache(maxsize=None)
def pitch(rng):
    phi, rms = P.nccf(L.long16(), *rng, L.SCALE)
    return phi, rms, P.dp(phi, rms, *rng)


@pytest.mark.parametrize('rng', [L.M_RANGE, L.W_RANGE], ids=['50-250', '100-600'])
def test_long16_leaves_no_pitch_decision_to_rounding(rng):
    phi, rms, f0 = pitch(rng)
    S = Q.stationarity(L.long16(), None, L.SCALE)
    margin, gap = P.margins_phi(phi, rms, *rng)
    margin_s = Q.margins_stat(phi, rms, S, *rng)
    print(f'long16 {rng}: path margin {margin:.3g}, candidate-rule gap {gap:.3g}, with the stationarity track {margin_s:.3g}')
    assert phi.shape[0] == rms.shape[0] == S.shape[0] == L.LONG16_FRAMES == 177
    assert margin >= MARGIN_FLOOR and gap >= MARGIN_FLOOR and margin_s >= MARGIN_FLOOR
    assert P.voiced(f0).sum() > 160 and P.voiced(Q.dp_stat(phi, rms, S, *rng)).sum() > 160


def test_long16_track_has_a_run_across_frame_64_and_one_from_frame_128():
    f0 = pitch(L.M_RANGE)[2]
    v = P.voiced(f0)
    assert tuple(np.flatnonzero(~v)) == L.LONG16_UNVOICED == (0, 1, 49, 127, 175, 176) and int(v.sum()) == 171
    assert L.voiced_runs(v) == [(2, 47), (50, 77), (128, 47)]                # 50 .. 126 crosses 64; 128 follows the reset at 127
    hz = L.long16_track()
    assert np.array_equal(H.voiced(hz), v)
    H.conditions(hz)
    u = H.phase_u(hz)
    assert u[63] != 0.0 and u[64] != 0.0 and u[127] == 0.0 and u[128] == 0.0 and u[129] != 0.0
    assert L.long16_mel().shape == (177, 80) and GL.frames_of(256 * 176) == 177 and GL.frames_of(256 * 64) == 65


# ---------------------------------------------------------------------------------------------- the harmonic phase
def _short_tracks():
    """the tracks test_gpu_harmonic.py runs: the recorded ones and its three edge tracks of 9 frames"""
    out = {k: hz for k, (_, hz) in H.parity_inputs(L.feats()).items()}
    alt = np.where(np.arange(9) % 2 == 0, 0.0, 110.37 + 3.1307 * np.arange(9))
    alt[-3:] = 131.21, 133.57, 0.0
    out.update(low=np.full(9, 40.5003), high=np.full(9, 999.0), alternating=alt)
    return out


def test_u_tracks_are_what_the_module_says():
    for F in L.U_FRAMES:
        g = L.u_track('glide', F)
        assert g.shape == (F,) and H.voiced(g).all() and g.max() < 1000.0
        for gap in L.U_GAPS:
            hz = L.u_track(f'gap{gap}', F)
            assert np.array_equal(np.flatnonzero(~H.voiced(hz)), [gap] if gap < F else [])
        a = L.u_track('alternating', F)
        assert not H.voiced(a)[::2].any() and H.voiced(a)[1::2].all() and not H.phase_u(a).any()
        assert not H.voiced(L.u_track('unvoiced', F)).any()
    assert [F for F, _ in L.U_RAGGED] == [64, 65, 128, 200]


def test_a_dropped_carry_shows_on_the_long_tracks_and_on_no_short_one():
    for F in L.U_FRAMES:
        hz = L.u_track('glide', F)
        want, wrong = H.phase_u(hz), L.u_carry_dropped(hz)
        assert np.array_equal(want[:64], wrong[:64])
        assert (F > 64) == (not np.array_equal(want, wrong)), F
        if F > 64:
            assert want[64] != wrong[64]                                     # the first frame of the second trip
    for gap in (62, 63, 65):                                                 # a reset near the edge does not hide it; ON the edge it does
        hz = L.u_track(f'gap{gap}', 129)
        assert not np.array_equal(H.phase_u(hz), L.u_carry_dropped(hz)), gap
    hz = L.u_track('gap64', 65)
    assert np.array_equal(H.phase_u(hz), L.u_carry_dropped(hz))
    assert not np.array_equal(H.phase_u(L.long16_track()), L.u_carry_dropped(L.long16_track()))
    for name, hz in _short_tracks().items():
        assert hz.shape[0] <= 49 and np.array_equal(H.phase_u(hz), L.u_carry_dropped(hz)), name


# ---------------------------------------------------------------------------------------------- long10
@functools.lru_cache(maxsize=None)
def stoi_ref(name):
    return SR.both_modes(*L.stoi_pairs()[name], 'loop')


@pytest.mark.parametrize('name', list(L.STOI_CUTS))
def test_long10_pairs_have_the_frames_the_module_says(name):
    x, y = L.stoi_pairs()[name]
    r = stoi_ref(name)
    margin = SR.mask_margin(x)
    chunks = [int(r['keep'][c:c + 256].sum()) for c in range(0, r['F'], 256)]
    print(f'{name}: {x.shape[0]} samples, F {r["F"]} K {r["K"]} S {r["S"]}, kept a chunk {chunks}, mask margin {margin:.3g} dB')
    assert x.shape == y.shape == (L.STOI_CUTS[name][1],) and (r['F'], r['K'], r['S']) == L.STOI_FKS[name]
    assert margin > MARGIN_FLOOR
    assert np.isfinite(r['score'][False]) and np.isfinite(r['score'][True])
    if name == 'whole':
        assert len(chunks) == 3 and all(0 < c < min(256, r['F'] - 256 * i) for i, c in enumerate(chunks))   # dropped in every chunk
    else:
        assert chunks == L.STOI_KEPT[name]


def test_the_72_row_batch_has_a_segment_in_every_row_from_64_on():
    rows = L.stoi_many_rows()
    assert len(rows) == L.MANY_ROWS == 72 and max(L.MANY_SHORT) < 64
    starts = set()
    for r, (x, y) in enumerate(rows):
        assert x.shape == y.shape
        F = SR.n_frames(x.shape[0])
        K = int(SR.keep_mask(SR.energies(x)).sum())
        S = max(K - 1 - SR.N + 1, 0)
        if r in L.MANY_SHORT:
            assert x.shape[0] == L.MANY_SHORT[r] and S == 0 and F in (30, 1)
        else:
            assert (x.shape[0], F, K, S) == (4096, 31, 31, 1) and SR.mask_margin(x) > MARGIN_FLOOR, r
            starts.add(x[:64].tobytes())
    assert len(starts) == 70                                                 # 70 different cuts


def _short_pairs():
    """test_gpu_stoi.py's recordings at 10 kHz"""
    out = {}
    for k, seed in (('u0', 1), ('u1', 2)):
        out[k] = SR.make_pair(signal.resample_poly(L.feats()[k + '_wav'].astype(np.float64), 5, 8), seed)[0]
    return out


@pytest.mark.parametrize('variant', ['base_not_carried', 'second_block_missing'])
def test_a_mask_that_forgets_its_first_chunk_shows_on_long10_and_on_no_short_pair(variant):
    told = []
    for name in L.STOI_CUTS:
        r = stoi_ref(name)
        inv, K = L.stoi_map(r['e'])
        assert K == r['K'] and np.array_equal(inv[:K], r['inv']) and (inv[K:] == -1).all()       # the emulation is the restatement
        bad, Kb = L.stoi_map(r['e'], variant)
        if Kb != K or not np.array_equal(bad, inv):
            told.append(name)
    # 256 frames are one chunk.  The last frames of f257 / f258 lie in long10's noise and are dropped: their second chunk writes nothing, so
    # a lost `base` still shows (K comes out as the second chunk's count, 0) but lost levels do not -- the whole signal and the two cuts
    # that keep frames 256 and 257 tell both
    assert told == {'base_not_carried': ['f257', 'f258', 'whole', 'k257', 'k258'], 'second_block_missing': ['whole', 'k257', 'k258']}[variant]
    for name, x in _short_pairs().items():
        e = SR.energies(x)
        assert e.shape[0] < 256
        (a, Ka), (b, Kb) = L.stoi_map(e), L.stoi_map(e, variant)
        assert Ka == Kb and np.array_equal(a, b), name


# ---------------------------------------------------------------------------------------------- the pitch fill
def test_a_fill_of_one_trip_shows_behind_the_513_sample_row_and_in_no_short_batch():
    wide = L.LONG16_FRAMES
    gaps = [wide - (n // 256 + 1) for n in L.PITCH_RAGGED]
    assert L.PITCH_RAGGED[0] == L.LONG16_SAMPLES and gaps == [0, 174, 112, 59] and -(-174 // 64) == 3
    told = [n for n in L.PITCH_RAGGED if not np.array_equal(L.pitch_fill(n // 256 + 1, wide), L.pitch_fill(n // 256 + 1, wide, 'one_trip'))]
    assert told == [513, 16400]
    for n in (2304, 513, 12345, 1100):                                       # test_gpu_pitch.py's ragged batch: 49 frames wide, 46 to fill at most
        assert np.array_equal(L.pitch_fill(n // 256 + 1, 49), L.pitch_fill(n // 256 + 1, 49, 'one_trip')), n


# ---------------------------------------------------------------------------------------------- the filter
def _short_filter_rows():
    """test_gpu_features_batch.py's rows"""
    f = L.feats()
    u1 = np.ascontiguousarray(f['u1_x'], np.float64)
    return {'513': u1[:513], '600': u1[:600], '1100': u1[:1100], '2305': u1[:2305], 'u1': FR.odd_length_fix(u1),
            'u0': np.ascontiguousarray(f['u0_x'], np.float64)}


@functools.lru_cache(maxsize=None)
def _restated(name):
    rows = dict(_short_filter_rows(), **L.filter_rows())
    return FR.filtfilt(rows[name], *FR.coefficients())


def test_filter_lengths_end_their_last_block_where_the_module_says():
    assert [(n + 36 - 1) % 256 + 1 for n in L.FILTER_N] == list(L.FILTER_LAST_BLOCK) == [255, 256, 1, 7, 8, 9, 256]
    assert [-(-(n + 36) // 256) for n in L.FILTER_N] == [3, 3, 4, 4, 4, 4, 4]                  # 768 ends on an edge after 3 blocks, 1024 after 4
    assert sorted({(x.shape[0] + 36) % 256 for x in _short_filter_rows().values()}) == [37, 93, 112, 124]
    assert L.long16_x().shape == (45170,) and all(L.filter_rows()[str(n)].shape == (n,) for n in L.FILTER_N)
    assert all(np.abs(L.filter_rows()[str(n)]).max() > 0.01 for n in L.FILTER_N)              # speech, not silence
    for name in ('733', '732', 'long'):                                                     # run in blocks, it is the restatement to the bit
        assert FR.same(L.filtfilt_blocks(L.filter_rows()[name]), _restated(name)), name


@pytest.mark.parametrize('variant,told', [('single_step_lost', ['733']), ('restart_at_closing_edge', ['732', '988']),
                                          ('short_tail_skipped', ['733', '739'])])
def test_a_filter_wrong_at_a_block_end_shows_on_the_new_lengths_and_on_no_short_row(variant, told):
    got = [name for name in L.filter_rows() if not FR.same(L.filtfilt_blocks(L.filter_rows()[name], variant), _restated(name))]
    assert got == told
    for name, x in _short_filter_rows().items():
        assert FR.same(L.filtfilt_blocks(x, variant), _restated(name)), name


def test_a_restart_at_every_block_edge_was_told_already():
    for name, x in _short_filter_rows().items():
        assert not FR.same(L.filtfilt_blocks(x, 'restart_at_every_edge'), _restated(name)), name
    assert not FR.same(L.filtfilt_blocks(L.filter_rows()['732'], 'restart_at_every_edge'), _restated('732'))
