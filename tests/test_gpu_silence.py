"""Silence removal on the GPU (csrc/silence.hip: ss_remove_silence and its three test hooks) against the float64 numpy restatement
tests/silence_ref.py, which tests/test_silence_ref_selftest.py checks on its own.

Everything is compared TO THE BIT, levels included: every operation of the definition is an IEEE double add, multiply, compare or copy in
a fixed order, so there is no tolerance to measure -- a mismatch is a bug, or a contraction the compiler slipped in.  Float arrays are
compared as int64 views, so that a NaN or a zero of the wrong sign cannot pass for the right one.

Inputs.  The smallest lengths that can go wrong (1 .. 769: J = 1 .. 4, a short last block below and above 128 samples, max_n no multiple of
256); a recording of 46 585 samples built from features.npz (noise at 1e-4, u0_x, noise, u1_x, noise: 116 of 182 blocks kept with one join
at Silence(40, 2, 6, 8), no level within a factor 0.99 of the threshold -- asserted on the CPU in the self-test); crafted level lattices
through ss_op_silence_mask (exact ties, every run rule at its boundary, 64-block chunk boundaries, the longest row the call accepts); a join
directly before a short last block through ss_op_silence_gather; ragged batches on guarded slabs with NaN behind every row; corrupt maps;
out-of-contract lengths; and extract_batch_sr end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy import signal

import guarded as G
import silence_ref as R
from speechsplit_amd import _capi, features

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAN = float('nan')
FADE = R.fade_gains()
SPEECH = R.speech_signal(np.load(os.path.join(GOLDEN, 'features.npz')))
SPEECH_OPTS = dict(ratio=R.ratio_of(40.0), hang=2, edge=6, pause=8)
REF = {}                                               # key -> reference; computed once, never changed


def _ref(key, x, o):
    if key not in REF:
        REF[key] = R.remove_silence(x, **o)
    return REF[key]


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.flatnonzero(got.view(np.int64).ravel() != ref.view(np.int64).ravel())
    assert bad.size == 0, (what, f'{bad.size} elements differ; first at {bad[0]}: {got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}')


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gp(g=FADE):
    return np.ascontiguousarray(g, np.float64).ctypes.data_as(C.POINTER(C.c_double))


def _pack(xs, max_n=None):
    """rows [B][max_n] with NaN behind every recording, and their lengths"""
    max_n = max(len(x) for x in xs) if max_n is None else max_n
    rows = np.full((len(xs), max_n), NAN)
    for r, x in enumerate(xs):
        rows[r, :len(x)] = x
    return rows, np.array([len(x) for x in xs], np.int32)


def dev_levels(x_t, n_t):
    B, max_n = x_t.shape
    e = torch.full((B, R.blocks_of(max_n)), NAN, dtype=torch.float64, device=DEV)
    _capi.check(_capi.lib().ss_op_silence_levels(_vp(x_t), _vp(n_t), B, max_n, _vp(e), _stream()))
    return e.cpu().numpy()


def dev_mask(E_rows, ratio, hang, edge, pause):
    """lattices of any lengths as one ragged call -> [(inv [K], K)] a row"""
    B, max_j = len(E_rows), max(len(e) for e in E_rows)
    e = np.full((B, max_j), NAN)
    for r, v in enumerate(E_rows):
        e[r, :len(v)] = v
    j_t = torch.tensor([len(v) for v in E_rows], dtype=torch.int32, device=DEV)
    inv = torch.full((B, max_j), -7, dtype=torch.int32, device=DEV)
    k = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    _capi.check(_capi.lib().ss_op_silence_mask(_vp(torch.from_numpy(e).to(DEV)), _vp(j_t), B, max_j, ratio, hang, edge, pause, _vp(inv), _vp(k),
                                               _stream()))
    inv, k = inv.cpu().numpy(), k.cpu().numpy()
    out = []
    for r in range(B):
        assert 1 <= k[r] <= len(E_rows[r]) and np.all(inv[r, k[r]:] == -1), (r, k[r])
        out.append(inv[r, :k[r]].copy())
    return out


def dev_remove(x_t, n_t, ratio, hang, edge, pause, y_t=None, maps=True):
    """ss_remove_silence itself -> (y [B][max_n], m [B], inv [B][Jmax] or None, k [B] or None) as numpy"""
    lib = _capi.lib()
    B, max_n = x_t.shape
    nbytes = lib.ss_silence_scratch_bytes(B, max_n)
    assert nbytes > 0
    scratch = G.out((nbytes // 8,), DEV, dtype=torch.float64, name='scratch')
    y = y_t if y_t is not None else torch.full((B, max_n), NAN, dtype=torch.float64, device=DEV)
    m = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    inv = torch.full((B, R.blocks_of(max_n)), -7, dtype=torch.int32, device=DEV) if maps else None
    k = torch.full((B,), -7, dtype=torch.int32, device=DEV) if maps else None
    _capi.check(lib.ss_remove_silence(_vp(x_t), _vp(n_t), B, max_n, ratio, hang, edge, pause, _gp(), _vp(y), _vp(m), _vp(inv), _vp(k),
                                      _vp(scratch.t), nbytes, _stream()))
    torch.cuda.synchronize()
    scratch.check(written=False)
    return y.cpu().numpy(), m.cpu().numpy(), inv.cpu().numpy() if maps else None, k.cpu().numpy() if maps else None


def _check_row(y_row, m, inv_row, k, ref, what):
    assert int(m) == ref['m'] and int(k) == ref['K'], (what, int(m), ref['m'], int(k), ref['K'])
    assert np.array_equal(inv_row[:k], ref['inv']) and np.all(inv_row[k:] == -1), what
    _same_bits(y_row[:ref['m']], ref['y'], what)
    assert np.all(y_row[ref['m']:].view(np.int64) == 0), (what, 'exact zeros behind m_b')


SMALL_OPTS = [dict(ratio=1e-2, hang=0, edge=0, pause=0), dict(ratio=1e-2, hang=1, edge=1, pause=-1), dict(ratio=0.5, hang=0, edge=0, pause=1)]


def _small(n):
    rng = np.random.default_rng(100 + n)
    return rng.uniform(-1.0, 1.0, n) * np.repeat(np.where(rng.uniform(size=-(-n // 128)) < 0.5, 1.0, 1e-3), 128)[:n]


@pytest.mark.parametrize('n', [1, 127, 128, 129, 255, 256, 257, 384, 511, 512, 513, 769])
def test_smallest_lengths(n):
    x = _small(n)
    x_t = torch.from_numpy(x[None]).to(DEV)
    _same_bits(dev_levels(x_t, None)[0], R.levels(x), f'levels n={n}')
    for o in SMALL_OPTS:
        ref = R.remove_silence(x, **o)
        y, m, inv, k = dev_remove(x_t, None, **o)
        _check_row(y[0], m[0], inv[0], k[0], ref, (n, o))
    # the same recording as a short row of a wider slab: max_n is no multiple of 256, NaN behind n
    rows, lens = _pack([x], max_n=n + 300)
    r_t, n_t = torch.from_numpy(rows).to(DEV), torch.from_numpy(lens).to(DEV)
    E = dev_levels(r_t, n_t)[0]
    _same_bits(E[:R.blocks_of(n)], R.levels(x), f'levels n={n} in a wider slab')
    assert np.all(E[R.blocks_of(n):].view(np.int64) == 0)
    ref = R.remove_silence(x, **SMALL_OPTS[0])
    y, m, inv, k = dev_remove(r_t, n_t, **SMALL_OPTS[0])
    _check_row(y[0], m[0], inv[0], k[0], ref, (n, 'wider slab'))


def test_speech_levels_and_the_whole_call_twice():
    ref = _ref('speech', SPEECH, SPEECH_OPTS)
    assert (len(ref['E']), ref['K'], int(np.sum(np.diff(ref['inv']) != 1))) == (182, 116, 1)
    x_t = torch.from_numpy(SPEECH[None]).to(DEV)
    _same_bits(dev_levels(x_t, None)[0], ref['E'], 'speech levels')
    first = dev_remove(x_t, None, **SPEECH_OPTS)
    _check_row(first[0][0], first[1][0], first[2][0], first[3][0], ref, 'speech')
    second = dev_remove(x_t, None, **SPEECH_OPTS, maps=False)                # without the optional outputs: the maps live in scratch
    _same_bits(second[0], first[0], 'two runs')
    assert np.array_equal(second[1], first[1])
    for name in ('tie', 'ends', 'ends_hang', 'pause_odd', 'pause_exact', 'flat'):          # the self-test's named inputs, whole chain
        x, o = R.INPUTS[name]
        y, m, inv, k = dev_remove(torch.from_numpy(x[None]).to(DEV), None, **o)
        _check_row(y[0], m[0], inv[0], k[0], R.remove_silence(x, **o), name)


def _lattice(spec):
    """levels from a string: 'A' a loud block (1.0), '.' a silent one (2^-20), 't' a block exactly AT the threshold of ratio 2^-4"""
    return np.array([{'A': 1.0, '.': 2.0 ** -20, 't': 2.0 ** -4}[c] for c in spec])


def test_crafted_lattices_drive_every_run_rule():
    cases = []                                                             # (lattice, options)
    tie = dict(ratio=2.0 ** -4, hang=0, edge=0, pause=0)
    for spec in ('AtA', 'tAt', 'AttttA', 'tttAttt', 'A', 't', '.', 'At', 'tA'):
        cases.append((_lattice(spec), tie))
    cases.append((_lattice('AtA') * 2.0 ** 40, tie))                       # the tie is exact at any power of two
    for pause in (0, 1, 4, 5):
        for run in (max(pause - 1, 1), max(pause, 1), pause + 1, pause + 4):
            for hang in (0, 1):
                cases.append((_lattice('AA' + '.' * (run + 2 * hang) + 'AA'), dict(ratio=1e-4, hang=hang, edge=0, pause=pause)))
    cases.append((_lattice('A' + '.' * 9 + 'A'), dict(ratio=1e-4, hang=0, edge=0, pause=-1)))
    for edge in (0, 1, 3, 50):                                             # edge = 0, below and above the run
        for spec in ('....AA....', 'A.........', '.........A', '...A', 'A...'):
            cases.append((_lattice(spec), dict(ratio=1e-4, hang=0, edge=edge, pause=-1)))
            cases.append((_lattice(spec), dict(ratio=1e-4, hang=2, edge=edge, pause=2)))
    for hang in (1, 2, 3, 100):                                            # hangovers that meet, overlap or swallow the whole row
        cases.append((_lattice('A....A'), dict(ratio=1e-4, hang=hang, edge=0, pause=0)))
        cases.append((_lattice('..A.....A..'), dict(ratio=1e-4, hang=hang, edge=1, pause=1)))
    for spec in ('.', '....', '.' * 70):                                   # a run touching both ends: nothing is active, everything is kept
        cases.append((np.zeros(len(spec)), dict(ratio=1e-4, hang=1, edge=0, pause=0)))
    cases.append((np.array([1.0, NAN, 1e-9, 1.0]), dict(ratio=1e-4, hang=0, edge=0, pause=0)))          # E_max is NaN
    cases.append((np.array([np.inf, 1.0, 1e-9]), dict(ratio=1e-4, hang=0, edge=0, pause=0)))            # E_max is not finite
    rng = np.random.default_rng(3)
    for J in (63, 64, 65, 127, 128, 129, 200, 1000, 8191):                 # the 64-block chunks' carried state, up to the longest row
        run = rng.integers(1, 12, J)
        E = np.repeat(np.where(np.arange(J) % 2 == 0, 1.0, 2.0 ** -20), run)[:J] * rng.uniform(0.5, 1.0, J)
        for o in (dict(ratio=1e-4, hang=0, edge=0, pause=0), dict(ratio=1e-4, hang=2, edge=3, pause=5), dict(ratio=1e-4, hang=1, edge=70, pause=-1)):
            cases.append((E, o))
        cases.append((np.concatenate((np.full(J - 1, 2.0 ** -20), [1.0])), dict(ratio=1e-4, hang=0, edge=66, pause=0)))      # active block last
        cases.append((np.concatenate(([1.0], np.full(J - 1, 2.0 ** -20))), dict(ratio=1e-4, hang=0, edge=66, pause=0)))      # ... and first
    groups = {}
    for E, o in cases:
        groups.setdefault(tuple(sorted(o.items())), []).append(E)
    ties = 0
    for key, rows in groups.items():                                       # one ragged call per set of options
        o = dict(key)
        for E, got in zip(rows, dev_mask(rows, **o)):
            ref = R.mask(E, **o)
            assert np.array_equal(got, ref), (o, len(E), got[:12], ref[:12])
            ties += int(np.any(E == o['ratio'] * np.nanmax(E))) if np.isfinite(E).all() and E.max() > 0 else 0
    assert ties >= 7                                                       # the seven lattices with a 't' beside an 'A' did tie exactly
    assert dev_mask([_lattice('AtA')], **tie)[0].tolist() == [0, 2]        # a block AT the threshold is silent


def dev_gather(x_t, n_t, inv_np, k_np, y_t=None):
    B, max_n = x_t.shape
    y = y_t if y_t is not None else torch.full((B, max_n), NAN, dtype=torch.float64, device=DEV)
    m = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    inv = torch.from_numpy(np.ascontiguousarray(inv_np, np.int32)).to(DEV)
    k = torch.from_numpy(np.ascontiguousarray(k_np, np.int32)).to(DEV)
    _capi.check(_capi.lib().ss_op_silence_gather(_vp(x_t), _vp(n_t), B, max_n, _vp(inv), _vp(k), _gp(), _vp(y), _vp(m), _stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy(), m.cpu().numpy()


def test_a_join_directly_before_a_short_last_block():
    x, _, inv = R.INPUTS['short_join']
    assert len(x) == 5 * 256 + 57
    ref = R.gather(x, inv)
    full = np.full((1, 6), -1, np.int32)
    full[0, :3] = inv
    y, m = dev_gather(torch.from_numpy(x[None]).to(DEV), None, full, [3])
    assert m[0] == 512 + 57 == len(ref)
    _same_bits(y[0, :m[0]], ref, 'short join')
    assert np.all(y[0, m[0]:].view(np.int64) == 0)
    assert not np.array_equal(y[0, 512:569], x[1280:1337])                 # the 57 samples are a fade, not a copy


def test_ragged_rows_equal_their_run_alone_on_guarded_slabs():
    xs = [SPEECH[18000:18000 + 12001], R.INPUTS['pause_odd'][0], SPEECH[15000:15000 + 4609]]
    o = dict(ratio=1e-4, hang=0, edge=1, pause=3)
    rows, lens = _pack(xs, max_n=12001 + 77)
    x_g = G.inp(torch.from_numpy(rows), DEV, name='x')
    y_g = G.out(rows.shape, DEV, dtype=torch.float64, name='y')
    n_t = torch.from_numpy(lens).to(DEV)
    y, m, inv, k = dev_remove(x_g.t, n_t, **o, y_t=y_g.t)
    G.check_all((x_g, y_g))
    joins = 0
    for r, x in enumerate(xs):
        ref = R.remove_silence(x, **o)
        _check_row(y[r], m[r], inv[r], k[r], ref, ('ragged', r))
        ya, ma, inva, ka = dev_remove(torch.from_numpy(x[None]).to(DEV), None, **o)                     # the recording alone
        _same_bits(y[r, :len(x)], ya[0], ('alone', r))
        assert m[r] == ma[0] and k[r] == ka[0] and np.array_equal(inv[r, :k[r]], inva[0, :ka[0]])
        joins += int(np.sum(np.diff(ref['inv']) != 1))
    assert joins >= 2
    e_g = G.out((3, R.blocks_of(rows.shape[1])), DEV, dtype=torch.float64, name='e')
    _capi.check(_capi.lib().ss_op_silence_levels(_vp(x_g.t), _vp(n_t), 3, rows.shape[1], _vp(e_g.t), _stream()))
    torch.cuda.synchronize()
    e_g.check()
    for r, x in enumerate(xs):
        _same_bits(e_g.t[r, :R.blocks_of(len(x))].cpu().numpy(), R.levels(x), ('ragged levels', r))


def test_a_corrupt_map_changes_numbers_never_addresses():
    x, o = R.INPUTS['pause_odd']
    n = len(x)
    J = R.blocks_of(n)
    rows, lens = _pack([x, x[:1000], x], max_n=n + 40)
    x_g = G.inp(torch.from_numpy(rows), DEV, name='x')
    n_t = torch.from_numpy(lens).to(DEV)
    Jmax = R.blocks_of(rows.shape[1])
    rng = np.random.default_rng(9)
    for trial, (inv, k) in enumerate([
            (np.full((3, Jmax), 2 ** 31 - 1), [2 ** 31 - 1, Jmax, 3]), (np.full((3, Jmax), -2 ** 31), [-2 ** 31, 0, -1]),
            (rng.integers(-10 ** 6, 10 ** 6, (3, Jmax)), [Jmax, Jmax, Jmax]), (np.tile(np.arange(Jmax)[::-1], (3, 1)), [J, 4, 1]),
            (rng.integers(-3, Jmax + 3, (3, Jmax)), [5, 900, 7])]):
        y_g = G.out(rows.shape, DEV, dtype=torch.float64, name=f'y (trial {trial})')
        y, m = dev_gather(x_g.t, n_t, inv, k, y_t=y_g.t)
        G.check_all((x_g, y_g))                                            # nothing outside y was written, and nothing of y was left out
        assert np.all((m >= 1) & (m <= lens)), (trial, m, lens)
        for r in range(3):
            assert np.isfinite(y[r]).all(), (trial, r)                     # nothing behind n_b (NaN) was read
            assert np.all(y[r, m[r]:] == 0.0)


def test_out_of_contract_lengths_spoil_only_their_row():
    x, o = R.INPUTS['ends']
    n = len(x)
    rows = np.tile(x, (4, 1))
    lens = np.array([0, n, -5, n + 1000], np.int32)                        # row b runs with min(max(n[b], 1), max_n) samples
    y_g = G.out(rows.shape, DEV, dtype=torch.float64, name='y')
    y, m, inv, k = dev_remove(torch.from_numpy(rows).to(DEV), torch.from_numpy(lens).to(DEV), **o, y_t=y_g.t)
    y_g.check()
    whole, one = R.remove_silence(x, **o), R.remove_silence(x[:1], **o)
    for r, ref in enumerate((one, whole, one, whole)):
        _check_row(y[r], m[r], inv[r], k[r], ref, ('lengths', r))


def test_remove_silence_gives_the_same_bits_at_every_max_rows():
    opts = features.Silence(40.0, 2, 6, 8)
    xs = [SPEECH, SPEECH[5000:30000], R.INPUTS['pause_odd'][0], SPEECH[:700], np.zeros(300)]
    refs = [R.remove_silence(x, opts.ratio, opts.hang, opts.edge, opts.pause_blocks) for x in xs]
    assert refs[0]['K'] == 116
    for max_rows in (1, 2, 16):
        ys, invs = features.remove_silence(xs, opts, max_rows=max_rows, device=DEV, return_maps=True)
        assert len(ys) == len(invs) == len(xs)
        for i, ref in enumerate(refs):
            _same_bits(ys[i], ref['y'], (max_rows, i))
            assert invs[i].dtype == np.int32 and np.array_equal(invs[i], ref['inv']), (max_rows, i)
    assert [len(y) for y in features.remove_silence(xs[3:], device=DEV)] == [r['m'] for r in refs[3:]]      # the defaults: Silence()
    track = np.arange(182)                                                 # frame-rate data of the original follows by track[inv]
    assert np.array_equal(track[invs[0]], refs[0]['inv'])


@pytest.mark.parametrize('device_draws', [False, True])
def test_extract_batch_sr_equals_the_chain_on_the_trimmed_recordings(device_draws):
    opts = features.Silence(40.0, 2, 6, 8)
    x48 = signal.resample_poly(SPEECH[3000:23000], 3, 1)                  # a recording at 48 kHz: the order "resample, then trim" is pinned
    xs, srs = [SPEECH, x48, SPEECH[2000:24000]], [16000, 48000, 16000]
    at16 = [xs[0], features.resample(x48, 48000, device=DEV), xs[2]]
    trimmed = [R.remove_silence(x, opts.ratio, opts.hang, opts.edge, opts.pause_blocks)['y'] for x in at16]
    assert all(len(t) < len(x) and len(t) >= features.MIN_SAMPLES for t, x in zip(trimmed, at16))
    more = {'device_draws': True} if device_draws else {}
    a, b = np.random.RandomState(226), np.random.RandomState(226)
    got = features.extract_batch_sr(xs, srs, a, 'M', device=DEV, silence=opts, **more)
    want = features.extract_batch_sr(trimmed, 16000, b, 'M', device=DEV, **more)
    for i, ((S, f0), (S2, f02)) in enumerate(zip(got, want)):
        assert S.shape == S2.shape == (len(trimmed[i]) // 256 + 1, 80), i
        assert np.array_equal(S.view(np.int32), S2.view(np.int32)) and np.array_equal(f0.view(np.int32), f02.view(np.int32)), i
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]              # the generator ends in the same state
    # a recording that trims below the minimum is refused by its index, with its new length
    short = np.concatenate((np.random.default_rng(1).uniform(-1, 1, 100), np.random.default_rng(2).uniform(-1, 1, 1900) * 1e-4))
    with pytest.raises(ValueError, match=r'recording 1 has 256 samples after silence removal'):
        features.extract_batch_sr([SPEECH, short], 16000, np.random.RandomState(1), 'M', device=DEV,
                                  silence=features.Silence(40.0, 0, 0, None), **more)
    one = features.extract_opt(x48, np.random.RandomState(226), 'M', device=DEV, sr=48000, silence=opts)   # the per-file path trims the same
    ref = features.extract(trimmed[1], np.random.RandomState(226), 'M', DEV)
    assert np.array_equal(one[0], ref[0]) and np.array_equal(one[1], ref[1])
