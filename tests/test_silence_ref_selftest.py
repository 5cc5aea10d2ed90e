"""CPU-only checks of the numpy restatement of silence removal (tests/silence_ref.py), which the GPU tests compare with to the bit: each
stage against an independent second form, the properties the definition promises, and every deliberate mistake (silence_ref.VARIANTS)
reported on the input named for it."""
import os

import numpy as np
import pytest

import silence_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OPTS = [dict(ratio=1e-4, hang=2, edge=6, pause=8), dict(ratio=1e-4, hang=0, edge=0, pause=0), dict(ratio=1e-3, hang=1, edge=2, pause=3),
        dict(ratio=1e-4, hang=3, edge=1, pause=-1), dict(ratio=0.5, hang=0, edge=0, pause=2)]


@pytest.fixture(scope='module')
def speech():
    return R.speech_signal(np.load(os.path.join(GOLD, 'features.npz')))


def _signals(speech):
    rng = np.random.default_rng(11)
    out = [v[0] for v in R.INPUTS.values()] + [speech[7000:21000], speech[:9001]]
    for n in (1, 127, 128, 129, 255, 256, 257, 384, 511, 512, 513, 769):
        out.append(rng.uniform(-1, 1, n) * np.where(rng.uniform(size=n) < 0.5, 1.0, 1e-3))
    return out


# ---------------------------------------------------------------------------------------------- second forms
def levels_reduceat(x):
    """the window energies from numpy's own (pairwise) sums: another order, so equal only within rounding"""
    n = x.shape[0]
    Q = np.add.reduceat(x * x, np.arange(0, n, R.QUARTER))
    Qp = np.concatenate(([0.0], Q, [0.0, 0.0, 0.0]))                        # Q_{-1} and those beyond the last count as nothing
    J = R.blocks_of(n)
    return np.array([Qp[2 * j:2 * j + 4].sum() for j in range(J)])


def mask_brute(E, ratio, hang, edge, pause):
    """the rule for each block on its own: look outwards from j for the ends of its run"""
    J = len(E)
    a = [bool(E[j] > ratio * np.max(E)) for j in range(J)]
    if not any(a):
        return np.arange(J, dtype=np.int32)
    d = [any(a[i] for i in range(J) if abs(i - j) <= hang) for j in range(J)]
    kept = []
    for j in range(J):
        if d[j]:
            kept.append(j)
            continue
        s = j
        while s > 0 and not d[s - 1]:
            s -= 1
        t = j
        while t < J - 1 and not d[t + 1]:
            t += 1
        run = t - s + 1
        pos, back = j - s, t - j                                           # blocks of the run in front of j and behind it
        if s == 0:
            ok = back < min(run, edge)
        elif t == J - 1:
            ok = pos < min(run, edge)
        elif pause < 0 or run <= pause:
            ok = True
        else:
            ok = pos < -(-pause // 2) or back < pause // 2
        if ok:
            kept.append(j)
    return np.array(kept, np.int32)


def gather_slices(x, inv):
    """slices of x concatenated, the cross-fades as whole-array expressions"""
    g = R.fade_gains()
    n, parts = x.shape[0], []
    for c, s in enumerate(inv):
        blk = x[256 * s:min(256 * s + 256, n)].copy()
        if c and inv[c - 1] + 1 != s:
            k = min(128, blk.shape[0])
            tail = x[256 * (inv[c - 1] + 1):256 * (inv[c - 1] + 1) + k]
            blk[:k] = tail * (1.0 - g[:k]) + blk[:k] * g[:k]
        parts.append(blk)
    return np.concatenate(parts)


def test_levels_agree_with_reduceat_sums(speech):
    for x in _signals(speech):
        E, E2 = R.levels(x), levels_reduceat(x)
        assert E.shape == E2.shape == (R.blocks_of(len(x)),)
        assert np.all(np.abs(E - E2) <= 1e-12 * np.abs(E2)), len(x)


def test_mask_equals_the_per_block_rule(speech):
    rng = np.random.default_rng(5)
    lattices = [R.levels(x) for x in _signals(speech)]
    for J in (1, 2, 3, 7, 40, 130):                                        # random two-level lattices: every run length and position
        for _ in range(6):
            lattices.append(np.where(rng.uniform(size=J) < 0.4, 1.0, 1e-6) * rng.uniform(0.5, 1.0, J))
    lattices += [np.zeros(9), np.full(5, np.inf)]
    for E in lattices:
        for o in OPTS:
            assert np.array_equal(R.mask(E, **o), mask_brute(E, **o)), (len(E), o)


def test_gather_equals_slicing_and_concatenation(speech):
    for x in _signals(speech):
        for o in OPTS:
            r = R.remove_silence(x, **o)
            assert np.array_equal(r['y'], gather_slices(x, r['inv'])), (len(x), o)
    x, _, inv = R.INPUTS['short_join']
    assert np.array_equal(R.gather(x, inv), gather_slices(x, inv)) and len(R.gather(x, inv)) == 512 + 57


# ---------------------------------------------------------------------------------------------- properties
def test_copied_blocks_are_the_source_to_the_bit_and_m_never_exceeds_n(speech):
    joins = 0
    for x in _signals(speech):
        for o in OPTS:
            r = R.remove_silence(x, **o)
            inv, y, n = r['inv'], r['y'], len(x)
            assert r['m'] == len(y) <= n and r['K'] == len(inv) >= 1
            assert np.all(np.diff(inv) > 0) and inv[0] >= 0 and inv[-1] < R.blocks_of(n)
            assert r['m'] == 256 * (r['K'] - 1) + R.block_len(int(inv[-1]), n)
            for c, s in enumerate(inv):
                src = x[256 * s:256 * s + R.block_len(int(s), n)]
                got = y[256 * c:256 * c + len(src)]
                if c == 0 or inv[c - 1] + 1 == s:
                    assert np.array_equal(got, src)
                else:
                    joins += 1
                    assert np.array_equal(got[128:], src[128:])
    assert joins >= 5                                                      # the join branch above did run


def test_identities(speech):
    for x in _signals(speech):
        J = R.blocks_of(len(x))
        r = R.remove_silence(x, 1e-4, hang=1, edge=J, pause=-1)           # only trims, and the edge keeps every block: nothing goes
        assert r['K'] == J and np.array_equal(r['y'], x)
    for n in (1, 300, 2048):
        r = R.remove_silence(np.zeros(n), 1e-4, 2, 0, 0)                  # E_max == 0: no block is active, every block is kept
        assert r['K'] == R.blocks_of(n) and np.array_equal(r['y'], np.zeros(n))


def test_a_second_pass_removes_nothing_more(speech):
    o = dict(ratio=R.ratio_of(40.0), hang=2, edge=6, pause=8)
    first = R.remove_silence(speech, **o)
    assert (len(first['E']), first['K'], int(np.sum(np.diff(first['inv']) != 1))) == (182, 116, 1)
    second = R.remove_silence(first['y'], **o)
    assert second['K'] == first['K'] and second['m'] == first['m']
    thr = o['ratio'] * first['E'].max()                                    # no level sits near the threshold: the GPU comparison is not a coin toss
    assert not np.any((first['E'] > 0.99 * thr) & (first['E'] < thr / 0.99))


# ---------------------------------------------------------------------------------------------- the deliberate mistakes
def test_there_are_at_least_twelve_variants_each_with_a_named_input():
    assert len(R.VARIANTS) >= 12 and set(R.VARIANTS) == set(R.VARIANT_INPUTS)
    assert all(name in R.INPUTS for name in R.VARIANT_INPUTS.values())


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_every_wrong_variant_is_reported(variant):
    name = R.VARIANT_INPUTS[variant]
    assert R.reported(R.run_named(name), R.run_named(name, variant), R.INPUTS[name][0]), (variant, name)


def test_the_tie_input_ties_exactly():
    x, o = R.INPUTS['tie']
    E = R.levels(x)
    assert E.max() == 512.0 and np.all(E[5:9] == o['ratio'] * E.max())
    assert R.mask(E, **o).tolist() == [0, 1, 2, 3, 4]
