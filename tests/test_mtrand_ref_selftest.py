"""mtrand_ref.py IS numpy.random.RandomState.rand -- every draw in every bit, and the generator state left behind -- and equality reports
ten wrong variants.  CPU only.

Seeds 0, 1, 225 and 2^32 - 1; start positions 0 and 1 (put there through set_state: numpy then serves the key's own first words), 2 and 623
(reached by drawing words off a fresh generator) and 624 (a fresh generator: the block is regenerated first); counts 0, 1, 2, 311, 312, 313,
624, 625 and 5000.  From an odd position a double straddles a regeneration -- its first word the last of one block, its second the first of
the next -- which is the smallest case at which that boundary can go wrong."""
import functools

import numpy as np
import pytest

from tests import mtrand_ref as R

SEEDS = [0, 1, 225, 2 ** 32 - 1]
POSITIONS = [0, 1, 2, 623, 624]
COUNTS = [0, 1, 2, 311, 312, 313, 624, 625, 5000]


@functools.lru_cache(maxsize=None)
def numpy_says(seed, pos, count):
    prng = R.generator_at(seed, pos)
    start = R.state_of(prng)
    draws = prng.rand(count)
    draws.setflags(write=False)
    return start, draws, prng


CASES = [(s, p, c) for s in SEEDS for p in POSITIONS for c in COUNTS]


@pytest.mark.parametrize('seed', SEEDS)
def test_the_restatement_is_numpy_in_every_draw_and_in_the_end_state(seed):
    for pos in POSITIONS:
        for count in COUNTS:
            start, want, prng = numpy_says(seed, pos, count)
            for fn in (R.rand, R.rand_chunked):
                got, state = fn(start, count)
                assert got.dtype == np.float64 and R.same(got, want), (fn.__name__, seed, pos, count)
                assert R.same_state(state, prng), (fn.__name__, seed, pos, count)


def test_an_odd_start_makes_a_double_straddle_a_regeneration():
    start, want, _ = numpy_says(225, 623, 2)
    a, st = R.genrand(start)
    assert st[1] == 624
    b, st = R.genrand(st)
    assert st[1] == 1 and st[0] != start[0]                                 # the second word came from the regenerated block
    assert R.to_double(a, b) == want[0]


def _reported(fn, **wrong):
    """the (seed, pos, count) cases at which the variant's draws or end state differ from numpy's"""
    hit = []
    for seed, pos, count in CASES:
        start, want, prng = numpy_says(seed, pos, count)
        got, state = fn(start, count, **wrong)
        if not (R.same(got, want) and R.same_state(state, prng)):
            hit.append((seed, pos, count))
    return hit


WRONG = [
    ('the >>5 and >>6 shifts swapped', R.rand, {'shifts_swapped': True}),
    ('the two words of a double in the other order', R.rand, {'words_swapped': True}),
    ('the >>18 tempering step dropped', R.rand, {'drop_18': True}),
    ('A applied on bit 31', R.rand, {'a_on_bit_31': True}),
    ('upper and lower masks swapped', R.rand, {'masks_swapped': True}),
    ('offset 396', R.rand, {'offset': 396}),
    ('division by 2^53 - 1', R.rand, {'divisor': 9007199254740991.0}),
    ("pos' off by one", R.rand, {'pos_off_by_one': True}),
    ('a 227-wide step that reads a stale x[n+1] at its chunk boundary', R.rand_chunked, {'stale_neighbour': True}),
    ('an end state that keeps only the consumed part of the last block', R.rand_chunked, {'keep_consumed_only': True}),
]


@pytest.mark.parametrize('what,fn,wrong', WRONG, ids=[w[0] for w in WRONG])
def test_equality_reports_the_wrong_variant(what, fn, wrong):
    hit = _reported(fn, **wrong)
    print(f'{what}: reported at {len(hit)} of {len(CASES)} cases')
    assert hit, what
    for seed in SEEDS:                                                      # at every seed, not by the luck of one
        assert any(h[0] == seed for h in hit), (what, seed)
