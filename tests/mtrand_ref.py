"""numpy.random.RandomState.rand restated: MT19937 and the conversion to double, the plain sequential definition in Python integers
(include/speechsplit_amd.h, ss_mt19937_rand).  A state is (key, pos): 624 words and a position in 0 .. 624.

    genrand(state)        -> (word, state'): one tempered 32-bit word, regenerating the whole block first when pos is 624, as numpy does
    rand(state, count)    -> (draws float64 [count], state'): draw i from two words, ((a >> 5) 2^26 + (b >> 6)) / 2^53

`rand` takes the wrong variants test_mtrand_ref_selftest.py must see reported as keyword switches; none of them is on by default.
`rand_chunked` is the arrangement the kernel uses -- 227 new words a step, the end state cut out of the running sequence -- with the mistakes
that arrangement invites as switches of its own."""
import numpy as np

N, M, A = 624, 397, 0x9908b0df
UPPER, LOWER, MASK = 0x80000000, 0x7fffffff, 0xffffffff
STEP = N - M                                                                # 227: word n + 624 needs nothing newer than n + 397


def state_of(prng):
    """(key as a list of Python integers, pos) of a numpy RandomState"""
    s = prng.get_state()
    assert s[0] == 'MT19937'
    return [int(v) for v in s[1]], int(s[2])


def generator_at(seed, pos):
    """a RandomState whose pos is `pos`: 624 fresh; 0 and 1 by set_state on the seeded key; 2 and 623 by drawing that many words"""
    prng = np.random.RandomState(seed)
    if pos in (0, 1):
        s = prng.get_state()
        prng.set_state((s[0], s[1], pos, 0, 0.0))
    elif pos != 624:
        prng.randint(0, 2 ** 32, size=pos, dtype=np.uint32)                 # one word each
    assert prng.get_state()[2] == pos
    return prng


def temper(y, drop_18=False):
    y ^= y >> 11
    y ^= (y << 7) & 0x9d2c5680
    y ^= (y << 15) & 0xefc60000
    if not drop_18:
        y ^= y >> 18
    return y & MASK


def next_word(xn, xn1, xm, a_on_bit_31=False, masks_swapped=False):
    """x[n + 624] from x[n], x[n + 1] and x[n + 397]"""
    up, low = (LOWER, UPPER) if masks_swapped else (UPPER, LOWER)
    y = (xn & up) | (xn1 & low)
    odd = (y >> 31) & 1 if a_on_bit_31 else y & 1
    return (xm ^ (y >> 1) ^ (A if odd else 0)) & MASK


def regenerate(key, offset=M, **kw):
    """the next block of 624 words, in place order: word n uses the NEW words wherever n + 1 or n + offset runs past the old block"""
    x = list(key)
    for n in range(N):
        x[n] = next_word(x[n], x[(n + 1) % N], x[(n + offset) % N], **kw)
    return x


def genrand(state, offset=M, drop_18=False, **kw):
    key, pos = state
    if pos >= N:
        key, pos = regenerate(key, offset, **kw), 0
    return temper(key[pos], drop_18), (key, pos + 1)


def to_double(a, b, shifts_swapped=False, words_swapped=False, divisor=9007199254740992.0):
    if words_swapped:
        a, b = b, a
    sa, sb = (6, 5) if shifts_swapped else (5, 6)
    return (float(a >> sa) * 67108864.0 + float(b >> sb)) / divisor


def rand(state, count, shifts_swapped=False, words_swapped=False, divisor=9007199254740992.0, pos_off_by_one=False, **kw):
    """count draws from state = (key, pos) -> (float64 [count], (key', pos')), one word at a time"""
    state = (list(state[0]), int(state[1]))
    out = np.empty(count, dtype=np.float64)
    for i in range(count):
        a, state = genrand(state, **kw)
        b, state = genrand(state, **kw)
        out[i] = to_double(a, b, shifts_swapped, words_swapped, divisor)
    if pos_off_by_one and count:
        state = (state[0], state[1] - 1)
    return out, state


def last_of_block_step(n0):
    """the word n in the step [n0, n0 + 227) with n = 623 mod 624, or -1: the chunk boundary where x[n + 1] belongs to the next block"""
    n = n0 + (N - 1 - n0) % N
    return n if n < n0 + STEP else -1


def rand_chunked(state, count, stale_neighbour=False, keep_consumed_only=False):
    """the same draws from the running sequence x[0 .. 623] = key, x[n + 624] = next_word(x[n], x[n + 1], x[n + 397]), built 227 words a step
    from a snapshot of what was there before the step; stream word j is temper(x[pos + j]); the end state is x[624 k .. 624 k + 623] and
    pos + 2 count - 624 k for k = (pos + 2 count - 1) // 624 (count == 0: the state as it was).
    stale_neighbour: the last word of the step that reaches the end of a block of 624 (n = 623 mod 624, whose x[n + 1] is the first word of the
    NEXT block, written a few steps earlier) takes the word that slot held one block before, as an array of 624 read too early would.
    keep_consumed_only: the end state carries the new block only as far as it was consumed, the old key behind that."""
    key, pos = list(state[0]), min(int(state[1]), N)
    if count == 0:
        return np.empty(0), (key, int(state[1]))
    tot = pos + 2 * count
    k = (tot - 1) // N
    x = key + [0] * (k * N)
    for n0 in range(0, k * N, STEP):
        for n in range(n0, min(n0 + STEP, k * N)):
            n1 = n + 1
            if stale_neighbour and n == last_of_block_step(n0):
                n1 -= N
            x[n + N] = next_word(x[n], x[n1], x[n + M])
    out = np.array([to_double(temper(x[pos + 2 * i]), temper(x[pos + 2 * i + 1])) for i in range(count)], dtype=np.float64)
    last = x[k * N:k * N + N]
    if keep_consumed_only and k:
        used = tot - k * N
        last = last[:used] + x[(k - 1) * N + used:k * N]
    return out, (last, tot - k * N)


def same(a, b):
    """float64 arrays equal in every bit"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_state(state, prng):
    """(key, pos) equals the numpy generator's"""
    key, pos = state_of(prng)
    return list(state[0]) == key and int(state[1]) == pos
