"""Numpy restatement of ss_remove_silence (include/speechsplit_amd.h): trim the ends of a recording and cap its pauses, in float64, with
the operations in the header's order so that it IS the definition to the bit -- Python floats and explicit loops wherever the order of a sum
matters (numpy's elementwise add and multiply are the same IEEE operations; its reductions are not used: they sum pairwise).

    levels(x)                              -> E [J]           quarter sums in order, then the 512-sample window's four quarters in order
    mask(E, ratio, hang, edge, pause)      -> inv [K]         the strict threshold, the hangover, the run rules
    gather(x, inv, g)                      -> y [m]           the kept blocks, with the cross-fade at every join
    remove_silence(x, ratio, hang, ...)    -> dict(y, m, inv, K, E)

`variant` switches in ONE deliberate mistake (VARIANTS); tests/test_silence_ref_selftest.py shows that each is reported on the input named
for it in VARIANT_INPUTS, so a kernel that made the same mistake would be caught by the GPU tests' bit comparison."""
import math

import numpy as np

BLOCK, QUARTER, FADE = 256, 128, 128

VARIANTS = ('ge_for_gt', 'no_leading_quarter', 'one_sided_hangover', 'leading_keeps_first', 'trailing_keeps_last', 'halves_swapped',
            'r_ge_pause', 'fade_from_block_a', 'g_without_half', 'fade_256', 'fade_not_clamped', 'emax_active_only', 'mean_for_sum')


def fade_gains(variant=None):
    """g[r] = 0.5 - 0.5 cos(pi (r + 0.5) / 128) with the C library's cosine; float64 [128] (the variants: another length or phase)"""
    n = 256 if variant == 'fade_256' else FADE
    half = 0.0 if variant == 'g_without_half' else 0.5
    return np.array([0.5 - 0.5 * math.cos(math.pi * (r + half) / n) for r in range(n)], dtype=np.float64)


def ratio_of(top_db):
    """what the Python layer passes for a threshold top_db decibels below the loudest block"""
    return 10.0 ** (-top_db / 10.0)


def blocks_of(n):
    return -(-n // BLOCK)


def block_len(j, n):
    return min(BLOCK, n - BLOCK * j)


def quarter_sums(x):
    """Q_q = sum of x[i]^2 over the quarter's own samples, in order, starting from its first term"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    sq = x * x                                                              # every product rounded on its own
    Q = np.zeros(-(-n // QUARTER))
    for q in range(Q.shape[0]):
        acc = float(sq[QUARTER * q])
        for i in range(QUARTER * q + 1, min(QUARTER * q + QUARTER, n)):
            acc = acc + float(sq[i])
        Q[q] = acc
    return Q


def levels(x, variant=None):
    """E_j = ((Q_{2j-1} + Q_{2j}) + Q_{2j+1}) + Q_{2j+2}: the quarters that exist, in that order"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    assert x.ndim == 1 and n >= 1
    Q = quarter_sums(x)
    E = np.zeros(blocks_of(n))
    for j in range(E.shape[0]):
        acc, count = None, 0
        for q in range(2 * j if variant == 'no_leading_quarter' else 2 * j - 1, 2 * j + 3):
            if 0 <= q < Q.shape[0]:
                acc = float(Q[q]) if acc is None else acc + float(Q[q])
                count += min(QUARTER, n - QUARTER * q)
        E[j] = acc / count if variant == 'mean_for_sum' else acc
    return E


def activity(E, ratio, variant=None):
    """a_j = E_j > ratio * E_max, strictly; E_max is NaN if a level is"""
    E = np.asarray(E, np.float64)
    if variant == 'emax_active_only':                                      # one pass: each block against the loudest active block so far
        a, top = np.zeros(E.shape[0], bool), -math.inf
        for j in range(E.shape[0]):
            if float(E[j]) > ratio * max(top, float(E[j])):
                a[j], top = True, max(top, float(E[j]))
        return a
    emax = math.nan if np.isnan(E).any() else float(E.max())
    thr = ratio * emax
    return np.array([float(v) >= thr if variant == 'ge_for_gt' else float(v) > thr for v in E], bool)


def mask(E, ratio, hang, edge, pause, variant=None):
    """inv int32 [K]: the kept blocks, ascending"""
    a = activity(E, ratio, variant)
    J = a.shape[0]
    if not a.any():
        return np.arange(J, dtype=np.int32)
    d = np.zeros(J, bool)
    for j in np.flatnonzero(a):
        d[max(j - hang, 0):(j + 1 if variant == 'one_sided_hangover' else j + hang + 1)] = True
    keep = d.copy()
    j = 0
    while j < J:
        if d[j]:
            j += 1
            continue
        s = j
        while j < J and not d[j]:
            j += 1
        t, R = j - 1, j - s                                                 # the run is blocks s .. t
        if s == 0:
            k = min(R, edge)
            if variant == 'leading_keeps_first':
                keep[s:s + k] = True
            else:
                keep[t + 1 - k:t + 1] = True
        elif t == J - 1:
            k = min(R, edge)
            if variant == 'trailing_keeps_last':
                keep[t + 1 - k:t + 1] = True
            else:
                keep[s:s + k] = True
        elif pause < 0 or (R >= pause if variant == 'r_ge_pause' else R <= pause):      # (cutting at R == pause keeps all its blocks: no mistake)
            keep[s:t + 1] = True
        else:
            first, last = (pause + 1) // 2, pause // 2
            if variant == 'halves_swapped':
                first, last = last, first
            keep[s:s + first] = True
            keep[t + 1 - last:t + 1] = True
    return np.flatnonzero(keep).astype(np.int32)


def gather(x, inv, g=None, variant=None):
    """y float64 [m]: output block c is block inv[c]; at a join its first min(128, its length) samples are
    x[256 (a + 1) + r] * (1.0 - g[r]) + x[256 inv[c] + r] * g[r], a = inv[c-1]: the difference and the two products first, then their sum"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    g = fade_gains(variant) if g is None else np.asarray(g, np.float64)
    K = len(inv)
    m = BLOCK * (K - 1) + block_len(int(inv[K - 1]), n)
    if variant == 'fade_not_clamped' and K > 1 and inv[K - 2] + 1 != inv[K - 1]:
        m = max(m, BLOCK * (K - 1) + len(g))
    y = np.zeros(m)
    xz = np.concatenate((x, np.zeros(BLOCK)))                               # only the variant reads behind n
    for c in range(K):
        s = int(inv[c])
        L = block_len(s, n)
        y[BLOCK * c:BLOCK * c + L] = x[BLOCK * s:BLOCK * s + L]
        if c > 0 and inv[c - 1] + 1 != s:
            a = int(inv[c - 1])
            tail = BLOCK * a if variant == 'fade_from_block_a' else BLOCK * (a + 1)
            for r in range(len(g) if variant == 'fade_not_clamped' else min(len(g), L)):
                og = 1.0 - float(g[r])
                p = float(xz[tail + r]) * og
                q = float(xz[BLOCK * s + r]) * float(g[r])
                y[BLOCK * c + r] = p + q
    return y


def remove_silence(x, ratio, hang=2, edge=6, pause=-1, g=None, variant=None):
    x = np.asarray(x, np.float64)
    E = levels(x, variant)
    inv = mask(E, ratio, hang, edge, pause, variant)
    y = gather(x, inv, g, variant)
    return dict(y=y, m=y.shape[0], inv=inv, K=inv.shape[0], E=E)


def reported(ref, got, x):
    """the selftest's and the issue's notion of a mistake being seen: another inv, K or m, or a sample at least 1e-9 of max |x| away"""
    if ref['K'] != got['K'] or ref['m'] != got['m'] or not np.array_equal(ref['inv'], got['inv']):
        return True
    return bool(np.max(np.abs(ref['y'] - got['y'])) >= 1e-9 * np.max(np.abs(x)))


# ---------------------------------------------------------------------------------------------- named inputs
def pattern(amps, last=BLOCK, seed=0):
    """one block of seeded uniform noise per entry of amps, scaled by it; the last block has `last` samples"""
    rng = np.random.default_rng(seed)
    n = BLOCK * (len(amps) - 1) + last
    return rng.uniform(-1.0, 1.0, n) * np.repeat(np.asarray(amps, np.float64), BLOCK)[:n]


def steps(amps, last=BLOCK):
    """the same with constant blocks: every square and every sum of them is exact when the amplitudes are powers of two"""
    n = BLOCK * (len(amps) - 1) + last
    return np.repeat(np.asarray(amps, np.float64), BLOCK)[:n].copy()


Q, L = 1e-4, 1.0            # a quiet and a loud block of `pattern`
# name -> (x, dict(ratio, hang, edge, pause)); the third entry, where present, is a crafted inv for `gather` alone
INPUTS = {
    # blocks 5 .. 8 lie wholly inside the 0.25 stretch: E = 512 / 16 = ratio * E_max EXACTLY, so they are silent under > and active under >=
    'tie': (steps([1.0] * 4 + [0.25] * 6), dict(ratio=2.0 ** -4, hang=0, edge=0, pause=-1)),
    'ends': (pattern([Q] * 6 + [L] * 3 + [Q] * 6, last=200, seed=1), dict(ratio=1e-4, hang=0, edge=2, pause=-1)),
    'ends_hang': (pattern([Q] * 6 + [L] * 3 + [Q] * 6, last=200, seed=2), dict(ratio=1e-4, hang=2, edge=0, pause=-1)),
    'pause_odd': (pattern([L] * 3 + [Q] * 8 + [L] * 3, seed=3), dict(ratio=1e-4, hang=0, edge=0, pause=3)),
    'pause_exact': (pattern([L] * 3 + [Q] * 8 + [L] * 3, seed=4), dict(ratio=1e-4, hang=0, edge=0, pause=6)),
    # a constant signal and a 3 dB threshold: the window of the short last block holds 185 samples of 512, so its SUM is below half the maximum
    'flat': (steps([1.0] * 6, last=57), dict(ratio=0.5, hang=0, edge=0, pause=-1)),
    # gather alone: a join directly before a short last block of 57 samples
    'short_join': (pattern([L, L, Q, Q, Q, L], last=57, seed=5), dict(ratio=1e-4, hang=0, edge=0, pause=-1), np.array([0, 1, 5], np.int32)),
}
VARIANT_INPUTS = {'ge_for_gt': 'tie', 'no_leading_quarter': 'ends', 'one_sided_hangover': 'ends_hang', 'leading_keeps_first': 'ends',
                  'trailing_keeps_last': 'ends', 'halves_swapped': 'pause_odd', 'r_ge_pause': 'pause_odd', 'fade_from_block_a': 'pause_odd',
                  'g_without_half': 'pause_odd', 'fade_256': 'pause_odd', 'fade_not_clamped': 'short_join', 'emax_active_only': 'ends',
                  'mean_for_sum': 'flat'}


def run_named(name, variant=None):
    """the restatement (or a variant of it) on a named input: the whole chain, or `gather` alone where the input brings its own inv"""
    entry = INPUTS[name]
    x, opts = entry[0], entry[1]
    if len(entry) == 3:
        y = gather(x, entry[2], None, variant)
        return dict(y=y, m=y.shape[0], inv=entry[2], K=len(entry[2]), E=None)
    return remove_silence(x, variant=variant, **opts)


def speech_signal(feats):
    """the GPU tests' recording: seeded noise at 1e-4, the fixture's u0_x, noise, u1_x, noise (feats: tests/golden/features.npz)"""
    rng = np.random.default_rng(7)
    noise = lambda n: rng.standard_normal(n) * 1e-4
    return np.concatenate((noise(8000), feats['u0_x'], noise(8000), feats['u1_x'], noise(8000)))
