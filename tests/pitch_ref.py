"""float64 numpy restatement of the pitch tracker (include/speechsplit_amd.h, "pitch tracker"; csrc/pitch.hip), written against the
header's text and not against the kernel: Talkin's RAPT core -- normalised cross-correlation candidates plus dynamic programming (Talkin
1995, "A robust algorithm for pitch tracking") -- with his published constants, without the spectral-stationarity term and the two-rate
search.  It is NOT a restatement of SPTK's rapt.

    nccf(x, lo, hi)        phi [F, K], rms [F]            the frame-independent half
    candidates(phi_i, ..)  [(L, v)] of one frame, state order
    dp(phi, rms, lo, hi)   f0 [F]                        the sequential half: ln(16000 / L), -1e10 for unvoiced frames
    track(x, lo, hi)       dp(*nccf(x, lo, hi), lo, hi)
    divergence(x, lo, hi)  the disagreement of nccf with itself under two summation orders: the scale of a parity bound
    margins(x, lo, hi)     how far the inputs are from a decision that rounding could flip

`variant` selects one of the WRONG stand-ins (test_pitch_ref_selftest.py proves each is reported); None is the algorithm."""
import math

import numpy as np

FS, HOP, W = 16000, 256, 120
CAND_TR, N_CANDS, LAG_WT, FREQ_WT, DOUBL_C, VTRAN_C, VTR_A_C, VO_BIAS, A_FACT = 0.3, 20, 0.3, 0.02, 0.35, 0.005, 0.5, 0.0, 10000.0
UNVOICED = -1e10
LN2 = math.log(2.0)
WRONG = ('no_mean', 'no_afact', 'no_lag_weight', 'lag_off_by_one', 'no_parabola', 'no_doubling', 'vtrans_swapped', 'tie_reversed', 'no_cap',
         'not_centred')


def lag_range(lo, hi):
    """(Lmin, Lmax, K)"""
    lmin, lmax = int(math.floor(FS / hi)), int(math.ceil(FS / lo))
    return lmin, lmax, lmax - lmin + 1


def frames_of(n):
    return n // HOP + 1


def _seq_sum(a, axis_len):
    """sum over the last axis, one term after the other"""
    acc = np.zeros(a.shape[:-1])
    for j in range(axis_len):
        acc = acc + a[..., j]
    return acc


def nccf(x, lo, hi, scale=32768.0, order='dot', variant=None):
    """phi [F, K] and rms [F] of the header's steps 1 and 2.  order 'dot': every sum through numpy's own reductions (np.sum, matmul);
    'seq': every sum term by term in index order."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    lmin, lmax, K = lag_range(lo, hi)
    S, F = W + lmax, frames_of(n)
    start = HOP * np.arange(F) - (0 if variant == 'not_centred' else S // 2)
    idx = start[:, None] + np.arange(S)[None, :]
    z = np.where((idx >= 0) & (idx < n), scale * x[np.clip(idx, 0, n - 1)], 0.0)
    total = z.sum(axis=1) if order == 'dot' else _seq_sum(z, S)
    y = z if variant == 'no_mean' else z - (total / S)[:, None]
    sq = y * y
    rms = np.sqrt((sq.sum(axis=1) if order == 'dot' else _seq_sum(sq, S)) / S + 1.0)
    ks = np.arange(lmin, lmax + 1) + (1 if variant == 'lag_off_by_one' else 0)
    ks = np.minimum(ks, lmax)                                            # (the stand-in's last lag stays inside the segment)
    head = y[:, :W]
    if order == 'dot':
        win = np.lib.stride_tricks.sliding_window_view(y, W, axis=1)     # [F, S - W + 1, W]: win[:, k] = y[k : k + W]
        tail = win[:, ks]
        num = np.matmul(tail, head[:, :, None])[:, :, 0]
        e = np.matmul(tail[:, :, None, :], tail[:, :, :, None])[:, :, 0, 0]
        e0 = np.matmul(head[:, None, :], head[:, :, None])[:, 0, 0]
    else:
        num, e, e0 = np.zeros((F, K)), np.zeros((F, K)), np.zeros(F)
        for j in range(W):
            shifted = y[:, ks + j]
            num = num + head[:, j:j + 1] * shifted
            e = e + shifted * shifted
            e0 = e0 + head[:, j] * head[:, j]
    phi = num / np.sqrt(e0[:, None] * e + (0.0 if variant == 'no_afact' else A_FACT))
    return phi, rms


def candidates(phi, lmin, lmax, variant=None):
    """step 3 for one frame's phi [K]: [(L, v)] in state order (state a is entry a - 1), and max_k phi_k"""
    phimax = float(phi.max())
    found = []
    for i in range(1, phi.shape[0] - 1):                                # Lmin < k < Lmax
        p, c, q = float(phi[i - 1]), float(phi[i]), float(phi[i + 1])
        if not (c > p and c >= q and c > 0.0 and c >= CAND_TR * phimax):
            continue
        k = lmin + i
        den = p - 2.0 * c + q
        delta = 0.5 * (p - q) / den if den < 0.0 and variant != 'no_parabola' else 0.0
        found.append((k + delta, c - 0.25 * (p - q) * delta, k))
    found.sort(key=(lambda t: (-t[1], -t[2])) if variant == 'tie_reversed' else (lambda t: (-t[1], t[2])))
    if variant != 'no_cap':
        found = found[:N_CANDS - 1]
    return [(L, v) for L, v, _ in found], phimax


def _lattice(phi, lmin, lmax, variant=None):
    """per frame: L [1 + m] (entry 0 unused) and the local costs d [1 + m] of step 4"""
    Ls, ds = [], []
    for i in range(phi.shape[0]):
        cand, phimax = candidates(phi[i], lmin, lmax, variant)
        L = np.array([1.0] + [c[0] for c in cand])
        v = np.array([0.0] + [c[1] for c in cand])
        d = 1.0 - v * (1.0 - (0.0 if variant == 'no_lag_weight' else LAG_WT) * L / lmax)
        d[0] = VO_BIAS + max(phimax, 0.0)
        Ls.append(L)
        ds.append(d)
    return Ls, ds


def _transitions(Lb, La, rr, variant=None):
    """t [from b, to a] between two frames; rr = rms_i / rms_{i-1}"""
    xi = np.log(La[None, :] / Lb[:, None])
    t = np.abs(xi)
    if variant != 'no_doubling':
        t = np.minimum(t, np.minimum(DOUBL_C + np.abs(xi - LN2), DOUBL_C + np.abs(xi + LN2)))
    t = FREQ_WT * t
    up, down = VTRAN_C + VTR_A_C / rr, VTRAN_C + VTR_A_C * rr            # unvoiced -> voiced, voiced -> unvoiced
    if variant == 'vtrans_swapped':
        up, down = down, up
    t[0, :] = up
    t[:, 0] = down
    t[0, 0] = 0.0
    return t


def _argmin(a, variant=None):
    """the lowest index on a tie"""
    return int(len(a) - 1 - np.argmin(a[::-1])) if variant == 'tie_reversed' else int(np.argmin(a))


def dp(phi, rms, lo, hi, variant=None):
    """the sequential half on phi [F, K], rms [F]: f0 [F]"""
    lmin, lmax, K = lag_range(lo, hi)
    phi, rms = np.asarray(phi, np.float64), np.asarray(rms, np.float64)
    assert phi.shape[1] == K
    Ls, ds = _lattice(phi, lmin, lmax, variant)
    F = len(Ls)
    D, back = ds[0].copy(), []
    for i in range(1, F):
        tot = D[:, None] + _transitions(Ls[i - 1], Ls[i], rms[i] / rms[i - 1], variant)
        bp = np.array([_argmin(tot[:, a], variant) for a in range(tot.shape[1])])
        D = ds[i] + tot[bp, np.arange(tot.shape[1])]
        back.append(bp)
    state = _argmin(D, variant)
    f0 = np.empty(F)
    for i in range(F - 1, -1, -1):
        f0[i] = math.log(FS / Ls[i][state]) if state else UNVOICED
        if i:
            state = int(back[i - 1][state])
    return f0


def track(x, lo, hi, scale=32768.0, variant=None):
    phi, rms = nccf(x, lo, hi, scale, 'dot', variant)
    return dp(phi, rms, lo, hi, variant)


def voiced(f0):
    return np.asarray(f0) != UNVOICED


def rel_diff(a, b):
    """max |a - b| over max |b|"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(b).max()), 1e-300))


def divergence(x, lo, hi, scale=32768.0):
    """max |phi_dot - phi_seq| (phi is O(1)) and max relative |rms_dot - rms_seq|, the larger of the two"""
    pa, ra = nccf(x, lo, hi, scale, 'dot')
    pb, rb = nccf(x, lo, hi, scale, 'seq')
    return max(float(np.abs(pa - pb).max()), float((np.abs(ra - rb) / rb).max()))


def margins(x, lo, hi, scale=32768.0):
    """(path margin, candidate-rule gap) of a waveform: margins_phi of its NCCF"""
    return margins_phi(*nccf(x, lo, hi, scale), lo, hi)


def margins_phi(phi, rms, lo, hi):
    """(path margin, candidate-rule gap).
    Path margin: min over frames of [the cheapest complete path through any OTHER state of that frame] - [the best path's cost], by a
    forward and a backward min-sum pass.  Candidate-rule gap: the smallest |phi_k - CAND_TR phimax| over the local maxima (the other four
    conditions of step 3 hold) and the smallest v_19 - v_20 where a frame has more than 19 candidates.  A rounding difference below both
    cannot change a decision."""
    lmin, lmax, K = lag_range(lo, hi)
    F = phi.shape[0]
    gap = math.inf
    for i in range(F):
        p = phi[i]
        phimax = float(p.max())
        mid = p[1:-1]
        peak = (mid > p[:-2]) & (mid >= p[2:]) & (mid > 0.0)
        if peak.any():
            gap = min(gap, float(np.abs(mid[peak] - CAND_TR * phimax).min()))
        cand, _ = candidates(p, lmin, lmax, 'no_cap')
        if len(cand) >= N_CANDS:
            gap = min(gap, cand[N_CANDS - 2][1] - cand[N_CANDS - 1][1])
    Ls, ds = _lattice(phi, lmin, lmax)
    T = [None] + [_transitions(Ls[i - 1], Ls[i], rms[i] / rms[i - 1]) for i in range(1, F)]
    alpha = [ds[0]]
    for i in range(1, F):
        alpha.append(ds[i] + (alpha[-1][:, None] + T[i]).min(axis=0))
    beta = [None] * F
    beta[F - 1] = np.zeros(len(ds[F - 1]))
    for i in range(F - 2, -1, -1):
        beta[i] = (T[i + 1] + (ds[i + 1] + beta[i + 1])[None, :]).min(axis=1)
    best = float(alpha[F - 1].min())
    margin = math.inf
    for i in range(F):
        through = np.sort(alpha[i] + beta[i])
        assert abs(through[0] - best) <= 1e-9 * max(1.0, abs(best))
        if len(through) > 1:
            margin = min(margin, float(through[1] - best))
    return margin, gap


def most_peaks(x, lo, hi, scale=32768.0):
    """the largest number of qualifying peaks (step 3, before the cap) in one frame"""
    lmin, lmax, _ = lag_range(lo, hi)
    return max(len(candidates(p, lmin, lmax, 'no_cap')[0]) for p in nccf(x, lo, hi, scale)[0])


# ---------------------------------------------------------------------------------------------- test signals
def tone(f0, n=FS, harmonics=5, amp=0.2):
    """sum_{h <= harmonics} amp / h sin(2 pi f0 h t)"""
    t = np.arange(n) / FS
    return sum(amp / h * np.sin(2.0 * np.pi * f0 * h * t) for h in range(1, harmonics + 1))


def composite():
    """quiet noise, a seven-harmonic glide 130 -> 145 Hz, louder noise, the glide reversed at half amplitude, zeros; 1e-3 noise over all"""
    rng = np.random.RandomState(3)
    f = np.linspace(130.0, 145.0, 4096)
    ph = 2.0 * np.pi * np.cumsum(f) / FS
    glide = sum(0.2 / h * np.sin(h * ph) for h in range(1, 8))
    parts = [1e-4 * rng.randn(2048), glide, 0.05 * rng.randn(3072), 0.5 * glide[::-1], np.zeros(1500)]
    x = np.concatenate(parts)
    return x + 1e-3 * rng.randn(x.shape[0])


def tie_case(lo=50.0, hi=250.0, frames=3):
    """phi [frames, K], rms: every frame holds the same two peaks (no refinement: equal neighbours) whose local costs are EQUAL to the bit,
    both below the unvoiced cost.  Staying costs nothing and changing does, so D(1) == D(2) at every frame and only the tie rule decides:
    the lowest state, which is the peak with the larger v.  Returns (phi, rms, ln(16000 / that peak's lag))."""
    lmin, lmax, K = lag_range(lo, hi)
    k1, k2 = lmin + 40, lmin + 150
    v1 = 0.8125
    target = 1.0 - v1 * (1.0 - LAG_WT * k1 / lmax)
    v2 = (1.0 - target) / (1.0 - LAG_WT * k2 / lmax)
    for _ in range(64):                                                  # walk the last bits until the two costs are the same double
        got = 1.0 - v2 * (1.0 - LAG_WT * k2 / lmax)
        if got == target:
            break
        v2 = np.nextafter(v2, 0.0 if got < target else 2.0)
    assert 1.0 - v2 * (1.0 - LAG_WT * k2 / lmax) == target and v2 > v1
    row = np.zeros(K)
    row[k1 - lmin], row[k2 - lmin] = v1, v2
    # state 1 is k2 (the larger v)
    return np.tile(row, (frames, 1)), np.ones(frames), math.log(FS / k2)


def _peaks(rows, lo, hi):
    """phi [len(rows), K] with isolated peaks {lag: value} (zero neighbours: no refinement, v = phi_k), and rms = 1"""
    lmin, _, K = lag_range(lo, hi)
    phi = np.zeros((len(rows), K))
    for i, row in enumerate(rows):
        for k, v in row.items():
            phi[i, k - lmin] = v
    return phi, np.ones(len(rows))


def cap_case():
    """(phi, rms) in (50, 250) whose middle frame has twenty peaks: nineteen at long lags and, with the SMALLEST v, one at lag 70, where the
    frames around it have their only peak.  The lag weight makes lag 70 the cheapest state of that frame, but it is the twentieth
    candidate: the cap drops it, and the best path has to leave lag 70 for one frame."""
    middle = {250 + 3 * i: 0.70 + 0.001 * i for i in range(19)}
    middle[70] = 0.69
    return _peaks([{70: 0.9}, middle, {70: 0.9}], 50.0, 250.0)


def doubling_case():
    """(phi, rms) in (50, 250): two frames at lag 100, then a choice between lag 200 (an octave down: the doubling term makes the jump cost
    FREQ_WT DOUBL_C instead of FREQ_WT ln 2) and lag 130, with local costs that make lag 200 win by 0.003 with the term and lose without"""
    return _peaks([{100: 0.9}, {100: 0.9}, {200: 0.8708, 130: 0.8}], 50.0, 250.0)
