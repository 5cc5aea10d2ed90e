"""float64 numpy restatement of the pitch tracker's spectral-stationarity term (include/speechsplit_amd.h, "spectral stationarity";
csrc/pitch.hip: stat_kernel and dp_kernel<STAT>), written against the header's text and not against the kernel: Talkin 1995 and get_f0's
get_stationarity / get_similarity as published, with the published constants.  Everything shared with the tracker -- the NCCF, the
candidates, the lattice, the frequency transitions, the tie rule, the test signals -- is pitch_ref.py's, unchanged.

    stationarity(x, n_frames, scale)     S [F]: per frame i >= 1 the Itakura distortion of the LPC predictor of the window 20 ms AFTER the
                                         frame on the signal of the window 20 ms BEFORE it, as 0.2 / (max(d, 1) - 0.8); S_0 = 0
    dp_stat(phi, rms, S, lo, hi)         pitch_ref.dp with VTR_S_C S_i added to both voicing transitions into frame i
    track_stat(x, lo, hi)                dp_stat(*nccf(x), stationarity(x), lo, hi)
    divergence_stat(x)                   max |S_dot - S_seq|: the disagreement of stationarity with itself under two summation orders
    margins_stat(phi, rms, S, lo, hi)    pitch_ref.margins_phi's forward / backward path margin, with the new transitions
    stat_case()                          a lattice on which the term alone decides whether a two-frame dip stays voiced

`variant` selects one of the WRONG stand-ins (test_pitch_stat_ref_selftest.py proves each is reported); None is the algorithm."""
import math

import numpy as np

from tests import pitch_ref as R

STAT_W, STAT_GAP, LPC_ORD, PREEMP, VTR_S_C = 480, 320, 18, 0.4, 0.5
FF = 1.0 / (1.0 + 10.0 ** -3)                                            # the 30 dB stabilising floor
WRONG_S = ('no_preemp', 'rect_window', 'no_floor', 'order_17', 'swapped', 'centred', 'no_offset')      # change S
WRONG_DP = ('up_only', 'voiced_too', 'prev_s')                                                          # change where S enters
WRONG = WRONG_S + WRONG_DP


def _dot(a, b, order):
    if order == 'dot':
        return float(np.dot(a, b))
    acc = 0.0
    for p, q in zip(a, b):
        acc = acc + float(p) * float(q)
    return acc


def lpc(y, order='dot', variant=None):
    """(rho [P + 1], a [P + 1], E) of one windowed signal y [480]: normalised, floored autocorrelation, Levinson-Durbin predictor, error"""
    P = 17 if variant == 'order_17' else LPC_ORD
    ff = 1.0 if variant == 'no_floor' else FF
    r = np.array([_dot(y[:STAT_W - k], y[k:], order) for k in range(P + 1)])
    rho, a, E = np.zeros(P + 1), np.zeros(P + 1), 1.0
    rho[0] = a[0] = 1.0
    if r[0] == 0.0:
        return rho, a, E
    rho[1:] = ff * r[1:] / r[0]
    for m in range(1, P + 1):
        if order == 'dot':
            acc = rho[m] + float(np.dot(a[1:m], rho[m - 1:0:-1]))
        else:
            acc = rho[m]
            for q in range(1, m):
                acc = acc + a[q] * rho[m - q]
        kappa = -acc / E
        new = a.copy()
        for q in range(1, m):
            new[q] = a[q] + kappa * a[m - q]
        new[m] = kappa
        a = new
        E = E * (1.0 - kappa * kappa)
    return rho, a, E


def itakura(rho_a, e_a, a_b, order='dot'):
    """d: the predictor a_b on the signal whose normalised autocorrelation is rho_a and whose own predictor leaves e_a"""
    P = a_b.shape[0] - 1
    c = np.array([_dot(a_b, a_b, order)] + [2.0 * _dot(a_b[:P + 1 - k], a_b[k:], order) for k in range(1, P + 1)])
    if order == 'dot':
        return (c[0] + float(np.dot(c[1:], rho_a[1:]))) / e_a
    acc = c[0]
    for k in range(1, P + 1):
        acc = acc + c[k] * rho_a[k]
    return acc / e_a


def window_signal(z, c, variant=None):
    """y [480] of the window centred on sample c of the scaled samples z (zero outside them)"""
    n = z.shape[0]
    idx = c - STAT_W // 2 + np.arange(STAT_W + 1)
    u = np.where((idx >= 0) & (idx < n), z[np.clip(idx, 0, n - 1)], 0.0)
    w = np.ones(STAT_W) if variant == 'rect_window' else 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(STAT_W) + 0.5) / STAT_W)
    return w * (u[1:] - (0.0 if variant == 'no_preemp' else PREEMP) * u[:-1])


def stationarity(x, n_frames=None, scale=32768.0, order='dot', variant=None, with_d=False):
    """S [n_frames] (default: pitch_ref.frames_of(len(x))); with_d: (S, d), d_0 = 1"""
    z = scale * np.asarray(x, np.float64)
    F = R.frames_of(z.shape[0]) if n_frames is None else n_frames
    S, D = np.zeros(F), np.ones(F)
    half = 0 if variant == 'centred' else STAT_GAP // 2
    for i in range(1, F):
        ya, yb = window_signal(z, R.HOP * i - half, variant), window_signal(z, R.HOP * i + half, variant)
        if variant == 'swapped':
            ya, yb = yb, ya
        rho_a, _, e_a = lpc(ya, order, variant)
        _, a_b, _ = lpc(yb, order, variant)
        D[i] = itakura(rho_a, e_a, a_b, order)
        S[i] = 0.2 / max(D[i], 1.0) if variant == 'no_offset' else min(0.2 / (max(D[i], 1.0) - 0.8), 1.0)
    return (S, D) if with_d else S


def divergence_stat(x, scale=32768.0):
    return float(np.abs(stationarity(x, None, scale, 'dot') - stationarity(x, None, scale, 'seq')).max())


def _transitions_stat(Lb, La, rr, s, variant=None):
    """pitch_ref._transitions with VTR_S_C s added to the two voicing transitions: t [from b, to a]"""
    t = R._transitions(Lb, La, rr)
    if variant == 'voiced_too':
        t = t + VTR_S_C * s
    t[0, :] = (R.VTRAN_C + R.VTR_A_C / rr) + VTR_S_C * s
    t[:, 0] = (R.VTRAN_C + R.VTR_A_C * rr) + (0.0 if variant == 'up_only' else VTR_S_C * s)
    t[0, 0] = 0.0
    return t


def _all_transitions(Ls, rms, S, variant=None):
    """[None, t_1, .. t_{F-1}]"""
    return [None] + [_transitions_stat(Ls[i - 1], Ls[i], rms[i] / rms[i - 1], S[i - 1] if variant == 'prev_s' else S[i], variant)
                     for i in range(1, len(Ls))]


def dp_stat(phi, rms, S, lo, hi, variant=None):
    """the sequential half with the term: f0 [F]"""
    lmin, lmax, K = R.lag_range(lo, hi)
    phi, rms, S = np.asarray(phi, np.float64), np.asarray(rms, np.float64), np.asarray(S, np.float64)
    assert phi.shape[1] == K and S.shape == rms.shape
    Ls, ds = R._lattice(phi, lmin, lmax)
    T = _all_transitions(Ls, rms, S, variant)
    F = len(Ls)
    D, back = ds[0].copy(), []
    for i in range(1, F):
        tot = D[:, None] + T[i]
        bp = np.array([R._argmin(tot[:, a]) for a in range(tot.shape[1])])
        D = ds[i] + tot[bp, np.arange(tot.shape[1])]
        back.append(bp)
    state = R._argmin(D)
    f0 = np.empty(F)
    for i in range(F - 1, -1, -1):
        f0[i] = math.log(R.FS / Ls[i][state]) if state else R.UNVOICED
        if i:
            state = int(back[i - 1][state])
    return f0


def track_stat(x, lo, hi, scale=32768.0, variant=None):
    phi, rms = R.nccf(x, lo, hi, scale)
    return dp_stat(phi, rms, stationarity(x, None, scale, 'dot', variant if variant in WRONG_S else None), lo, hi,
                   variant if variant in WRONG_DP else None)


def margins_stat(phi, rms, S, lo, hi):
    """the path margin of pitch_ref.margins_phi under the new transitions: min over frames of [the cheapest complete path through any
    OTHER state of that frame] - [the best path's cost]"""
    lmin, lmax, _ = R.lag_range(lo, hi)
    Ls, ds = R._lattice(np.asarray(phi, np.float64), lmin, lmax)
    F = len(Ls)
    T = _all_transitions(Ls, np.asarray(rms, np.float64), np.asarray(S, np.float64))
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
    return margin


STAT_CASE_HEIGHTS = (0.9, 0.9, 0.9, 0.25, 0.25, 0.9, 0.9, 0.9)
STAT_CASE_TRACKS = {'zeros': np.zeros(8), 'ones': np.ones(8), 'edges': np.array([1.0, 1.0, 1.0, 0.05, 1.0, 0.05, 1.0, 1.0]),
                    'low': np.full(8, 0.08)}


def stat_case():
    """(phi, rms) in (50, 250), 8 frames, constant rms: every frame has one peak h_i exp(-((k - 133) / 6)^2), strong but for a two-frame dip
    at frames 3 and 4.  With S = 0 the dip is cut out of the voiced region; with S = 1 (a steady spectrum) leaving and re-entering voicing
    costs 0.5 more each way and every frame stays voiced; with S = 0.05 at frames 3 and 5 (the spectrum changes there) the dip is cut out
    again; with S = 0.08 everywhere the two half-terms together (0.08) outweigh what cutting the dip saves (0.052) and one alone (0.04)
    does not, so every frame stays voiced only if the term enters BOTH transitions.  STAT_CASE_TRACKS holds the four S tracks."""
    lmin, _, K = R.lag_range(50.0, 250.0)
    k = lmin + np.arange(K)
    phi = np.array([h * np.exp(-((k - 133.0) / 6.0) ** 2) for h in STAT_CASE_HEIGHTS])
    return phi, np.ones(len(STAT_CASE_HEIGHTS))
