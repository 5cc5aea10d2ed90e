"""A float64 numpy restatement of the F0-guided harmonic mel inversion and the harmonic start phases (ss_mel_to_linear_harmonic,
ss_harmonic_phase; csrc/vocoder.hip), written from the text of include/speechsplit_amd.h and not from the kernel.  The yardstick of
test_gpu_harmonic.py, proven on wrong stand-ins by test_harmonic_ref_selftest.py.  Importing it needs no GPU.

Per voiced frame (f finite, 40 <= f <= 1000 Hz), with amp = 10^((100 mel - 100 + 16) / 20), B the [513, n_mels] basis, P = pinv(B):

    H = min(floor(f_top / f), 190);  p_h = (h f) / 15.625;  D[k, h] = 512 W(k - p_h)
    W(d) = 0.5 s(d) + 0.25 s(d - 1) + 0.25 s(d + 1) for |d| < 2, else 0;  s = sinc
    a = 0; y = a; t = 1;  n_iter times:  r = (D y) B - amp;  g = D^T (B r);  an = max(y - g / L, 0);  tn = (1 + sqrt(1 + 4 t^2)) / 2
                                         y = an + ((t - 1) / tn) (an - a);  t = tn;  a = an
    L = (max_h sum_m A[m, h]) (max_m sum_h A[m, h]),  A = B^T D
    mag_h = D a;  res = max(amp - mag_h B, 0);  mag_n = max(res P, 0);  S = max(sqrt(mag_h^2 + mag_n^2), floor);  w = mag_h / sqrt(..)

Unvoiced frames keep the magnitude they are handed and get w = 0.  Two summation orders that share no code inside the fit:

    order='dense'    A = B^T D is formed and every product is a numpy matmul (BLAS: blocked, fused multiply-adds)
    order='kernel'   the kernel's order: A is never formed; a bin's model runs over the harmonics that cover it in ascending h, a band's sum
                     over its run of bins in bin order (nnls_ref's packed basis), a bin's gradient over the covering bands in band order, a
                     harmonic's gradient over its four bins, L through the same three products on ones, res P term by term in band order

Their disagreement measures how far n_iter rounds amplify the rounding of one sum: the conditioning figure the GPU bound is derived from.

Start phases: u (cycles) by the header's recurrence, h_k = min(max(rint(k / p_1), 1), H), phi_h = 2 pi frac(h_k u + 0.5 (k mod 2)),
phase0 = arg(w e^{i phi_h} + sqrt(1 - w^2) e^{i phi_rand}); unvoiced frames and exact zeros keep phi_rand.

`variant` (self-test only; the fit's in dense order) swaps in ONE deliberate fault, a name from WRONG_FIT or WRONG_PHASE."""
import math

import numpy as np

from tests import nnls_ref as N

NBIN, BIN_HZ, HARM_MAX = 513, 15.625, 190
WRONG_FIT = ('no_projection', 'rect_lobe', 'wide_lobe', 'shifted_bins', 'no_f_top', 'short_h', 'raw_residual', 'plain_sum', 'double_step')
WRONG_PHASE = ('floor_hk', 'no_half_cycle', 'no_trapezoid', 'no_restart')
DISAGREEMENT_CAP = 1e-11                                               # what the self-test holds the dense / kernel disagreement under
GPU_BOUND_CAP = 1e-9
EPS = 2.0 ** -52
ITERS = (0, 1, 50)


def voiced(f):
    f = np.asarray(f, np.float64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(f) & (f >= 40.0) & (f <= 1000.0)


def to_hz(f0):
    """features.pitch_track's convention (ln Hz, -1e10 unvoiced) -> Hz, 0 on unvoiced frames"""
    f = np.asarray(f0, np.float64)
    ok = np.isfinite(f) & (f > -1e9)
    return np.where(ok, np.exp(np.where(ok, f, 0.0)), 0.0)


def count(f, f_top=7600.0, variant=None):
    H = int(min(math.floor((8000.0 if variant == 'no_f_top' else f_top) / f), HARM_MAX))
    return H - 1 if variant == 'short_h' else H


def lobe(d, variant=None):
    d = np.asarray(d, np.float64)
    s = np.sinc(d) if variant == 'rect_lobe' else 0.5 * np.sinc(d) + 0.25 * np.sinc(d - 1.0) + 0.25 * np.sinc(d + 1.0)
    return np.where(np.abs(d) < (3.0 if variant == 'wide_lobe' else 2.0), s, 0.0)


def atoms(f, f_top=7600.0, variant=None):
    """(H, first bin [H], weights [H, width]) of a voiced frame: harmonic h's weights on bins first .. first + width - 1 (width 4)"""
    H = count(f, f_top, variant)
    p = (np.arange(1, H + 1) * float(f)) / BIN_HZ + (1.0 if variant == 'shifted_bins' else 0.0)
    half = 3 if variant == 'wide_lobe' else 2
    k0 = np.floor(p).astype(np.int64) - (half - 1)
    ks = k0[:, None] + np.arange(2 * half)[None, :]
    wt = np.where((ks >= 0) & (ks < NBIN), 512.0 * lobe(ks - p[:, None], variant), 0.0)
    return H, k0, wt


def dictionary(f, f_top=7600.0, variant=None):
    """D [513, H]"""
    H, k0, wt = atoms(f, f_top, variant)
    D = np.zeros((NBIN, H))
    for j in range(wt.shape[1]):
        ks = k0 + j
        ok = (ks >= 0) & (ks < NBIN)
        D[ks[ok], np.flatnonzero(ok)] = wt[ok, j]
    return D


def lipschitz(A):
    """||A||_1 ||A||_inf of a non-negative A"""
    return float(A.sum(axis=0).max() * A.sum(axis=1).max())


def _finish(mag_h, mag_n, floor, variant=None):
    q = mag_h + mag_n if variant == 'plain_sum' else np.sqrt(mag_h * mag_h + mag_n * mag_n)
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.where(q > 0.0, mag_h / q, 0.0)
    return np.maximum(q, floor), share


def _fit_dense(amp, f, B, P, n_iter, f_top, floor, variant):
    D = dictionary(f, f_top, variant)
    A = B.T @ D
    L = lipschitz(A)
    step = (1.0 / L if L > 0.0 else 0.0) * (2.0 if variant == 'double_step' else 1.0)
    a = np.zeros(D.shape[1])
    y, t = a, 1.0
    for _ in range(n_iter):
        g = A.T @ (A @ y - amp)
        an = y - step * g
        if variant != 'no_projection':
            an = np.maximum(an, 0.0)
        tn = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        y, t, a = an + ((t - 1.0) / tn) * (an - a), tn, an
    mag_h = D @ a
    res = amp - mag_h @ B
    if variant != 'raw_residual':
        res = np.maximum(res, 0.0)
    S, share = _finish(mag_h, np.maximum(res @ P, 0.0), floor, variant)
    return S, share, a


def _fit_kernel(amp, fs, B, P, n_iter, f_top, floor):
    """all voiced frames at once: amp [V, n_mels], fs [V] -> S [V, 513], share [V, 513], a [V, 190]"""
    V, n = amp.shape
    bd = N._Banded(N.pack(B), n)
    k0, wt, Hs = np.zeros((V, HARM_MAX), np.int64), np.zeros((V, HARM_MAX, 4)), np.zeros(V, np.int64)
    for v, f in enumerate(fs):
        Hs[v], k, w = atoms(f, f_top)
        k0[v, :Hs[v]], wt[v, :Hs[v]] = k, w
    Hmax = int(Hs.max())
    live = np.arange(HARM_MAX)[None, :] < Hs[:, None]
    rows = np.arange(V)[:, None]
    cols = k0[:, :, None] + np.arange(4)[None, None, :]                # up to 515: three columns of padding behind bin 512

    def model_of(y):                                                   # a bin's sum over the covering harmonics, ascending h
        mdl = np.zeros((V, NBIN + 3))
        for h in range(Hmax):
            mdl[rows, cols[:, h, :]] += wt[:, h, :] * y[:, h, None]
        return mdl[:, :NBIN]

    def atom_dot(grad):                                                # a harmonic's sum over its four bins, bin order
        gp = np.concatenate([grad, np.zeros((V, 3))], axis=1)
        g = np.zeros((V, HARM_MAX))
        for j in range(4):
            g = g + wt[:, :, j] * gp[rows, cols[:, :, j]]
        return g

    zero = np.zeros((V, n))
    row_sums = bd.residual(model_of(live.astype(np.float64)), zero).max(axis=1)
    col_sums = atom_dot(bd.gradient(np.ones((V, n)))).max(axis=1)
    L = row_sums * col_sums
    with np.errstate(divide='ignore'):
        step = np.where(L > 0.0, 1.0 / L, 0.0)[:, None]
    a = np.zeros((V, HARM_MAX))
    y, t = a, 1.0
    for _ in range(n_iter):
        g = atom_dot(bd.gradient(bd.residual(model_of(y), amp)))
        an = np.maximum(y - step * g, 0.0)
        tn = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        y, t, a = an + ((t - 1.0) / tn) * (an - a), tn, an
    mag_h = model_of(a)
    res = np.maximum(-bd.residual(mag_h, amp), 0.0)                    # amp - sum, to the bit the negative of sum - amp
    s = np.zeros((V, NBIN))
    for m in range(n):                                                 # res P term by term, m ascending
        s = s + res[:, m:m + 1] * P[m][None, :]
    S, share = _finish(mag_h, np.maximum(s, 0.0), floor)
    return S, share, a


def mel_to_linear_harmonic(mel, f0_hz, basis, mag_in, n_iter=50, f_top=7600.0, floor=1e-10, order='dense', inv_basis=None, variant=None,
                           return_a=False):
    """mel [F, n_mels] on the [0, 1] dB scale, f0_hz [F] in Hz, mag_in [F, 513] (the route's magnitude) -> (mag [F, 513], share [F, 513]);
    with return_a also the fitted amplitudes, one array [H] per voiced frame"""
    B = np.asarray(basis, np.float64)
    assert order in ('dense', 'kernel') and (variant is None or (variant in WRONG_FIT and order == 'dense'))
    P = np.linalg.pinv(B) if inv_basis is None else np.asarray(inv_basis, np.float64)
    f0_hz = np.asarray(f0_hz, np.float64)
    amp = N.amplitudes(np.asarray(mel, np.float32))
    mag, share = np.array(mag_in, np.float64), np.zeros((amp.shape[0], NBIN))
    assert mag.shape == share.shape and f0_hz.shape == (amp.shape[0],)
    vs = np.flatnonzero(voiced(f0_hz))
    amps = []
    if order == 'kernel' and vs.size:
        mag[vs], share[vs], a = _fit_kernel(amp[vs], f0_hz[vs], B, P, n_iter, f_top, floor)
        amps = [a[i, :count(f0_hz[v], f_top)] for i, v in enumerate(vs)]
    elif vs.size:
        for v in vs:
            mag[v], share[v], a = _fit_dense(amp[v], f0_hz[v], B, P, n_iter, f_top, floor, variant)
            amps.append(a)
    return (mag, share, amps) if return_a else (mag, share)


def phase_u(f0_hz, variant=None):
    """u [F] in cycles; every operation is one float64 operation, none fused"""
    f = [float(x) for x in np.asarray(f0_hz, np.float64)]
    v = voiced(f0_hz)
    u = [0.0] * len(f)
    last = 0.0
    for i in range(1, len(f)):
        if v[i] and v[i - 1]:
            inc = 0.016 * f[i] if variant == 'no_trapezoid' else 0.008 * (f[i - 1] + f[i])
            t = u[i - 1] + inc
            u[i] = t - math.floor(t)
        elif v[i] and variant == 'no_restart':
            u[i] = last
        if v[i]:
            last = u[i]
    return np.array(u)


def harmonic_phase(f0_hz, share, rand_phase, f_top=7600.0, variant=None):
    """f0_hz [F], share and rand_phase [F, 513] (rand_phase None: zeros) -> phase0 [F, 513]"""
    assert variant is None or variant in WRONG_PHASE
    f0_hz, share = np.asarray(f0_hz, np.float64), np.asarray(share, np.float64)
    rand = np.zeros(share.shape) if rand_phase is None else np.asarray(rand_phase, np.float64)
    u = phase_u(f0_hz, variant)
    out = rand.copy()
    k = np.arange(NBIN)
    for i in np.flatnonzero(voiced(f0_hz)):
        p1, H = f0_hz[i] / BIN_HZ, count(f0_hz[i], f_top)
        hk = np.minimum(np.maximum((np.floor if variant == 'floor_hk' else np.rint)(k / p1), 1.0), float(H))
        t = hk * u[i] + (0.0 if variant == 'no_half_cycle' else 0.5 * (k % 2))
        phi = 2.0 * np.pi * (t - np.floor(t))
        w = share[i]
        c = np.sqrt(np.maximum(1.0 - w * w, 0.0))
        re, im = w * np.cos(phi) + c * np.cos(rand[i]), w * np.sin(phi) + c * np.sin(rand[i])
        out[i] = np.where((re == 0.0) & (im == 0.0), rand[i], np.arctan2(im, re))
    return out


def rel_diff(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def abs_diff(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def phase_diff(a, b):
    """max |e^{ia} - e^{ib}|"""
    return float(np.abs(np.exp(1j * np.asarray(a)) - np.exp(1j * np.asarray(b))).max())


# ---- the parity inputs, their conditioning and the conditions they have to hold
def parity_inputs(feats):
    """name -> (mel float32 [F, 80], f0_hz [F]) through features.npz's own basis: u1 cut to 4 / 5 / 9 / 41 frames by
    griffinlim_ref.PARITY_SLICES, and u0; the F0 is pitch_ref.track(x, 50, 250) of the whole utterance, cut like the mel.  The leading
    frames of u1 are silence, so the 4-, 5- and 9-frame slices would be unvoiced throughout: their LAST two frames take a fixed F0 instead
    (the u1 track's median voiced value, times 1 and times 1.01), documented here and nowhere hidden: no frame is dropped."""
    from tests import griffinlim_ref as R
    from tests import pitch_ref
    basis = np.asarray(feats['mel_basis'], np.float64)
    out = {}
    hz1 = to_hz(pitch_ref.track(feats['u1_wav'], 50.0, 250.0))
    med = float(np.median(hz1[voiced(hz1)]))
    for F, cut in R.PARITY_SLICES.items():
        mel = R.melspec(np.asarray(feats['u1_wav'], np.float64)[:cut], basis).astype(np.float32)
        hz = hz1[:F].copy()
        if not voiced(hz).any():
            hz[-2:] = med, 1.01 * med
        assert mel.shape[0] == F == hz.shape[0]
        out[f'u1_{F}'] = (mel, hz)
    mel0 = R.melspec(np.asarray(feats['u0_wav'], np.float64), basis).astype(np.float32)
    hz0 = to_hz(pitch_ref.track(feats['u0_wav'], 50.0, 250.0))
    assert mel0.shape[0] == hz0.shape[0]
    out['u0'] = (mel0, hz0)
    return out


def conditions(f0_hz, f_top=7600.0, tol=1e-9):
    """raise unless no rounding can flip a decision on this track: no k / p_1 within tol of a half-integer, no voiced f within tol
    (relative) of 40, 1000 or a value where floor(f_top / f) steps"""
    f0_hz = np.asarray(f0_hz, np.float64)
    k = np.arange(NBIN)
    for f in f0_hz[voiced(f0_hz)]:
        q = k / (f / BIN_HZ)
        assert np.abs(q - np.floor(q) - 0.5).min() > tol, f
        assert abs(f / 40.0 - 1.0) > tol and abs(f / 1000.0 - 1.0) > tol, f
        x = f_top / f
        assert min(x - math.floor(x), math.ceil(x) - x) > tol * x or x > HARM_MAX + 1, f


def full(mel, f0_hz, basis, inv_basis, rand, n_iter, f_top=7600.0, floor=1e-10, order='kernel'):
    """the pseudo-inverse route, the harmonic fit on top and the start phases: (S, share, phase0)"""
    from tests import griffinlim_ref as R
    S, share = mel_to_linear_harmonic(mel, f0_hz, basis, R.mel_to_linear(mel, inv_basis, floor), n_iter, f_top, floor, order, inv_basis)
    return S, share, harmonic_phase(f0_hz, share, rand, f_top)


def disagreement(mel, f0_hz, basis, inv_basis, rand, n_iter):
    """(the kernel-order (S, share, phase0), their distances from the dense order's: S relative to max |S|, share absolute, phase0 as
    |e^{ia} - e^{ib}|)"""
    ker = full(mel, f0_hz, basis, inv_basis, rand, n_iter, order='kernel')
    den = full(mel, f0_hz, basis, inv_basis, rand, n_iter, order='dense')
    return ker, (rel_diff(den[0], ker[0]), abs_diff(den[1], ker[1]), phase_diff(den[2], ker[2]))


def gpu_bound(d):
    """100 x a two-order disagreement, capped at 1e-9.  A disagreement below one unit of double rounding (the two orders take the same
    sums, as at n_iter 0) counts as 2^-52: the device's pow, sincos and atan2 still round, and no reference measures below that."""
    return min(GPU_BOUND_CAP, 100.0 * max(d, EPS))
