"""STOI and ESTOI as include/speechsplit_amd.h defines them ("waveform scores"), restated in numpy -- in two summation orders that share no
transform code:

    order='loop'    every sum one term at a time, index ascending (numpy.cumsum is such a sum), as the header fixes it and the kernels of
                    csrc/stoi.hip do it; the transform is an explicit 257 x 256 DFT matrix.
    order='numpy'   numpy's own reductions (pairwise sums, numpy.mean) and numpy.fft.rfft.

Their disagreement on an input is this definition's own rounding noise there; the GPU tests take their bounds from it.  `variant` switches
on ONE deliberate mistake at a time (tests/test_stoi_ref_selftest.py measures how far each lies from the definition).  Host only."""
import math

import numpy as np

EPS = 2.0 ** -52
FRAME, HOP, NFFT, NBIN = 256, 128, 512, 257
J, N, BETA, RANGE_DB, FS = 15, 30, -15.0, 40.0, 10000
LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174)
HI = (9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
VARIANTS = ('upper_edge_inclusive', 'range_30db', 'last_frame_included', 'n_29', 'no_clipping', 'beta_minus_5', 'no_alpha',
            'no_mean_removal', 'own_mask_for_y', 'window_twice', 'estoi_without_columns')


def window():
    """w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257) with the C library's cosine (math.cos), as the library's host code evaluates it"""
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 1) / 257.0) for i in range(FRAME)])


W = window()


def bands(n_bands=J, first=150.0, fs=FS, nfft=NFFT):
    """(lo, hi): third-octave bands, centre 150 * 2^(j/3), edges a sixth of an octave either side, each at the nearest bin k fs / nfft"""
    f = np.arange(nfft // 2 + 1) * (fs / nfft)
    cf = first * 2.0 ** (np.arange(n_bands) / 3.0)
    lo = [int(np.argmin(np.abs(f - c * 2.0 ** (-1.0 / 6.0)))) for c in cf]
    hi = [int(np.argmin(np.abs(f - c * 2.0 ** (1.0 / 6.0)))) for c in cf]
    return lo, hi


def _sum(a, axis, order):
    if order == 'numpy':
        return np.sum(a, axis=axis)
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
    if a.shape[-1] == 0:
        return np.zeros(a.shape[:-1])
    return np.cumsum(a, axis=-1)[..., -1]


def n_frames(n):
    return (n - FRAME) // HOP + 1 if n >= FRAME else 0


def _framed(x, F):
    return np.lib.stride_tricks.sliding_window_view(x, FRAME)[::HOP][:F] if F else np.zeros((0, FRAME))


def energies(x, order='loop'):
    """e_f in dB for f < F"""
    x = np.asarray(x, dtype=np.float64)
    t = _framed(x, n_frames(x.shape[0])) * W
    return 20.0 * np.log10(np.sqrt(_sum(t * t, 1, order)) + EPS)


def keep_mask(e, range_db=RANGE_DB):
    return e > (e.max() - range_db) if e.size else np.zeros(0, bool)


def mask_margin(x, order='loop'):
    """min_f |e_f - (max - 40)| in dB: how far the threshold decision is from flipping"""
    e = energies(x, order)
    return float(np.abs(e - (e.max() - RANGE_DB)).min()) if e.size else float('inf')


def overlap_add(x, inv, w2=False):
    """the compacting gather: sample s = frame s / 128 - 1's second half first, then frame s / 128's first half; window applied once"""
    K = len(inv)
    if K == 0:
        return np.zeros(0)
    w = W * W if w2 else W
    fr = np.stack([x[HOP * f:HOP * f + FRAME] for f in inv]) * w            # [K][256]: the products
    out = np.empty(HOP * (K - 1) + FRAME)
    out[:HOP] = fr[0, :HOP]
    out[-HOP:] = fr[-1, HOP:]
    if K > 1:
        out[HOP:-HOP] = (fr[:-1, HOP:] + fr[1:, :HOP]).reshape(-1)           # earlier frame's term + later frame's term
    return out


def overlap_scale(x, inv):
    """per sample of overlap_add's output: the larger magnitude of the (at most two) products it adds -- the scale an ulp bound on the
    sample is taken at (two products, one add: each product is within an ulp and a half of its own size, the add within half an ulp)"""
    K = len(inv)
    if K == 0:
        return np.zeros(0)
    fr = np.abs(np.stack([x[HOP * f:HOP * f + FRAME] for f in inv]) * W)
    out = np.empty(HOP * (K - 1) + FRAME)
    out[:HOP] = fr[0, :HOP]
    out[-HOP:] = fr[-1, HOP:]
    if K > 1:
        out[HOP:-HOP] = np.maximum(fr[:-1, HOP:], fr[1:, :HOP]).reshape(-1)
    return out


def compact(x, y, order='loop', variant=None):
    """-> dict(e, keep, inv, K, xp, yp)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e = energies(x, order)
    keep = keep_mask(e, 30.0 if variant == 'range_30db' else RANGE_DB)
    inv = np.flatnonzero(keep)
    inv_y = np.flatnonzero(keep_mask(energies(y, order))) if variant == 'own_mask_for_y' else inv
    if variant == 'own_mask_for_y':                                          # the two must still have one length
        k = min(len(inv), len(inv_y))
        inv, inv_y = inv[:k], inv_y[:k]
    w2 = variant == 'window_twice'
    return dict(e=e, keep=keep, inv=inv, K=len(inv), xp=overlap_add(x, inv, w2), yp=overlap_add(y, inv_y, w2))


def frames_below(length):
    """transform frames of a signal: the starts 128 m strictly below length - 256"""
    return -(-(length - FRAME) // HOP) if length > FRAME else 0


_DFT = None


def _dft():
    global _DFT
    if _DFT is None:
        ki = (np.arange(NBIN)[:, None] * np.arange(FRAME)[None, :]) % NFFT
        ang = 2.0 * np.pi * ki / NFFT
        _DFT = (np.cos(ang), -np.sin(ang))
    return _DFT


def spectra(sig, M, order='loop'):
    """|X_m[k]|^2 as (re^2 + im^2) [M][257] of the windowed, zero-padded frames at 128 m"""
    fr = (_framed(np.asarray(sig, dtype=np.float64), M) if M else np.zeros((0, FRAME))) * W
    if order == 'numpy':
        X = np.fft.rfft(fr, NFFT, axis=1)
        re, im = X.real, X.imag
    else:
        c, s = _dft()
        re = _sum(fr[:, None, :] * c[None], 2, 'loop')
        im = _sum(fr[:, None, :] * s[None], 2, 'loop')
    return re * re + im * im


def envelopes(sig, lo=LO, hi=HI, order='loop', variant=None, M=None):
    """[J][M] band envelopes of a signal (x' or y')"""
    if M is None:
        M = frames_below(len(sig)) + (1 if variant == 'last_frame_included' and len(sig) >= FRAME else 0)
    p = spectra(sig, M, order)
    inc = 1 if variant == 'upper_edge_inclusive' else 0
    return np.stack([np.sqrt(_sum(p[:, a:b + inc], 1, order)) for a, b in zip(lo, hi)]) if M else np.zeros((len(lo), 0))


def _normalise(v, axis, order, centre=True):
    if centre:
        mean = np.mean(v, axis=axis, keepdims=True) if order == 'numpy' else np.expand_dims(_sum(v, axis, order) / v.shape[axis], axis)
        v = v - mean
    return v / (np.expand_dims(np.sqrt(_sum(v * v, axis, order)), axis) + EPS)


def segment_scores(X, Y, extended=False, order='loop', variant=None):
    """d_s [S] from envelopes [J][M]"""
    n = 29 if variant == 'n_29' else N
    Jn, M = X.shape
    S = M - n + 1
    if S < 1:
        return np.zeros(0)
    xs = np.lib.stride_tricks.sliding_window_view(X, n, axis=1).transpose(1, 0, 2)       # [S][J][n]
    ys = np.lib.stride_tricks.sliding_window_view(Y, n, axis=1).transpose(1, 0, 2)
    centre = variant != 'no_mean_removal'
    if not extended:
        beta = -5.0 if variant == 'beta_minus_5' else BETA
        clip = 1.0 + 10.0 ** (-beta / 20.0)
        alpha = np.sqrt(_sum(xs * xs, 2, order)) / (np.sqrt(_sum(ys * ys, 2, order)) + EPS)
        yp = ys if variant == 'no_alpha' else alpha[:, :, None] * ys
        if variant != 'no_clipping':
            yp = np.minimum(yp, xs * clip)
        xn, yn = _normalise(xs, 2, order, centre), _normalise(yp, 2, order, centre)
        return _sum(_sum(xn * yn, 2, order), 1, order) / Jn
    xn, yn = _normalise(xs, 2, order, centre), _normalise(ys, 2, order, centre)
    if variant != 'estoi_without_columns':
        xn, yn = _normalise(xn, 1, order, centre), _normalise(yn, 1, order, centre)
    return _sum(_sum(xn * yn, 1, order), 1, order) / n


def stoi(x, y, extended=False, order='loop', variant=None, lo=LO, hi=HI):
    """-> dict(score, S, K, F, d, X, Y, xp, yp, inv, e): the whole definition on one aligned pair at 10 kHz"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    c = compact(x, y, order, variant)
    X, Y = envelopes(c['xp'], lo, hi, order, variant), envelopes(c['yp'], lo, hi, order, variant)
    d = segment_scores(X, Y, extended, order, variant)
    S = len(d)
    score = float(_sum(d, 0, order) / S) if S >= 1 else float('nan')
    return dict(score=score, S=S, K=c['K'], F=n_frames(x.shape[0]), d=d, X=X, Y=Y, **{k: c[k] for k in ('xp', 'yp', 'inv', 'e', 'keep')})


def both_modes(x, y, order='loop'):
    """stoi(...) for STOI and ESTOI from one compaction and one pair of envelopes: the dict of `stoi` with score / d / S keyed by `extended`"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    c = compact(x, y, order)
    X, Y = envelopes(c['xp'], LO, HI, order), envelopes(c['yp'], LO, HI, order)
    r = dict(K=c['K'], F=n_frames(x.shape[0]), X=X, Y=Y, score={}, d={}, **{k: c[k] for k in ('xp', 'yp', 'inv', 'e', 'keep')})
    for ext in (False, True):
        d = segment_scores(X, Y, ext, order)
        r['S'] = len(d)
        r['d'][ext] = d
        r['score'][ext] = float(_sum(d, 0, order) / len(d)) if len(d) >= 1 else float('nan')
    return r


def two_orders(x, y, extended=False):
    """the definition's own rounding noise on this input: |score(loop) - score(numpy)| and the envelopes' max-norm disagreement"""
    a, b = stoi(x, y, extended, 'loop'), stoi(x, y, extended, 'numpy')
    assert a['K'] == b['K'] and np.array_equal(a['inv'], b['inv'])
    env = 0.0
    if a['X'].size:
        env = max(float(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()) for k in ('X', 'Y'))
    sc = abs(a['score'] - b['score']) if a['S'] >= 1 else 0.0
    return sc, env


def make_pair(u_wav, seed):
    """The GPU tests' pair from a 10 kHz recording: x = the recording with two stretches scaled by 1e-3 and 3e-3 (so that the mask removes
    frames), y = x gated (every fourth 40 ms stretch at a tenth) plus white noise at 5 dB SNR."""
    x = np.array(u_wav, dtype=np.float64)
    n = x.shape[0]
    x[(7 * n) // 10:(7 * n) // 10 + n // 10] *= 1e-3                        # both behind sample 4096: the short cases keep every frame
    x[(17 * n) // 20:(17 * n) // 20 + n // 12] *= 3e-3
    rng = np.random.RandomState(seed)
    gate = np.where((np.arange(n) // 400) % 4 == 3, 0.1, 1.0)
    noise = rng.standard_normal(n)
    noise *= np.sqrt(np.mean(x * x) / np.mean(noise * noise)) * 10.0 ** (-5.0 / 20.0)
    return x, x * gate + noise
