"""A restatement of ss_filtfilt (csrc/filtfilt.hip), written from the text of include/speechsplit_amd.h in plain Python floats: every product
and every sum below is one IEEE double operation, rounded on its own, in the header's order.  The yardstick of test_gpu_features_batch.py,
held against scipy.signal.filtfilt and the fixture, and proven on wrong stand-ins, by test_filtfilt_ref_selftest.py.  Importing it needs no GPU.

    Extension.  i = j - 18, j in [0, n + 36): ext[j] = 2 x[0] - x[-i] (i < 0); x[i] (0 <= i < n); 2 x[n-1] - x[2(n-1) - i] (i >= n)
    Step.       y = b0*u + z0; z_i = (b_{i+1}*u + z_{i+1}) - a_{i+1}*y, i = 0..3; z4 = b5*u - a5*y
    Pass 1.     z = zi * ext[0]; v[j] = step(ext[j]), j ascending
    Pass 2.     z = zi * v[n+35]; w[j] = step(v[j]), j descending
    Output.     y[i] = w[i + 18]
    Epilogue.   out[i] = y[i]*gain + (r[i] - 0.5)*dither_scale; without r: y[i]*gain

The comparison used everywhere is `same`: array equality -- no tolerance between 0 and the 3e-7 by which any other arrangement of this filter's
arithmetic misses scipy means anything.

`variant` (self-test only) swaps in ONE deliberate fault, a name from WRONG; None is the definition."""
from fractions import Fraction

import numpy as np
from scipy import signal

NCOEF, PAD = 6, 18
MIN_SAMPLES = 513
GAIN, DITHER_SCALE = 0.96, 1e-06                                        # make_spect_f0.py:54-55
WRONG = ('even_extension', 'pad17', 'zi_unscaled', 'second_pass_from_v0', 'two_forward_passes', 'contracted_step', 'gain_after_dither')


def coefficients():
    """(b [6], a [6], zi [5]) of the reference's filter: utils.py:10-14 at make_spect_f0.py:51's arguments, and scipy's steady state"""
    b, a = signal.butter(5, 30 / (0.5 * 16000), btype='high', analog=False)
    return b, a, signal.lfilter_zi(b, a)


def same(got, want):
    """array equality: the same shape, both float64, every element equal (NaN equals nothing)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape and bool(np.array_equal(got, want))


def _fma(x, y, z):
    """x * y + z rounded once (the fault of 'contracted_step'), exactly, through rationals"""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def extend(x, pad=PAD, variant=None):
    x = [float(v) for v in x]
    n = len(x)
    out = []
    for j in range(n + 2 * pad):
        i = j - pad
        if i < 0:
            out.append(x[-i] if variant == 'even_extension' else 2.0 * x[0] - x[-i])
        elif i < n:
            out.append(x[i])
        else:
            out.append(x[2 * (n - 1) - i] if variant == 'even_extension' else 2.0 * x[n - 1] - x[2 * (n - 1) - i])
    return out


def run(u, b, a, z, variant=None):
    """step over the list u in order from the state z (a list of 5, updated in place) -> the list of y"""
    b0, b1, b2, b3, b4, b5 = (float(v) for v in b)
    _, a1, a2, a3, a4, a5 = (float(v) for v in a)
    z0, z1, z2, z3, z4 = z
    out = []
    if variant == 'contracted_step':
        for x in u:
            y = _fma(b0, x, z0)
            z0 = _fma(-a1, y, _fma(b1, x, z1))
            z1 = _fma(-a2, y, _fma(b2, x, z2))
            z2 = _fma(-a3, y, _fma(b3, x, z3))
            z3 = _fma(-a4, y, _fma(b4, x, z4))
            z4 = _fma(-a5, y, b5 * x)
            out.append(y)
    else:
        for x in u:
            y = b0 * x + z0
            z0 = (b1 * x + z1) - a1 * y
            z1 = (b2 * x + z2) - a2 * y
            z2 = (b3 * x + z3) - a3 * y
            z3 = (b4 * x + z4) - a4 * y
            z4 = b5 * x - a5 * y
            out.append(y)
    z[:] = [z0, z1, z2, z3, z4]
    return out


def filtfilt(x, b, a, zi, gain=1.0, r=None, dither_scale=0.0, variant=None):
    """x float64 [n], n >= 513; b, a [6] with a[0] == 1; zi [5]; r float64 [n] or None -> float64 [n]"""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and x.shape[0] >= MIN_SAMPLES and len(b) == NCOEF and len(a) == NCOEF and len(zi) == NCOEF - 1 and float(a[0]) == 1.0
    n = x.shape[0]
    pad = PAD - 1 if variant == 'pad17' else PAD
    zi = [float(v) for v in zi]
    ext = extend(x, pad, variant)
    v = run(ext, b, a, [s if variant == 'zi_unscaled' else s * ext[0] for s in zi], variant)
    if variant == 'two_forward_passes':
        w = run(v, b, a, [s * v[0] for s in zi], variant)
    else:
        start = v[0] if variant == 'second_pass_from_v0' else v[-1]
        w = run(v[::-1], b, a, [s if variant == 'zi_unscaled' else s * start for s in zi], variant)[::-1]
    y = w[pad:pad + n]
    gain, dither_scale = float(gain), float(dither_scale)
    if r is None:
        return np.array([s * gain for s in y], np.float64)
    r = [float(s) for s in np.asarray(r, np.float64)]
    assert len(r) == n
    if variant == 'gain_after_dither':
        return np.array([(s + (t - 0.5) * dither_scale) * gain for s, t in zip(y, r)], np.float64)
    return np.array([s * gain + (t - 0.5) * dither_scale for s, t in zip(y, r)], np.float64)


def odd_length_fix(x):
    """make_spect_f0.py:52-53: a recording whose length is a multiple of 256 gets one sample of 1e-6 appended"""
    x = np.asarray(x, np.float64)
    return np.concatenate((x, np.array([1e-06]))) if x.shape[0] % 256 == 0 else x
