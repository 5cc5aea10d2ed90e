"""The restatement of ss_filtfilt (filtfilt_ref.py) against scipy and the fixture, on the CPU: it IS scipy.signal.filtfilt to the bit on every
input the GPU tests use, with the dither it is the fixture's waveform exactly, and the comparison it is used with (array equality) reports each
of seven wrong stand-ins on every one of those inputs.

Inputs: features.npz's u0_x (12345 samples), u1_x with its appended sample (10240 + 1), and u1_x cut to 513, 600 and 1100 samples."""
import functools
import os

import numpy as np
import pytest
from scipy import signal

from tests import filtfilt_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('u0', 'u1', '513', '600', '1100')


@functools.lru_cache(maxsize=None)
def inputs():
    f = np.load(os.path.join(GOLD, 'features.npz'))
    u1 = R.odd_length_fix(f['u1_x'])
    assert u1.shape == (10241,) and u1[-1] == 1e-06
    return {'u0': np.ascontiguousarray(f['u0_x'], np.float64), 'u1': u1, '513': f['u1_x'][:513].copy(), '600': f['u1_x'][:600].copy(),
            '1100': f['u1_x'][:1100].copy()}


@functools.lru_cache(maxsize=None)
def dither(name):
    """the draw make_spect_f0.py:55 makes for this input as a speaker's first recording (the fixture's speaker for u0 / u1)"""
    f = np.load(os.path.join(GOLD, 'features.npz'))
    seed = {'u0': int(f['u0_spk']), 'u1': int(f['u1_spk'])}.get(name, 7)
    return np.random.RandomState(seed).rand(inputs()[name].shape[0])


@functools.lru_cache(maxsize=None)
def scipys(name):
    b, a, _ = R.coefficients()
    return signal.filtfilt(b, a, inputs()[name])


def test_the_comparison_is_array_equality():
    a = np.array([1.0, 2.0, 3.0])
    assert R.same(a, a.copy())
    assert not R.same(a, np.nextafter(a, 4.0)) and not R.same(a, a[:2]) and not R.same(a, a.astype(np.float32))
    assert not R.same(np.array([np.nan]), np.array([np.nan]))


def test_coefficients_are_the_references_filter():
    b, a, zi = R.coefficients()
    assert b.shape == (6,) and a.shape == (6,) and zi.shape == (5,) and a[0] == 1.0
    assert np.all(np.abs(np.roots(a)) < 1.0) and np.abs(np.roots(a)).min() > 0.98          # the poles that make direct form ill-conditioned
    assert np.allclose(b / b[0], [1, -5, 10, -10, 5, -1])                                   # five zeros at z = 1: a high-pass


@pytest.mark.parametrize('name', NAMES)
def test_restatement_is_scipys_filtfilt_bit_for_bit(name):
    b, a, zi = R.coefficients()
    got = R.filtfilt(inputs()[name], b, a, zi)
    assert R.same(got, scipys(name)), float(np.abs(got - scipys(name)).max())


@pytest.mark.parametrize('name', ['u0', 'u1'])
def test_with_the_dither_it_is_the_fixtures_waveform(name):
    f = np.load(os.path.join(GOLD, 'features.npz'))
    b, a, zi = R.coefficients()
    got = R.filtfilt(inputs()[name], b, a, zi, R.GAIN, dither(name), R.DITHER_SCALE)
    assert R.same(got, np.ascontiguousarray(f[name + '_wav'], np.float64)), float(np.abs(got - f[name + '_wav']).max())


@pytest.mark.parametrize('name', NAMES)
def test_scaling_and_dither_are_make_spect_f0s_line(name):
    b, a, zi = R.coefficients()
    want = scipys(name) * 0.96 + (dither(name) - 0.5) * 1e-06
    assert R.same(R.filtfilt(inputs()[name], b, a, zi, R.GAIN, dither(name), R.DITHER_SCALE), want)
    assert R.same(R.filtfilt(inputs()[name], b, a, zi, R.GAIN), scipys(name) * 0.96)


@pytest.mark.parametrize('variant', R.WRONG)
@pytest.mark.parametrize('name', NAMES)
def test_every_wrong_variant_is_reported(name, variant):
    b, a, zi = R.coefficients()
    if variant == 'gain_after_dither':
        want = scipys(name) * 0.96 + (dither(name) - 0.5) * 1e-06
        got = R.filtfilt(inputs()[name], b, a, zi, R.GAIN, dither(name), R.DITHER_SCALE, variant=variant)
    else:
        want = scipys(name)
        got = R.filtfilt(inputs()[name], b, a, zi, variant=variant)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert not R.same(got, want)
