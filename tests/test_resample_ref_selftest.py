"""The restatement of ss_resample (resample_ref.py) against scipy on the CPU: it IS scipy.signal.resample_poly to the bit at every rate pair
and length below, and the comparison it is used with (array equality) reports each of seven wrong stand-ins.

Rate pairs: to 16000 Hz from 48000, 44100, 32000, 24000, 22050, 11025 and 8000 Hz, and from 16000 Hz to 48000, 44100 and 8000 Hz.
Lengths: 1, 2, 5, 17, 255, 256, 257, 769 and 1539 samples, heads of features.npz's u0_x.

Which inputs show which wrong variant (asserted below; where a variant CANNOT show, equality is asserted instead, or the reason is given):
    descending_order    needs an output of three or more terms whose two orders round differently: asserted at every pair on 255 samples and
                        more (85 .. 4617 outputs of 20 .. 61 terms each).  One or two terms commute, so 1 and 2 samples cannot show it.
    centre_off_by_one   every pair, every length: already y[0] of one sample takes the neighbouring tap.
    h_not_scaled_by_up  every pair with up > 1, every length.  At 1/3 and 1/2 (up = 1) the two filters are the same array: equality asserted.
    floor_length        the lengths at which n up / down is not whole; where it is whole (at 2/1 and 3/1 always) the two lengths agree:
                        equality asserted.
    cutoff_from_min     every pair with min(up, down) > 1 (160/441, 320/441, 2/3, 640/441, 441/160), every length.  Where min(up, down) is 1 the
                        variant's cutoff is 1, which is no filter and firwin refuses it: it cannot be stated there.
    kaiser_beta_6       every pair, every length.
    reads_behind_n      every pair, every length, given a buffer that holds something behind n (here: the recording goes on): the filter's
                        half length is at least 10 up, so the last output always reaches behind n.  With zeros behind n it cannot show."""
import functools
import os

import numpy as np
import pytest
from scipy import signal

from tests import resample_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PAIRS = [(48000, 16000), (44100, 16000), (32000, 16000), (24000, 16000), (22050, 16000), (11025, 16000), (8000, 16000),
         (16000, 48000), (16000, 44100), (16000, 8000)]
LENGTHS = [1, 2, 5, 17, 255, 256, 257, 769, 1539]
IDS = [f'{a}-{b}' for a, b in PAIRS]


@functools.lru_cache(maxsize=None)
def signal_x():
    x = np.ascontiguousarray(np.load(os.path.join(GOLD, 'features.npz'))['u0_x'], np.float64)
    assert x.shape[0] >= 2 * max(LENGTHS) and np.all(x[:max(LENGTHS) + 400] != 0.0)
    return x


@functools.lru_cache(maxsize=None)
def scipys(sr_in, sr_out, n):
    return signal.resample_poly(signal_x()[:n], sr_out, sr_in)


def test_the_comparison_is_array_equality():
    a = np.array([1.0, 2.0, 3.0])
    assert R.same(a, a.copy())
    assert not R.same(a, np.nextafter(a, 4.0)) and not R.same(a, a[:2]) and not R.same(a, a.astype(np.float32))
    assert not R.same(np.array([np.nan]), np.array([np.nan]))


def test_ratios_lengths_and_filters():
    assert [R.ratio(a, b) for a, b in PAIRS] == [(1, 3), (160, 441), (1, 2), (2, 3), (320, 441), (640, 441), (2, 1), (3, 1), (441, 160), (1, 2)]
    assert [R.out_len(n, 160, 441) for n in (1, 2, 441, 442)] == [1, 1, 160, 161]
    for up, down in ((1, 3), (160, 441), (640, 441), (3, 1)):
        h = R.design(up, down)
        assert h.shape == (20 * max(up, down) + 1,) and np.array_equal(h, h[::-1]) and abs(h.sum() - up) < 1e-9 * up
    assert np.array_equal(R.design(2, 6), R.design(1, 3))                                   # reduced first, as scipy does


@pytest.mark.parametrize('sr_in,sr_out', PAIRS, ids=IDS)
def test_restatement_is_scipys_resample_poly_bit_for_bit(sr_in, sr_out):
    up, down = R.ratio(sr_in, sr_out)
    h = R.design(up, down)
    for n in LENGTHS:
        want = scipys(sr_in, sr_out, n)
        got = R.resample(signal_x()[:n], up, down, h)
        assert R.same(got, want), (n, got.shape, want.shape)
        behind = signal_x()[:n + 300].copy()
        behind[n:] = np.nan                                                                 # nothing at or behind x[n] is read
        assert R.same(R.resample(behind, up, down, h, n=n), want), n


def _shows(variant, up, down, n):
    """True: the variant must differ on this input; False: it must agree; None: it cannot be stated or need not differ"""
    if variant == 'descending_order':
        return True if n >= 255 else None
    if variant == 'h_not_scaled_by_up':
        return up > 1
    if variant == 'floor_length':
        return n * up % down != 0
    if variant == 'cutoff_from_min':
        return True if min(up, down) > 1 else None
    return True


@pytest.mark.parametrize('variant', R.WRONG)
@pytest.mark.parametrize('sr_in,sr_out', PAIRS, ids=IDS)
def test_every_wrong_variant_is_reported(sr_in, sr_out, variant):
    up, down = R.ratio(sr_in, sr_out)
    shown = 0
    for n in LENGTHS:
        expect = _shows(variant, up, down, n)
        if expect is None:
            continue
        h = R.design(up, down, variant if variant in R.DESIGN_VARIANTS else None)
        if variant == 'reads_behind_n':
            got = R.resample(signal_x()[:n + 400], up, down, h, n=n, variant=variant)       # the recording goes on behind n
        else:
            got = R.resample(signal_x()[:n], up, down, h, variant=None if variant in R.DESIGN_VARIANTS else variant)
        assert np.isfinite(got).all()
        assert R.same(got, scipys(sr_in, sr_out, n)) == (not expect), (variant, n)
        shown += bool(expect)
    cannot = {'cutoff_from_min': min(up, down) == 1, 'h_not_scaled_by_up': up == 1, 'floor_length': down == 1}
    assert shown or cannot.get(variant, False), variant
