"""A restatement of ss_resample (csrc/resample.hip), written from the text of include/speechsplit_amd.h: every product and every sum below is
one IEEE double operation, rounded on its own, in the header's order.  The yardstick of test_gpu_resample.py, held against
scipy.signal.resample_poly, and proven on wrong stand-ins, by test_resample_ref_selftest.py.  Importing it needs no GPU.

    half = (n_taps - 1) / 2; m_b = ceil(n up / down)
    y[m] = 0.0 + sum over k of x[k] * h[m*down + half - k*up],  over exactly the k with 0 <= k < n and 0 <= m*down + half - k*up < n_taps,
           k ascending: acc = 0.0, then acc = acc + x[k] * h[..] for each such k in turn
    x[k] for k >= n is never read: the range of k bounds the loop
    h = firwin(20 max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up for the reduced up / down (`design`)

The valid k of one output are a contiguous range, so the sum is run for all outputs at once: step i adds the i-th term of every output that has
one (numpy multiplies and adds element by element, each rounded on its own -- there is no fused operation in `a * b` followed by `c + d`).

The comparison used everywhere is `same`: array equality.  Summing the same taps in descending order already differs in the last place, so
no tolerance above 0 means anything.

`variant` (self-test only) swaps in ONE deliberate fault, a name from WRONG; None is the definition."""
import math

import numpy as np
from scipy import signal

WRONG = ('descending_order', 'centre_off_by_one', 'h_not_scaled_by_up', 'floor_length', 'cutoff_from_min', 'kaiser_beta_6', 'reads_behind_n')
DESIGN_VARIANTS = ('h_not_scaled_by_up', 'cutoff_from_min', 'kaiser_beta_6')


def same(got, want):
    """array equality: the same shape, both float64, every element equal (NaN equals nothing)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape and bool(np.array_equal(got, want))


def ratio(sr_in, sr_out):
    """(up, down) from sr_in to sr_out Hz, reduced"""
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n, up, down):
    return -(-n * up // down)


def design(up, down, variant=None):
    """the filter the Python layer passes: scipy.signal.resample_poly's default for the reduced up / down"""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    top = min(up, down) if variant == 'cutoff_from_min' else max(up, down)
    assert top > 1, 'a cutoff of 1 is no filter: this variant cannot be stated where min(up, down) is 1'
    h = signal.firwin(20 * max(up, down) + 1, 1.0 / top, window=('kaiser', 6.0 if variant == 'kaiser_beta_6' else 5.0))
    return h if variant == 'h_not_scaled_by_up' else h * up


def resample(x, up, down, h, n=None, variant=None):
    """x float64 [>= n] (n None: all of it), h float64 [n_taps], n_taps odd -> float64 [ceil(n up / down)].  Nothing at or behind x[n] is
    read (the variant 'reads_behind_n' does: a padded-tap form that runs k up to the end of the buffer)."""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    n = x.shape[0] if n is None else int(n)
    n_taps = h.shape[0]
    assert x.ndim == 1 and h.ndim == 1 and n_taps % 2 == 1 and 1 <= n <= x.shape[0] and up >= 1 and down >= 1
    half = (n_taps - 1) // 2 + (1 if variant == 'centre_off_by_one' else 0)
    m_b = n * up // down if variant == 'floor_length' else out_len(n, up, down)
    reach = x.shape[0] if variant == 'reads_behind_n' else n
    t = np.arange(m_b, dtype=np.int64) * down + half                     # the tap input 0 meets
    k_lo = np.maximum(0, -((n_taps - 1 - t) // up))                       # ceil((t - (n_taps - 1)) / up): the tap index stays below n_taps
    k_hi = np.minimum(reach - 1, t // up)                                 # and at or above 0
    count = k_hi - k_lo + 1
    acc = np.zeros(m_b)
    for i in range(int(count.max()) if m_b else 0):
        live = count > i
        k = (k_hi - i if variant == 'descending_order' else k_lo + i)[live]
        prod = x[k] * h[t[live] - k * up]
        acc[live] = acc[live] + prod
    return acc
