"""A float64 numpy restatement of the non-negative mel inversion (ss_mel_to_linear_nnls, csrc/vocoder.hip), written from the text of
include/speechsplit_amd.h.  The yardstick of test_gpu_mel_nnls.py, proven on wrong stand-ins by test_nnls_ref_selftest.py.  Importing it
needs no GPU.

    amp = 10^((100 mel - 100 + 16) / 20);  x = max(amp . P, 0);  y = x;  t = 1
    n_iter times:  r = y . B - amp;  g = r . B^T;  xn = max(y - step g, 0);  tn = (1 + sqrt(1 + 4 t^2)) / 2
                   y = xn + ((t - 1) / tn) (xn - x);  t = tn;  x = xn
    mag = max(x, floor)

with B the [513, n_mels] basis and P = pinv(B).  Two summation orders that share no code inside the iteration:

    order='dense'   the two products are numpy matmuls (BLAS: blocked, fused multiply-adds)
    order='band'    the kernel's order, from the PACKED basis (pack(), the header's layout restated): band m's sum runs over its run of bins
                    in bin order and amp is subtracted last; bin k's sum runs over the bands that cover it in band order

Their disagreement measures how far n_iter rounds amplify the rounding of one sum: the conditioning figure the GPU bound is derived from
(disagreement(), test_nnls_ref_selftest.py).

`variant` (self-test only, dense order) swaps in ONE deliberate fault, a name from WRONG; None is the definition."""
import numpy as np

NBIN = 513
WRONG = ('no_projection', 'half_step', 'no_momentum', 'stale_momentum', 'tn_momentum', 'zero_start', 'short_bands', 'shifted_bands', 'no_16db')
DISAGREEMENT_CAP = 1e-11                                               # what the self-test holds the dense / band disagreement under
SMALLEST_WRONG = 6.6e-4                                                # the smallest distance of a wrong variant (self-test, asserted there)


def step_of(basis):
    """1 / lambda_max(B^T B), what the Python layer passes as `step`"""
    B = np.asarray(basis, np.float64)
    return 1.0 / float(np.linalg.eigvalsh(B.T @ B)[-1])


def amplitudes(mel, variant=None):
    off = 0.0 if variant == 'no_16db' else 16.0
    return 10.0 ** ((100.0 * np.asarray(mel, np.float64) - 100.0 + off) / 20.0)


def pack(basis):
    """[513, n_mels] -> the packed form, 2 n_mels + W doubles: (first bin, run length) per band, then every band's run of weights in bin
    order, band after band.  A band whose non-zeros are not one contiguous run, or a weight that is negative or not finite, is refused."""
    B = np.asarray(basis, np.float64)
    assert B.ndim == 2 and B.shape[0] == NBIN
    if not (np.isfinite(B).all() and (B >= 0.0).all()):
        raise ValueError('negative or non-finite weight')
    head, weights = [], []
    for m in range(B.shape[1]):
        nz = np.flatnonzero(B[:, m])
        if nz.size and nz[-1] - nz[0] + 1 != nz.size:
            raise ValueError(f'band {m} is not one contiguous run')
        head += [float(nz[0]) if nz.size else 0.0, float(nz.size)]
        weights.append(B[nz, m])
    return np.concatenate([np.asarray(head)] + weights)


def unpack(packed, n_mels):
    """packed -> (first [n_mels], length [n_mels], offset [n_mels + 1] into the weights, weights [W])"""
    p = np.asarray(packed, np.float64)
    lo, ln = p[0:2 * n_mels:2].astype(np.int64), p[1:2 * n_mels:2].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ln)])
    w = p[2 * n_mels:]
    assert off[-1] == w.shape[0] and (lo >= 0).all() and (lo + ln <= NBIN).all()
    return lo, ln, off, w


class _Banded:
    """the two banded products in the kernel's order, vectorised over frames (and over the bands / bins that have an i-th term)"""

    def __init__(self, packed, n_mels):
        lo, ln, off, self.w = unpack(packed, n_mels)
        self.n = n_mels
        # i-th term of every band that has one: (bands, their bin lo + i, their weight index off + i)
        self.band_terms = []
        for i in range(int(ln.max()) if n_mels else 0):
            ms = np.flatnonzero(ln > i)
            self.band_terms.append((ms, lo[ms] + i, off[ms] + i))
        # j-th covering band (in band order) of every bin that has one: (bins, that band, the weight index)
        cover = [[] for _ in range(NBIN)]
        for m in range(n_mels):
            for i in range(int(ln[m])):
                cover[lo[m] + i].append((m, off[m] + i))
        self.bin_terms = []
        for j in range(max(len(c) for c in cover)):
            ks = np.array([k for k in range(NBIN) if len(cover[k]) > j], np.int64)
            self.bin_terms.append((ks, np.array([cover[k][j][0] for k in ks]), np.array([cover[k][j][1] for k in ks])))

    def residual(self, y, amp):
        s = np.zeros((y.shape[0], self.n))
        for ms, ks, ws in self.band_terms:
            s[:, ms] = s[:, ms] + y[:, ks] * self.w[ws]
        return s - amp

    def gradient(self, r):
        g = np.zeros((r.shape[0], NBIN))
        for ks, ms, ws in self.bin_terms:
            g[:, ks] = g[:, ks] + r[:, ms] * self.w[ws]
        return g


def _wrong_basis(B, variant):
    """(the basis of y . B, the basis of r . B^T) of a variant"""
    if variant == 'short_bands':                                       # each band's last bin dropped, in both products
        Bs = B.copy()
        for m in range(B.shape[1]):
            nz = np.flatnonzero(B[:, m])
            if nz.size:
                Bs[nz[-1], m] = 0.0
        return Bs, Bs
    if variant == 'shifted_bands':                                     # r . B^T reads band m + 1's weights for band m
        return B, np.roll(B, -1, axis=1)
    return B, B


def mel_to_linear_nnls(mel, basis, n_iter=200, step=None, floor=1e-10, order='dense', inv_basis=None, variant=None):
    """mel [F, n_mels] on the [0, 1] dB scale, basis [513, n_mels] -> float64 [F, 513]"""
    B = np.asarray(basis, np.float64)
    assert order in ('dense', 'band') and (variant is None or (variant in WRONG and order == 'dense'))
    P = np.linalg.pinv(B) if inv_basis is None else np.asarray(inv_basis, np.float64)
    if step is None:
        step = step_of(B)
    if variant == 'half_step':
        step = 0.5 * step
    amp = amplitudes(mel, variant)
    x = np.maximum(amp @ P, 0.0)
    if variant == 'zero_start':
        x = np.zeros_like(x)
    y, t = x, 1.0
    if order == 'band':
        bd = _Banded(pack(B), B.shape[1])
    else:
        Bf, Bt = _wrong_basis(B, variant)
    for _ in range(n_iter):
        if order == 'band':
            g = bd.gradient(bd.residual(y, amp))
        else:
            g = (y @ Bf - amp) @ Bt.T
        xn = y - step * g
        if variant != 'no_projection':
            xn = np.maximum(xn, 0.0)
        tn = 1.0 if variant == 'no_momentum' else (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta = (tn - 1.0) / tn if variant == 'tn_momentum' else (t - 1.0) / tn
        y, t, x = xn + beta * (xn - (y if variant == 'stale_momentum' else x)), tn, xn
    return np.maximum(x, floor)


def residual(mag, mel, basis):
    """|| mag . B - amp || / || amp ||: how consistent a magnitude is with the mel it was made from"""
    amp = amplitudes(mel)
    return float(np.linalg.norm(np.asarray(mag, np.float64) @ np.asarray(basis, np.float64) - amp) / np.linalg.norm(amp))


def rel_diff(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- the parity inputs and their conditioning
ITERS = (1, 50, 200)


def parity_mel(u1_wav, frames, basis):
    """float32 [frames, n_mels]: griffinlim_ref.melspec of the leading samples of u1_wav that griffinlim_ref.PARITY_SLICES names"""
    from tests import griffinlim_ref as R
    mel = R.melspec(np.asarray(u1_wav, np.float64)[:R.PARITY_SLICES[frames]], basis).astype(np.float32)
    assert mel.shape[0] == frames
    return mel


def disagreement(mel, basis, n_iter, inv_basis=None, step=None):
    """(the band-order result, its distance from the dense one relative to max |x|)"""
    band = mel_to_linear_nnls(mel, basis, n_iter, step, order='band', inv_basis=inv_basis)
    return band, rel_diff(mel_to_linear_nnls(mel, basis, n_iter, step, order='dense', inv_basis=inv_basis), band)
