"""A float64 numpy restatement of the vocoder (csrc/vocoder.hip): the STFT / ISTFT pair of utils.py:18-31's framing, Griffin-Lim with momentum
as published (Perraudin, Balazs and Sondergaard 2013; librosa's form) and the mel -> linear-magnitude step.  The yardstick of
test_gpu_vocoder.py, proven on wrong stand-ins by test_griffinlim_ref_selftest.py.  Importing it needs no GPU.

    frame f   = padded samples [256 f, 256 f + 1024), the n-sample signal reflect-padded by 512 (the edge sample is not repeated)
    window    = 0.5 - 0.5 cos(2 pi i / 1024)                          (periodic Hann)
    stft      = rfft(window * frame)                                  [F, 513] complex, F = (n + 256) // 256
    istft     = overlap-add of window * irfft(spec[f]) in frame order, each sample divided by the sum of window^2 over the frames that
                cover it (1.5 in the interior, down to 1.25 inside the kept range), trimmed by 512 at both ends: n = 256 (F - 1) samples
    griffin_lim:  ang = exp(i phase0); tprev = 0
                  n_iter times:  r = stft(istft(S ang));  a = r - momentum / (1 + momentum) tprev;  tprev = r;  ang = a / (|a| + 1e-16)
                  x = istft(S ang)

Every function takes `transform`: 'fft' (numpy.fft, pocketfft) or 'dft' (a product with an explicit 1024 x 513 matrix of twiddles).  The two
share no code below the framing, so their disagreement measures how far the iteration amplifies the rounding of a transform: the
conditioning figure the GPU bound is derived from (test_griffinlim_ref_selftest.py).  mel_to_linear has no transform in it.

`variant` (self-test only) swaps in ONE deliberate fault, a name from WRONG; None is the definition."""
import numpy as np

NFFT, HOP, NBIN = 1024, 256, 513
WRONG = ('symmetric_hann', 'const_norm', 'zero_pad', 'plain_momentum', 'stale_tprev', 'no_final_istft', 'hop_off_by_one')

_I = np.arange(NFFT)
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * _I / NFFT)
_SYM = 0.5 - 0.5 * np.cos(2.0 * np.pi * _I / (NFFT - 1))               # the fault: scipy's sym=True window

# the explicit transform: cos / sin of 2 pi (k t mod 1024) / 1024 from one 1024-entry table whose zeros are exact
_TAB = 2.0 * np.pi * _I / NFFT
_COS, _SIN = np.cos(_TAB), np.sin(_TAB)
_COS[[256, 768]] = 0.0
_SIN[[0, 512]] = 0.0
_KT = (_I[:, None] * np.arange(NBIN)[None, :]) % NFFT                  # [1024 t, 513 k]
_MC, _MS = _COS[_KT], _SIN[_KT]
_WK = np.full(NBIN, 2.0)
_WK[[0, NBIN - 1]] = 1.0


def _rfft(frames, transform):
    if transform == 'fft':
        return np.fft.rfft(frames, axis=-1)
    assert transform == 'dft'
    return frames @ _MC - 1j * (frames @ _MS)


def _irfft(spec, transform):
    """numpy.fft.irfft's convention: the imaginary parts of bins 0 and 512 are ignored, scale 1 / 1024"""
    if transform == 'fft':
        return np.fft.irfft(spec, n=NFFT, axis=-1)
    assert transform == 'dft'
    return ((spec.real * _WK) @ _MC.T - (spec.imag * _WK) @ _MS.T) / NFFT


def frames_of(n):
    return (n + HOP) // HOP if n >= NFFT // 2 + 1 else 0


def stft(x, transform='fft', variant=None):
    """x float64 [n], n >= 513 -> complex128 [frames_of(n), 513]"""
    x = np.asarray(x, np.float64)
    F = frames_of(x.shape[0])
    assert F >= 1
    xp = np.pad(x, NFFT // 2, mode='constant' if variant == 'zero_pad' else 'reflect')
    hop = HOP - 1 if variant == 'hop_off_by_one' else HOP
    w = _SYM if variant == 'symmetric_hann' else WINDOW
    fr = np.stack([xp[hop * f:hop * f + NFFT] for f in range(F)])
    return _rfft(fr * w, transform)


def istft(spec, transform='fft', variant=None):
    """complex [F, 513], F >= 4 -> float64 [256 (F - 1)]"""
    spec = np.asarray(spec)
    F = spec.shape[0]
    assert F >= 4 and spec.shape[1] == NBIN
    w = _SYM if variant == 'symmetric_hann' else WINDOW
    fr = _irfft(spec, transform) * w
    y = np.zeros(HOP * (F - 1) + NFFT)
    norm = np.zeros_like(y)
    for f in range(F):                                                # the fixed order the kernel's gather uses
        y[HOP * f:HOP * f + NFFT] += fr[f]
        norm[HOP * f:HOP * f + NFFT] += w * w
    keep = slice(NFFT // 2, NFFT // 2 + HOP * (F - 1))
    return y[keep] / (1.5 if variant == 'const_norm' else norm[keep])


def griffin_lim(S, n_iter=32, momentum=0.99, phase0=None, transform='fft', variant=None):
    """S float64 [F, 513] magnitudes, phase0 float64 [F, 513] or None (zeros) -> float64 [256 (F - 1)]"""
    S = np.asarray(S, np.float64)
    ang = np.ones(S.shape, np.complex128) if phase0 is None else np.exp(1j * np.asarray(phase0, np.float64))
    c = momentum if variant == 'plain_momentum' else momentum / (1.0 + momentum)
    tprev = tolder = np.zeros(S.shape, np.complex128)
    x = None
    for _ in range(n_iter):
        x = istft(S * ang, transform, variant)
        r = stft(x, transform, variant)
        a = r - c * (tolder if variant == 'stale_tprev' else tprev)
        tolder, tprev = tprev, r
        ang = a / (np.abs(a) + 1e-16)
    if variant == 'no_final_istft' and x is not None:
        return x
    return istft(S * ang, transform, variant)


def mel_to_linear(mel, inv_basis, floor=1e-10):
    """mel [F, n_mels] (the [0, 1] dB scale of melspec) , inv_basis float64 [n_mels, 513] -> float64 [F, 513]:
    amp = 10^((100 mel - 100 + 16) / 20), mag = max(floor, amp . inv_basis)"""
    amp = 10.0 ** ((100.0 * np.asarray(mel, np.float64) - 100.0 + 16.0) / 20.0)
    return np.maximum(floor, amp @ np.asarray(inv_basis, np.float64))


def melspec(x, mel_basis, transform='fft'):
    """make_spect_f0.py:57-60 in float64 (no cast): x [n], mel_basis [513, n_mels] -> [frames, n_mels]"""
    mag = np.abs(stft(x, transform))
    db = 20.0 * np.log10(np.maximum(10.0 ** (-100.0 / 20.0), mag @ np.asarray(mel_basis, np.float64))) - 16.0
    return (db + 100.0) / 100.0


def rel_diff(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- the parity inputs and their conditioning
PARITY_SLICES = {4: 768, 5: 1024, 9: 2048, 41: None}                   # frames -> leading samples of features.npz's u1_wav
MOMENTA = (0.0, 0.99)
DIVERGENCE_CAP = 1e-10                                                 # what the self-test holds the fft / dft disagreement under


def parity_input(u1_wav, frames):
    """(S [frames, 513] = |stft| of the slice, seeded phases [frames, 513]): magnitudes of real speech.  (demo_conversion.npz's mels are an
    untrained model's near-silence -- out_R: max |x| 3e-4 -- on which the two transforms end 2e-7 apart after 32 rounds: no parity input.)"""
    S = np.abs(stft(np.asarray(u1_wav, np.float64)[:PARITY_SLICES[frames]]))
    assert S.shape[0] == frames
    return S, np.random.default_rng(100 + frames).uniform(-np.pi, np.pi, S.shape)


def divergence(S, phase0, n_iter=32):
    """The largest fft-against-dft disagreement of griffin_lim over zero / given phases and both momenta, relative to max |x|: how far n_iter
    rounds amplify the rounding of a transform on this input."""
    return max(rel_diff(griffin_lim(S, n_iter, m, p, 'dft'), griffin_lim(S, n_iter, m, p, 'fft')) for p in (None, phase0) for m in MOMENTA)
