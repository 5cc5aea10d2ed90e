"""Mel spectrograms back to waveforms: a Griffin-Lim vocoder on the GPU (csrc/vocoder.hip through the C ABI), the checkpoint-free stand-in
for the last cell of the reference's demo.ipynb (WaveNet with an external checkpoint, which stays out of scope).

It inverts what this project itself defines (features.py / csrc/features.hip): the [0, 1] dB scale and the mel basis of `melspectrogram`,
and the 1024-point periodic-Hann STFT at hop 256 with reflect padding.  The mel basis is inverted by its pseudo-inverse
(`numpy.linalg.pinv`), floored -- the default, inversion='pinv' -- or, with inversion='nnls', by the non-negative solution that projected
FISTA reaches from there on the device (ss_mel_to_linear_nnls: what librosa does with NNLS, here without an external library), and
Griffin-Lim with momentum (Perraudin et al. 2013, librosa's form) finds a phase.  With an F0 track (`f0=`) the voiced frames are replaced by
a harmonic fit -- one amplitude per harmonic, ss_mel_to_linear_harmonic -- and the phase search starts from harmonic phases
(ss_harmonic_phase); without one nothing changes.  L frames become 256 (L - 1) samples, and `melspectrogram` of those has L frames again.  float64 throughout; the same bits on
every run; the starting phases are inputs, drawn on the host.  No engine needed."""
import ctypes as C
import wave

import numpy as np
import torch

from . import _capi, features
from .convert import plan_batches

NBIN = 513
MIN_FRAMES = 4                                     # reflect padding by 512 needs 513 samples


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_PINV = {}


def _inv_basis(mel_basis):
    """float64 [n_mels, 513]: the pseudo-inverse of the [513, n_mels] basis `melspectrogram` takes (None: the project's own filter bank)"""
    if mel_basis is None:
        if None not in _PINV:
            _PINV[None] = np.linalg.pinv(features.mel_filter_bank().T.astype(np.float64))
        return _PINV[None]
    mb = np.asarray(mel_basis, np.float64)
    if mb.ndim != 2 or mb.shape[0] != NBIN:
        raise ValueError('mel_basis must be [513, n_mels] (1024-point transform)')
    return np.linalg.pinv(mb)


INVERSIONS = ('pinv', 'nnls')
_NNLS = {}


def _check_inversion(who, inversion):
    if inversion not in INVERSIONS:
        raise ValueError(f"{who}: inversion is 'pinv' or 'nnls', not {inversion!r}")


def _nnls_basis(mel_basis):
    """(packed float64 [2 n_mels + weights], step): ss_mel_nnls_pack's form of the [513, n_mels] basis and 1 / lambda_max(B^T B);
    packed once for the project's own filter bank (None), as _inv_basis"""
    if mel_basis is None and None in _NNLS:
        return _NNLS[None]
    mb = np.ascontiguousarray(features.mel_filter_bank().T if mel_basis is None else mel_basis, dtype=np.float64)
    if mb.ndim != 2 or mb.shape[0] != NBIN:
        raise ValueError('mel_basis must be [513, n_mels] (1024-point transform)')
    lib = _capi.lib()
    size = lib.ss_mel_nnls_pack(C.c_void_p(mb.ctypes.data), mb.shape[1], None, 0)
    if size < 0:
        _capi.check(-1)
    packed = np.empty(size, np.float64)
    if lib.ss_mel_nnls_pack(C.c_void_p(mb.ctypes.data), mb.shape[1], C.c_void_p(packed.ctypes.data), size) != size:
        _capi.check(-1)
    out = packed, 1.0 / float(np.linalg.eigvalsh(mb.T @ mb)[-1])
    if mel_basis is None:
        _NNLS[None] = out
    return out


def _mel_to_linear_nnls(mel_dev, inv_dev, packed_dev, frames_dev, n_iter, step, floor):
    """_mel_to_linear's shapes, packed_dev float64 [2 n_mels + weights]: n_iter rounds of projected FISTA from the clipped pseudo-inverse"""
    B, T, n_mels = mel_dev.shape
    mag = torch.empty(B, T, NBIN, dtype=torch.float64, device=mel_dev.device)
    _capi.check(_capi.lib().ss_mel_to_linear_nnls(_ptr(mel_dev), _ptr(inv_dev), _ptr(packed_dev), packed_dev.numel(), _ptr(frames_dev), B, T,
                                                  n_mels, int(n_iter), float(step), float(floor), _ptr(mag), _stream()))
    return mag


def _mel_to_linear(mel_dev, inv_dev, frames_dev, floor):
    """mel_dev float32 [B, T, n_mels], inv_dev float64 [n_mels, 513], frames_dev int32 [B] or None -> float64 [B, T, 513], all on one device"""
    B, T, n_mels = mel_dev.shape
    mag = torch.empty(B, T, NBIN, dtype=torch.float64, device=mel_dev.device)
    _capi.check(_capi.lib().ss_mel_to_linear(_ptr(mel_dev), _ptr(inv_dev), _ptr(frames_dev), B, T, n_mels, float(floor), _ptr(mag), _stream()))
    return mag


def f0_hz(f0):
    """A track in features.pitch_track's convention (ln Hz, -1e10 on unvoiced frames) -> float64 Hz, 0 on unvoiced frames: what the
    harmonic calls take.  Anything that is not finite counts as unvoiced."""
    f = np.asarray(f0, np.float64)
    ok = np.isfinite(f) & (f > -1e9)
    with np.errstate(over='ignore'):
        hz = np.exp(np.where(ok, f, 0.0))
    return np.where(ok & np.isfinite(hz), hz, 0.0)


def _check_f0(who, f0, lens):
    """one track -> [track]; every track's length must be its mel's"""
    tracks = list(f0) if isinstance(f0, (list, tuple)) else [f0]
    tracks = [np.asarray(t, np.float64) for t in tracks]
    if len(tracks) != len(lens) or any(t.ndim != 1 or t.shape[0] != n for t, n in zip(tracks, lens)):
        raise ValueError(f'{who}: f0 must hold one track per mel, each as long as its mel')
    return [f0_hz(t) for t in tracks]


def _mel_to_linear_harmonic(mel_dev, f0hz_dev, inv_dev, packed_dev, frames_dev, n_iter, f_top, floor, mag_dev):
    """_mel_to_linear's shapes, f0hz_dev float64 [B, T] in Hz, mag_dev [B, T, 513] filled by either route: the voiced frames of mag_dev are
    overwritten with the harmonic fit (ss_mel_to_linear_harmonic); returns the harmonic share float64 [B, T, 513]"""
    B, T, n_mels = mel_dev.shape
    share = torch.empty(B, T, NBIN, dtype=torch.float64, device=mel_dev.device)
    _capi.check(_capi.lib().ss_mel_to_linear_harmonic(_ptr(mel_dev), _ptr(f0hz_dev), _ptr(inv_dev), _ptr(packed_dev), packed_dev.numel(),
                                                      _ptr(frames_dev), B, T, n_mels, float(f_top), int(n_iter), float(floor), _ptr(mag_dev),
                                                      _ptr(share), _stream()))
    return share


def _harmonic_phase(f0hz_dev, share_dev, rand_dev, frames_dev, f_top):
    """f0hz_dev [B, T], share_dev [B, T, 513], rand_dev the same or None (zeros) -> the start phases float64 [B, T, 513]"""
    lib = _capi.lib()
    B, T = f0hz_dev.shape
    nbytes = lib.ss_harmonic_phase_scratch_bytes(B, T)
    if nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=f0hz_dev.device)
    phase0 = torch.empty(B, T, NBIN, dtype=torch.float64, device=f0hz_dev.device)
    _capi.check(lib.ss_harmonic_phase(_ptr(f0hz_dev), _ptr(share_dev), _ptr(rand_dev), _ptr(frames_dev), B, T, float(f_top), _ptr(phase0),
                                      _ptr(scratch), nbytes, _stream()))
    return phase0


def mel_to_linear(mel, mel_basis=None, floor=1e-10, device='cuda', inversion='pinv', nnls_iter=200, f0=None, harmonic_iter=50,
                  f_top=7600.0, return_share=False):
    """mel float [L, n_mels] on `melspectrogram`'s [0, 1] dB scale -> float64 [L, 513] tensor on `device`:
    max(floor, 10^((100 mel - 100 + 16) / 20) . pinv(mel_basis)).  mel_basis [513, n_mels] defaults to features.mel_filter_bank().T.
    inversion='nnls': nnls_iter rounds of projected FISTA from there towards the non-negative magnitude whose mel is the given one
    (ss_mel_to_linear_nnls; step 1 / lambda_max(B^T B)), then the floor.
    f0 [L] (features.pitch_track's convention; it has to belong to this mel): the voiced frames are replaced by the harmonic fit of
    ss_mel_to_linear_harmonic, harmonic_iter rounds, harmonics up to f_top Hz.  return_share: (magnitude, harmonic share [L, 513])."""
    _check_inversion('mel_to_linear', inversion)
    m = torch.as_tensor(np.ascontiguousarray(mel, dtype=np.float32)).to(device)
    if m.dim() != 2 or m.shape[0] < MIN_FRAMES:
        raise ValueError(f'mel_to_linear: mel must be [L, n_mels] with L >= {MIN_FRAMES}')
    inv = torch.as_tensor(_inv_basis(mel_basis)).to(device)
    if inv.shape[0] != m.shape[1]:
        raise ValueError(f'mel_to_linear: mel has {m.shape[1]} bands, the basis {inv.shape[0]}')
    hz = _check_f0('mel_to_linear', f0, [m.shape[0]])[0] if f0 is not None else None
    if inversion == 'nnls' or hz is not None:
        packed, step = _nnls_basis(mel_basis)
        packed = torch.as_tensor(packed).to(device)
    if inversion == 'nnls':
        mag = _mel_to_linear_nnls(m[None], inv, packed, None, nnls_iter, step, floor)
    else:
        mag = _mel_to_linear(m[None], inv, None, floor)
    if hz is None:
        return (mag[0], torch.zeros_like(mag[0])) if return_share else mag[0]
    share = _mel_to_linear_harmonic(m[None], torch.from_numpy(hz[None]).to(device), inv, packed, None, harmonic_iter, f_top, floor, mag)
    return (mag[0], share[0]) if return_share else mag[0]


def griffin_lim_mag(mag_dev, phase0_dev, frames_dev, n_iter, momentum):
    """The C call on device tensors: mag float64 [B, T, 513], phase0 the same or None (zeros), frames int32 [B] or None ->
    float64 [B, 256 (T - 1)]; row b's samples beyond 256 (frames[b] - 1) are zeros."""
    lib = _capi.lib()
    B, T = mag_dev.shape[:2]
    nbytes = lib.ss_griffinlim_scratch_bytes(B, T)
    if nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=mag_dev.device)
    wav = torch.empty(B, lib.ss_griffinlim_samples(T), dtype=torch.float64, device=mag_dev.device)
    _capi.check(lib.ss_griffinlim(_ptr(mag_dev), _ptr(phase0_dev), _ptr(frames_dev), B, T, int(n_iter), float(momentum), _ptr(wav),
                                  _ptr(scratch), nbytes, _stream()))
    return wav


def prepare(mels, phases=None, generator=None):
    """Host side of griffin_lim: (single, [mel float32 [L, n_mels]], [phase float64 [L, 513]] or None).  phases: None draws uniform
    [-pi, pi) phases from `generator` (default numpy.random.default_rng(0)) per utterance, in INPUT order -- so the draws, and with them the
    result, do not depend on how the utterances are batched; 'zero' starts from zero phases; else one [L, 513] array per utterance."""
    single = not isinstance(mels, (list, tuple))
    ms = [np.ascontiguousarray(m, dtype=np.float32) for m in ([mels] if single else mels)]
    for m in ms:
        if m.ndim != 2 or m.shape[0] < MIN_FRAMES or m.shape[1] != ms[0].shape[1]:
            raise ValueError(f'griffin_lim: every mel must be [L, n_mels] with L >= {MIN_FRAMES} and one n_mels')
    if isinstance(phases, str):
        if phases != 'zero':
            raise ValueError("griffin_lim: phases is None, 'zero' or one [L, 513] array per utterance")
        return single, ms, None
    if phases is None:
        gen = generator if generator is not None else np.random.default_rng(0)
        ps = [gen.uniform(-np.pi, np.pi, (m.shape[0], NBIN)) for m in ms]
    else:
        ps = [np.ascontiguousarray(p, dtype=np.float64) for p in ([phases] if single else phases)]
        if len(ps) != len(ms) or any(p.shape != (m.shape[0], NBIN) for p, m in zip(ps, ms)):
            raise ValueError('griffin_lim: phases must hold one [L, 513] array per utterance')
    return single, ms, ps


def griffin_lim(mels, n_iter=60, momentum=0.99, phases=None, generator=None, max_rows=16, device='cuda', mel_basis=None, floor=1e-10,
                inversion='pinv', nnls_iter=200, f0=None, harmonic_iter=50, f_top=7600.0):
    """One mel [L, 80] (or a list of them, any lengths >= 4) -> float64 numpy waveform(s) of 256 (L - 1) samples at 16 kHz, in input order.
    The utterances run as ragged batches of at most max_rows rows in convert.plan_batches order; every row is the result of running it alone,
    so the result does not depend on max_rows.  phases / generator: see prepare().  inversion / nnls_iter: see mel_to_linear().
    f0: one track or a list matching `mels` (features.pitch_track's convention: ln Hz, -1e10 unvoiced; each as long as its mel, and it has
    to belong to that mel -- features.f0_from_norm gives a converted utterance's).  The chosen inversion fills the magnitude, the harmonic
    fit (harmonic_iter rounds, harmonics up to f_top Hz) overwrites the voiced frames, and Griffin-Lim starts from the harmonic phases mixed
    with the drawn (or given, or zero) ones by the harmonic share.  Without f0 nothing changes."""
    _check_inversion('griffin_lim', inversion)
    single, ms, ps = prepare(mels, phases, generator)
    inv = torch.as_tensor(_inv_basis(mel_basis)).to(device)
    if ms and inv.shape[0] != ms[0].shape[1]:
        raise ValueError(f'griffin_lim: mel has {ms[0].shape[1]} bands, the basis {inv.shape[0]}')
    hzs = _check_f0('griffin_lim', f0, [m.shape[0] for m in ms]) if f0 is not None else None
    if inversion == 'nnls' or hzs is not None:
        packed, step = _nnls_basis(mel_basis)
        packed = torch.as_tensor(packed).to(device)
    out = [None] * len(ms)
    for batch in plan_batches([m.shape[0] for m in ms], max_rows):
        lens = [ms[i].shape[0] for i in batch]
        T = lens[-1]
        mel = np.zeros((len(batch), T, ms[0].shape[1]), np.float32)
        ph = np.zeros((len(batch), T, NBIN)) if ps is not None else None
        for n, i in enumerate(batch):
            mel[n, :lens[n]] = ms[i]
            if ph is not None:
                ph[n, :lens[n]] = ps[i]
        frames = torch.tensor(lens, dtype=torch.int32, device=device)
        if inversion == 'nnls':
            mag = _mel_to_linear_nnls(torch.from_numpy(mel).to(device), inv, packed, frames, nnls_iter, step, floor)
        else:
            mag = _mel_to_linear(torch.from_numpy(mel).to(device), inv, frames, floor)
        ph = torch.from_numpy(ph).to(device) if ph is not None else None
        if hzs is not None:
            hz = np.zeros((len(batch), T))
            for n, i in enumerate(batch):
                hz[n, :lens[n]] = hzs[i]
            hz = torch.from_numpy(hz).to(device)
            share = _mel_to_linear_harmonic(torch.from_numpy(mel).to(device), hz, inv, packed, frames, harmonic_iter, f_top, floor, mag)
            ph = _harmonic_phase(hz, share, ph, frames, f_top)
        wav = griffin_lim_mag(mag, ph, frames, n_iter, momentum).cpu().numpy()
        for n, i in enumerate(batch):
            out[i] = wav[n, :256 * (lens[n] - 1)].copy()
    return out[0] if single else out


def save_wav(path, wav, sr=16000):
    """16-bit mono PCM through the standard library's `wave`; samples are clipped to [-1, 1]"""
    pcm = np.round(np.clip(np.asarray(wav, np.float64), -1.0, 1.0) * 32767.0).astype('<i2')
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sr))
        f.writeframes(pcm.tobytes())
