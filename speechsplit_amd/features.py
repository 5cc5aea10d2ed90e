"""Offline feature extraction (reference make_spect_f0.py with utils.py:10-42) -- SURVEY.md section 8(f) row N4: a recording in, the
(mel, f0) pair the model consumes out.  `extract` is the reference's loop body, `make_spect_f0` its directory walk.

What runs where.  `extract` (one recording, the default): the 5th-order 30 Hz Butterworth high-pass applied forwards and backwards
(`signal.filtfilt`, make_spect_f0.py:54) and the 1e-6 dither from the per-speaker generator (:55) run on the host in scipy / numpy; the STFT
magnitude -> mel projection -> dB -> [0, 1] scaling, the pitch track and the F0 normalisation run on the GPU (csrc/features.hip and
csrc/pitch.hip through the C ABI).  `extract_batch` (a speaker's recordings at once; `make_spect_f0(..., max_rows=N)`): only the odd-length fix
and the dither DRAW stay on the host -- it is the speaker's numpy stream.  The recordings and their draws go to the device in one copy and
run as ragged batches through ss_filtfilt (csrc/filtfilt.hip: scipy's filtfilt to the bit, then the scaling and dither), ss_melspec_batch (the
vocoder's FFT in place of the direct DFT), ss_pitch_track and ss_f0_normalize_batch; one copy per batch brings the results back.  Its F0 is
`extract`'s to the bit and its spectrogram within 1e-6.  With `device_draws=True` (a keyword of `extract_batch_sr` and
`make_spect_f0_batched`; `extract_batch` and `make_spect_f0` keep their pinned argument lists) the draw runs on the device too: `rand_dev` (csrc/mtrand.hip)
continues the speaker's generator -- numpy's MT19937 stream and its conversion to double, bit for bit -- for all the recordings' draws at once
and hands the state back to prng; ss_dither_rows gathers each batch's rows out of that stream, and the upload carries the recordings only.
The same numbers, so the same features; the default (False) makes exactly the host's calls.

Sample rates.  The chain runs at 16 kHz, as the reference asserts (make_spect_f0.py:51).  Recordings at any other rate are brought there
first by `resample` / `resample_dev` (csrc/resample.hip: scipy.signal.resample_poly with scipy's default filter, to the bit, on ragged
batches): `extract(..., sr=)`, `extract_batch_sr` and `make_spect_f0(..., resample=True)`, which reads files with `read_audio`.  The defaults
are the 16 kHz path unchanged; `read_wav` still refuses every other rate by name.

Silence.  Nothing above looks at where the speech is.  `remove_silence` / `remove_silence_dev` (csrc/silence.hip) trim the room tone at both
ends of a recording and cap the pauses inside it, in whole 256-sample blocks (a removed block is a removed mel frame) with a 128-sample
cross-fade at every join; `Silence` holds the options, and `extract_batch_sr`, `extract_opt` and `make_spect_f0_opt` take one as
`silence=` (keyword-only, default None: the calls and the bits are unchanged).  It runs at 16 kHz, behind the resampler and in front of the
odd-length fix and the dither draw.  It is a definition of its own (include/speechsplit_amd.h), pinned to the bit against
tests/silence_ref.py; parity with `librosa.effects.trim` / `split`, which users of the reference reach for, is UNPINNED.

Two parts of the reference come from libraries that are absent here, and both are restated from the published algorithm instead:
  * the mel filter bank (`librosa.filters.mel`, make_spect_f0.py:15): `mel_filter_bank`, Slaney's Auditory-Toolbox mel scale and area
    normalisation with librosa's defaults.  Parity against librosa itself is UNPINNED (nothing of the reference's could be run to produce a
    vector); the function is pinned against hand-computed closed-form values of the published definition for three filters (linear
    region, across 1 kHz, top band: tests/test_capi_host.py::test_mel_filter_bank_closed_form_slaney_values) and its published properties.
  * the F0 track (`pysptk.sptk.rapt`, :64): `pitch_track`, the published core of RAPT (Talkin 1995: normalised cross-correlation
    candidates plus dynamic programming, Talkin's constants) in RAPT's otype=2 output convention -- ln(F0 in Hz), -1e10 for unvoiced frames,
    one value per 256-sample hop.  It is a Talkin-style tracker, NOT a port of SPTK: the two-rate search is left out and the
    spectral-stationarity term is off unless `stationarity=True` asks for it (`pitch_track`, `extract_opt`, `extract_batch_sr`,
    `make_spect_f0_opt`; include/speechsplit_amd.h states the algorithm completely), and agreement with SPTK's own RAPT stays UNPINNED.
    It is pinned against float64 numpy restatements (tests/pitch_ref.py, tests/pitch_stat_ref.py) and against harmonic tones of known F0.
The spectrogram half is pinned by tests/golden/features.npz, generated from the reference's own `butter_highpass` / `pySTFT` /
`speaker_normalization`."""
import ctypes as C
import math
import os
import pickle
import wave

import numpy as np
import torch
from scipy import signal

from . import _capi
from .convert import plan_batches

MIN_SAMPLES = 513                                  # reflect padding by 512


def _hz_to_mel(f):
    """Slaney's mel scale (Auditory Toolbox; librosa's default, htk=False): linear below 1 kHz (200/3 Hz per mel), logarithmic above
    (27 mels per factor of 6.4)."""
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mel = f / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, mel)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filter_bank(sr=16000, n_fft=1024, n_mels=80, fmin=90.0, fmax=7600.0):
    """The basis make_spect_f0.py:15 takes from `librosa.filters.mel(16000, 1024, fmin=90, fmax=7600, n_mels=80)` (and transposes),
    restated from the published algorithm with librosa's defaults: n_mels + 2 band edges equally spaced on Slaney's mel scale, one
    triangle per band over the 1 + n_fft/2 FFT bin frequencies, each scaled by 2 / (its band's width in Hz) ('slaney' norm: unit area).
    Returns float32 [n_mels, 1 + n_fft // 2]; `melspectrogram` wants its transpose.  Pinned against the closed form, not against librosa (see the module docstring)."""
    fft_f = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


def butter_highpass(cutoff, fs, order=5):
    """utils.py:10-14"""
    nyq = 0.5 * fs
    b, a = signal.butter(order, cutoff / nyq, btype='high', analog=False)
    return b, a


def preprocess_wav(x, prng, fs=16000):
    """make_spect_f0.py:49-54: the odd-length fix, high-pass filtfilt, 0.96 scaling and dither.  x float64 [n]."""
    assert fs == 16000
    if x.shape[0] % 256 == 0:
        x = np.concatenate((x, np.array([1e-06])), axis=0)
    b, a = butter_highpass(30, 16000, order=5)
    y = signal.filtfilt(b, a, x)
    return y * 0.96 + (prng.rand(y.shape[0]) - 0.5) * 1e-06


def melspectrogram(wav, mel_basis, device='cuda'):
    """make_spect_f0.py:57-60 on the GPU.  wav float64 [n] (after preprocess_wav), mel_basis float64 [513, n_mels] ->
    float32 [frames, n_mels] tensor on `device`."""
    lib = _capi.lib()
    w = torch.as_tensor(np.ascontiguousarray(wav, dtype=np.float64)).to(device)
    mb = torch.as_tensor(np.ascontiguousarray(mel_basis, dtype=np.float64)).to(device)
    if mb.shape[0] != 513:
        raise ValueError('mel_basis must be [513, n_mels] (1024-point transform)')
    frames = lib.ss_melspec_frames(w.numel())
    out = torch.empty(frames, mb.shape[1], device=device)
    _capi.check(lib.ss_melspec(C.c_void_p(w.data_ptr()), w.numel(), C.c_void_p(mb.data_ptr()), mb.shape[1], C.c_void_p(out.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def normalize_f0(f0_rapt, device='cuda'):
    """make_spect_f0.py:64-66 + utils.py:35-42.  f0_rapt float [n] with -1e10 for unvoiced frames -> float32 [n] tensor."""
    lib = _capi.lib()
    f = torch.as_tensor(np.ascontiguousarray(f0_rapt, dtype=np.float64)).to(device)
    out = torch.empty(f.numel(), device=device)
    _capi.check(lib.ss_f0_normalize(C.c_void_p(f.data_ptr()), f.numel(), C.c_void_p(out.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def f0_from_norm(f0norm, mean, std):
    """The inverse of the reference's speaker normalisation (utils.py:35-42), on the host: the normalised contour [n] in [0, 1] with 0 on
    unvoiced frames, plus the mean and standard deviation of a speaker's voiced ln F0 -> float64 [n] in pitch_track's convention:
    ln F0 = (2 f0norm - 1) 4 std + mean on voiced frames, -1e10 where f0norm is 0.  It is how a converted utterance gets the Hz contour
    vocoder.griffin_lim(f0=...) takes: the contour the model was fed, with the statistics of the speaker whose pitch the output carries.
    (The normalisation clips at +-4 std, so a clipped frame comes back at the clip.)"""
    x = np.asarray(f0norm, np.float64)
    mean, std = float(mean), float(std)
    if x.ndim != 1:
        raise ValueError('f0_from_norm: f0norm must be [n]')
    if not (np.isfinite(mean) and np.isfinite(std) and std > 0.0):
        raise ValueError('f0_from_norm: mean must be finite and std finite and positive')
    return np.where(x != 0.0, (2.0 * x - 1.0) * 4.0 * std + mean, -1e10)


def f0_range(gender):
    """make_spect_f0.py:40-45: the search range in Hz by the speaker's gender"""
    if gender == 'M':
        return 50, 250
    if gender == 'F':
        return 100, 600
    raise ValueError(f"f0_range: gender must be 'M' or 'F', not {gender!r}")


def _stat_flag(who, stationarity):
    """the `stationarity` option of `who`: True or False, anything else is refused by name"""
    if not isinstance(stationarity, bool):
        raise TypeError(f'{who}: stationarity must be True or False, not {stationarity!r}')
    return stationarity


def pitch_track_dev(wav_dev, n_dev, lo, hi, scale=32768.0, *, stationarity=False):
    """The C call on device tensors: wav float64 [B, max_n], n int32 [B] or None (every row has max_n samples) -> float64 [B, frames] of
    ln(F0 in Hz), -1e10 for unvoiced frames and behind a row's own frames.  stationarity=True runs ss_pitch_track_stat: the tracker with
    RAPT's spectral-stationarity term in the voicing transitions (an LPC analysis per frame); False is ss_pitch_track."""
    _stat_flag('pitch_track_dev', stationarity)
    lib = _capi.lib()
    B, max_n = wav_dev.shape
    size, track = (lib.ss_pitch_stat_scratch_bytes, lib.ss_pitch_track_stat) if stationarity else (lib.ss_pitch_scratch_bytes, lib.ss_pitch_track)
    nbytes = size(B, max_n, float(lo), float(hi))
    if nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=wav_dev.device)
    f0 = torch.empty(B, lib.ss_melspec_frames(max_n), dtype=torch.float64, device=wav_dev.device)
    _capi.check(track(C.c_void_p(wav_dev.data_ptr()), C.c_void_p(n_dev.data_ptr()) if n_dev is not None else None, B, max_n,
                    float(scale), float(lo), float(hi), C.c_void_p(f0.data_ptr()), C.c_void_p(scratch.data_ptr()), nbytes,
                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return f0


def filtfilt_dev(x_dev, n_dev, b, a, zi, gain=1.0, dither_dev=None, dither_scale=0.0):
    """The C call on device tensors: x float64 [B, max_n], n int32 [B] or None, host coefficients b [6], a [6] (a[0] == 1), zi [5],
    dither float64 [B, max_n] of uniform draws or None -> float64 [B, max_n]: scipy.signal.filtfilt(b, a, row) * gain + (dither - 0.5) *
    dither_scale on each row's own samples, bit for bit, zeros behind them.  Only 6 coefficients (a 5th-order filter, pad length 18)."""
    lib = _capi.lib()
    b, a, zi = (np.ascontiguousarray(v, dtype=np.float64) for v in (b, a, zi))
    for name, v, k in (('b', b, 6), ('a', a, 6), ('zi', zi, 5)):
        if v.shape != (k,):
            raise ValueError(f'filtfilt_dev: {name} must have {k} entries (6 coefficients, pad length 18: the only order provided), not {v.shape}')
    B, max_n = x_dev.shape
    nbytes = lib.ss_filtfilt_scratch_bytes(B, max_n)
    if nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x_dev.device)
    y = torch.empty_like(x_dev)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    _capi.check(lib.ss_filtfilt(C.c_void_p(x_dev.data_ptr()), C.c_void_p(n_dev.data_ptr()) if n_dev is not None else None, B, max_n,
                                ptr(b), ptr(a), ptr(zi), float(gain), C.c_void_p(dither_dev.data_ptr()) if dither_dev is not None else None,
                                float(dither_scale), C.c_void_p(y.data_ptr()), C.c_void_p(scratch.data_ptr()), nbytes,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y


def melspec_batch_dev(wav_dev, n_dev, mel_basis_dev):
    """The C call on device tensors: wav float64 [B, max_n], n int32 [B] or None, mel_basis float64 [513, n_mels] -> float32
    [B, frames, n_mels], zeros behind a row's own frames."""
    lib = _capi.lib()
    B, max_n = wav_dev.shape
    if mel_basis_dev.shape[0] != 513:
        raise ValueError('mel_basis must be [513, n_mels] (1024-point transform)')
    out = torch.empty(B, lib.ss_melspec_frames(max_n), mel_basis_dev.shape[1], device=wav_dev.device)
    _capi.check(lib.ss_melspec_batch(C.c_void_p(wav_dev.data_ptr()), C.c_void_p(n_dev.data_ptr()) if n_dev is not None else None, B, max_n,
                                     C.c_void_p(mel_basis_dev.data_ptr()), mel_basis_dev.shape[1], C.c_void_p(out.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def f0_normalize_batch_dev(f0_dev, n_dev, max_n, unvoiced=0.0):
    """The C call on device tensors: f0 float64 [B, frames] (pitch_track_dev's output for max_n samples), n int32 [B] or None -> float32
    [B, frames]: normalize_f0 on each row's own frames, `unvoiced` in unvoiced frames and behind them."""
    lib = _capi.lib()
    B = f0_dev.shape[0]
    out = torch.empty(B, f0_dev.shape[1], device=f0_dev.device)
    _capi.check(lib.ss_f0_normalize_batch(C.c_void_p(f0_dev.data_ptr()), C.c_void_p(n_dev.data_ptr()) if n_dev is not None else None, B,
                                          int(max_n), float(unvoiced), C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def rand_dev(prng, count, device='cuda'):
    """`prng.rand(count)` on the GPU (csrc/mtrand.hip: numpy's MT19937 stream, to the bit): a float64 device tensor [count], and prng left
    exactly where prng.rand(count) would have left it.  The generator's key and pos go up (625 words), ss_mt19937_rand continues them, the 625
    words come back and are put into prng with set_state; has_gauss and cached_gaussian are carried over unchanged.  prng must be a
    numpy.random.RandomState on MT19937: anything else is a TypeError (a Generator or another bit generator is another stream)."""
    if not isinstance(prng, np.random.RandomState):
        raise TypeError(f'rand_dev: prng must be a numpy.random.RandomState, not {type(prng).__name__}')
    st = prng.get_state(legacy=False)
    if st.get('bit_generator') != 'MT19937':
        raise TypeError(f"rand_dev: prng must run on MT19937, not {st.get('bit_generator')!r}")
    count = int(count)
    if count < 0:
        raise ValueError(f'rand_dev: count must not be negative, not {count}')
    out = torch.empty(count, dtype=torch.float64, device=device)
    if count == 0:
        return out
    words = np.empty(625, dtype=np.uint32)
    words[:624] = st['state']['key']
    words[624] = st['state']['pos']
    state = torch.from_numpy(words.view(np.int32)).to(device)
    _capi.check(_capi.lib().ss_mt19937_rand(C.c_void_p(state.data_ptr()), count, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    words = state.cpu().numpy().view(np.uint32)
    prng.set_state(('MT19937', words[:624].copy(), int(words[624]), int(st['has_gauss']), float(st['gauss'])))
    return out


def dither_rows_dev(draws_dev, first_dev, n_dev, max_n):
    """The C call on device tensors: draws float64 [count], first int64 [B], n int32 [B] -> float64 [B, max_n]: row b holds
    draws[first[b] : first[b] + n[b]], zeros behind -- the dither layout filtfilt_dev takes."""
    B = first_dev.shape[0]
    out = torch.empty(B, int(max_n), dtype=torch.float64, device=draws_dev.device)
    _capi.check(_capi.lib().ss_dither_rows(C.c_void_p(draws_dev.data_ptr()), draws_dev.numel(), C.c_void_p(first_dev.data_ptr()),
                                           C.c_void_p(n_dev.data_ptr()), B, int(max_n), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def rate_ratio(sr_in, sr_out=16000):
    """(up, down) of a conversion from sr_in to sr_out Hz, reduced as scipy.signal.resample_poly reduces them"""
    if int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f'rate_ratio: sample rates must be positive integers, not {sr_in!r} -> {sr_out!r}')
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    if up > 1024 or down > 1024:
        raise ValueError(f'rate_ratio: {sr_in} -> {sr_out} Hz reduces to {up}/{down}; both must be at most 1024')
    return up, down


def resample_filter(up, down):
    """The FIR scipy.signal.resample_poly designs by default for the reduced up / down: a Kaiser-5.0 windowed sinc of 20 max(up, down) + 1
    taps with its cutoff at the lower of the two Nyquist rates, scaled by up.  float64 [n_taps]; ss_resample takes it as an input."""
    top = max(up, down)
    return signal.firwin(20 * top + 1, 1.0 / top, window=('kaiser', 5.0)) * up


def resample_len(n, up, down):
    """ss_resample_len: the output samples of n input samples, ceil(n up / down)"""
    return -(-int(n) * up // down)


def resample_dev(x_dev, n_dev, up, down, h_dev):
    """The C call on device tensors: x float64 [B, max_n], n int32 [B] or None, h float64 [n_taps] -> float64 [B, ceil(max_n up / down)]:
    scipy.signal.resample_poly(row, up, down, window=h / up) on each row's own samples, bit for bit, zeros behind its own outputs."""
    lib = _capi.lib()
    B, max_n = x_dev.shape
    M = lib.ss_resample_len(max_n, up, down)
    nbytes = lib.ss_resample_scratch_bytes(up, h_dev.numel())
    if M < 0 or nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x_dev.device)
    y = torch.empty(B, M, dtype=torch.float64, device=x_dev.device)
    _capi.check(lib.ss_resample(C.c_void_p(x_dev.data_ptr()), C.c_void_p(n_dev.data_ptr()) if n_dev is not None else None, B, max_n, up, down,
                                C.c_void_p(h_dev.data_ptr()), h_dev.numel(), C.c_void_p(y.data_ptr()),
                                C.c_void_p(scratch.data_ptr()) if nbytes else None, nbytes,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y


def _resample_group(xs, up, down, max_rows, device):
    """recordings of one rate (float64 [n] each) through resample_dev as ragged batches in plan_batches order -> one device tensor
    [ceil(n up / down)] a recording, in input order.  Nothing is brought back and nothing waits for the device."""
    h = torch.from_numpy(resample_filter(up, down)).to(device)
    out = [None] * len(xs)
    for batch in plan_batches([x.shape[0] for x in xs], max_rows):
        lens = [xs[i].shape[0] for i in batch]
        rows = np.zeros((len(batch), lens[-1]))
        for r, i in enumerate(batch):
            rows[r, :lens[r]] = xs[i]
        y = resample_dev(torch.from_numpy(rows).to(device), torch.tensor(lens, dtype=torch.int32, device=device), up, down, h)
        for r, i in enumerate(batch):
            out[i] = y[r, :resample_len(lens[r], up, down)]
    return out


def resample(xs, sr_in, sr_out=16000, max_rows=16, device='cuda'):
    """scipy.signal.resample_poly(x, sr_out, sr_in) on the GPU (csrc/resample.hip), to the bit.  One float64 waveform [n] (or a list of
    them, any lengths >= 1) at sr_in Hz -> float64 numpy [ceil(n sr_out / sr_in)] in input order.  The recordings run as ragged batches of at
    most max_rows rows in convert.plan_batches order; every row is the result of running it alone, so the result does not depend on max_rows.
    sr_in == sr_out returns copies, as scipy does."""
    single = not isinstance(xs, (list, tuple))
    ws = [np.ascontiguousarray(x, dtype=np.float64) for x in ([xs] if single else xs)]
    for i, w in enumerate(ws):
        if w.ndim != 1 or w.shape[0] < 1:
            raise ValueError(f'resample: recording {i} must be [n] with n >= 1, not {w.shape}')
    up, down = rate_ratio(sr_in, sr_out)
    if up == down:
        out = [w.copy() for w in ws]
    else:
        out = [y.cpu().numpy() for y in _resample_group(ws, up, down, max_rows, device)]
    return out[0] if single else out


class Silence:
    """The options of silence removal (`remove_silence`, and the `silence=` keyword of `extract_batch_sr`, `extract_opt` and
    `make_spect_f0_opt`), immutable and validated by name.  top_db: a block of 256 samples is active when the energy of the 512-sample
    window centred on it lies less than top_db decibels below the loudest block's (finite, > 0; the device gets the ratio
    10 ** (-top_db / 10) and takes no logarithm).  hang: blocks on either side of an active block that count as speech.  edge: silent blocks
    kept at either end.  pause: the longest pause, in blocks, left inside; None leaves the pauses alone and only trims.
    include/speechsplit_amd.h (ss_remove_silence) states the definition completely."""
    __slots__ = ('top_db', 'hang', 'edge', 'pause')

    def __init__(self, top_db=40.0, hang=2, edge=6, pause=None):
        if isinstance(top_db, bool) or not isinstance(top_db, (int, float)) or not math.isfinite(top_db) or not top_db > 0:
            raise ValueError(f'Silence: top_db must be a finite number above 0, not {top_db!r}')
        if not 0.0 < 10.0 ** (-float(top_db) / 10.0) < 1.0:
            raise ValueError(f'Silence: top_db must leave the ratio 10 ** (-top_db / 10) inside (0, 1), not {top_db!r}')
        for name, v in (('hang', hang), ('edge', edge)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 2 ** 31 - 1:
                raise ValueError(f'Silence: {name} must be an integer in 0 .. 2^31 - 1, not {v!r}')
        if pause is not None and (isinstance(pause, bool) or not isinstance(pause, int) or not 0 <= pause <= 2 ** 31 - 1):
            raise ValueError(f'Silence: pause must be None or an integer in 0 .. 2^31 - 1, not {pause!r}')
        for name, v in (('top_db', float(top_db)), ('hang', hang), ('edge', edge), ('pause', pause)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError('Silence is immutable')

    def __delattr__(self, name):
        raise AttributeError('Silence is immutable')

    def __repr__(self):
        return f'Silence(top_db={self.top_db!r}, hang={self.hang!r}, edge={self.edge!r}, pause={self.pause!r})'

    def __eq__(self, other):
        return isinstance(other, Silence) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))

    @property
    def ratio(self):
        """what ss_remove_silence takes: the threshold as a share of the loudest block's energy"""
        return 10.0 ** (-self.top_db / 10.0)

    @property
    def pause_blocks(self):
        """what ss_remove_silence takes: -1 for None"""
        return -1 if self.pause is None else self.pause


def _silence_opts(who, opts):
    if not isinstance(opts, Silence):
        raise TypeError(f'{who}: silence must be a Silence, not {opts!r}')
    return opts


def silence_fade():
    """g[r] = 0.5 - 0.5 cos(pi (r + 0.5) / 128), r = 0 .. 127, with the C library's cosine (math.cos): the fade-in gains ss_remove_silence
    takes as a host array.  float64 [128]."""
    return np.array([0.5 - 0.5 * math.cos(math.pi * (r + 0.5) / 128.0) for r in range(128)], dtype=np.float64)


def remove_silence_dev(x_dev, n_dev, opts):
    """The C call on device tensors: x float64 [B, max_n], n int32 [B] or None (every row has max_n samples), opts a Silence ->
    (y float64 [B, max_n], m int32 [B], inv int32 [B, ceil(max_n / 256)], k int32 [B]): each row's kept 256-sample blocks in order with a
    128-sample cross-fade at every join and zeros behind its new length m; inv lists the kept blocks (-1 behind the k of them)."""
    _silence_opts('remove_silence_dev', opts)
    lib = _capi.lib()
    B, max_n = x_dev.shape
    nbytes = lib.ss_silence_scratch_bytes(B, max_n)
    if nbytes < 0:
        _capi.check(-1)
    dev = x_dev.device
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    y = torch.empty_like(x_dev)
    m, k = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    inv = torch.empty(B, (max_n + 255) // 256, dtype=torch.int32, device=dev)
    g = silence_fade()
    _capi.check(lib.ss_remove_silence(C.c_void_p(x_dev.data_ptr()), C.c_void_p(n_dev.data_ptr()) if n_dev is not None else None, B, max_n,
                                      opts.ratio, opts.hang, opts.edge, opts.pause_blocks, g.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.c_void_p(y.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(inv.data_ptr()), C.c_void_p(k.data_ptr()),
                                      C.c_void_p(scratch.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return y, m, inv, k


def _silence_group(ws, opts, max_rows, device):
    """recordings at 16 kHz (device tensors or numpy arrays, float64 [n] each) through remove_silence_dev as ragged batches in plan_batches
    order -> (one device tensor [m] a recording, the new lengths, each recording's kept blocks as a device tensor), in input order.  One small
    copy per batch brings the new lengths and block counts back; the samples stay on the device."""
    out, lens, maps = [None] * len(ws), [0] * len(ws), [None] * len(ws)
    for batch in plan_batches([w.shape[0] for w in ws], max_rows):
        rows = [ws[i].shape[0] for i in batch]
        x = torch.zeros(len(batch), rows[-1], dtype=torch.float64, device=device)
        for r, i in enumerate(batch):
            x[r, :rows[r]] = torch.as_tensor(ws[i]).to(device)
        y, m, inv, k = remove_silence_dev(x, torch.tensor(rows, dtype=torch.int32, device=device), opts)
        mk = torch.stack((m, k)).cpu().numpy()
        for r, i in enumerate(batch):
            lens[i] = int(mk[0, r])
            out[i] = y[r, :lens[i]]
            maps[i] = inv[r, :int(mk[1, r])]
    return out, lens, maps


def remove_silence(xs, opts=Silence(), max_rows=16, device='cuda', return_maps=False):
    """Trim the silence at both ends of recordings at 16 kHz and cap the pauses inside them, on the GPU (csrc/silence.hip; `Silence` has the
    options and include/speechsplit_amd.h the definition).  A list of float64 [n] (any lengths >= 1) -> a list of float64 numpy arrays in input
    order.  The recordings run as ragged batches of at most max_rows rows in convert.plan_batches order; every row is the result of running it
    alone, so the result is the same bits whatever max_rows.  return_maps=True returns (ys, invs) with each recording's kept 256-sample
    blocks, ascending (int32): a removed block is a removed mel frame, so frame-rate data of the original follows by `track[inv]`."""
    _silence_opts('remove_silence', opts)
    ws = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    for i, w in enumerate(ws):
        if w.ndim != 1 or w.shape[0] < 1:
            raise ValueError(f'remove_silence: recording {i} must be [n] with n >= 1, not {w.shape}')
    ys, _, maps = _silence_group(ws, opts, max_rows, device)
    ys = [y.cpu().numpy() for y in ys]
    return (ys, [v.cpu().numpy() for v in maps]) if return_maps else ys


def pitch_track(wavs, lo, hi, max_rows=16, device='cuda', *, stationarity=False):
    """make_spect_f0.py:64 with the Talkin-style tracker of csrc/pitch.hip in place of `sptk.rapt(wav.astype(np.float32) * 32768, fs, 256,
    min=lo, max=hi, otype=2)`.  One float64 waveform [n] at 16 kHz (or a list of them, any lengths >= 513) -> float64 numpy track(s)
    [n // 256 + 1] in input order.  The samples are rounded through float32 and scaled by 32768, as the reference does.  The utterances run
    as ragged batches of at most max_rows rows in convert.plan_batches order; every row is the result of running it alone, so the result
    does not depend on max_rows.  stationarity=True adds RAPT's spectral-stationarity term (`pitch_track_dev`); with False the calls and the
    bits are those of the tracker without it."""
    more = {'stationarity': True} if _stat_flag('pitch_track', stationarity) else {}
    single = not isinstance(wavs, (list, tuple))
    ws = [np.ascontiguousarray(w, dtype=np.float64).astype(np.float32).astype(np.float64) for w in ([wavs] if single else wavs)]
    for w in ws:
        if w.ndim != 1 or w.shape[0] < MIN_SAMPLES:
            raise ValueError(f'pitch_track: every waveform must be [n] with n >= {MIN_SAMPLES}')
    out = [None] * len(ws)
    for batch in plan_batches([w.shape[0] for w in ws], max_rows):
        lens = [ws[i].shape[0] for i in batch]
        wav = np.zeros((len(batch), lens[-1]))
        for r, i in enumerate(batch):
            wav[r, :lens[r]] = ws[i]
        f0 = pitch_track_dev(torch.from_numpy(wav).to(device), torch.tensor(lens, dtype=torch.int32, device=device), lo, hi, **more).cpu().numpy()
        for r, i in enumerate(batch):
            out[i] = f0[r, :lens[r] // 256 + 1].copy()
    return out[0] if single else out


def read_wav(path):
    """16-bit mono PCM at 16 kHz through the standard library's `wave` -> float64 [n] in [-1, 1) (samples / 32768, as soundfile reads
    them): the counterpart of vocoder.save_wav.  Any other format is refused by name."""
    with wave.open(path, 'rb') as f:
        ch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if ch != 1:
            raise ValueError(f'read_wav: {path}: {ch} channels; mono only')
        if width != 2:
            raise ValueError(f'read_wav: {path}: {8 * width}-bit samples; 16-bit PCM only')
        if sr != 16000:
            raise ValueError(f'read_wav: {path}: sample rate {sr}; 16000 Hz only')
        pcm = np.frombuffer(f.readframes(n), '<i2')
    return pcm.astype(np.float64) / 32768.0


def read_audio(path):
    """Mono PCM of 8, 16, 24 or 32 bits at ANY sample rate through the standard library's `wave` -> (x float64 [n], sr).  Samples are scaled
    by 2^(bits - 1), 8-bit ones (unsigned in the file) centred on 128 first, as soundfile reads them.  Float and extensible WAV files and more
    than one channel are refused by name."""
    try:
        f = wave.open(path, 'rb')
    except wave.Error as e:
        raise ValueError(f'read_audio: {path}: {e}; integer PCM WAV only (float and extensible formats are not read)') from None
    with f:
        ch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if ch != 1:
            raise ValueError(f'read_audio: {path}: {ch} channels; mono only')
        if width not in (1, 2, 3, 4):
            raise ValueError(f'read_audio: {path}: {8 * width}-bit samples; 8, 16, 24 or 32-bit PCM only')
        raw = np.frombuffer(f.readframes(n), np.uint8)
    if width == 1:
        pcm = raw.astype(np.int64) - 128
    elif width == 3:
        b = raw.reshape(-1, 3).astype(np.int64)
        pcm = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
        pcm = pcm - ((pcm & 0x800000) << 1)                                # sign of the 24-bit value
    else:
        pcm = raw.view('<i2' if width == 2 else '<i4')
    return pcm.astype(np.float64) / float(1 << (8 * width - 1)), sr


def extract(x, prng, gender, device='cuda', mel_basis=None, unvoiced=0.0, sr=16000):
    """The loop body of make_spect_f0.py:49-74 for one recording x float64 [n] at 16 kHz: (S float32 [F, 80], f0_norm float32 [F]).
    A recording at another rate `sr` is brought to 16 kHz first (`resample`: scipy.signal.resample_poly on the GPU, to the bit).
    prng is the speaker's numpy RandomState (the dither draws from it, so recordings of one speaker go through in the reference's order).
    mel_basis [513, n_mels] defaults to mel_filter_bank().T, the reference's.  f0_norm is in [0, 1] on voiced frames and `unvoiced` elsewhere:
    0 by default, which `quantize_f0` reads as unvoiced (<= 0); the reference's speaker_normalization leaves its -1e10 marker in those frames
    (utils.py:39-41 touch the voiced frames only), and that is what its files carry -- make_spect_f0 passes unvoiced=-1e10.
    (Its argument list is pinned; `extract_opt` takes the same and `stationarity` by keyword.)"""
    return _extract(x, prng, gender, device, mel_basis, unvoiced, sr, False)


def extract_opt(x, prng, gender, *, device='cuda', mel_basis=None, unvoiced=0.0, sr=16000, stationarity=False, silence=None):
    """`extract` with its options by keyword, and the ones it cannot take: stationarity=True tracks the pitch with RAPT's
    spectral-stationarity term (`pitch_track(..., stationarity=True)`); silence=Silence(...) removes silence at 16 kHz first
    (`remove_silence`: behind the resampler, in front of the odd-length fix and the dither draw).  With False and None it is `extract`: the
    same calls, the same bits."""
    if silence is not None:
        return _extract(x, prng, gender, device, mel_basis, unvoiced, sr, _stat_flag('extract_opt', stationarity),
                        _silence_opts('extract_opt', silence))
    return _extract(x, prng, gender, device, mel_basis, unvoiced, sr, _stat_flag('extract_opt', stationarity))


def _extract(x, prng, gender, device, mel_basis, unvoiced, sr, stationarity, silence=None):
    """extract's body; `stationarity` is handed to pitch_track only when it is set, and remove_silence runs only when `silence` is, so that the
    defaults make the earlier calls"""
    x = np.asarray(x, np.float64)
    if sr != 16000:
        x = resample(x, sr, 16000, device=device)
    if silence is not None:
        x = remove_silence([x], silence, device=device)[0]
        if x.shape[0] + (x.shape[0] % 256 == 0) < MIN_SAMPLES:
            raise ValueError(f'extract_opt: recording 0 has {x.shape[0]} samples after silence removal; it must have n >= {MIN_SAMPLES}')
    wav = preprocess_wav(x, prng)
    S = melspectrogram(wav, mel_filter_bank().T.astype(np.float64) if mel_basis is None else mel_basis, device).cpu().numpy()
    lo, hi = f0_range(gender)
    f0_rapt = pitch_track(wav, lo, hi, device=device, **({'stationarity': True} if stationarity else {}))
    f0_norm = normalize_f0(f0_rapt, device).cpu().numpy()
    assert len(S) == len(f0_rapt)
    return S.astype(np.float32), np.where(f0_rapt != -1e10, f0_norm, np.float32(unvoiced)).astype(np.float32)


def stage_batches(xs, prng, max_rows, host_draws=True):
    """The host side of extract_batch: the odd-length fix (make_spect_f0.py:52-53) on every recording, the dither draws from the speaker's
    generator IN INPUT ORDER (so they do not depend on max_rows), then the plan_batches batches packed into one float64 buffer.  Returns
    (flat, lens, batches): batch k = (indices, offset, B, max_n) has its recordings at flat[offset : offset + B * max_n] as [B, max_n] (zeros
    behind each row) and their draws in the B * max_n entries after that; lens int32 holds the batches' row lengths one after another.
    host_draws=False (the draw on the device) makes no draw and leaves the draws' halves out: flat is half as long."""
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    for i, x in enumerate(xs):
        if x.ndim != 1:
            raise ValueError(f'extract_batch: recording {i} must be [n], not {x.shape}')
        if x.shape[0] % 256 == 0:
            xs[i] = x = np.concatenate((x, np.array([1e-06])), axis=0)
        if x.shape[0] < MIN_SAMPLES:
            raise ValueError(f'extract_batch: recording {i} has {x.shape[0]} samples; every recording must be [n] with n >= {MIN_SAMPLES}')
    draws = [prng.rand(x.shape[0]) for x in xs] if host_draws else None
    plan = plan_batches([x.shape[0] for x in xs], max_rows)
    batches, off = [], 0
    for idx in plan:
        B, max_n = len(idx), xs[idx[-1]].shape[0]
        batches.append((idx, off, B, max_n))
        off += (2 if host_draws else 1) * B * max_n
    flat = np.zeros(off)
    for idx, o, B, max_n in batches:
        xb = flat[o:o + B * max_n].reshape(B, max_n)
        for r, i in enumerate(idx):
            xb[r, :xs[i].shape[0]] = xs[i]
        if host_draws:
            rb = flat[o + B * max_n:o + 2 * B * max_n].reshape(B, max_n)
            for r, i in enumerate(idx):
                rb[r, :xs[i].shape[0]] = draws[i]
    lens = np.array([xs[i].shape[0] for idx, _, _, _ in batches for i in idx], dtype=np.int32)
    return flat, lens, batches


def _draw_offsets(lens_in_order, batches):
    """where each batch row's draws begin in one prng.rand(sum of the lengths): the prefix sums of the lengths IN INPUT ORDER, listed in the
    batches' row order (int64, one after another as stage_batches lists the lengths)"""
    start = np.concatenate(([0], np.cumsum(lens_in_order, dtype=np.int64)[:-1])) if len(lens_in_order) else np.zeros(0, np.int64)
    return np.array([start[i] for idx in batches for i in idx], dtype=np.int64)


def extract_batch(xs, prng, gender, max_rows=16, device='cuda', mel_basis=None, unvoiced=0.0):
    """`extract` for a speaker's recordings xs (a list of float64 [n] at 16 kHz) with the whole chain on the GPU: a list of (S, f0_norm), the
    same as calling `extract` on each recording in order with the same prng -- f0_norm to the bit, S within 1e-6 (an FFT in place of the direct
    DFT).  The recordings and their dither draws go up in one copy and run as ragged batches of at most max_rows rows in plan_batches order;
    every row is the result of running it alone, so the result does not depend on max_rows.  One copy per batch brings S and f0_norm back.
    (Its argument list is pinned; the draw on the device is `extract_batch_sr(xs, 16000, ..., device_draws=True)`.)"""
    return _extract_batch(xs, prng, gender, max_rows, device, mel_basis, unvoiced, False)


def _extract_batch(xs, prng, gender, max_rows, device, mel_basis, unvoiced, device_draws, stationarity=False):
    """extract_batch, with the draw on the host or (device_draws) on the GPU: one `rand_dev` for the sum of the (fixed-up) lengths in input
    order -- the same numbers, and prng is left in the same state -- and one ss_dither_rows a batch hands each row its stretch; the upload
    then carries the recordings only."""
    f0_range(gender)                                                    # an unknown gender stops the call before a draw is made
    flat, lens, batches = stage_batches(xs, prng, max_rows, **({'host_draws': False} if device_draws else {}))
    chain = _Chain(gender, device, mel_basis, unvoiced, stationarity)
    flat_dev, lens_dev = torch.from_numpy(flat).to(device), torch.from_numpy(lens).to(device)
    if device_draws:
        own = np.zeros(len(xs), dtype=np.int64)                         # the fixed-up lengths in input order
        own[[i for idx, _, _, _ in batches for i in idx]] = lens
        draws = rand_dev(prng, int(own.sum()), device)
        first_dev = torch.from_numpy(_draw_offsets(own, [idx for idx, _, _, _ in batches])).to(device)
    out, row = [None] * len(xs), 0
    for idx, o, B, max_n in batches:
        x = flat_dev[o:o + B * max_n].view(B, max_n)
        if device_draws:
            r = dither_rows_dev(draws, first_dev[row:row + B], lens_dev[row:row + B], max_n)
        else:
            r = flat_dev[o + B * max_n:o + 2 * B * max_n].view(B, max_n)
        for i, feats in zip(idx, chain(x, r, lens_dev[row:row + B], lens[row:row + B])):
            out[i] = feats
        row += B
    return out


class _Chain:
    """The four device calls of extract_batch on one batch: x, r float64 [B, max_n] (recordings after the odd-length fix, their dither draws)
    and the rows' lengths on the device (n) and on the host (lens) -> [(S, f0_norm)] a row, after one copy back."""

    def __init__(self, gender, device, mel_basis, unvoiced, stationarity=False):
        self.lo, self.hi = f0_range(gender)
        self.more = {'stationarity': True} if stationarity else {}         # handed to pitch_track_dev only when it is set
        self.b, self.a = butter_highpass(30, 16000, order=5)
        self.zi = signal.lfilter_zi(self.b, self.a)
        self.mb = torch.as_tensor(np.ascontiguousarray(mel_filter_bank().T if mel_basis is None else mel_basis, dtype=np.float64)).to(device)
        self.unvoiced = unvoiced

    def __call__(self, x, r, n, lens):
        B, max_n = x.shape
        wav = filtfilt_dev(x, n, self.b, self.a, self.zi, 0.96, r, 1e-06)
        S = melspec_batch_dev(wav, n, self.mb)
        f0 = pitch_track_dev(wav.float().double(), n, self.lo, self.hi, **self.more)     # the float32 round trip of make_spect_f0.py:64
        f0n = f0_normalize_batch_dev(f0, n, max_n, self.unvoiced)
        F, M = S.shape[1], S.shape[2]
        both = torch.cat((S.reshape(B, F * M), f0n), dim=1).cpu().numpy()
        out = []
        for k in range(B):
            Fi = int(lens[k]) // 256 + 1
            out.append((both[k, :F * M].reshape(F, M)[:Fi].copy(), both[k, F * M:F * M + Fi].copy()))
        return out


def _to_16k(xs, ratios, max_rows, device):
    """recordings with their reduced (up, down) to 16 kHz -> one device tensor a recording, in input order: grouped by rate, each group
    through ss_resample as ragged batches (a recording at 16 kHz is uploaded as it is)"""
    wav16 = [None] * len(xs)
    for ratio in sorted(set(ratios)):
        group = [i for i, q in enumerate(ratios) if q == ratio]
        if ratio == (1, 1):
            ys = [torch.from_numpy(xs[i]).to(device) for i in group]
        else:
            ys = _resample_group([xs[i] for i in group], ratio[0], ratio[1], max_rows, device)
        for i, y in zip(group, ys):
            wav16[i] = y
    return wav16


def extract_batch_sr(xs, sr, prng, gender, max_rows=16, device='cuda', mel_basis=None, unvoiced=0.0, *, device_draws=False,
                     stationarity=False, silence=None):
    """`extract_batch` for recordings at any sample rate: sr is one rate in Hz for all of xs, or one a recording.  The same as
    extract_batch([scipy.signal.resample_poly(x, 16000, sr) ...], prng, gender, ...), to the bit, with the resampling on the GPU in front of the
    chain and nothing brought back between them: the recordings are grouped by rate and each group runs through ss_resample as ragged batches in
    plan_batches order; the odd-length fix and the dither draws then apply to the RESAMPLED lengths -- ceil(n 16000 / sr), which the host knows
    without waiting for the device -- with the draws in input order; then extract_batch's four calls on batches of the resampled recordings.
    With every rate 16000 this IS extract_batch: the same calls on the same data.  device_draws=True makes the dither draw on the GPU: one
    `rand_dev` for the sum of the fixed-up (resampled) lengths in input order -- the same numbers, prng left in the same state -- and one
    ss_dither_rows a batch; the default makes exactly the host's calls.  stationarity=True tracks the pitch with RAPT's
    spectral-stationarity term (`pitch_track_dev(..., stationarity=True)`); with False the calls and the bits are today's.  (`extract_batch`'s
    argument list is pinned, so this is also the batched entry point for that option at 16 kHz.)  silence=Silence(...) removes silence at
    16 kHz (`remove_silence_dev`: behind the resampler, in front of the odd-length fix and the draws): the same as extract_batch_sr on the
    trimmed recordings at 16000 Hz, to the bit.  The new lengths come back in one small copy per batch; the fix, the draws in input order and
    the 513-sample minimum then apply to them as they apply to resampled lengths, and a recording that ends shorter is refused by its
    index with its new length.  With None the calls and the bits are today's."""
    _stat_flag('extract_batch_sr', stationarity)
    if silence is not None:
        _silence_opts('extract_batch_sr', silence)
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    srs = [sr] * len(xs) if np.ndim(sr) == 0 else list(sr)
    if len(srs) != len(xs):
        raise ValueError(f'extract_batch_sr: {len(srs)} sample rates for {len(xs)} recordings')
    if silence is None and all(s == 16000 for s in srs):
        if stationarity:
            return _extract_batch(xs, prng, gender, max_rows, device, mel_basis, unvoiced, bool(device_draws), True)
        if device_draws:
            return _extract_batch(xs, prng, gender, max_rows, device, mel_basis, unvoiced, True)
        return extract_batch(xs, prng, gender, max_rows, device, mel_basis, unvoiced)
    ratios = [rate_ratio(s, 16000) for s in srs]
    for i, x in enumerate(xs):
        if x.ndim != 1 or x.shape[0] < 1:
            raise ValueError(f'extract_batch_sr: recording {i} must be [n], not {x.shape}')
    own = [resample_len(x.shape[0], up, down) for x, (up, down) in zip(xs, ratios)]      # samples at 16 kHz
    if silence is not None:
        f0_range(gender)                                                                   # an unknown gender stops the call before any device work
        wav16, own, _ = _silence_group(_to_16k(xs, ratios, max_rows, device), silence, max_rows, device)
    lens = [m + 1 if m % 256 == 0 else m for m in own]                                     # after the odd-length fix
    for i, n in enumerate(lens):
        if n < MIN_SAMPLES:
            if silence is not None:
                raise ValueError(f'extract_batch_sr: recording {i} has {own[i]} samples after silence removal; every recording must have '
                                 f'n >= {MIN_SAMPLES}')
            raise ValueError(f'extract_batch_sr: recording {i} has {n} samples at 16 kHz; every recording must have n >= {MIN_SAMPLES}')
    f0_range(gender)
    plan = plan_batches(lens, max_rows)
    if device_draws:
        draws = rand_dev(prng, sum(lens), device)                                          # input order, whatever the grouping
        first_dev = torch.from_numpy(_draw_offsets(lens, plan)).to(device)
    else:
        draws = [prng.rand(n) for n in lens]                                               # input order, whatever the grouping
    if silence is None:
        wav16 = _to_16k(xs, ratios, max_rows, device)                                      # device tensors [own[i]]
    chain = _Chain(gender, device, mel_basis, unvoiced, stationarity)
    out, row = [None] * len(xs), 0
    for idx in plan:
        B, max_n = len(idx), lens[idx[-1]]
        x = torch.zeros(B, max_n, dtype=torch.float64, device=device)
        rb = None if device_draws else np.zeros((B, max_n))
        for k, i in enumerate(idx):
            x[k, :own[i]] = wav16[i]
            if lens[i] > own[i]:
                x[k, own[i]] = 1e-06
            if not device_draws:
                rb[k, :lens[i]] = draws[i]
        rows = [lens[i] for i in idx]
        n_dev = torch.tensor(rows, dtype=torch.int32, device=device)
        r = dither_rows_dev(draws, first_dev[row:row + B], n_dev, max_n) if device_draws else torch.from_numpy(rb).to(device)
        for i, feats in zip(idx, chain(x, r, n_dev, rows)):
            out[i] = feats
        row += B
    return out


def make_spect_f0(root_dir='assets/wavs', target_dir='assets/spmel', target_dir_f0='assets/raptf0', spk2gen='assets/spk2gen.pkl',
                  device='cuda', resample=False, max_rows=None):
    """The directory walk of make_spect_f0.py:28-74: root_dir/<speaker>/<name>.wav -> target_dir/<speaker>/<name>.npy (S, float32 [F, 80])
    and target_dir_f0/<speaker>/<name>.npy (f0_norm, float32 [F], -1e10 in unvoiced frames as the reference's files); speakers and files in sorted order, one RandomState(int(speaker[1:])) per
    speaker.  spk2gen: a {speaker: 'M' | 'F'} dict, or the path of the reference's pickle of one.  max_rows=None runs `extract` file by file; an
    integer runs each speaker's files through `extract_batch` in batches of at most that many rows (the same F0 files, mel files within
    1e-6).  resample=False reads 16 kHz files only (`read_wav`, which refuses every other rate by name, as the reference asserts); True reads
    mono PCM of any rate and width (`read_audio`) and brings it to 16 kHz on the GPU first, writing the files the 16 kHz path writes for
    scipy.signal.resample_poly(x, 16000, sr).  Returns the (speaker, name) pairs written.  (Its argument list is pinned; the batched walk
    with its further options is `make_spect_f0_batched`, and `make_spect_f0_opt` takes every option, `stationarity` among them.)"""
    return _walk(root_dir, target_dir, target_dir_f0, spk2gen, device, resample, max_rows, False)


def make_spect_f0_batched(root_dir='assets/wavs', target_dir='assets/spmel', target_dir_f0='assets/raptf0', spk2gen='assets/spk2gen.pkl',
                          max_rows=16, *, device='cuda', resample=False, device_draws=False):
    """`make_spect_f0(..., max_rows=max_rows)`, the walk through `extract_batch_sr`, with that path's own options by keyword.
    device_draws=True draws each speaker's dither on the GPU (`rand_dev`: numpy's stream to the bit), so the files written are the same,
    byte for byte.  Returns the (speaker, name) pairs written."""
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or max_rows < 1:
        raise ValueError(f'make_spect_f0_batched: max_rows must be a positive integer, not {max_rows!r}')
    if not isinstance(device_draws, bool):
        raise TypeError(f'make_spect_f0_batched: device_draws must be True or False, not {device_draws!r}')
    return _walk(root_dir, target_dir, target_dir_f0, spk2gen, device, resample, max_rows, device_draws)


def make_spect_f0_opt(root_dir='assets/wavs', target_dir='assets/spmel', target_dir_f0='assets/raptf0', spk2gen='assets/spk2gen.pkl', *,
                      device='cuda', resample=False, max_rows=None, device_draws=False, stationarity=False, silence=None):
    """The walk of `make_spect_f0` (max_rows=None: file by file) and of `make_spect_f0_batched` (an integer) with every option by keyword,
    and the ones their pinned argument lists cannot take: stationarity=True tracks the pitch with RAPT's spectral-stationarity term;
    silence=Silence(...) removes silence from every recording at 16 kHz first (`remove_silence`).  With False and None it writes the files
    those two write.  Returns the (speaker, name) pairs written."""
    if max_rows is not None and (isinstance(max_rows, bool) or not isinstance(max_rows, int) or max_rows < 1):
        raise ValueError(f'make_spect_f0_opt: max_rows must be None or a positive integer, not {max_rows!r}')
    if not isinstance(device_draws, bool):
        raise TypeError(f'make_spect_f0_opt: device_draws must be True or False, not {device_draws!r}')
    if device_draws and max_rows is None:
        raise ValueError('make_spect_f0_opt: device_draws needs the batched walk (max_rows)')
    if silence is not None:
        return _walk(root_dir, target_dir, target_dir_f0, spk2gen, device, resample, max_rows, device_draws,
                     _stat_flag('make_spect_f0_opt', stationarity), _silence_opts('make_spect_f0_opt', silence))
    return _walk(root_dir, target_dir, target_dir_f0, spk2gen, device, resample, max_rows, device_draws,
                 _stat_flag('make_spect_f0_opt', stationarity))


def _walk(root_dir, target_dir, target_dir_f0, spk2gen, device, resample, max_rows, device_draws, stationarity=False, silence=None):
    """make_spect_f0's walk; device_draws, stationarity and silence are handed on only when they are set, so that the default makes the
    earlier calls"""
    more = {'device_draws': True} if device_draws else {}
    if stationarity:
        more['stationarity'] = True
    if silence is not None:
        more['silence'] = silence
    if not isinstance(resample, bool):
        raise TypeError(f'make_spect_f0: resample must be True or False, not {resample!r} (max_rows goes by keyword)')
    if not isinstance(spk2gen, dict):
        with open(spk2gen, 'rb') as f:
            spk2gen = pickle.load(f)
    dir_name, subdirs, _ = next(os.walk(root_dir))
    done = []
    for subdir in sorted(subdirs):
        os.makedirs(os.path.join(target_dir, subdir), exist_ok=True)
        os.makedirs(os.path.join(target_dir_f0, subdir), exist_ok=True)
        _, _, files = next(os.walk(os.path.join(dir_name, subdir)))
        f0_range(spk2gen[subdir])                                      # an unknown gender stops the walk before anything is written
        prng = np.random.RandomState(int(subdir[1:]))
        names = sorted(files)
        read = (lambda name: read_audio(os.path.join(dir_name, subdir, name))) if resample else \
            (lambda name: (read_wav(os.path.join(dir_name, subdir, name)), 16000))
        if max_rows is not None:
            recs = [read(name) for name in names]
            feats = extract_batch_sr([x for x, _ in recs], [sr for _, sr in recs], prng, spk2gen[subdir], max_rows, device,
                                     unvoiced=-1e10, **more) if names else []
        for k, name in enumerate(names):
            if max_rows is not None:
                S, f0_norm = feats[k]
            else:
                x, sr = read(name)
                if silence is not None:
                    S, f0_norm = _extract(x, prng, spk2gen[subdir], device, None, -1e10, sr, stationarity, silence)
                else:
                    S, f0_norm = _extract(x, prng, spk2gen[subdir], device, None, -1e10, sr, True) if stationarity else \
                        extract(x, prng, spk2gen[subdir], device, unvoiced=-1e10, sr=sr)
            np.save(os.path.join(target_dir, subdir, name[:-4]), S, allow_pickle=False)
            np.save(os.path.join(target_dir_f0, subdir, name[:-4]), f0_norm, allow_pickle=False)
            done.append((subdir, name[:-4]))
    return done
