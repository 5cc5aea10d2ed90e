"""Scores of a conversion on the GPU (csrc/dtw.hip through the C ABI): the mel-cepstral distortion between two mel spectrograms of
different lengths along a dynamic-time-warping path, and the F0 and voicing error along the same path.

The definitions are the header's (include/speechsplit_amd.h, "conversion scores"): cepstra are rows 1 .. n_ceps of the orthonormal DCT-II of
the mel bands (row 0, the level, is left out); the frame distance is 50 sqrt(2) times the Euclidean distance of the cepstra -- this project's
mels are S = (dB + 100) / 100, so ln|A| = (100 S - 84) ln 10 / 20 and the usual (10 / ln 10) sqrt(2 sum dc^2) in dB becomes that scale on
the cepstra of S; DTW takes steps (1,1), (1,0), (0,1) of weight 1 with both ends fixed, the diagonal winning a tie, then (i-1, j), with no
band and no slope constraint; mcd_db is the path's total cost over its length.  F0 tracks are features.pitch_track's: ln Hz, -1e10 for
unvoiced frames.  float64 throughout; the same bits on every run, whatever the batching.  No engine needed.

Waveforms are scored by `stoi` (csrc/stoi.hip): the short-time objective intelligibility measure and its extended form of a degraded
waveform against a time-aligned clean one, as the header's "waveform scores" section defines them."""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from .convert import plan_batches

SCALE = 50.0 * math.sqrt(2.0)                      # (10 / ln 10) sqrt(2) * (100 ln 10 / 20): dB per unit of cepstral distance of S
UNVOICED = -1e10


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def dct_basis(n_ceps=24, n_mels=80):
    """float64 [n_ceps, n_mels]: rows d = 1 .. n_ceps of the orthonormal DCT-II, sqrt(2 / n_mels) cos(pi d (m + 1/2) / n_mels)"""
    n_ceps, n_mels = int(n_ceps), int(n_mels)
    if not 1 <= n_mels <= 128:
        raise ValueError('dct_basis: n_mels outside 1 .. 128')
    if not 1 <= n_ceps <= 40:
        raise ValueError('dct_basis: n_ceps outside 1 .. 40')
    d = np.arange(1, n_ceps + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / n_mels) * np.cos(np.pi * d * (m + 0.5) / n_mels)


def cepstra_dev(mel_dev, len_dev, dct_dev):
    """The C call on device tensors: mel float32 [B, T, n_mels], len int32 [B] or None, dct float64 [n_ceps, n_mels] -> float64
    [B, T, n_ceps]; rows at or beyond a row's length are zeros."""
    B, T, n_mels = mel_dev.shape
    out = torch.empty(B, T, dct_dev.shape[0], dtype=torch.float64, device=mel_dev.device)
    _capi.check(_capi.lib().ss_mel_cepstra(_ptr(mel_dev), _ptr(len_dev), B, T, n_mels, _ptr(dct_dev), dct_dev.shape[0], _ptr(out),
                                           _stream(mel_dev)))
    return out


def dtw_dev(fx_dev, tx_dev, fy_dev, ty_dev, scale=SCALE, want_path=True):
    """The C call on device tensors: fx float64 [B, Tx, dim], fy float64 [B, Ty, dim], tx / ty int32 [B] or None ->
    (out float64 [B, 3] = total, P, mcd; path int32 [B, Tx + Ty - 1, 2] with -1 beyond P; path_len int32 [B]); the last two are None
    without want_path."""
    lib = _capi.lib()
    B, Tx, dim = fx_dev.shape
    Ty = fy_dev.shape[1]
    nbytes = lib.ss_dtw_scratch_bytes(B, Tx, Ty)
    if nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=fx_dev.device)
    out = torch.empty(B, 3, dtype=torch.float64, device=fx_dev.device)
    path = torch.empty(B, Tx + Ty - 1, 2, dtype=torch.int32, device=fx_dev.device) if want_path else None
    plen = torch.empty(B, dtype=torch.int32, device=fx_dev.device) if want_path else None
    _capi.check(lib.ss_dtw(_ptr(fx_dev), _ptr(tx_dev), _ptr(fy_dev), _ptr(ty_dev), B, Tx, Ty, dim, float(scale), _ptr(out), _ptr(path),
                           _ptr(plen), _ptr(scratch), nbytes, _stream(fx_dev)))
    return out, path, plen


def path_f0_stats_dev(path_dev, plen_dev, f0x_dev, f0y_dev):
    """The C call on device tensors: path int32 [B, Tx + Ty - 1, 2], path_len int32 [B] or None, f0x float64 [B, Tx], f0y float64 [B, Ty]
    -> float64 [B, 5] = n_vv, n_vu, f0_rmse_cents, f0_corr, vuv_error."""
    B, Tx = f0x_dev.shape
    Ty = f0y_dev.shape[1]
    if tuple(path_dev.shape) != (B, Tx + Ty - 1, 2):
        raise ValueError(f'path_f0_stats_dev: path must be [B, Tx + Ty - 1, 2] = {(B, Tx + Ty - 1, 2)}, got {tuple(path_dev.shape)}')
    out = torch.empty(B, 5, dtype=torch.float64, device=f0x_dev.device)
    _capi.check(_capi.lib().ss_path_f0_stats(_ptr(path_dev), _ptr(plen_dev), _ptr(f0x_dev), _ptr(f0y_dev), B, Tx, Ty, _ptr(out),
                                             _stream(f0x_dev)))
    return out


def score_batch(mel_x, tx, mel_y, ty, f0x, f0y, dct, device, want_path):
    """One ragged batch, host arrays in and out: mel_x float32 [B, Tx, n_mels] and mel_y float32 [B, Ty, n_mels] padded behind each row's
    own tx[b] / ty[b] frames, f0x float64 [B, Tx] / f0y float64 [B, Ty] or None, dct float64 [n_ceps, n_mels] ->
    (out [B, 3], stats [B, 5] or None, path [B, Tx + Ty - 1, 2] or None, path_len [B] or None)."""
    dct_d = torch.from_numpy(dct).to(device)
    tx_d = torch.tensor(tx, dtype=torch.int32, device=device)
    ty_d = torch.tensor(ty, dtype=torch.int32, device=device)
    cx = cepstra_dev(torch.from_numpy(mel_x).to(device), tx_d, dct_d)
    cy = cepstra_dev(torch.from_numpy(mel_y).to(device), ty_d, dct_d)
    need_path = want_path or f0x is not None
    out, path, plen = dtw_dev(cx, tx_d, cy, ty_d, SCALE, need_path)
    stats = None
    if f0x is not None:
        stats = path_f0_stats_dev(path, plen, torch.from_numpy(f0x).to(device), torch.from_numpy(f0y).to(device)).cpu().numpy()
    if not want_path:
        path = plen = None
    return (out.cpu().numpy(), stats, path.cpu().numpy() if path is not None else None, plen.cpu().numpy() if plen is not None else None)


def _mels(name, arg):
    ms = [np.ascontiguousarray(m, dtype=np.float32) for m in arg]
    for m in ms:
        if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError(f'mcd_dtw: {name}: every mel must be [T, n_mels] with T >= 1')
    return ms


def _f0s(name, arg, ms):
    fs = [np.ascontiguousarray(f, dtype=np.float64) for f in arg]
    if len(fs) != len(ms):
        raise ValueError(f'mcd_dtw: {name}: one F0 track per mel ({len(fs)} tracks, {len(ms)} mels)')
    for f, m in zip(fs, ms):
        if f.shape != (m.shape[0],):
            raise ValueError(f"mcd_dtw: {name}: an F0 track's length must be its mel's ({f.shape} against {m.shape[0]} frames)")
    return fs


def mcd_dtw(xs, ys, f0x=None, f0y=None, n_ceps=24, max_rows=16, device='cuda', return_paths=False):
    """Mels xs[n] [Tx, n_mels] against ys[n] [Ty, n_mels] (lists, or one pair of arrays): one dict per pair, in input order, with
    ``mcd_db`` (the DTW path's cost over its length, in dB), ``total`` (the cost) and ``path_len``.  With f0x / f0y (ln Hz, -1e10 unvoiced,
    one value per frame: features.pitch_track's output) also ``f0_rmse_cents``, ``f0_corr``, ``vuv_error`` and ``n_voiced`` (the path steps
    where both frames are voiced) along the same path; with return_paths also ``path``, int32 [P, 2] of (i, j).  The pairs run as ragged
    batches of at most max_rows rows in convert.plan_batches order of max(Tx, Ty); every row is the result of running it alone, so the
    result does not depend on max_rows.  One pair in, one dict out."""
    single = not isinstance(xs, (list, tuple))
    if single:
        xs, ys = [xs], [ys]
        f0x = None if f0x is None else [f0x]
        f0y = None if f0y is None else [f0y]
    mx, my = _mels('xs', xs), _mels('ys', ys)
    if len(mx) != len(my):
        raise ValueError(f'mcd_dtw: ys: one mel per mel of xs ({len(my)} against {len(mx)})')
    if (f0x is None) != (f0y is None):
        raise ValueError('mcd_dtw: f0x and f0y: give both or neither')
    fx = fy = None
    if f0x is not None:
        fx, fy = _f0s('f0x', f0x, mx), _f0s('f0y', f0y, my)
    res = [None] * len(mx)
    if not mx:
        return res
    n_mels = mx[0].shape[1]
    for name, ms in (('xs', mx), ('ys', my)):
        if any(m.shape[1] != n_mels for m in ms):
            raise ValueError(f'mcd_dtw: {name}: every mel must have the same n_mels ({n_mels})')
    dct = dct_basis(n_ceps, n_mels)
    for batch in plan_batches([max(a.shape[0], b.shape[0]) for a, b in zip(mx, my)], max_rows):
        tx, ty = [mx[i].shape[0] for i in batch], [my[i].shape[0] for i in batch]
        Tx, Ty = max(tx), max(ty)
        bx, by = np.zeros((len(batch), Tx, n_mels), np.float32), np.zeros((len(batch), Ty, n_mels), np.float32)
        gx = np.full((len(batch), Tx), UNVOICED) if fx is not None else None
        gy = np.full((len(batch), Ty), UNVOICED) if fx is not None else None
        for n, i in enumerate(batch):
            bx[n, :tx[n]], by[n, :ty[n]] = mx[i], my[i]
            if fx is not None:
                gx[n, :tx[n]], gy[n, :ty[n]] = fx[i], fy[i]
        out, stats, path, plen = score_batch(bx, tx, by, ty, gx, gy, dct, device, bool(return_paths))
        for n, i in enumerate(batch):
            r = {'mcd_db': float(out[n, 2]), 'total': float(out[n, 0]), 'path_len': int(out[n, 1])}
            if stats is not None:
                r.update(f0_rmse_cents=float(stats[n, 2]), f0_corr=float(stats[n, 3]), vuv_error=float(stats[n, 4]),
                         n_voiced=int(stats[n, 0]))
            if return_paths:
                r['path'] = np.ascontiguousarray(path[n, :int(plen[n])], dtype=np.int32)
            res[i] = r
    return res[0] if single else res


# ---------------------------------------------------------------------------------------------- waveform scores (csrc/stoi.hip)
STOI_SR = 10000
STOI_FRAME, STOI_HOP, STOI_NFFT, STOI_BANDS, STOI_FIRST_HZ = 256, 128, 512, 15, 150.0


def stoi_bands(n_bands=STOI_BANDS, first_hz=STOI_FIRST_HZ, sr=STOI_SR, n_fft=STOI_NFFT):
    """(lo, hi), two lists of n_bands ints: third-octave bands with centres first_hz * 2^(j/3) and edges a sixth of an octave either side,
    each edge at the nearest of the bin frequencies k sr / n_fft; band j sums bins lo[j] .. hi[j] - 1."""
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sr / n_fft)
    cf = first_hz * 2.0 ** (np.arange(int(n_bands), dtype=np.float64) / 3.0)
    lo = [int(np.argmin(np.abs(f - c * 2.0 ** (-1.0 / 6.0)))) for c in cf]
    hi = [int(np.argmin(np.abs(f - c * 2.0 ** (1.0 / 6.0)))) for c in cf]
    return lo, hi


def stoi_frames(n):
    """frames of n samples at 10 kHz: floor((n - 256) / 128) + 1, none below 256 samples"""
    return (int(n) - STOI_FRAME) // STOI_HOP + 1 if n >= STOI_FRAME else 0


def _int_array(v):
    return (C.c_int * len(v))(*[int(a) for a in v])


def stoi_dev(x_dev, y_dev, n_dev, extended=False, bands=None):
    """The C call on device tensors: x, y float64 [B, max_n] at 10 kHz, n int32 [B] or None -> float64 [B, 3] = score, S, K."""
    lib = _capi.lib()
    B, max_n = x_dev.shape
    lo, hi = bands if bands is not None else stoi_bands()
    nbytes = lib.ss_stoi_scratch_bytes(B, max_n)
    if nbytes < 0:
        _capi.check(-1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x_dev.device)
    out = torch.empty(B, 3, dtype=torch.float64, device=x_dev.device)
    _capi.check(lib.ss_stoi(_ptr(x_dev), _ptr(y_dev), _ptr(n_dev), B, max_n, _int_array(lo), _int_array(hi), len(lo), int(bool(extended)),
                            _ptr(out), _ptr(scratch), nbytes, _stream(x_dev)))
    return out


def stoi_compact_dev(x_dev, y_dev, n_dev, inv_dev=None, k_dev=None):
    """The test hook on device tensors: x, y float64 [B, max_n], n int32 [B] or None -> (e float64 [B, F], inv int32 [B, F], K int32 [B],
    x' and y' float64 [B, 128 (F - 1) + 256]).  With inv_dev and k_dev given the energies and the mask are skipped (e is None) and the
    gather runs through the given map."""
    B, max_n = x_dev.shape
    F = max(stoi_frames(max_n), 1)
    L = STOI_HOP * (F - 1) + STOI_FRAME
    from_map = inv_dev is not None
    e = None if from_map else torch.empty(B, F, dtype=torch.float64, device=x_dev.device)
    inv = inv_dev if from_map else torch.empty(B, F, dtype=torch.int32, device=x_dev.device)
    k = k_dev if from_map else torch.empty(B, dtype=torch.int32, device=x_dev.device)
    xp, yp = (torch.empty(B, L, dtype=torch.float64, device=x_dev.device) for _ in range(2))
    _capi.check(_capi.lib().ss_op_stoi_compact(_ptr(x_dev), _ptr(y_dev), _ptr(n_dev), B, max_n, int(from_map), _ptr(e), _ptr(inv), _ptr(k),
                                               _ptr(xp), _ptr(yp), _stream(x_dev)))
    return e, inv, k, xp, yp


def stoi_envelopes_dev(sig_dev, len_dev, bands=None):
    """The test hook on device tensors: sig float64 [B, max_len], len int32 [B] or None -> float64 [B, n_bands, ceil((max_len - 256) / 128)],
    zeros at and behind a row's own frames."""
    B, max_len = sig_dev.shape
    lo, hi = bands if bands is not None else stoi_bands()
    M = max(-(-(max_len - STOI_FRAME) // STOI_HOP), 1)
    env = torch.empty(B, len(lo), M, dtype=torch.float64, device=sig_dev.device)
    _capi.check(_capi.lib().ss_op_stoi_bands(_ptr(sig_dev), _ptr(len_dev), B, max_len, _int_array(lo), _int_array(hi), len(lo), _ptr(env),
                                             _stream(sig_dev)))
    return env


def stoi_pairs(refs, degs):
    """Host side of `stoi`: float64 copies of every pair, each cut to the shorter of the two"""
    single = not isinstance(refs, (list, tuple))
    if single:
        refs, degs = [refs], [degs]
    if len(refs) != len(degs):
        raise ValueError(f'stoi: degs: one degraded waveform per reference ({len(degs)} against {len(refs)})')
    pairs = []
    for i, (r, d) in enumerate(zip(refs, degs)):
        r, d = np.ascontiguousarray(r, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        if r.ndim != 1 or d.ndim != 1 or r.shape[0] < 1 or d.shape[0] < 1:
            raise ValueError(f'stoi: pair {i}: waveforms must be [n] with n >= 1, not {r.shape} and {d.shape}')
        n = min(r.shape[0], d.shape[0])
        pairs.append((r[:n], d[:n]))
    return single, pairs


def stoi_batch(x, y, n, extended, device):
    """One ragged batch, host arrays in and out: x, y float64 [B, max_n] at 10 kHz, n the rows' lengths -> out [B, 3]"""
    n_d = torch.tensor(n, dtype=torch.int32, device=device)
    return stoi_dev(torch.from_numpy(x).to(device), torch.from_numpy(y).to(device), n_d, extended).cpu().numpy()


def stoi(refs, degs, sr=16000, extended=False, max_rows=16, device='cuda'):
    """STOI (``extended=True``: ESTOI) of degraded waveforms degs[n] against time-aligned clean ones refs[n] (lists of 1-D waveforms at
    ``sr`` Hz, or one pair): one dict per pair, in input order, with ``stoi`` (the score; NaN when fewer than 31 frames survive the
    silent-frame removal), ``segments`` (the 30-frame segments averaged over), ``frames_kept`` and ``frames``.  Each pair is cut to the
    shorter of the two; both are brought to 10 kHz with features.resample (skipped when sr == 10000).  The pairs run as ragged batches of
    at most max_rows rows in convert.plan_batches order; every row is the result of running it alone, so the bits do not depend on
    max_rows.  The measure needs sample 0 of one waveform to BE sample 0 of the other: a vocoded mel against the recording it came from,
    or a conversion that keeps the rhythm against its source."""
    from . import features                              # features imports plan_batches from convert as this module does
    single, pairs = stoi_pairs(refs, degs)
    res = [None] * len(pairs)
    if not pairs:
        return res
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    if int(sr) != STOI_SR:
        both = features.resample(xs + ys, sr, STOI_SR, max_rows=max_rows, device=device)
        xs, ys = both[:len(pairs)], both[len(pairs):]
    lens = [x.shape[0] for x in xs]
    for batch in plan_batches(lens, max_rows):
        n = [lens[i] for i in batch]
        max_n = max(n[-1], STOI_FRAME)                  # the C call takes at least one frame's room; a shorter row scores NaN
        bx, by = np.zeros((len(batch), max_n)), np.zeros((len(batch), max_n))
        for r, i in enumerate(batch):
            bx[r, :n[r]], by[r, :n[r]] = xs[i], ys[i]
        out = stoi_batch(bx, by, n, bool(extended), device)
        for r, i in enumerate(batch):
            res[i] = {'stoi': float(out[r, 0]), 'segments': int(out[r, 1]), 'frames_kept': int(out[r, 2]), 'frames': stoi_frames(n[r])}
    return res[0] if single else res
