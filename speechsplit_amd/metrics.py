"""Scores of a conversion on the GPU (csrc/dtw.hip through the C ABI): the mel-cepstral distortion between two mel spectrograms of
different lengths along a dynamic-time-warping path, and the F0 and voicing error along the same path.

The definitions are the header's (include/speechsplit_amd.h, "conversion scores"): cepstra are rows 1 .. n_ceps of the orthonormal DCT-II of
the mel bands (row 0, the level, is left out); the frame distance is 50 sqrt(2) times the Euclidean distance of the cepstra -- this project's
mels are S = (dB + 100) / 100, so ln|A| = (100 S - 84) ln 10 / 20 and the usual (10 / ln 10) sqrt(2 sum dc^2) in dB becomes that scale on
the cepstra of S; DTW takes steps (1,1), (1,0), (0,1) of weight 1 with both ends fixed, the diagonal winning a tie, then (i-1, j), with no
band and no slope constraint; mcd_db is the path's total cost over its length.  F0 tracks are features.pitch_track's: ln Hz, -1e10 for
unvoiced frames.  float64 throughout; the same bits on every run, whatever the batching.  No engine needed."""
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
