"""The conversion scores of include/speechsplit_amd.h restated in float64 numpy, independently of csrc/dtw.hip: cepstra, the DTW recurrence
with its tie order, the backtrack, and the F0 / voicing statistics along a path.  It is the yardstick of tests/test_gpu_dtw.py and is
itself checked by tests/test_dtw_ref_selftest.py (brute force over all monotone paths, symmetry, and the WRONG variants below).

Sums run term by term in the header's order (order='terms'); order='numpy' hands the same sums to numpy's reductions (pairwise / BLAS), and
`two_orders` is the disagreement of the DTW total between the two: the yardstick's own error, from which the GPU tests' bounds come.
`variant` selects one of the WRONG stand-ins; None is the definition."""
import math

import numpy as np

SCALE = 50.0 * math.sqrt(2.0)
UNVOICED = -1e10
WRONG = ('tie_swapped', 'le_for_lt', 'no_diagonal', 'open_end', 'first_row_not_accumulated', 'first_col_not_accumulated',
         'squared_distance', 'scale_under_root', 'norm_tx_plus_ty', 'dct_row0_kept', 'dct_unnormalised', 'voiced_if_either',
         'corr_no_mean', 'cents_ln10')


def dct_basis(n_ceps, n_mels, variant=None):
    """rows 1 .. n_ceps of the orthonormal DCT-II"""
    first = 0 if variant == 'dct_row0_kept' else 1
    d = np.arange(first, first + n_ceps, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    b = np.cos(np.pi * d * (m + 0.5) / n_mels)
    if variant == 'dct_unnormalised':
        return b
    b = math.sqrt(2.0 / n_mels) * b
    if variant == 'dct_row0_kept':
        b[0] /= math.sqrt(2.0)
    return b


def cepstra(mel, dct, order='terms'):
    """mel [T, n_mels] (any float type) x dct [n_ceps, n_mels] -> float64 [T, n_ceps]"""
    x = np.asarray(mel, np.float64)
    if order == 'numpy':
        return x @ dct.T
    acc = np.zeros((x.shape[0], dct.shape[0]))
    for m in range(x.shape[1]):
        acc += x[:, m:m + 1] * dct[None, :, m]
    return acc


def distances(fx, fy, scale, order='terms', variant=None):
    """[Tx, Ty]: scale * sqrt(sum_k (fx[i][k] - fy[j][k])^2)"""
    if order == 'numpy':
        acc = ((fx[:, None, :] - fy[None, :, :]) ** 2).sum(-1)
    else:
        acc = np.zeros((fx.shape[0], fy.shape[0]))
        for k in range(fx.shape[1]):
            df = fx[:, None, k] - fy[None, :, k]
            acc += df * df
    if variant == 'squared_distance':
        return scale * acc
    if variant == 'scale_under_root':
        return np.sqrt(scale * acc)
    return scale * np.sqrt(acc)


def dtw_matrix(d, variant=None):
    """The recurrence on a distance matrix, one anti-diagonal at a time.  Returns (D [Tx, Ty], code [Tx, Ty] with 0 = from (i-1, j-1),
    1 = from (i-1, j), 2 = from (i, j-1), margin [Tx, Ty] = second-best minus best predecessor, inf where there is only one)."""
    Tx, Ty = d.shape
    Dp = np.full((Tx + 1, Ty + 1), np.inf)                        # Dp[i + 1, j + 1] = D[i, j]; row / column 0 are the absent predecessors
    code = np.zeros((Tx, Ty), np.int8)
    margin = np.full((Tx, Ty), np.inf)
    order = (0, 2, 1) if variant == 'tie_swapped' else (0, 1, 2)
    for s in range(Tx + Ty - 1):
        i = np.arange(max(0, s - Ty + 1), min(Tx - 1, s) + 1)
        j = s - i
        cand = [Dp[i, j], Dp[i, j + 1], Dp[i + 1, j]]
        if variant == 'no_diagonal' and s > 0:
            cand[0] = np.where(np.isfinite(cand[1]) | np.isfinite(cand[2]), np.inf, cand[0])
        best = np.full(len(i), np.inf)
        arg = np.full(len(i), order[0], np.int8)
        for n, c in enumerate(order):
            m = (cand[c] <= best) if (variant == 'le_for_lt' and n > 0) else (cand[c] < best)
            best = np.where(m, cand[c], best)
            arg = np.where(m, c, arg).astype(np.int8)
        srt = np.sort(np.stack(cand), axis=0)
        with np.errstate(invalid='ignore'):
            margin[i, j] = np.where(np.isfinite(srt[1]), srt[1] - srt[0], np.inf)
        if s == 0:
            best = np.zeros(1)
        if variant == 'first_row_not_accumulated':
            best = np.where((i == 0) & (j > 0), 0.0, best)
        if variant == 'first_col_not_accumulated':
            best = np.where((j == 0) & (i > 0), 0.0, best)
        Dp[i + 1, j + 1] = d[i, j] + best
        code[i, j] = arg
    return Dp[1:, 1:], code, margin


def backtrack(code, end=None):
    """the path from `end` (default the far corner) to (0, 0), first step to last, int32 [P, 2]"""
    i, j = (code.shape[0] - 1, code.shape[1] - 1) if end is None else end
    steps = [(i, j)]
    while i > 0 or j > 0:
        c = 2 if i == 0 else (1 if j == 0 else int(code[i, j]))
        if c != 2:
            i -= 1
        if c != 1:
            j -= 1
        steps.append((i, j))
    return np.array(steps[::-1], np.int32)


def dtw(fx, fy, scale=SCALE, order='terms', variant=None):
    """-> (total, path int32 [P, 2], mcd)"""
    D, code, _ = dtw_matrix(distances(fx, fy, scale, order, variant), variant)
    end = (D.shape[0] - 1, int(np.argmin(D[-1]))) if variant == 'open_end' else None
    path = backtrack(code, end)
    total = float(D[tuple(path[-1])])
    return total, path, total / ((fx.shape[0] + fy.shape[0]) if variant == 'norm_tx_plus_ty' else len(path))


def path_margin(fx, fy, scale=SCALE):
    """the smallest gap between the best and the second-best predecessor over the cells on the optimal path: what a rounding difference
    in D must stay below for the path to be THE path"""
    D, code, margin = dtw_matrix(distances(fx, fy, scale))
    path = backtrack(code)
    return float(margin[path[:, 0], path[:, 1]].min())


def two_orders(fx, fy, scale=SCALE):
    """|total under numpy's reductions - total term by term| / total"""
    a, b = dtw(fx, fy, scale, 'terms')[0], dtw(fx, fy, scale, 'numpy')[0]
    return abs(a - b) / abs(a) if a else abs(b)


def voiced(v):
    return np.isfinite(v) & (v > -1e9)


def f0_stats(path, f0x, f0y, variant=None):
    """-> (n_vv, n_vu, f0_rmse_cents, f0_corr, vuv_error), sums in path order, one term at a time"""
    lx, ly = np.asarray(f0x, np.float64)[path[:, 0]], np.asarray(f0y, np.float64)[path[:, 1]]
    vx, vy = voiced(lx), voiced(ly)
    both = (vx | vy) if variant == 'voiced_if_either' else (vx & vy)
    n_vv, n_vu = int(both.sum()), int((vx ^ vy).sum())
    sq = sx = sy = 0.0
    for a, b in zip(lx[both], ly[both]):
        sq += (a - b) * (a - b)
        sx += a
        sy += b
    unit = 1200.0 / math.log(10.0 if variant == 'cents_ln10' else 2.0)
    rmse = unit * math.sqrt(sq / n_vv) if n_vv else float('nan')
    corr = float('nan')
    if n_vv >= 2:
        mx, my = (0.0, 0.0) if variant == 'corr_no_mean' else (sx / n_vv, sy / n_vv)
        sxx = syy = sxy = 0.0
        for a, b in zip(lx[both], ly[both]):
            sxx += (a - mx) * (a - mx)
            syy += (b - my) * (b - my)
            sxy += (a - mx) * (b - my)
        if sxx > 0.0 and syy > 0.0:
            corr = sxy / math.sqrt(sxx * syy)
    return n_vv, n_vu, rmse, corr, n_vu / len(path)


def score(mel_x, mel_y, n_ceps=24, f0x=None, f0y=None, variant=None):
    """the whole chain as metrics.mcd_dtw defines it -> dict"""
    dct = dct_basis(n_ceps, np.asarray(mel_x).shape[1], variant)
    total, path, mcd = dtw(cepstra(mel_x, dct), cepstra(mel_y, dct), SCALE, 'terms', variant)
    r = {'mcd_db': mcd, 'total': total, 'path_len': len(path), 'path': path}
    if f0x is not None:
        n_vv, _, rmse, corr, vuv = f0_stats(path, f0x, f0y, variant)
        r.update(f0_rmse_cents=rmse, f0_corr=corr, vuv_error=vuv, n_voiced=n_vv)
    return r


def warped(x, Ty, seed):
    """a time-warped noisy copy of the mel x [Tx, n]: rows of x at Ty sorted uniform indices, plus N(0, 0.01), clipped to [0, 1] and rounded
    through float32"""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.integers(0, x.shape[0], Ty))
    y = np.asarray(x, np.float64)[idx] + rng.normal(0.0, 0.01, (Ty, x.shape[1]))
    return np.clip(y, 0.0, 1.0).astype(np.float32)


def brute_force(d):
    """the cheapest monotone path through a small distance matrix by enumerating all of them -> (total, the set of optimal paths as tuples)"""
    Tx, Ty = d.shape
    best, paths = np.inf, []

    def walk(i, j, cost, steps):
        nonlocal best, paths
        cost = cost + d[i, j]
        steps = steps + ((i, j),)
        if i == Tx - 1 and j == Ty - 1:
            if cost < best:
                best, paths = cost, [steps]
            elif cost == best:
                paths.append(steps)
            return
        if i + 1 < Tx and j + 1 < Ty:
            walk(i + 1, j + 1, cost, steps)
        if i + 1 < Tx:
            walk(i + 1, j, cost, steps)
        if j + 1 < Ty:
            walk(i, j + 1, cost, steps)

    walk(0, 0, 0.0, ())
    return float(best), set(paths)
