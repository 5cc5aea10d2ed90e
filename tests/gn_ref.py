"""float64 references and per-element worst-case rounding budgets for the GroupNorm + ReLU kernels of csrc/elementwise.hip (16 channels per
group, biased variance over 16 x L, eps = 1e-5 inside the square root), plus the input families the tests use.  Plain numpy; no GPU.

Layout: x, y, dy, dx [B, T, C] (the real rows of the haloed slabs), gamma / beta [C], stats [B, C/16, 2] = (mean, rstd), lens [B] or None.

THE BUDGETS.  Worst-case (every rounding at its bound, all with the same sign), first order in u = 2^-24 with the (1 + ..) factors kept
where they are cheap; nothing is fitted.  nit = ceil(L / 16) is the number of rows a thread owns.  Per group: n = 16 L elements,
A = mean |x|, m, var, rstd = (var + eps)^-1/2 the float64 statistics.

 forward, register kernel (gn_relu_fwd_kernel, gn_relu_gather_kernel; T <= 256)
   dm    = (nit + 5) u A          mean.  A thread adds nit quads (a+b)+(c+d) in a chain: an element passes at most 2 + nit additions; the 64
                                  partials meet in float64 (nothing); float(sum): 1; inv_n = 1 / (16 L), 16 L exact: 1; the product: 1.
   theta = (4 nit + 6) u          relative error of the computed sum of squares AROUND THE COMPUTED MEAN: (x - mean) rounded once and squared:
                                  2; a chain of 4 nit fused multiply-adds: 4 nit; float(sum), inv_n, the product: 3; one of slack for the
                                  float64 sum and second-order terms.  The sum around the computed mean is n (var + (m - mean)^2) exactly.
   kappa = (theta var + (1 + theta) dm^2) / (var + eps)      relative error of (var + eps)
   rho   = kappa / (2 (1 - kappa)) + 3 u                     relative error of rstd: (1 + k)^-1/2 <= 1 + k / (2 (1 - k)); the addition of eps
                                  (half of u after the root), sqrtf and the division, both correctly rounded (the library is built so): 2.5 u.
   E     = (1 + rho) (1 + u)^2 - 1                           gn_h = (x - mean) * rstd: two more roundings
   dh    = dm rstd (1 + E) + |h| E
   dz    = (|gamma| dh + u |z|) (1 + u)                      gn_z is ONE fused multiply-add.  ReLU is 1-Lipschitz: dz judges y, and it is
                                  the kink bound: the kernel's branch may differ from the float64 sign only where |z| <= dz.
 forward, chunked kernels (T > 256): the sums are float64, so the nit terms drop.
   dm    = 3 u |m| + n 2^-53 A    float(sum), inv_n, product; the float64 sum of n terms
   theta = 6 u                    (x - mean) rounded and squared: 2; float(sum), inv_n, product: 3; one of slack (float64 sum, second order)
 backward (gn_relu_bwd_kernel), against the float64 backward UNDER THE KERNEL'S MASK, with g = mask dy gamma, M1 = mean g, M2 = mean g h,
 dx = rstd (g - M1 - h M2).  The kernel recomputes h from x and the forward's stats, so its h carries dh and its rstd carries rho.
   e     = bound on the error of the incoming dy (0: dy is an input; the scatter form: (k + 2) u sum |w src| for k fused terms)
   dg    = u |g| + |gamma| e                                 dz * gamma rounded
   dM1   = (4 nit + 5) u mean|g| + mean(|gamma| e)           chain of 4 nit additions, the rounding of g, float / inv_n / product, one slack
   dM2   = (4 nit + 6) u mean(|g| (|h| + dh)) + mean(|g| dh + |gamma| e (|h| + dh))      the same with the product rounded, plus dh
   inner = dg + dM1 + dh |M2| + (|h| + dh) dM2 + 3 u (|g| + |M1| + (|h| + dh) (|M2| + dM2))      three roundings of the bracket
   ddx   = rstd (1 + rho + u) inner + |dx| (rho + u)
 column sums d_gamma, d_beta, d_bias (fp32): a thread chain of nit terms, 16 row groups added in a chain, the B utterances added onto the
 accumulator a0 (atomics in any order, or B + 1 ordered additions in deterministic mode):
   dcol  = (nit + 16 + p) u S + P + (B + 1) u (|a0| + S)     S = sum of the |terms| as the kernel has them, p = 1 if a term is a rounded
                                  product (d_gamma), P = sum of the terms' own error bounds (|dz| dh for d_gamma, ddx for d_bias)."""
import numpy as np

U = 2.0 ** -24
EPS = 1e-5
F32 = np.float32
T_LIST = (1, 2, 15, 16, 17, 128, 129, 192, 193, 255, 256)
FAMILIES = ('benign', 'offset100', 'offset1000', 'constant', 'constant_beta0', 'tiny_variance', 'outlier', 'mixed')
CONST = F32(3.7)


def make_case(family, B, T, C, seed):
    """(x [B,T,C], gamma [C], beta [C]) float32 of one input family, from a seeded numpy generator.  Families apply per group of 16 channels."""
    rng = np.random.default_rng([seed, B, T, C, FAMILIES.index(family)])
    n = rng.standard_normal((B, T, C))
    gamma = 1.0 + 0.3 * rng.standard_normal(C)
    beta = 0.2 * rng.standard_normal(C)
    x = n.copy()
    if family == 'offset100':
        x = 100.0 + n
    elif family == 'offset1000':
        x = 1000.0 + n
    elif family in ('constant', 'constant_beta0'):
        x[:, :, 16:32] = CONST                              # group 1 is constant: var = 0, h = 0, y = relu(beta), rstd = 1 / sqrt(eps)
        if family == 'constant_beta0':
            beta[16:32] = 0.0                               # z = 0 exactly wherever the computed mean is exact: the branch is "not taken"
    elif family == 'tiny_variance':
        x = 5.0 + np.sqrt(1e-5) * n
    elif family == 'outlier':
        x[:, T // 2, 5] = 1e4                               # |h| approaches sqrt(16 T), the bound act_scales relies on
    elif family == 'mixed':
        g = (np.arange(C) // 16) % 4                        # the four groups of a 64-channel block: means 10 g, scales 2^(2g - 2)
        x = 10.0 * g + n * 2.0 ** (2 * g - 2)
    else:
        assert family == 'benign'
    return x.astype(F32), gamma.astype(F32), beta.astype(F32)


def _groups(a, L=None):
    """[B,T,C] -> [B, L or T, C/16, 16]"""
    B, T, C = a.shape
    return a[:, :T if L is None else L].reshape(B, -1, C // 16, 16)


def _lens(lens, B, T):
    return np.full(B, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)


def stats(x, lens=None):
    """float64 (mean, var, A = mean|x|) per (b, group) over the row's own frames; NaN for a row of no frames."""
    x = np.asarray(x, np.float64)
    B, T, C = x.shape
    m, v, a = (np.full((B, C // 16), np.nan) for _ in range(3))
    for b, L in enumerate(_lens(lens, B, T)):
        if L:
            g = _groups(x[b:b + 1], L)[0]                   # [L, G, 16]
            m[b] = g.mean(axis=(0, 2))
            v[b] = ((g - m[b][None, :, None]) ** 2).mean(axis=(0, 2))
            a[b] = np.abs(g).mean(axis=(0, 2))
    return m, v, a


def _per_channel(s):
    return np.repeat(s, 16, axis=1)[:, None, :]             # [B, G] -> [B, 1, C]


def forward(x, gamma, beta, lens=None):
    """float64 forward -> dict(h, z, y, mean, var, rstd, A); rows t >= lens[b] have h = z = y = 0."""
    x = np.asarray(x, np.float64)
    B, T, C = x.shape
    m, v, a = stats(x, lens)
    rstd = 1.0 / np.sqrt(v + EPS)
    live = (np.arange(T)[None, :] < _lens(lens, B, T)[:, None])[:, :, None]
    with np.errstate(invalid='ignore'):
        h = np.where(live, (np.where(live, x, 0.0) - _per_channel(m)) * _per_channel(rstd), 0.0)
    z = np.where(live, h * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64), 0.0)
    return dict(h=h, z=z, y=np.maximum(z, 0.0), mean=m, var=v, rstd=rstd, A=a, live=live)


def forward_budget(x, gamma, beta, lens=None, long_path=False):
    """dict(dm [B,G], rho [B,G], dh, dz [B,T,C]) -- the docstring's forward budget around forward(x, ...)."""
    f = forward(x, gamma, beta, lens)
    B, T, C = f['h'].shape
    L = _lens(lens, B, T)[:, None].astype(np.float64)
    nit = np.ceil(L / 16.0)
    var, A, m = f['var'], f['A'], f['mean']
    if long_path:
        dm = 3 * U * np.abs(m) + 16 * L * 2.0 ** -53 * A
        theta = 6 * U
    else:
        dm = (nit + 5) * U * A
        theta = (4 * nit + 6) * U
    kappa = (theta * var + (1 + theta) * dm ** 2) / (var + EPS)
    with np.errstate(invalid='ignore', divide='ignore'):    # (a row of no frames has NaN statistics: its budget is masked out below)
        rho = np.where(kappa < 1, kappa / (2 * (1 - kappa)), np.inf) + 3 * U
        E = (1 + rho) * (1 + U) ** 2 - 1
        dh = _per_channel(dm * f['rstd'] * (1 + E)) + np.abs(f['h']) * _per_channel(E)
    dz = (np.abs(np.asarray(gamma, np.float64)) * dh + U * np.abs(f['z'])) * (1 + U)
    dh, dz = np.where(f['live'], dh, 0.0), np.where(f['live'], dz, 0.0)
    return dict(f, dm=dm, rho=rho, dh=dh, dz=dz, nit=nit)


def gather(y, i0, lam, nrows):
    """oracle/interp_np.interp_apply's semantics in float64 with float32 weights: row r < nrows[b] = (1 - lam) y[i0] + lam y[i0 + 1]
    (row T reads as zeros), rows past nrows zero.  (1 - lam) is the float32 difference, as the kernels take it."""
    y = np.asarray(y, np.float64)
    B, T, C = y.shape
    P = i0.shape[1]
    yp = np.concatenate([y, np.zeros((B, 1, C))], 1)
    out = np.zeros((B, P, C))
    for b in range(B):
        n = int(nrows[b])
        l = np.asarray(lam[b, :n], F32)
        ol = (F32(1) - l).astype(np.float64)[:, None]
        out[b, :n] = ol * yp[b, i0[b, :n]] + l.astype(np.float64)[:, None] * yp[b, i0[b, :n] + 1]
    return out


def scatter_adjoint(src, i0, lam, nrows, T):
    """dy[t] = sum_{i0[r] == t} (1 - lam[r]) src[r] + sum_{i0[r] == t - 1} lam[r] src[r] over r < nrows, float64 (weights as in gather);
    also the budget of the kernel's fused-multiply-add chain: (k + 2) u sum |w src| with k the number of terms of the element."""
    src = np.asarray(src, np.float64)
    B, P, C = src.shape
    dy, ab, k = np.zeros((B, T + 1, C)), np.zeros((B, T + 1, C)), np.zeros((B, T + 1, 1))
    for b in range(B):
        for r in range(int(nrows[b])):
            l = F32(lam[b, r])
            w0, w1, i = float(F32(1) - l), float(l), int(i0[b, r])
            dy[b, i] += w0 * src[b, r]
            dy[b, i + 1] += w1 * src[b, r]
            ab[b, i] += abs(w0) * np.abs(src[b, r])
            ab[b, i + 1] += abs(w1) * np.abs(src[b, r])
            k[b, i] += 1
            k[b, i + 1] += 1
    return dy[:, :T], ((k + 2) * U * ab)[:, :T]


def _gmean(a):
    """[B,T,C] -> per-(b, group) mean over (T, 16), broadcast back to [B,1,C]"""
    B, T, C = a.shape
    return _per_channel(a.reshape(B, T, C // 16, 16).mean(axis=(1, 3)))


def backward(x, dy, gamma, beta, mask):
    """float64 backward for a given ReLU mask [B,T,C] (bool) -> dict(dx [B,T,C], dgamma, dbeta, dbias [C], g, h, M1, M2)."""
    f = forward(x, gamma, beta)
    ga = np.asarray(gamma, np.float64)
    dz = np.where(mask, np.asarray(dy, np.float64), 0.0)
    g = dz * ga
    M1, M2 = _gmean(g), _gmean(g * f['h'])
    dx = _per_channel(f['rstd']) * (g - M1 - f['h'] * M2)
    return dict(dx=dx, dgamma=(dz * f['h']).sum((0, 1)), dbeta=dz.sum((0, 1)), dbias=dx.sum((0, 1)), g=g, h=f['h'], M1=M1, M2=M2, dz=dz)


def backward_budget(x, dy, gamma, beta, mask, acc0=(0.0, 0.0, 0.0), dy_err=None):
    """The docstring's backward budgets around backward(...): dict(ddx [B,T,C], dgamma, dbeta, dbias [C]).  acc0: the values (numbers or
    [C]) the three accumulators held before; dy_err: per-element bound on the error of the incoming dy (scatter form)."""
    fb = forward_budget(x, gamma, beta)
    r = backward(x, dy, gamma, beta, mask)
    B, T, C = r['dx'].shape
    nit = float(np.ceil(T / 16.0))
    ga = np.abs(np.asarray(gamma, np.float64))
    e = np.zeros_like(r['dx']) if dy_err is None else np.where(mask, dy_err, 0.0)
    g, h, dh = np.abs(r['g']), np.abs(r['h']), fb['dh']
    rho, rstd = _per_channel(fb['rho']), _per_channel(fb['rstd'])
    dg = U * g + ga * e
    dM1 = (4 * nit + 5) * U * _gmean(g) + _gmean(ga * e)
    dM2 = (4 * nit + 6) * U * _gmean(g * (h + dh)) + _gmean(g * dh + ga * e * (h + dh))
    aM1, aM2 = np.abs(r['M1']), np.abs(r['M2'])
    inner = dg + dM1 + dh * aM2 + (h + dh) * dM2 + 3 * U * (g + aM1 + (h + dh) * (aM2 + dM2))
    ddx = rstd * (1 + rho + U) * inner + np.abs(r['dx']) * (rho + U)
    a0 = [np.abs(np.broadcast_to(np.asarray(a, np.float64), (C,))) for a in acc0]
    adz = np.abs(r['dz']) + e

    def col(S, P, p, a):
        S, P = S.sum((0, 1)), P.sum((0, 1))
        return (nit + 16 + p) * U * S + P + (B + 1) * U * (a + S)
    return dict(ddx=ddx, dgamma=col(adz * (h + dh), adz * dh + e * h, 1, a0[0]), dbeta=col(adz, e, 0, a0[1]),
                dbias=col(np.abs(r['dx']) + ddx, ddx, 0, a0[2]), fwd=fb, ref=r)


def mask_violations(mask, z_ref, dz, h_exact_zero=None, beta=None):
    """The kink rule: the branch taken (mask, bool) may differ from z_ref > 0 only where |z_ref| <= dz.  And where the kernel's own h is
    exactly zero (h_exact_zero, bool [B,T,C]: the computed mean equals x bit for bit) z is beta exactly: the branch is beta > 0 -- z = 0 is
    "not taken".  Returns the number of violating elements."""
    bad = (mask != (z_ref > 0)) & (np.abs(z_ref) > dz)
    if h_exact_zero is not None:
        bad |= h_exact_zero & (mask != (np.asarray(beta, np.float64)[None, None, :] > 0))
    return int(bad.sum())


def ratio(err, budget):
    """worst |err| / budget; 0 / 0 counts as 0, anything over a zero budget as inf"""
    err, budget = np.abs(np.asarray(err, np.float64)), np.asarray(budget, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, 0.0, err / budget)
    q = np.where(np.isnan(np.asarray(err)), np.inf, q)
    return float(q.max()) if q.size else 0.0


def bf16_rne(a):
    """float32 -> the bfloat16 bit patterns (uint16) of round-to-nearest-even, as v_cvt_pk_bf16_f32 rounds finite values"""
    b = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
