"""float64 references, worst-case rounding budgets, fp32 operation-order emulations and the input families for the kernels that stand between
the heavy families of a training step: mse_loss / ce_loss / finish_loss and the column sums (csrc/elementwise.hip), the decoder-input kernels
(build_dec_in[_compact], dec_in_grad[_compact]) and spk_grad (csrc/input_grads.hip).  Plain numpy (torch only to measure K); no GPU.

THE BUDGETS.  Worst case, first order in u = 2^-24 (the unit roundoff of fp32), every term written out; nothing is fitted to a kernel.

 MSE  (mse_kernel: grid (8, B), 256 threads, element i of utterance b in thread i % 2048, trips i / 2048; finish_loss_kernel in float64)
   d_out   4 u |ref| + 2^-126          ref = (o - y) * 2 / n * grad_scale in float64.  Four roundings: the subtraction, float(2 / n), the
                                       multiply by grad_scale, the final product.  2^-126: a result below the smallest normal.
   loss    (k + 8 + 3) u |ref| + (k + 8 + 3) 2^-126,   k = ceil(T C / 2048)
                                       every term e * e is non-negative, so relative errors add.  k: the per-thread chain s += e * e; 8: the
                                       256-wide tree; 3: the product e * e, float(1 / n) and the final cast (the float64 sum of 8 B partials
                                       costs 2^-53).  Counted strictly the chain is k - 1 (the first addition onto 0 is exact) and the rounded
                                       subtraction, squared, adds 2: k + 12 in all; the bound kept here is the tighter k + 11.  The absolute
                                       floor: e * e and every partial sum below 2^-126 may be rounded to the subnormal grid or flushed.
 CE   (ce_kernel: one wavefront per row, lane l owns classes l, l + 64, ..; butterfly reductions; finish_loss_kernel in float64)
   with mx = max_c x_c, se = sum_c exp(x_c - mx), p_c = exp(x_c - mx) / se (float64), gs = float(1 / (B T)) * grad_scale as the launcher
   rounds it, and the per-element unit  w_c = 1 + |x_c - mx| + |log se|:
   d_out   gs (K u w_c p_c + (ceil(C / 64) + 6) u p_c + u |p_c - 1{c = y}|)
                                       K u w_c: the log-softmax value (x_c - mx) - log se as fp32 computes it -- the two roundings of the
                                       differences (u |x_c - mx|, u |.|), logf (a few ulp of |log se|) and expf (a few ulp, relative: the 1);
                                       ceil(C / 64) + 6: the relative error of se (lane chain, six butterfly levels) which moves every p_c;
                                       the last term: the rounding of p_c - 1{c = y}.  Where p_c == 0 (a logit of -inf) the budget is 0.
   row loss  K u (1 + |log se|) + (ceil(C / 64) + 6) u + u |x_y - mx| + u |loss_row|
   loss    mean(row loss budgets) + 2 u |loss|        float(1 / n) and the final cast; the sum of the rows is float64.
   NOTHING here scales with |mx| alone: shifting a row by a constant leaves the budget where it was.  The kernel's former order
   (lse = mx + logf(se), then expf(x_c - lse)) rounds lse to ulp(|mx|) / 2 and carries that into every exponent: at |mx| = 1000 a relative
   error of 3e-5 in every p_c, hundreds of budgets.
   K cannot be derived: it is the accuracy of the device's expf / logf.  It is NOT taken from the kernel under test: K = 4 * K_MEASURED,
   K_MEASURED = the worst error of float32 torch.log_softmax on the CPU against float64 over ce_cases(), in units of u w_c (measure_k());
   device transcendentals are specified to a few ulp where the CPU's are within one.
 COLUMN SUMS  (colsum_kernel: float64 throughout, one rounding to fp32, one fp32 addition onto the output)
   ref = float32(float32(sum64) + out0);  budget  u (|sum| + |sum + out0|) + R 2^-53 sum |v|
 DECODER INPUT  forward: pure indexing, exact.  Gradient: an ascending fp32 chain of f terms -- bit-equal to dec_in_grad_chain(), and within
   (f - 1) u sum |terms| of float64.  The compact form copies: exact.
 SPEAKER GRADIENT  (spk_grad_kernel)  (rows + per + parts + 3) u sum |terms|,  terms = dg[b][r][g] W[g][col0 + j];
   parts = floor(1024 / E), per = ceil(2 H4 / parts): rows - 1 additions of the time chain, per fused multiply-adds, parts additions of the
   slices, and 3 of slack for the products' own rounding carried through."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
F32 = np.float32
K_MEASURED = 1.74       # measure_k() over ce_cases() on the CPU gives 1.7383 (the 'equal' family: the result's own rounding plus logf's); rounded up
K = 4 * K_MEASURED


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ MSE
MSE_SHAPES = ((1, 1, 80), (3, 8, 80), (1, 26, 80), (2, 256, 80))
MSE_FAMILIES = ('normal', 'equal', 'mag1e3', 'mag1e-20')
GRAD_SCALES = (1.0, 0.25, 1.0 / 3.0)


def mse_case(family, B, T, C, seed=0):
    rng = np.random.default_rng([seed, B, T, C, MSE_FAMILIES.index(family)])
    o, y = rng.standard_normal((B, T, C)), rng.standard_normal((B, T, C))
    if family == 'equal':
        y = o
    elif family == 'mag1e3':
        o, y = 1e3 * o, 1e3 * y
    elif family == 'mag1e-20':
        o, y = 1e-20 * o, 1e-20 * y
    return o.astype(F32), y.astype(F32)


def mse_ref(o, y, grad_scale):
    """(loss, d_out) in float64; grad_scale is taken as the float32 value the kernel is handed."""
    e = o.astype(np.float64) - y.astype(np.float64)
    return float(np.mean(e * e)), e * (2.0 / e.size) * float(F32(grad_scale))


def mse_budget(o, y, grad_scale):
    loss, d = mse_ref(o, y, grad_scale)
    k = cdiv(o.shape[1] * o.shape[2], 2048) + 8 + 3
    return k * U * abs(loss) + k * TINY, 4 * U * np.abs(d) + TINY


def block_tree(v):
    """the 256-wide halving tree of mse_kernel over the last axis (fp32)"""
    v = v.astype(F32)
    w = 128
    while w:
        v = (v[..., :w] + v[..., w:2 * w]).astype(F32)
        w //= 2
    return v[..., 0]


def mse_emulate(o, y, grad_scale, drop_two_over_n=False):
    """mse_kernel + finish_loss_kernel in their own fp32 operation order."""
    B, T, C = o.shape
    n = T * C
    e = (o.reshape(B, n) - y.reshape(B, n)).astype(F32)
    gs = F32(F32(1.0 if drop_two_over_n else 2.0 / (B * n)) * F32(grad_scale))
    d = (e * gs).astype(F32)
    k = cdiv(n, 2048)
    sq = np.zeros((B, k * 2048), F32)
    sq[:, :n] = (e * e).astype(F32)
    chain = np.add.accumulate(sq.reshape(B, k, 8, 256), axis=1, dtype=F32)[:, -1]          # [B, 8, 256]: trips in order
    part = block_tree(chain)                                                               # [B, 8]
    loss = F32(part.astype(np.float64).sum() * float(F32(1.0 / (B * n))))
    return float(loss), d.reshape(B, T, C)


# ------------------------------------------------------------------------------------------------ CE
CE_CLASSES = (2, 63, 64, 65, 257)
CE_BT = ((1, 1), (3, 8))
CE_FAMILIES = ('normal', 'equal', 'target_dominant', 'other_dominant', 'offset+1000', 'offset-1000', 'neg_inf')


def ce_case(family, B, T, C, seed=0):
    """(logits [B,T,C] f32, targets [B,T] i32).  Targets include class 0 and class C - 1.  The offset families are the 'normal' draw of the
    same shape, shifted: ce_case('normal') is their unshifted case."""
    fam = 'normal' if family.startswith('offset') else family
    rng = np.random.default_rng([seed, B, T, C, CE_FAMILIES.index(fam)])
    x = rng.standard_normal((B, T, C))
    y = rng.integers(0, C, size=(B, T))
    y.reshape(-1)[0] = 0
    y.reshape(-1)[-1] = C - 1
    rows = np.arange(B * T)
    if family == 'equal':
        x[:] = 0.75
    elif family == 'target_dominant':
        x.reshape(B * T, C)[rows, y.reshape(-1)] += 60.0
    elif family == 'other_dominant':
        x.reshape(B * T, C)[rows, (y.reshape(-1) + 1) % C] += 60.0
    elif family == 'offset+1000':
        x = 1000.0 + x
    elif family == 'offset-1000':
        x = -1000.0 + x
    elif family == 'neg_inf':                 # some non-target classes, never the target, never the whole row
        hit = rng.random((B, T, C)) < 0.3
        hit.reshape(B * T, C)[rows, y.reshape(-1)] = False
        x[hit] = -np.inf
    return x.astype(F32), y.astype(np.int32)


def ce_cases():
    for C in CE_CLASSES:
        for B, T in CE_BT:
            for fam in CE_FAMILIES:
                yield fam, B, T, C


def ce_gs(B, T, grad_scale):
    """the factor the launcher hands the kernel: float(1 / n) * grad_scale, in fp32"""
    return float(F32(F32(1.0 / (B * T)) * F32(grad_scale)))


def _logsoftmax64(x):
    x = x.astype(np.float64)
    mx = x.max(axis=-1, keepdims=True)
    with np.errstate(divide='ignore'):
        lse = np.log(np.exp(x - mx).sum(axis=-1, keepdims=True))
    return x - mx, lse


def ce_ref(x, y, grad_scale):
    """(loss, row losses [B,T], d_out [B,T,C]) in float64 (log-softmax)."""
    B, T, C = x.shape
    a, lse = _logsoftmax64(x)
    ls = a - lse
    onehot = np.eye(C)[y]
    rowloss = -np.take_along_axis(ls, y[..., None].astype(np.int64), -1)[..., 0]
    return float(rowloss.mean()), rowloss, (np.exp(ls) - onehot) * ce_gs(B, T, grad_scale)


def ce_units(x):
    """w_c = 1 + |x_c - mx| + |log se| (inf where the logit is -inf)"""
    a, lse = _logsoftmax64(x)
    return 1.0 + np.abs(a) + np.abs(lse)


def ce_budget(x, y, grad_scale, k=K):
    """(loss budget, row-loss budgets, d_out budgets)"""
    B, T, C = x.shape
    a, lse = _logsoftmax64(x)
    p = np.exp(a - lse)
    onehot = np.eye(C)[y]
    w = 1.0 + np.abs(a) + np.abs(lse)
    red = cdiv(C, 64) + 6
    with np.errstate(invalid='ignore'):
        core = np.where(p == 0.0, 0.0, k * U * w * p + red * U * p)
    bd = ce_gs(B, T, grad_scale) * (core + np.where(p == 0.0, 0.0, U * np.abs(p - onehot)))
    ay = np.take_along_axis(a, y[..., None].astype(np.int64), -1)[..., 0]
    rowloss = lse[..., 0] - ay
    brow = k * U * (1.0 + np.abs(lse[..., 0])) + red * U + U * np.abs(ay) + U * np.abs(rowloss)
    return float(brow.mean() + 2 * U * abs(rowloss.mean())), brow, bd


def measure_k():
    """The worst error of float32 torch.log_softmax on the CPU against float64 over ce_cases(), in units of u w_c."""
    import torch
    worst = 0.0
    for fam, B, T, C in ce_cases():
        x, _ = ce_case(fam, B, T, C)
        a, lse = _logsoftmax64(x)
        got = torch.log_softmax(torch.from_numpy(x), dim=-1).double().numpy()
        fin = np.isfinite(a)
        err = np.abs(got[fin] - (a - lse)[fin]) / (U * ce_units(x)[fin])
        worst = max(worst, float(err.max()))
    return worst


def _butterfly(v, op):
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lane ^ o])
    return v[:, 0]


def ce_emulate(x, y, grad_scale, order='fixed', mean_over_btc=False):
    """ce_kernel + finish_loss_kernel in their own fp32 operation order, numpy's float32 exp / log standing in for expf / logf.  order 'fixed':
    (x - mx) - logf(se); 'lse': the former mx + logf(se) order.  Returns (loss, row losses, d_out)."""
    B, T, C = x.shape
    R = B * T
    xr = x.reshape(R, C).astype(F32)
    k = cdiv(C, 64)
    pad = np.full((R, k * 64), -np.inf, F32)
    pad[:, :C] = xr
    lanes = pad.reshape(R, k, 64)
    mx = _butterfly(np.maximum.reduce(lanes, axis=1), np.maximum)
    ex = np.exp((lanes - mx[:, None, None]).astype(F32)).astype(F32)
    se = _butterfly(np.add.accumulate(ex, axis=1, dtype=F32)[:, -1], lambda a, b: (a + b).astype(F32))
    n = R * C if mean_over_btc else R
    gs = F32(F32(1.0 / n) * F32(grad_scale))
    onehot = np.eye(C, dtype=F32)[y.reshape(R)]
    xy = xr[np.arange(R), y.reshape(R)]
    lg = np.log(se).astype(F32)
    if order == 'fixed':
        pr = np.exp(((xr - mx[:, None]).astype(F32) - lg[:, None]).astype(F32)).astype(F32)
        row = (lg - (xy - mx).astype(F32)).astype(F32)
    else:
        lse = (mx + lg).astype(F32)
        pr = np.exp((xr - lse[:, None]).astype(F32)).astype(F32)
        row = (lse - xy).astype(F32)
    d = ((pr - onehot).astype(F32) * gs).astype(F32)
    loss = F32(row.astype(np.float64).sum() * float(F32(1.0 / n)))
    return float(loss), row.reshape(B, T), d.reshape(B, T, C)


# ------------------------------------------------------------------------------------------------ column sums
COLSUM_R = (1, 4, 15, 16, 17, 33, 520)


def colsum_scratch_doubles(cols):
    nb = cdiv(cols, 64)
    return (cdiv(1024, nb) + 1) * nb * 64


def colsum_chunks(R, cols, scratch=True):
    """(chunks, rows per chunk) as colsum_launch picks them"""
    chunks = cdiv(1024, cdiv(cols, 64)) if scratch else 1
    chunks = max(1, min(chunks, cdiv(R, 16)))
    rpc = cdiv(R, chunks)
    return cdiv(R, rpc), rpc


def colsum_case(family, R, cols, seed=0):
    rng = np.random.default_rng([seed, R, cols, 0 if family == 'normal' else 1])
    v = rng.standard_normal((R, cols))
    if family == 'cancelling':                # +-1e4 pairs plus N(0, 1e-3): the sum is the small part
        big = 1e4 * (1.0 + rng.random((cdiv(R, 2), cols)))
        pairs = np.concatenate([big, -big])[:2 * (R // 2)]
        v = 1e-3 * v
        v[:2 * (R // 2)] += pairs[rng.permutation(2 * (R // 2))]
    return v.astype(F32)


def colsum_ref(v, out0):
    """(float32 result, budget) per column: float32(float32(sum64) + out0)"""
    s = v.astype(np.float64).sum(axis=0)
    o = out0.astype(np.float64)
    ref = (s.astype(F32) + out0.astype(F32)).astype(F32)
    return ref, U * (np.abs(s) + np.abs(s + o)) + v.shape[0] * 2.0 ** -53 * np.abs(v.astype(np.float64)).sum(axis=0)


def colsum_emulate(v, out0, scratch=True, skip_last_chunk=False, fp32_order=None):
    """colsum_kernel's order: per chunk four row lanes in float64, lanes in order, chunks by lane k % 4 in order, lanes in order; one cast, one
    fp32 addition.  Mutants: skip_last_chunk drops the last (short) chunk; fp32_order (a permutation of the chunks) adds fp32 chunk sums in
    that order, as arrival-order fp32 atomics would."""
    R, cols = v.shape
    chunks, rpc = colsum_chunks(R, cols, scratch)
    v64 = v.astype(np.float64)
    parts = []
    for ch in range(chunks):
        blk = v64[ch * rpc:min(R, (ch + 1) * rpc)]
        lanes = [blk[rl::4].sum(axis=0) if blk[rl::4].size else np.zeros(cols) for rl in range(4)]
        parts.append(((lanes[0] + lanes[1]) + lanes[2]) + lanes[3])
    if skip_last_chunk and chunks > 1:
        parts = parts[:-1]
    if fp32_order is not None:
        acc = out0.astype(F32)
        for ch in fp32_order:
            acc = (acc + parts[ch].astype(F32)).astype(F32)
        return acc
    if len(parts) == 1:
        tot = parts[0]
    else:
        lanes = [sum(parts[rl::4], np.zeros(cols)) for rl in range(4)]
        tot = ((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]
    return (tot.astype(F32) + out0.astype(F32)).astype(F32)


# ------------------------------------------------------------------------------------------------ decoder input
HALO = 2
# (H, freq) per source; emb_dim; zero padding columns behind the speaker columns (4: ld % 4 == 0, dec_in_from_codes moves float4s; 5: it cannot).
# 'compact' and 'single' have one freq and admit the compact form.
DEC_SETS = {
    'compact': (((8, 8), (1, 8), (32, 8)), 82, 4),
    'mixed': (((8, 8), (3, 1), (32, 4)), 82, 5),
    'single': (((8, 8),), 0, 4),
}
DEC_T = (8, 16, 64)
DEC_B = (1, 3)


def small_lstm_ld(H):
    return 2 * H if H > 32 or H & (H - 1) == 0 else (2 * H + 3) // 4 * 4


def dec_layout(name):
    """([(H, freq, col, ld_i)], emb_dim, emb_col, ld): sources side by side, then the speaker columns, then the zero padding columns"""
    srcs, E, pad = DEC_SETS[name]
    out, col = [], 0
    for H, f in srcs:
        out.append((H, f, col, small_lstm_ld(H)))
        col += 2 * H
    return out, E, col, col + E + pad


def dec_in_ref(slabs, layout, emb, B, T, f=0, same_frame=False):
    """The index reference.  slabs[i] [B, T+4, 2H_i] (haloed).  Returns the real rows [B, T, ld] (f == 0) or the compact [B, T/f, ld].
    same_frame (a mutant): both halves sampled at the block's first frame."""
    srcs, E, emb_col, ld = layout
    rows = np.arange(0, T, f) if f else np.arange(T)
    out = np.zeros((B, len(rows), ld), F32)
    for (H, fr, col, _), o in zip(srcs, slabs):
        blk = rows // fr
        last = blk * fr if same_frame else blk * fr + fr - 1
        out[:, :, col:col + H] = o[:, last + HALO, :H]
        out[:, :, col + H:col + 2 * H] = o[:, blk * fr + HALO, H:2 * H]
    if E:
        out[:, :, emb_col:emb_col + E] = emb[:, None, :]
    return out


def dec_in_grad_chain(d_in, layout, B, T, frames=None):
    """dec_in_grad_kernel's own order: per source the real rows [B, T, 2H] of d_o -- zero at the unsampled frames, the ascending fp32 chain over
    the block's f frames at the sampled one.  d_in [B, T, ld] real rows.  frames (a mutant): sum that many frames instead of f.
    Returns [(chain result f32, float64 sum, sum |terms|)] per source."""
    srcs = layout[0]
    res = []
    for H, fr, col, _ in srcs:
        nb = T // fr
        blk = d_in[:, :, col:col + 2 * H].reshape(B, nb, fr, 2 * H)
        use = blk[:, :, :fr if frames is None else frames]
        chain = np.add.accumulate(use.astype(F32), axis=2, dtype=F32)[:, :, -1] if use.shape[2] else np.zeros((B, nb, 2 * H), F32)
        s64, sabs = blk.astype(np.float64).sum(axis=2), np.abs(blk.astype(np.float64)).sum(axis=2)
        g, r64, ra = np.zeros((B, T, 2 * H), F32), np.zeros((B, T, 2 * H)), np.zeros((B, T, 2 * H))
        for dst, src in ((g, chain), (r64, s64), (ra, sabs)):
            dst[:, fr - 1::fr, :H] = src[:, :, :H]              # forward half: the block's last frame
            dst[:, 0::fr, H:] = src[:, :, H:]                   # backward half: its first
        res.append((g, r64, ra))
    return res


# ------------------------------------------------------------------------------------------------ speaker gradient
SPK_E = (1, 81, 256, 513, 1024)
SPK_H4 = (4, 2048)
SPK_ROWS = (1, 12, 260)
SPK_THREADS = 1024


def spk_split(H4, E):
    parts = SPK_THREADS // E
    return parts, cdiv(2 * H4, parts)


def spk_ref(dg, w_f, w_r, col0, E):
    """(float64 result [B, E], budget [B, E]).  dg [B, rows, 2 H4], w_f / w_r [H4, >= col0 + E]."""
    B, rows, G = dg.shape
    H4 = G // 2
    W = np.concatenate([w_f, w_r])[:, col0:col0 + E].astype(np.float64)
    d = dg.astype(np.float64)
    ref = d.sum(axis=1) @ W
    parts, per = spk_split(H4, E)
    return ref, (rows + per + parts + 3) * U * (np.abs(d).sum(axis=1) @ np.abs(W))


def spk_emulate(dg, w_f, w_r, col0, E, drop_last_slice=False):
    """spk_grad_kernel's own order: the fp32 time chain, `parts` slices of `per` fused multiply-adds, the slices added in order."""
    B, rows, G = dg.shape
    H4 = G // 2
    W = np.concatenate([w_f, w_r])[:, col0:col0 + E].astype(np.float64)
    S = np.add.accumulate(dg.astype(F32), axis=1, dtype=F32)[:, -1].astype(np.float64)          # [B, G]
    parts, per = spk_split(H4, E)
    out = np.zeros((B, E), F32)
    for p in range(parts):
        g0, g1 = p * per, min(G, p * per + per)
        if drop_last_slice and g0 < G and g1 == G:
            continue
        acc = np.zeros((B, E), F32)
        for g in range(g0, g1):
            acc = (S[:, g, None] * W[None, g] + acc.astype(np.float64)).astype(F32)            # one fused multiply-add
        out = (out + acc).astype(F32)
    return out
