"""Float64 restatement of the GEMM descriptors (GemmDesc / ImgGemmDesc, speechsplit_amd/csrc/common.h) on flat buffers, numpy only.

ADDRESSING (the comment on `Operand`): element (row, col) of batch b of an operand lives at
    off + b * bstride + row * ld + (col // seglen) * segstride + col % seglen           (seglen == 0: + col)
A(m, k) is stored at (row m, col k), or at (row k, col m) when the operand is reduction-major (TA; the same for B(n, k) and TB); the result
goes to c_off + b * cstride + m * ldc + n.  With the image GEMM's row map (rm_T > 0) logical row m of A and of C is memory row
(m // rm_T) * rm_TP + m % rm_T.  The row mask lets row m be stored only if (m + row_off) % row_period lies in [row_lo, row_hi); every other
element of C -- masked rows, the halo rows the row map skips, the gaps between rows and batches -- keeps its prior BITS.

OPERAND ROUNDING per family (`rounded_terms`):
    f32      none (v_mfma_f32_32x32x2_f32 multiplies fp32 values).
    bf16x3   none: x = h + m + l exactly (truncation splits); the kernel drops the products m.l, l.m and l.l.  h keeps the top 8 significand
             bits, so |x - h| < 2^-7 |x|, |m| < 2^-7 |x|, |l| < 2^-15 |x|; the dropped terms are below (2 * 2^-22 + 2^-30) |a||b| < 2^-21 |a||b|
             (gemm_bf16x3.hip's header quotes the typical size, 2^-24).  The sharp bar carries this worst case: DROP_BF16X3 = 8 units of 2^-24.
    bf16     each operand rounded to bf16, nearest even (v_cvt_pk_bf16_f32); one product.
    f16x2    y = s x (s a power of two, exact), hi = fp16(y) to nearest, lo = fp16(y - hi) (y - hi is exact in fp32; v_fma_mix rounds once);
             the products hi.hi + hi.lo + lo.hi (lo.lo is dropped by the kernel AND by this reference), times 1 / (s_a s_b).  s is the fixed 16,
             or the word behind a_pre_scale / b_pre_scale, or pow2_scale_of(amax) (restated below from common.h).
The image format v2 (`pack_image`) and the plain bf16 image (`pack_bf16`) are restated too: per aligned group of eight elements 16 bytes of
hi pieces, then 16 bytes of lo pieces.

TWO JUDGEMENTS per written element (`judge`), neither fitted to what a GPU returns:
  sharp   against the float64 contraction of the ROUNDED pieces, so that only fp32 accumulation is left:
              |C - ref| <= (k_len + ksplit + EPI + drop) * 2^-24 * (sum_k |a||b| + |bias| + |C0|)
          k_len: the longest k-slice, ceil(ceil(K / kt) / ksplit) * kt capped at K -- one rounding per accumulated product of an fp32 fma chain
          (the kernels' split-K boundaries are multiples of the k-tile kt: 16 in gemm_f32.hip, 32 in gemm_bf16x3.hip and gemm_img.hip, 64 in
          the single-piece image form; 32 is used where the kernel is the launcher's choice -- the longest slice of the 16-wide kernel is
          never longer).  ksplit: the additions that bring the slices together in C (one atomic add per slice, or ksplit - 1 additions in
          splitk_reduce plus the one onto C; without a split, the one `*c += v` of GEMM_ACCUM).  EPI = 2: `acc * unscale` (exact for a power
          of two unless it underflows; counted) and `+ bv`, counted from the epilogues of the three kernels.  drop: DROP_BF16X3 for bf16x3, else 0.
          The bf16 x 3 and fp16 x 2 kernels issue six / three MFMAs per 16 k, i.e. more accumulations than products; their extra terms are
          2^-8 / 2^-10 of the leading one, so the accumulator they round is the same and the first-order count stays one per k.
          profiles/r04/mfma_round_probe.txt (rms relative error 2.4e-7 at K = 256 where this bar allows 1.5e-5 of sum |a||b|) gives no reason to
          widen the fma-chain bound for how the MFMA accumulates: no factor is applied.
  honest  against the float64 product of the UNROUNDED operands, at the project's existing bars -- 5e-6 for the fp32-grade families and the
          upper edge 1e-2 of test_gemm_bf16_mode's band for bf16 x 1 (its lower edge, 1e-4 in the max-norm, is asserted by the tests that use
          it) -- but per element: the bar times min(max |ref|, sum_k |a||b| + |bias| + |C0|).  That is never wider than the max-norm bar, and
          for a row or column of small magnitude it is as much smaller as that row is.  fp16 x 2 only: the per-element side also carries the
          format's absolute floor (gemm_bf16x3.hip: "an absolute floor of 2^-25 / s" -- the lo piece is rounded to fp16's denormal spacing
          2^-24), sum_k (2^-25 / s_a) |b| + (2^-25 / s_b) |a|: an element 2^-13 of the scale's range keeps 3 bits of its lo piece, and a
          reduction of ONE such product cannot be 5e-6 of itself (seen at K = 1; the max-norm side of the min still holds it).
  untouched  every element of the C buffer outside the write set keeps its bits (compared as integers; NaN payloads included).
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPI = 2
DROP_BF16X3 = 8
FAMILIES = ('f32', 'bf16x3', 'bf16', 'f16x2')
HONEST = {'f32': 5e-6, 'bf16x3': 5e-6, 'f16x2': 5e-6, 'bf16': 1e-2}


class Geom:
    """Placement of one operand in its flat buffer, in elements."""

    def __init__(self, off=0, ld=0, bstride=0, seglen=0, segstride=0):
        self.off, self.ld, self.bstride, self.seglen, self.segstride = int(off), int(ld), int(bstride), int(seglen), int(segstride)

    def tuple(self):
        return (self.off, self.ld, self.bstride, self.seglen, self.segstride)

    def replace(self, **k):
        g = Geom(*self.tuple())
        for n, v in k.items():
            setattr(g, n, int(v))
        return g


class Desc:
    """One launch.  family: 'f32' | 'bf16x3' | 'bf16' | 'f16x2'; sa / sb: the fp16 x 2 scales; kt: the kernel's k-tile."""

    def __init__(self, A, B, c_off, ldc, cstride, M, N, K, batch=1, ta=False, tb=False, accum=False, family='f32', row_mask=(0, 0, 0, 0),
                 rm=(0, 0), ksplit=1, sa=16.0, sb=16.0, kt=32):
        self.A, self.B, self.c_off, self.ldc, self.cstride = A, B, int(c_off), int(ldc), int(cstride)
        self.M, self.N, self.K, self.batch, self.ta, self.tb, self.accum = M, N, K, batch, bool(ta), bool(tb), bool(accum)
        self.family, self.row_mask, self.rm, self.ksplit, self.sa, self.sb, self.kt = family, tuple(row_mask), tuple(rm), ksplit, float(sa), float(sb), kt
        assert family in FAMILIES

    def replace(self, **k):
        d = Desc.__new__(Desc)
        d.__dict__.update(self.__dict__)
        d.__dict__.update(k)
        return d

    def k_len(self):
        tiles = -(-self.K // self.kt)
        return min(self.K, -(-tiles // self.ksplit) * self.kt)

    def slices(self):
        """[(kbeg, kend)] of the ksplit slices, as every kernel cuts them (empty slices included)."""
        per = -(-(-(-self.K // self.kt)) // self.ksplit) * self.kt
        return [(min(self.K, s * per), min(self.K, (s + 1) * per)) for s in range(self.ksplit)]


def pow2_scale_of(m):
    """common.h: the power of two that brings a measured maximum m into [128, 256), capped to 2^-126 .. 2^60."""
    e = (int(np.asarray(m, F32).view(np.uint32)) >> 23) & 0xFF
    se = min(187, max(1, 261 - e))
    return float(np.asarray(se << 23, np.uint32).view(F32))


def _map_rows(m, rm):
    return m if rm[0] <= 0 else (m // rm[0]) * rm[1] + m % rm[0]


def operand_index(g, X, K, batch, T, rm=(0, 0)):
    """int64 [batch, X, K]: where the logical element (x, k) of each batch lives in the flat buffer."""
    x = _map_rows(np.arange(X, dtype=np.int64), rm)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    row, col = (k, x) if T else (x, k)
    if g.seglen:
        col = (col // g.seglen) * g.segstride + col % g.seglen
    return g.off + np.arange(batch, dtype=np.int64)[:, None, None] * g.bstride + (row * g.ld + col)[None]


def a_index(d):
    return operand_index(d.A, d.M, d.K, d.batch, d.ta, d.rm)


def b_index(d):
    return operand_index(d.B, d.N, d.K, d.batch, d.tb)


def c_index(d):
    m = _map_rows(np.arange(d.M, dtype=np.int64), d.rm)[:, None]
    return d.c_off + np.arange(d.batch, dtype=np.int64)[:, None, None] * d.cstride + (m * d.ldc + np.arange(d.N, dtype=np.int64)[None, :])[None]


def written_rows(d):
    p, off, lo, hi = d.row_mask
    if p <= 0:
        return np.ones(d.M, bool)
    q = (np.arange(d.M) + off) % p
    return (q >= lo) & (q < hi)


def bf16_rne(x):
    """float32 -> the bf16 value nearest to it (ties to even), as float32; NaN stays NaN."""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    out = r.view(F32).copy()
    nan = np.isnan(np.asarray(x, F32))
    out[nan] = np.nan
    return out.reshape(np.shape(x))


def split_f16(x, s):
    """(hi, lo) as float16 arrays: hi = fp16(s x), lo = fp16(s x - hi), each rounded once."""
    with np.errstate(over='ignore', invalid='ignore'):
        y = np.asarray(x, F32) * F32(s)
        hi = y.astype(np.float16)
        lo = (y - hi.astype(F32)).astype(np.float16)
    return hi, lo


def pack_image(flat, s):
    """Image format v2 of a flat float32 buffer (length % 8 == 0, groups of eight aligned to its start): uint16 [len / 8, 16], per group the
    eight hi pieces then the eight lo pieces.  `.view(np.float32).reshape(-1)` has the fp32 buffer's length."""
    flat = np.asarray(flat, F32).reshape(-1, 8)
    hi, lo = split_f16(flat, s)
    return np.concatenate([hi.view(np.uint16), lo.view(np.uint16)], axis=1)


def pack_bf16(flat):
    """The plain bf16 image: uint16 bit patterns, round to nearest even."""
    return (bf16_rne(np.asarray(flat, F32).reshape(-1)).view(np.uint32) >> 16).astype(np.uint16)


def rounded_terms(family, a, b, sa=16.0, sb=16.0):
    """[(A_piece, B_piece)] float64 arrays whose products the family sums, and the factor that undoes the scales."""
    if family in ('f32', 'bf16x3'):
        return [(a.astype(F64), b.astype(F64))], 1.0
    if family == 'bf16':
        return [(bf16_rne(a).astype(F64), bf16_rne(b).astype(F64))], 1.0
    ah, al = (p.astype(F64) for p in split_f16(a, sa))
    bh, bl = (p.astype(F64) for p in split_f16(b, sb))
    return [(ah, bl), (al, bh), (ah, bh)], 1.0 / (sa * sb)


class Ref:
    pass


def _mm(p, q):
    """[b, m, k] x [b, n, k] -> [b, m, n]"""
    with np.errstate(invalid='ignore'):
        return np.matmul(p, q.transpose(0, 2, 1))


def reference(d, a, b, c0, bias=None):
    """Expected values of one launch.  a, b: flat float32 buffers; c0: the C buffer before the launch; bias: float32 [N] or None."""
    r = Ref()
    r.d = d
    A, B = np.asarray(a, F32)[a_index(d)], np.asarray(b, F32)[b_index(d)]
    terms, unscale = rounded_terms(d.family, A, B, d.sa, d.sb)
    r.sharp = sum(_mm(p, q) for p, q in terms) * unscale
    r.honest = _mm(A.astype(F64), B.astype(F64))
    ra, rb = terms[-1]                                       # |rounded a||rounded b| from the leading pieces
    r.S = _mm(np.abs(ra), np.abs(rb)) * unscale
    r.idx = c_index(d)
    assert np.unique(r.idx).size == r.idx.size, 'the C elements of this descriptor overlap'
    r.rows = written_rows(d)
    add = np.zeros_like(r.sharp)
    if bias is not None:
        add = add + np.asarray(bias, F32).astype(F64)[None, None, :]
    r.C0 = np.asarray(c0, F32)[r.idx].astype(F64) if d.accum else np.zeros_like(r.sharp)
    with np.errstate(invalid='ignore'):
        r.sharp = r.sharp + add + r.C0
        r.honest = r.honest + add + r.C0
        r.S = r.S + np.abs(add) + np.abs(r.C0)
    drop = DROP_BF16X3 if d.family == 'bf16x3' else 0
    r.units = d.k_len() + d.ksplit + EPI + drop
    r.bar_sharp = r.units * U * r.S
    top = float(np.abs(r.honest[:, r.rows]).max()) if r.rows.any() else 0.0
    per_element = HONEST[d.family] * r.S
    if d.family == 'f16x2':                                  # the format's absolute floor: 2^-25 / s per operand element
        per_element = per_element + 2.0 ** -25 * (_mm(np.ones_like(A, F64), np.abs(B).astype(F64)) / d.sa + _mm(np.abs(A).astype(F64), np.ones_like(B, F64)) / d.sb)
    r.bar_honest = np.minimum(HONEST[d.family] * top, per_element)
    return r


def judge(ref, c_before, c_after):
    """Compare the C buffer after a launch with `ref`.  Returns (failures, figures): failures is a list of 'sharp' / 'honest' / 'untouched' /
    'nonfinite', figures the worst ratio of an error to each bar (1.0 = at the bar)."""
    d = ref.d
    before = np.ascontiguousarray(c_before, F32).view(np.uint32)
    after = np.ascontiguousarray(c_after, F32).view(np.uint32)
    idx = ref.idx[:, ref.rows]
    keep = np.ones(before.size, bool)
    keep[idx.reshape(-1)] = False
    fails = []
    stray = int((before[keep] != after[keep]).sum())
    if stray:
        fails.append('untouched')
    got = np.asarray(c_after, F32)[idx].astype(F64)
    fig = {'untouched': stray}
    if not np.isfinite(got).all():
        fails.append('nonfinite')
    with np.errstate(invalid='ignore', divide='ignore'):
        for name, exp, bar in (('sharp', ref.sharp, ref.bar_sharp), ('honest', ref.honest, ref.bar_honest)):
            err = np.abs(got - exp[:, ref.rows])
            b = bar[:, ref.rows]
            ratio = np.where(err == 0, 0.0, err / b)            # error against a zero bar: infinite
            ratio = np.where(np.isfinite(got), ratio, np.inf)
            worst = float(ratio.max()) if ratio.size else 0.0
            fig[name] = worst
            if name == 'honest':                                # the suite's older measure, max |error| / max |ref| (test_gemm_bf16_mode's band)
                fig['maxnorm'] = float(np.nanmax(err) / (np.abs(exp[:, ref.rows]).max() + 1e-300)) if err.size else 0.0
            if not worst <= 1.0:
                fails.append(name)
    return fails, fig


def spans(d):
    """Elements each flat buffer must have: (a, b, c)."""
    return int(a_index(d).max()) + 1, int(b_index(d).max()) + 1, int(c_index(d).max()) + 1


# ---- a float32 restatement of each family (the CPU self-test's stand-in for a kernel) and its wrong variants --------------------------
VARIANTS = ('bias_every_slice', 'mask_shifted', 'mask_ignored_value', 'mask_ignored_zero', 'segment_wrap_early', 'segstride_not_on_image',
            'cstride_ignored', 'shared_b_strided', 'rm_TP_as_rm_T', 'accum_overwrites', 'scale_not_undone', 'lo_hi_dropped', 'k_tile_skipped',
            'bf16_single_rounding')


def simulate(d, a, b, c0, bias=None, variant=None):
    """What a kernel of d.family leaves in the C buffer: float32 pieces, float32 accumulation slice by slice, the epilogue in float32.
    variant: None (correct) or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    v = variant
    dr = d                                                    # the descriptor the (wrong) kernel reads with
    if v == 'segment_wrap_early':
        dr = d.replace(A=d.A.replace(seglen=d.A.seglen - 1))
    elif v == 'segstride_not_on_image':
        dr = d.replace(A=d.A.replace(seglen=0))
    elif v == 'shared_b_strided':
        dr = d.replace(B=d.B.replace(bstride=d.N * d.B.ld))
    elif v == 'rm_TP_as_rm_T':
        dr = d.replace(rm=(d.rm[0], d.rm[0]))
    elif v == 'mask_shifted':
        dr = d.replace(row_mask=(d.row_mask[0], d.row_mask[1] + 1) + d.row_mask[2:])
    elif v in ('mask_ignored_value', 'mask_ignored_zero'):
        dr = d.replace(row_mask=(0, 0, 0, 0))
    if v == 'cstride_ignored':
        dr = dr.replace(cstride=0)
    fam = 'bf16' if v == 'bf16_single_rounding' else d.family
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    A, B = a[a_index(dr) % a.size], b[b_index(dr) % b.size]
    terms, unscale = rounded_terms(fam, A, B, d.sa, d.sb)
    if v == 'lo_hi_dropped':
        terms = [t for i, t in enumerate(terms) if i != 1]
    if v == 'scale_not_undone':
        unscale *= d.sa
    out = np.array(c0, F32, copy=True)
    idx = c_index(dr)
    rows = written_rows(dr)
    acc = out[idx].copy() if (d.accum and v != 'accum_overwrites') else np.zeros(idx.shape, F32)
    sl = d.slices()
    for s, (k0, k1) in enumerate(sl):
        if v == 'k_tile_skipped' and s == max(i for i, (p, q) in enumerate(sl) if q > p):
            k1 = max(k0, k1 - ((k1 - k0 - 1) % d.kt + 1))
        part = np.zeros(idx.shape, F32)
        for p, q in terms:
            part = part + np.einsum('bmk,bnk->bmn', p[:, :, k0:k1].astype(F32), q[:, :, k0:k1].astype(F32)).astype(F32)
        part = part * F32(unscale)
        if bias is not None and (s == 0 or v == 'bias_every_slice'):
            part = part + np.asarray(bias, F32)[None, None, :]
        acc = acc + part
    if v == 'mask_ignored_zero':
        acc[:, ~written_rows(d)] = 0
    for bi in range(d.batch):                                # batch by batch: a later batch overwrites an earlier one where they collide
        out[idx[bi][rows]] = acc[bi][rows]
    return out
