"""References for the re-layout and guard kernels of a training step (csrc/elementwise.hip, input_grads.hip): conv_pack / _many / _dx,
conv_unpack_grad[s], prep_run, transpose2d, copy_rows, act_scales and param_guard.  Plain numpy, no device.

Everything here is EXACT: these kernels move values (bit copies), add two fp32 numbers once (one IEEE rounding: numpy's float32 addition),
round fp32 to bf16 (to nearest even) or decide by comparisons.  So the budget of every check is zero differing BITS; there is no tolerance
to derive.  Results are compared as integers, so -0.0 against +0.0 and one NaN payload against another count as differences.

  conv_pack      wf [Co][5][Cp], wf[co][k][c] = w[co][c][k], zero for Ci <= c < Cp; wb [Ci][5][Co], wb[ci][k][co] = w[co][ci][4 - k]
  conv_unpack    g [Co][Ci][5], g[co][ci][k] = gp[co][k][ci] (or g +=); columns Ci <= c < Cp of gp are never read
  prep           dst = a + b, or (b None) the bits of a
  copy_rows      rows t < L_b = min(max(len[b], 0), T) copied, +0.0 behind them
  act_scales     bound = fmaf(sqrtf(16 T), max|gamma|, max|beta|) in fp32; min(16, largest power of two s >= 2^-20 with bound s <= 32768); a bound
                 of +inf keeps 16; NaN elements do not enter the maxima
  param_guard    word | 4 if any element is NaN, infinite or has |p| >= limit, else the word as it was

The images beside wf / wb / dst are compared on the device with ss_op_split_image of the fp32 result (format v2) and here with bf16_bits
(the bf16 data path)."""
from fractions import Fraction

import numpy as np

F32 = np.float32
RANGE_BIT = 4                                               # SS_STATUS_RANGE
CONV_SHAPES = ((4, 1, 4), (8, 3, 4), (64, 5, 8), (512, 80, 80), (512, 81, 84))      # (Co, Ci, Cp)
DX_SHAPES = CONV_SHAPES[:3] + ((3, 7, 0), (5, 1, 0), (257, 3, 0), (1, 1, 0))          # conv_pack_dx: any Ci and Co (Cp unused)
TRANSPOSE_SIZES = (1, 31, 32, 33, 257)
ACT_C = (64, 100, 512)
GUARD_N = (4, 1024, 4 * 131072 + 4)                         # the last: one float4 beyond a whole sweep of 512 x 256 threads
PREP_STRIDE = 64 * 256                                      # elements (float4 or scalar) one sweep of the prep grid covers


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def n_diff(a, b):
    """elements whose bits differ (the figure a test prints: its budget is 0)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int(np.count_nonzero(bits(a) != bits(b)))


def signed_zeros(a, rng, frac=0.05):
    """put -0.0 and +0.0 into a random fraction of a (in place): a copy that goes through an addition loses the sign"""
    flat = a.reshape(-1)
    k = rng.random(flat.size)
    flat[k < frac] = F32(-0.0)
    flat[(k >= frac) & (k < 2 * frac)] = F32(0.0)
    if flat.size >= 3:                                      # both zeros occur however small the array
        flat[flat.size // 3], flat[2 * flat.size // 3] = F32(-0.0), F32(0.0)
    return a


def bf16_bits(a):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; a NaN stays a (quiet) NaN"""
    u = bits(np.asarray(a, F32)).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(a, F32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


# ------------------------------------------------------------------------------------------------ conv packs
def conv_weight(Co, Ci, seed=0):
    rng = np.random.default_rng([11, Co, Ci, seed])
    return signed_zeros(rng.standard_normal((Co, Ci, 5)).astype(F32), rng)


def conv_pack_ref(w, Cp):
    Co, Ci, _ = w.shape
    wf = np.zeros((Co, 5, Cp), F32)
    wf[:, :, :Ci] = w.transpose(0, 2, 1)
    return wf, conv_pack_dx_ref(w)


def conv_pack_dx_ref(w):
    return np.ascontiguousarray(w[:, :, ::-1].transpose(1, 2, 0))          # [Ci][5][Co], taps flipped


def conv_pack_emulated(w, Cp, flip=True, pad_zero=True):
    """the kernel's own index arithmetic, element by element (flat index -> (co, k, cp) and (ci, k, co)); the switches make the mutants"""
    Co, Ci, _ = w.shape
    wf = np.empty(Co * 5 * Cp, F32)
    for i in range(wf.size):
        cp, k, co = i % Cp, (i // Cp) % 5, i // (5 * Cp)
        wf[i] = w[co, cp, k] if cp < Ci else (F32(0) if pad_zero else w[co, cp % Ci, k])
    wb = np.empty(Ci * 5 * Co, F32)
    for q in range(wb.size):
        co, k, ci = q % Co, (q // Co) % 5, q // (5 * Co)
        wb[q] = w[co, ci, 4 - k if flip else k]
    return wf.reshape(Co, 5, Cp), wb.reshape(Ci, 5, Co)


def packed_grad(Co, Ci, Cp, pad, seed=0):
    """a packed gradient [Co][5][Cp] whose padding columns hold `pad` (the guard NaN: they are never read)"""
    rng = np.random.default_rng([12, Co, Ci, Cp, seed])
    gp = signed_zeros(rng.standard_normal((Co, 5, Cp)).astype(F32), rng)
    gp[:, :, Ci:] = pad
    return gp


def conv_unpack_ref(gp, Ci, g0=None):
    v = np.ascontiguousarray(gp[:, :, :Ci].transpose(0, 2, 1))             # [Co][Ci][5]
    return v if g0 is None else (g0 + v).astype(F32)                       # one fp32 addition per element


def conv_unpack_emulated(gp, Ci, g0=None, swapped=False):
    Co, _, Cp = gp.shape
    flat, out = gp.reshape(-1), np.empty(Co * Ci * 5, F32)
    for i in range(out.size):
        k, ci, co = i % 5, (i // 5) % Ci, i // (5 * Ci)
        if swapped:                                         # mutant: (ci, k) taken in [Co][Ci][5] order from the pack
            k, ci = (i // Ci) % 5, i % Ci
        out[i] = flat[(co * 5 + k) * Cp + ci]
    out = out.reshape(Co, Ci, 5)
    return out if g0 is None else (g0 + out).astype(F32)


# ------------------------------------------------------------------------------------------------ prep
def prep_ref(a, b=None):
    return a.copy() if b is None else (a + b).astype(F32)


def prep_emulated(a, b, vec, plus_zero=False):
    """the kernel's two paths; plus_zero: the scalar path as it was, a + (b ? b : 0.f)"""
    if b is not None:
        return (a + b).astype(F32)
    if vec or not plus_zero:
        return a.copy()
    return (a + F32(0)).astype(F32)


def prep_takes_vec(n, *byte_addresses):
    return n % 4 == 0 and all(p % 16 == 0 for p in byte_addresses)


# ------------------------------------------------------------------------------------------------ copy_rows
def ragged_len(length, T):
    return min(max(int(length), 0), T)


def copy_rows_ref(src, lens=None):
    """src [B][T][C] -> what the destination's real rows hold"""
    out = src.copy()
    if lens is not None:
        for b, n in enumerate(lens):
            out[b, ragged_len(n, src.shape[1]):] = F32(0)
    return out


# ------------------------------------------------------------------------------------------------ act_scales
def f32_round(x):
    """a Fraction -> the nearest float32, ties to even, overflow to inf (x >= 0)"""
    with np.errstate(over='ignore'):
        f = F32(min(float(x), 3.5e38))                      # within one float32 ulp of the answer (inf beyond the range)
    if np.isinf(f):
        top = Fraction(float(np.finfo(F32).max))
        return f if x - top >= Fraction(2) ** 103 else F32(np.finfo(F32).max)          # half an ulp above the largest finite value rounds up
    cands = [c for c in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))) if np.isfinite(c)]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(bits(np.array([c], F32))[0]) & 1))
    return F32(best)


def act_bound(gamma, beta, T):
    """fmaf(sqrtf(16 T), max|gamma|, max|beta|) in fp32; NaN elements do not enter the maxima (fmaxf); C = 0 gives 0"""
    rt = np.sqrt(F32(16.0) * F32(T), dtype=F32)
    with np.errstate(invalid='ignore'):
        mg = F32(np.fmax.reduce(np.abs(np.asarray(gamma, F32)), initial=F32(0)))
        mb = F32(np.fmax.reduce(np.abs(np.asarray(beta, F32)), initial=F32(0)))
    if np.isinf(mg) or np.isinf(mb):
        return F32(np.inf)
    return f32_round(Fraction(float(rt)) * Fraction(float(mg)) + Fraction(float(mb)))


def act_scale_ref(bound):
    """min(16, the largest power of two s >= 2^-20 with bound * s <= 32768); +inf keeps 16"""
    if np.isinf(bound):
        return F32(16)
    for k in range(4, -21, -1):
        if Fraction(float(bound)) * Fraction(2) ** k <= 32768:
            return F32(2.0 ** k)
    return F32(2.0 ** -20)


def act_scale_emulated(bound, inf_keeps=True):
    """the kernel's loop; inf_keeps False: the loop as it was, which runs +inf down to the floor"""
    bound, sc = F32(bound), F32(16)
    if not inf_keeps or bound < F32(np.inf):
        with np.errstate(over='ignore'):
            while sc > F32(2.0 ** -20) and bound * sc > F32(32768):
                sc = sc * F32(0.5)
    return sc


def act_cases(T):
    """(name, gamma-max, beta-max): the extreme sits in the LAST element of the block; T = 64 makes sqrtf(16 T) = 32 exactly"""
    up = np.nextafter(F32(64), F32(np.inf))
    return (('bound=2048', F32(64), F32(0)), ('just-above', up, F32(0)), ('above-by-beta', F32(64), F32(1e-3)), ('ordinary', F32(1.5), F32(0.25)),
            ('below', np.nextafter(F32(64), F32(0)), F32(0)), ('negative', F32(-300), F32(-7)), ('mid', F32(1e6), F32(3)), ('huge', F32(1e30), F32(1)),
            ('overflow', F32(3e38), F32(0)), ('inf-gamma', F32(np.inf), F32(0)), ('inf-beta', F32(1), F32(-np.inf)), ('nan-gamma', F32(np.nan), F32(0.5)),
            ('nan-beta', F32(2), F32(np.nan)), ('zero', F32(0), F32(0)), ('floor', F32(1e36), F32(0)))


def act_block(C, gmax, bmax, seed):
    """gamma, beta of C channels, the extremes gmax / bmax in the LAST element and every other magnitude below 0.9 min(1, |extreme|) (0.9 where
    the extreme is not finite)"""
    rng = np.random.default_rng([13, C, seed])

    def others(extreme):
        return (rng.uniform(-0.9, 0.9, C) * (min(1.0, abs(float(extreme))) if np.isfinite(extreme) else 1.0)).astype(F32)
    g, b = others(gmax), others(bmax)
    g[-1], b[-1] = gmax, bmax
    return g, b


# ------------------------------------------------------------------------------------------------ param_guard
def guard_ref(p, limit, word):
    with np.errstate(invalid='ignore'):
        bad = bool(np.any(~(np.abs(np.asarray(p, F32)) < F32(limit))))
    return (int(word) | RANGE_BIT) & 0xFFFFFFFF if bad else int(word) & 0xFFFFFFFF


def guard_emulated(p, limit, word, strict=True, drop_last=False, set_word=False):
    """mutants: `> limit` instead of `>= limit`, the last float4 not looked at, the word written instead of OR-ed"""
    p = np.asarray(p, F32)
    if drop_last:
        p = p[:-4]
    with np.errstate(invalid='ignore'):
        bad = bool(np.any(~(np.abs(p) < F32(limit)))) if strict else bool(np.any(np.abs(p) > F32(limit)) or np.any(np.isnan(p)))
    if not bad:
        return int(word) & 0xFFFFFFFF
    return RANGE_BIT if set_word else (int(word) | RANGE_BIT) & 0xFFFFFFFF


def guard_values(limit):
    """(name, value, bad)"""
    lim = F32(limit)
    return (('nan', F32(np.nan), True), ('+inf', F32(np.inf), True), ('-inf', F32(-np.inf), True), ('limit', lim, True), ('-limit', -lim, True),
            ('below', np.nextafter(lim, F32(0)), False), ('-below', -np.nextafter(lim, F32(0)), False))


def guard_arena(n, seed=0):
    rng = np.random.default_rng([14, n, seed])
    return signed_zeros(rng.uniform(-2000, 2000, n).astype(F32), rng, 0.01)
