"""Cases, references and budgets for the resampling kernels of csrc/interp.hip launched alone (tests/test_gpu_interp_ops.py).  The
references are oracle/interp_np.py (the numpy restatement of the reference's InterpLnr and quantize_f0_torch); what is here builds the
batches that sweep the draws and hit the plan's edges, the quantiser's clamp, and the scatter's float64 reference with its budget.

PLAN, GATHER, QUANTISER: bit-exact against the oracle (the index path is integer arithmetic on one correctly rounded fp32 division; the
value path is two fp32 products and one sum, rounded separately; the class is one fp32 product, one rint).  Budget: zero differing bits.

SCATTER: dx(i) = sum over n terms w_r dy_r, the weights fl32(1 - lam_r) and lam_r, accumulated by one fp32 chain of fused multiply-adds from
0.  Step k of the chain rounds once: s_k = (s_{k-1} + t_k)(1 + d_k), |d_k| <= u = 2^-24, the product t_k being exact inside the fma.  To first
order the error is sum_k d_k (t_1 + .. + t_k), at most u sum_k sum_{j<=k} |t_j| <= n u sum|t|.  Budget per element: n 2^-24 sum|terms|
against the float64 sum of the same terms (each term is exact in float64: 24 x 24 bits).  A frame with no term has budget 0: exactly zero."""
import numpy as np

from oracle import interp_np as O

F32 = np.float32
U = 2.0 ** -24
S = 7
PLAN_B = 512
PLAN_T = 224                                                # 7 segments of at most 32 frames
PLAN_P = (8, 64, 192, 256, 512)
GATHER_C = (1, 3, 64, 81, 128, 256, 520)                    # block sizes 64 / 128 / 256 (plain) and 64 / 128 (image: C % 8 == 0)
GATHER_IMG_C = (64, 128, 256, 520)
SCATTER_C = (1, 64, 130, 256)
QUANT_CM = (1, 80, 129)
NOH = 257


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def n_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int(np.count_nonzero(bits(a) != bits(b)))


# ------------------------------------------------------------------------------------------------ plan batches
def integer_quotient_scales(lo=0.5, hi=1.5):
    """[(scale, lane)] with scale a float32 in [lo, hi): fl32(lane / scale) is an integer while the float64 quotient is not -- the draws
    where floor() of a wider or a reciprocal-based division lands one frame lower (or lam comes out as ~1 instead of 0)"""
    found = []
    for lane in range(1, 64):
        for k in range(int(np.ceil(lane / hi)), int(np.floor(lane / lo)) + 1):
            c = F32(lane / k)
            for sc in (np.nextafter(c, F32(0)), c, np.nextafter(c, F32(2))):
                if not lo <= sc < hi:
                    continue
                q32 = F32(lane) / sc
                q64 = float(lane) / float(sc)
                if q32 == k and q64 != k:
                    found.append((sc, lane))
    return found


def reference_draws(rng, n):
    """model.py:392-393, 399-402: scales = rand + 0.5 in fp32, len_seg = randint(19, 32)"""
    return (rng.random((n, S), dtype=F32) + F32(0.5)).astype(F32), rng.integers(19, 32, (n, S)).astype(np.int32)


def stretched_draws(rng, n):
    """the stretching end of the reference's ranges (tests/test_gpu_frame_range.py): scales in [1.3, 1.5), len_seg in 28 .. 31"""
    return (F32(1.3) + F32(0.2) * rng.random((n, S), dtype=F32)).astype(F32), rng.integers(28, 32, (n, S)).astype(np.int32)


def plan_batch(T=PLAN_T, B=PLAN_B, seed=0):
    """(scales f32 [B, S], len_seg i32 [B, S], len_seq i32 [B], classes): the reference-range family with lengths from 0 .. T, the stretched
    family at full length, and hand-made rows; classes maps an edge's name to the rows made for it"""
    rng = np.random.default_rng([21, T, seed])
    rows, cls = [], {}

    def add(name, sc, ls, n):
        cls.setdefault(name, []).append(len(rows))
        rows.append((np.asarray(sc, F32), np.asarray(ls, np.int32), int(n)))
    sc, ls = reference_draws(rng, 40)
    for i, n in enumerate((0, 1, 2, 3, T - 1, T) * 2):
        add(f'len_seq={n}', sc[i], ls[i], n)
    for name, v in (('scale=0.5', F32(0.5)), ('scale=1.0', F32(1.0)), ('scale=1.5-', np.nextafter(F32(1.5), F32(0)))):
        for k, n in enumerate((T, T // 2)):
            add(name, np.full(S, v, F32), ls[12 + k], n)
    quot = integer_quotient_scales()
    for k in range(0, min(len(quot), 16 * S), S):
        chunk = [q[0] for q in quot[k:k + S]]
        add('integer-quotient', (chunk + [F32(1)] * S)[:S], np.full(S, 32, np.int32), T)
    for name, seg in (('len_seg=1', [1] * S), ('len_seg=2', [2] * S), ('len_seg=32', [32] * S), ('len_seg-mixed', [1, 32, 2, 32, 1, 19, 32])):
        for k in range(2):
            add(name, sc[20 + k], seg, T)
    st_sc, st_ls = stretched_draws(rng, 64)
    for i in range(64):
        add('stretched', st_sc[i], st_ls[i], T)
    n_ref = B - len(rows)
    sc, ls = reference_draws(rng, n_ref)
    for i, n in enumerate(rng.integers(0, T + 1, n_ref)):
        add('reference', sc[i], ls[i], n)
    assert len(rows) == B
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int32), cls)


def plan_ref(scales, len_seg, len_seq, T, P, ncand=64):
    """the oracle's plan with the inverse map: i0, lam, counts, nrows, start"""
    assert ncand % 2 == 0
    i0, lam, counts, nrows = O.interp_plan(scales.reshape(-1), len_seg.reshape(-1), len_seq, max_len_seg=ncand // 2, max_len_pad=P)
    return i0, lam, counts, nrows, O.interp_start(i0, nrows, T)


def plan_edges(scales, len_seg, len_seq, T, P, ncand=64):
    """which edge classes the batch holds at this P (each must be non-empty where it can occur)"""
    i0, lam, counts, nrows, start = plan_ref(scales, len_seg, len_seq, T, P, ncand)
    j = np.arange(ncand, dtype=F32)
    per_seg = np.zeros(scales.shape, np.int64)              # kept candidates per segment
    off = np.concatenate([np.zeros((len(len_seq), 1), np.int64), np.cumsum(len_seg, 1)[:, :-1]], 1)
    for s in range(scales.shape[1]):
        fl = np.floor((j[None, :] / scales[:, s:s + 1]).astype(F32))
        per_seg[:, s] = ((fl < len_seg[:, s:s + 1] - 1) & (fl + off[:, s:s + 1] < len_seq[:, None] - 1)).sum(1)
    assert np.array_equal(per_seg.sum(1), counts)
    ends = np.cumsum(per_seg, 1)
    cut_mid = (counts > P) & ~(ends == P).any(1)            # the truncation falls inside a segment
    return {'dead': int((nrows == 0).sum()), 'full': int((nrows == P).sum()), 'truncated': int((counts > P).sum()),
            'cut-mid-segment': int(cut_mid.sum()), 'partial': int(((nrows > 0) & (nrows < P)).sum()),
            'lam=0 rows': int(((lam == 0) & (np.arange(P)[None, :] < nrows[:, None])).sum()),
            'empty segment': int(((per_seg == 0) & (len_seq[:, None] > off + 1)).sum()), 'max count': int(counts.max())}


# ------------------------------------------------------------------------------------------------ value path
def small_plan(T, P, B=8, seed=0):
    """a plan for the value-path tests: reference-range draws, lengths from 2 .. T with one dead and one full-length utterance; collisions
    (scales above 1: two rows share i0) and skipped frames (scales below 1) both occur"""
    rng = np.random.default_rng([22, T, P, seed])
    sc, ls = reference_draws(rng, B)
    sc[1], sc[2] = F32(1.4), F32(0.6)
    n = rng.integers(2, T + 1, B).astype(np.int32)
    n[0], n[1], n[2], n[3] = 0, T, T, 1
    i0, lam, counts, nrows, start = plan_ref(sc, ls, n, T, P)
    return dict(scales=sc, len_seg=ls, len_seq=n, i0=i0, lam=lam, counts=counts, nrows=nrows, start=start)


def gather_input(B, T, C, len_seq, fill, seed=0):
    """x [B][T][C]: normal values, -0.0, and magnitudes down to 1e-38 whose products with lam are subnormal; rows at or beyond len_seq hold `fill`"""
    rng = np.random.default_rng([23, B, T, C, seed])
    x = rng.standard_normal((B, T, C)).astype(F32)
    k = rng.random((B, T, C))
    x[k < 0.05] = F32(-0.0)
    tiny = (k >= 0.05) & (k < 0.25)
    x[tiny] = (x[tiny] * F32(10.0) ** rng.integers(-38, -30, int(tiny.sum())).astype(F32)).astype(F32)
    for b, n in enumerate(len_seq):
        x[b, int(n):] = fill
    return x


def quant_class(f, noh=NOH):
    """the oracle's class with the kernel's clamp: 0 when not f > 0 (unvoiced, -0.0, NaN), else min(rint(f * 255) + 1, noh - 1)"""
    f = np.asarray(f, F32)
    with np.errstate(invalid='ignore'):
        voiced = f > 0
        idx = np.rint(np.where(voiced, f, F32(0)) * F32(255)).astype(np.int64) + 1
    inside = voiced & (f <= 1)
    assert np.array_equal(idx[inside], O.quantize_f0(f[inside]))                             # the oracle wherever it is defined
    return np.where(voiced, np.minimum(idx, noh - 1), 0).astype(np.int32)


def half_way_values():
    """fl32((k + 0.5) / 255), k = 0 .. 254: the fp32 product with 255 is exactly k + 0.5 for every k (asserted), so rint decides by parity"""
    v = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(F32)
    assert np.array_equal((v * F32(255)).astype(F32), (np.arange(255) + 0.5).astype(F32))
    return v


def quant_case(P=256, T=256, CM=80, seed=0):
    """Three utterances.  0 and 1: every scale 1.0 and len_seg 32, so row r reads frame i0 with lam = 0; the frames carry the 255 half-way
    values, 0, -0.0, the smallest subnormal (class 1), 1.0 (256), 1.5 (clamped to 256) and NaN (0).  2: reference-range draws over a track
    of voiced frames with -1e10 (unvoiced) neighbours, lam in (0, 1).  Rows behind nrows are dead."""
    rng = np.random.default_rng([24, P, T, CM, seed])
    sc, ls = reference_draws(rng, 3)
    sc[:2], ls[:2] = F32(1.0), 32
    n = np.array([T, T, T - 7], np.int32)
    i0, lam, counts, nrows, start = plan_ref(sc, ls, n, T, P)
    assert not lam[:2].any() and nrows[0] == nrows[1] >= 186 and (nrows < P).all()
    # (the NaN goes last, behind a filler: the row in front of it reads it as its neighbour, 0 * NaN, and is NaN too -- in the oracle as well)
    special = np.array([0.0, -0.0, np.float32(1e-45), 1.0, 1.5, 0.5, 1.0 / 255.0, 0.75, np.nan], F32)
    vals = np.concatenate([half_way_values(), special])
    f0 = np.full((3, T), F32(0.25), F32)
    frames = [(b, int(i)) for b in range(2) for i in i0[b, :nrows[b]]]
    assert len(frames) >= len(vals) and len(set(frames)) == len(frames)
    for (b, i), v in zip(frames, vals):
        f0[b, i] = v
    voiced = rng.random(T) < 0.6
    f0[2] = np.where(voiced, rng.random(T).astype(F32), F32(-1e10))
    mel = rng.random((3, T, CM)).astype(F32)
    rows = [(b, r) for b in range(2) for r in range(nrows[b])][:len(vals)]                   # the row that reads vals[k] with lam = 0
    return dict(scales=sc, len_seg=ls, len_seq=n, i0=i0, lam=lam, nrows=nrows, f0=f0, mel=mel, vals=vals, rows=rows)


def quant_ref(case, yo_ld, noh=NOH):
    """qidx [B][P], ymel [B][P][CM], one-hot [B][P][yo_ld] (padding columns zero)"""
    i0, lam, nrows = case['i0'], case['lam'], case['nrows']
    f = O.interp_apply(case['f0'][:, :, None], i0, lam, nrows)[:, :, 0]
    q = quant_class(f, noh)
    q[np.arange(i0.shape[1])[None, :] >= nrows[:, None]] = 0
    oh = np.zeros(q.shape + (yo_ld,), F32)
    np.put_along_axis(oh, q[..., None].astype(np.int64), F32(1), axis=-1)
    return q, O.interp_apply(case['mel'], i0, lam, nrows), oh, f


# ------------------------------------------------------------------------------------------------ scatter
def scatter_ref(dy, i0, lam, nrows, T):
    """float64 sums of the kernel's terms, sum|terms| and the number of terms, each [B][T][C] ([B][T] for the count)"""
    B, P, C = dy.shape
    ref, mag, cnt = np.zeros((B, T, C)), np.zeros((B, T, C)), np.zeros((B, T), np.int64)
    one = F32(1)
    for b in range(B):
        for r in range(int(nrows[b])):
            i, l = int(i0[b, r]), lam[b, r]
            for frame, w in ((i, float(one - l)), (i + 1, float(l))):
                t = w * dy[b, r].astype(np.float64)
                ref[b, frame] += t
                mag[b, frame] += np.abs(t)
                cnt[b, frame] += 1
    return ref, mag, cnt


def scatter_budget(mag, cnt):
    return cnt[:, :, None] * U * mag


def scatter_emulated(dy, i0, lam, nrows, T, start=None, swap=False, drop=None):
    """the kernel's order: per frame, rows with i0 == i ascending (weight 1 - lam), then rows with i0 == i - 1 (weight lam), one fp32 chain
    of fused multiply-adds (emulated as a float64 product-and-sum rounded to fp32: the product is exact, the float64 sum adds a rounding of
    2^-53 relative, nothing beside the budget).  Mutants: swap (neighbour weights exchanged), start (an inverse map given from outside: off by
    one), drop = (b, r) (one contributing row left out)."""
    B, P, C = dy.shape
    st = O.interp_start(i0, nrows, T) if start is None else start
    dx = np.zeros((B, T, C), F32)
    one = F32(1)
    for b in range(B):
        for i in range(T):
            acc = np.zeros(C, F32)
            a0, a1 = st[b, i], st[b, i + 1]
            b0, b1 = (st[b, i - 1], a0) if i > 0 else (0, 0)
            for lo, hi, first in ((a0, a1, True), (b0, b1, False)):
                for r in range(lo, hi):
                    if drop == (b, r):
                        continue
                    w = (one - lam[b, r]) if first != swap else lam[b, r]
                    acc = (float(w) * dy[b, r].astype(np.float64) + acc.astype(np.float64)).astype(F32)
            dx[b, i] = acc
    return dx
