"""Every GEMM descriptor feature in isolation against float64 (pytest -m gpu): ss_op_gemm_desc / ss_op_gemm_img_desc hand a whole GemmDesc /
ImgGemmDesc to launch_gemm / launch_gemm_img, and tests/gemm_ref.py restates the descriptor on the same flat buffers.

Every result is judged per element, twice (gemm_ref's docstring derives both bars): SHARP against the float64 contraction of the family's
rounded pieces, bar (k_len + ksplit + 2 [+ 8 for bf16 x 3]) * 2^-24 * (sum |a||b| + |bias| + |C0|); HONEST against the float64 product of the
unrounded operands, 5e-6 (bf16 x 1: 1e-2) of min(max |ref|, sum |a||b| + ...).  Every element of the C buffer outside the write set must keep
its bits.  Operand rows are scaled by powers of two over 2^6 on each side, so the magnitudes of one result span 2^12 and a max-norm would hide
the small rows and columns.  The input buffers hold NaN wherever the descriptor does not point; C holds NaNs and distinct values beforehand.

Families of launch_gemm: 'bf16x3' (default), 'f16x2', 'bf16', and 'f32' = ss_tune("gemm_mode", 0), the fp32-MFMA kernel in its vector-load
form.  Whatever launch_gemm sends to the fp32-MFMA kernel in mode 1 (A reduction-major with B K-contiguous, unaligned operands, segments
shorter than a k-tile) is judged as that kernel computes: fp32 products, bf16-rounded under GEMM_BF16.

Each test prints `FIG <test> <case> sharp=<worst ratio> honest=<worst ratio>` (1.0 = at the bar)."""
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import gemm_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu
F32 = np.float32
LAYOUTS = {'NT': (False, False), 'NN_tb': (False, True), 'TN': (True, True), 'TA_only': (True, False)}
FAMILIES = ('bf16x3', 'f16x2', 'bf16', 'f32')


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


class Tuned:
    """ss_tune values for the duration of a block, back at the defaults afterwards whatever happens."""
    DEFAULTS = {'gemm_mode': 1, 'gemm_want': 1024, 'gemm_ws': 0, 'gemm_tr': 1, 'gemm_pipe': 1}

    def __init__(self, E, **kv):
        self.E, self.kv = E, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.E.tune(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.E.tune(k, self.DEFAULTS[k])


def r8(n):
    return -(-n // 8) * 8


def dense(rows, cols, batch=1, off=8, pad=8, gap=16):
    ld = r8(cols) + pad
    return (off, ld, rows * ld + gap if batch > 1 else 0, 0, 0)


def scaled(rng, X, K, spread=6):
    return (rng.standard_normal((X, K)) * 2.0 ** -rng.integers(0, spread + 1, (X, 1))).astype(F32)


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(M, N, K, layout, batch=1, ksplit=1, accum=False, c0='zero', bias=False, shared_b=False, ageom=None, bgeom=None, cgeom=None,
            row_mask=(0, 0, 0, 0), rm=(0, 0), a_scale=1.0, slab_a=False, slab_b=False, seed=0):
    """The descriptor and its buffers, made once per case and never changed.  Geometries: (off, ld, bstride, seglen, segstride)."""
    ta, tb = LAYOUTS[layout]
    rng = np.random.default_rng(zlib.crc32(repr((M, N, K, layout, batch, ksplit, seed)).encode()))
    ageom = ageom or dense(K if ta else M, M if ta else K, batch)
    bgeom = bgeom or dense(K if tb else N, N if tb else K, 1 if shared_b else batch, off=16)
    c_rows = M if rm[0] <= 0 else (M // rm[0]) * rm[1]
    cgeom = cgeom or (4, N + 4, c_rows * (N + 4) + 12 if batch > 1 else 0)
    p = Problem()
    p.d = R.Desc(R.Geom(*ageom), R.Geom(*bgeom), cgeom[0], cgeom[1], cgeom[2], M, N, K, batch, ta, tb, accum=accum or ksplit > 1, row_mask=row_mask, rm=rm,
                 ksplit=ksplit)
    na, nb, nc = R.spans(p.d)
    p.a, p.b = np.full(na, np.nan, F32), np.full(nb, np.nan, F32)
    if slab_a:                                              # overlapping rows: the slab itself is the data
        p.a[:] = (rng.standard_normal(na) * 2.0 ** -rng.integers(0, 7, na)).astype(F32)
    else:
        p.a[R.a_index(p.d).reshape(-1)] = (np.stack([scaled(rng, M, K) for _ in range(batch)]) * F32(a_scale)).reshape(-1)
    if slab_b:
        p.b[:] = (rng.standard_normal(nb) * 2.0 ** -rng.integers(0, 7, nb)).astype(F32)
    else:
        nbm = 1 if shared_b or batch == 1 else batch
        p.b[R.b_index(p.d)[:nbm].reshape(-1)] = np.stack([scaled(rng, N, K) for _ in range(nbm)]).reshape(-1)
    p.bias = (0.05 * scaled(rng, 1, N)[0]) if bias else None
    p.c0 = (rng.standard_normal(nc) * 3).astype(F32)
    p.c0[::7] = np.nan                                      # prior bits that must survive include NaNs
    p.c0[3::11] = np.asarray(0x7FC12345, np.uint32).view(F32)
    idx = R.c_index(p.d)[:, R.written_rows(p.d)].reshape(-1)
    if p.d.accum:
        p.c0[idx] = rng.standard_normal(idx.size).astype(F32) * F32(a_scale) if c0 == 'rand' else 0
    return p


def vec_ok(g):
    """gemm_f32.hip's vec_ok: the buffers themselves start on 256-byte boundaries."""
    return g.off % 4 == 0 and g.ld % 4 == 0 and g.bstride % 4 == 0 and g.seglen % 4 == 0 and g.segstride % 4 == 0


def judged_as(family, d):
    """(family the result is judged as, k-tile): launch_gemm's choice between its two kernels, restated."""
    seg_ok = all(g.seglen == 0 or g.seglen >= 32 for g in (d.A, d.B))
    f32k = family == 'f32' or (d.ta and not d.tb) or not (vec_ok(d.A) and vec_ok(d.B)) or not seg_ok
    if f32k:
        return ('bf16' if family == 'bf16' else 'f32'), 16
    return family, 32


def bf16_band(fam, d, fig, tag):
    """The lower edge of test_gemm_bf16_mode's band: a bf16 x 1 result that is closer than 1e-4 (max-norm) to the product of the UNROUNDED
    operands did not round them.  Each operand carries a relative error uniform in +-2^-9 (rms 1.1e-3), a product 1.6e-3; over K terms of
    random sign the largest elements are off by ~1.6e-3 sqrt(K) sigma against max |ref| ~ 3 sqrt(K) sigma: ~5e-4.  Asserted where there are
    enough terms and elements for that estimate (K >= 8, M N >= 64)."""
    if fam == 'bf16' and d.K >= 8 and d.M * d.N >= 64:
        assert fig['maxnorm'] > 1e-4, (tag, fig)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def word(v):
    return torch.tensor([v], dtype=torch.float32, device='cuda')


def launch(E, p, family, *, want=0, part=None, amax=(None, None), pre_scale=(None, None), imgs=(None, None), guard=False, sa=16.0, sb=16.0,
           tag='', bits_of=None, ref=None):
    """One ss_op_gemm_desc launch of problem p judged against gemm_ref; returns the C buffer (numpy).  amax / pre_scale: python floats that
    are put behind device words; imgs: scales to split the operand images with (None: no image); guard: A, B, C, the images and the partial
    slabs end where guard memory begins; ref: reference_of(...) of the same case, where a caller launches it more than once."""
    d = p.d
    fam, kt = judged_as(family, d)
    ref = ref or reference_of(p, family, sa, sb)
    if guard:
        ga, gb, gc = G.inp(torch.from_numpy(p.a), 'cuda', name='A'), G.inp(torch.from_numpy(p.b), 'cuda', name='B'), \
            G.out((p.c0.size,), 'cuda', fill=torch.from_numpy(p.c0), name='C')
        a, b, c = ga.t, gb.t, gc.t
    else:
        a, b, c = dev(p.a), dev(p.b), dev(p.c0)
    ai = None if imgs[0] is None else torch.from_numpy(R.pack_image(np.concatenate([p.a, np.zeros(-p.a.size % 8, F32)]), imgs[0]).view(F32).reshape(-1))
    bi = None if imgs[1] is None else torch.from_numpy(R.pack_image(np.concatenate([p.b, np.zeros(-p.b.size % 8, F32)]), imgs[1]).view(F32).reshape(-1))
    pt = None
    extra = []
    if guard:
        gi = [None if x is None else G.inp(x, 'cuda', name=n) for x, n in ((ai, 'A image'), (bi, 'B image'))]
        extra = [g for g in gi if g is not None]
        ai, bi = (None if g is None else g.t for g in gi)
        assert all(g.t.data_ptr() % 32 == 0 for g in extra)          # (an image off its 32-byte alignment would be refused, not read)
        if part:
            gp = G.out((d.batch * d.ksplit * d.M * d.N,), 'cuda', fill=float('nan'), name='partial slabs')
            extra.append(gp)
            pt = gp.t
    else:
        ai, bi = (None if x is None else x.cuda() for x in (ai, bi))
        if part:
            pt = torch.full((d.batch * d.ksplit * d.M * d.N,), float('nan'), device='cuda')
    with Tuned(E, gemm_mode=0 if family == 'f32' else 1, gemm_want=want if want > 0 else 1024):
        E.reset_variants()                                  # a caller that reads ss_debug_last_variant afterwards reads THIS launch's record
        E.gemm_desc(a, d.A.tuple(), b, d.B.tuple(), c, (d.c_off, d.ldc, d.cstride), d.M, d.N, d.K, batch=d.batch, ta=d.ta, tb=d.tb, accumulate=d.accum,
                    bf16=family == 'bf16', f16x2=family == 'f16x2', bias=dev(p.bias), want=want, row_mask=d.row_mask, ksplit=d.ksplit,
                    amax_a=None if amax[0] is None else word(amax[0]), amax_b=None if amax[1] is None else word(amax[1]), a_img=ai, b_img=bi,
                    a_pre_scale=None if pre_scale[0] is None else word(pre_scale[0]), b_pre_scale=None if pre_scale[1] is None else word(pre_scale[1]),
                    part=pt)
        torch.cuda.synchronize()
    if guard:
        G.check_all([ga, gb, gc] + extra)
    out = c.cpu().numpy()
    fails, fig = R.judge(ref, p.c0, out)
    print(f'FIG {tag} family={family} judged_as={fam} want={want} sharp={fig["sharp"]:.3g} honest={fig["honest"]:.3g} untouched={fig["untouched"]}')
    assert not fails, (tag, family, fails, fig)
    bf16_band(fam, d, fig, tag)
    if bits_of is not None:
        assert np.array_equal(out.view(np.uint32), bits_of.view(np.uint32)), (tag, 'bits differ')
    return out


def reference_of(p, family, sa=16.0, sb=16.0):
    """gemm_ref's expected values of problem p as launch_gemm's kernel of `family` computes them."""
    fam, kt = judged_as(family, p.d)
    return R.reference(p.d.replace(family=fam, kt=kt, sa=sa, sb=sb), p.a, p.b, p.c0, p.bias)


def wants(M, N, batch=1, ksplit=1):
    """`want` values that make launch_layout pick 128 x 128, 128 x 64 and 64 x 64 (where the shape admits them)."""
    t = lambda bm, bn: -(-M // bm) * -(-N // bn) * batch * ksplit
    w = [1 << 30]
    if M > 64 and t(128, 64) > t(128, 128):
        w.append(t(128, 128) + 1)
    if M > 64 and N > 64:
        w.append(1)
    return w


SHAPES = ((65, 65), (130, 132), (136, 264), (1, 64), (63, 1), (64, 63))


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('family', FAMILIES)
def test_layouts_tiles_and_shapes(E, family, layout):
    """All four layouts (A reduction-major with B K-contiguous included: it must WORK in every mode), every tile through `want` (the
    fp32-MFMA kernel takes its tile from ss_tune("gemm_want")), M x N at and around the tile edges."""
    for M, N in SHAPES:
        p = problem(M, N, 40, layout)
        for w in wants(M, N):
            launch(E, p, family, want=w, tag=f'layouts {layout} {M}x{N}x40')


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('family', FAMILIES)
def test_k_and_split_k(E, family, layout):
    """K at and around the k-tiles, split-K 1, 2, 3 and 5 (empty slices) through atomics and through ordered partial slabs (bits identical
    over two runs), a small bias with a split (added once), ACCUM onto a random C0 without one."""
    M, N = 72, 68
    for K in (1, 8, 31, 32, 33, 72, 100):
        for ks in (1, 2, 3, 5):
            p = problem(M, N, K, layout, ksplit=ks)
            tag = f'ksplit {layout} {M}x{N}x{K} ks={ks}'
            launch(E, p, family, want=1, tag=tag + ' atomics')
            if ks > 1:
                first = launch(E, p, family, want=1, part=True, tag=tag + ' part')
                if judged_as(family, p.d)[1] == 32:         # the kernel with the partial slabs: a fixed order
                    launch(E, p, family, want=1, part=True, tag=tag + ' part again', bits_of=first)
    for ks in (2, 3):
        launch(E, problem(M, N, 100, layout, ksplit=ks, bias=True), family, tag=f'ksplit {layout} bias ks={ks}')
        launch(E, problem(M, N, 100, layout, ksplit=ks, bias=True), family, part=True, tag=f'ksplit {layout} bias part ks={ks}')
    launch(E, problem(M, N, 100, layout, accum=True, c0='rand', bias=True), family, tag=f'ksplit {layout} accum onto C0')
    launch(E, problem(M, N, 100, layout, ksplit=3, c0='rand'), family, part=True, tag=f'ksplit {layout} ks=3 part onto C0')


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('family', FAMILIES)
def test_alignment_paths(E, family, layout):
    """Transposing reads off (an extent that is no multiple of 4 on an aligned base) and the scalar fallback (base off by 4 bytes, ld % 4 != 0)."""
    ta, tb = LAYOUTS[layout]
    for M, N in ((130, 132), (134, 131)):
        for w in wants(M, N):
            launch(E, problem(M, N, 40, layout), family, want=w, tag=f'align {layout} {M}x{N} quad')
    M, N, K = 130, 132, 40
    ra, rb = (K, M) if ta else (M, K), (K, N) if tb else (N, K)      # (rows, columns) as stored
    for name, ag, bg in (('A base + 4 B', (9, r8(ra[1]) + 8, 0, 0, 0), None), ('B base + 4 B', None, (13, r8(rb[1]) + 8, 0, 0, 0)),
                         ('lda % 4 = 1', (8, r8(ra[1]) + 5, 0, 0, 0), None), ('ldb % 4 = 2', None, (8, r8(rb[1]) + 6, 0, 0, 0))):
        p = problem(M, N, K, layout, ageom=ag, bgeom=bg)
        assert judged_as(family, p.d)[1] == 16
        for w in wants(M, N):                              # the scalar instances of all three tiles
            launch(E, p, family, want=w, tag=f'align {layout} {name}')
        launch(E, problem(M, N, 100, layout, ksplit=3, bias=True, ageom=ag, bgeom=bg), family, tag=f'align {layout} {name} ks=3 bias')


def conv_problem(Ci, N=48, B=3, T=40, pad=0, **kw):
    """The k = 5 convolution over haloed slabs [B][T + 4][Ci] read as ONE matrix with overlapping rows: A K-contiguous, seglen = Ci, segstride = ld."""
    ld = Ci + pad
    return problem(B * (T + 4) - 4, N, 5 * Ci, 'NT', ageom=(8, ld, 0, Ci, ld), slab_a=True, **kw)


def wgrad_problem(Ci, Co=72, R_=128, pad=0, **kw):
    """The conv weight gradient: dW[tap * Ci + ci][co] = sum_r x[r + tap][ci] dy[r][co] -- TN, A reduction-major with segmented COLUMNS."""
    ld = Ci + pad
    return problem(5 * Ci, Co, R_, 'TN', ageom=(8, ld, 0, Ci, ld), slab_a=True, **kw)


@pytest.mark.parametrize('family', FAMILIES)
def test_segments(E, family):
    for Ci in (32, 64):
        for pad in (0, 8):
            for w in wants(128, 48):
                launch(E, conv_problem(Ci, pad=pad), family, want=w, tag=f'segments conv Ci={Ci} ld={Ci + pad}')
            for w in wants(5 * Ci, 72):
                launch(E, wgrad_problem(Ci, pad=pad), family, want=w, tag=f'segments wgrad Ci={Ci} ld={Ci + pad}')
        launch(E, conv_problem(Ci, bias=True, ksplit=2), family, want=1, tag=f'segments conv Ci={Ci} ks=2 bias')
        launch(E, wgrad_problem(Ci, ksplit=3), family, want=1, part=True, tag=f'segments wgrad Ci={Ci} ks=3 part')
    # seglen 16: shorter than the 32-wide k-tile, so launch_gemm must send it to the fp32-MFMA kernel (seg_ok) -- and the result must hold
    for prob in (conv_problem(16), wgrad_problem(16), conv_problem(16, ksplit=2)):
        assert judged_as(family, prob.d)[1] == 16
        launch(E, prob, family, want=1, tag='segments seglen=16')


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('family', FAMILIES)
def test_batches(E, family, layout):
    """batch 3 with bstride / cstride larger than a dense matrix, B shared (bstride 0), batch 2 x ksplit 3 through partial slabs."""
    for w in wants(72, 68, 3):
        launch(E, problem(72, 68, 40, layout, batch=3, bias=True), family, want=w, tag=f'batch {layout} 3')
        launch(E, problem(72, 68, 40, layout, batch=3, shared_b=True), family, want=w, tag=f'batch {layout} 3 shared B')
    p = problem(72, 68, 100, layout, batch=2, ksplit=3)
    first = launch(E, p, family, want=1, part=True, tag=f'batch {layout} 2 ks=3 part')
    if judged_as(family, p.d)[1] == 32:
        launch(E, p, family, want=1, part=True, tag=f'batch {layout} 2 ks=3 part again', bits_of=first)
    launch(E, p, family, want=1, tag=f'batch {layout} 2 ks=3 atomics')


@pytest.mark.parametrize('family', FAMILIES)
def test_row_mask_over_haloed_slabs(E, family):
    """4 utterances of T = 36 in slabs of TP = 40 rows contracted as ONE matrix of 4 * 40 - 4 rows: a 64-row and a 128-row tile cut both fall
    inside an utterance; the halo rows keep their bits (C is pre-filled with distinct patterns, NaNs among them)."""
    M, mask = 4 * 40 - 4, (40, 2, 2, 38)
    for layout in ('NT', 'NN_tb'):
        for w in wants(M, 72):
            launch(E, problem(M, 72, 40, layout, row_mask=mask, bias=True), family, want=w, tag=f'mask {layout}')
        launch(E, problem(M, 72, 40, layout, row_mask=mask, accum=True, c0='rand'), family, want=1, tag=f'mask {layout} accum')
        launch(E, problem(M, 72, 100, layout, row_mask=mask, ksplit=3), family, want=1, part=True, tag=f'mask {layout} ks=3 (part given)')
    launch(E, conv_problem(32, B=4, T=36, row_mask=mask, bias=True), family, want=1, tag='mask conv')


@pytest.mark.parametrize('layout', ['NT', 'NN_tb', 'TN'])
def test_measured_and_fixed_scales(E, layout):
    """fp16 x 2: amax words at 2^-30, 1, 250 and 2^20 of an operand scaled to match; amax 0 with a zero operand; fixed scales 4 and 64 with
    matching images; an image that is offered but not usable (K % 8 != 0) -- the in-loop split with the same scale, equal to the sharp bar."""
    ta, tb = LAYOUTS[layout]
    for s in (2.0 ** -30, 1.0, 250.0 / 4, 2.0 ** 20):
        p = problem(72, 136, 72, layout, a_scale=s, seed=1)
        amax = float(np.nanmax(np.abs(p.a)))
        for w in wants(72, 136):
            launch(E, p, 'f16x2', want=w, amax=(amax, None), sa=R.pow2_scale_of(amax), tag=f'amax {layout} A at {s:g}')
        pg = problem(72, 136, 72, layout, a_scale=s, seed=1, ksplit=2, c0='rand')
        launch(E, pg, 'f16x2', want=1, amax=(amax, 4.0), sa=R.pow2_scale_of(amax), sb=R.pow2_scale_of(4.0), part=True, tag=f'amax {layout} both, ks=2')
    pz = problem(72, 136, 72, layout, a_scale=0.0)
    out = launch(E, pz, 'f16x2', amax=(0.0, None), sa=R.pow2_scale_of(0.0), tag=f'amax {layout} zero operand')
    assert not np.isnan(out[R.c_index(pz.d).reshape(-1)]).any() and not out[R.c_index(pz.d).reshape(-1)].any()
    for s in (4.0, 64.0):
        p = problem(136, 136, 72, layout)
        for w in wants(136, 136):
            launch(E, p, 'f16x2', want=w, pre_scale=(s, None), sa=s, tag=f'pre_scale {layout} A {s:g} in-loop')
            launch(E, p, 'f16x2', want=w, pre_scale=(s, s), imgs=(s, s), sa=s, sb=s, tag=f'pre_scale {layout} {s:g} both images')
            launch(E, p, 'f16x2', want=w, pre_scale=(None, s), imgs=(None, s), sb=s, tag=f'pre_scale {layout} {s:g} B image')
        q = problem(136, 136, 68, layout)                   # K % 8 != 0: a K-contiguous operand's image cannot be taken
        launch(E, q, 'f16x2', want=1, pre_scale=(s, s), imgs=(s, s), sa=s, sb=s, tag=f'pre_scale {layout} {s:g} images offered, K = 68')


@pytest.mark.parametrize('family', FAMILIES)
def test_inside_guard_memory(E, family):
    """One case per family and feature group with A, B and C flush against guard memory (tests/guarded.py)."""
    mask = (40, 2, 2, 38)
    for tag, p, kw in (('layout', problem(130, 132, 40, 'TN'), dict(want=1)), ('ta only', problem(65, 65, 40, 'TA_only'), {}),
                       ('split', problem(72, 68, 100, 'NN_tb', ksplit=3), dict(part=True, want=1)), ('conv', conv_problem(32, bias=True), dict(want=1)),
                       ('wgrad', wgrad_problem(32), dict(want=1)), ('batch', problem(72, 68, 40, 'NT', batch=3, shared_b=True), {}),
                       ('mask', problem(156, 72, 40, 'NT', row_mask=mask, bias=True), dict(want=1))):
        launch(E, p, family, guard=True, tag=f'guard {tag}', **kw)


# ---- the image GEMM ---------------------------------------------------------------------------------------------------------------------
def launch_img(E, p, *, bf16=False, cfg=-1, part=False, scales=(None, None), guard=False, tag='', bits_of=None):
    """One ss_op_gemm_img_desc launch of problem p; the images are packed by gemm_ref from p's fp32 buffers."""
    d = p.d
    sa, sb = (16.0 if s is None else s for s in scales)
    ref = R.reference(d.replace(family='bf16' if bf16 else 'f16x2', kt=64 if bf16 else 32, sa=sa, sb=sb), p.a, p.b, p.c0, p.bias)
    pad = lambda x: np.concatenate([x, np.zeros(-x.size % 8, F32)])
    if bf16:
        ia, ib = (torch.from_numpy(R.pack_bf16(pad(x)).view(np.int16)).view(torch.bfloat16) for x in (p.a, p.b))
    else:
        ia, ib = (torch.from_numpy(R.pack_image(pad(x), s).view(F32).reshape(-1)) for x, s in ((p.a, sa), (p.b, sb)))
    if guard:
        ga, gb, gc = G.inp(ia, 'cuda', name='A image'), G.inp(ib, 'cuda', name='B image'), G.out((p.c0.size,), 'cuda', fill=torch.from_numpy(p.c0), name='C')
        a, b, c = ga.t, gb.t, gc.t
    else:
        a, b, c = ia.cuda(), ib.cuda(), dev(p.c0)
    pt = torch.full((d.batch * d.ksplit * d.M * d.N,), float('nan'), device='cuda') if part else None
    E.gemm_img_desc(a, d.A.tuple(), b, d.B.tuple(), c, (d.c_off, d.ldc, d.cstride), d.M, d.N, d.K, batch=d.batch, ta=d.ta, tb=d.tb, accumulate=d.accum,
                    bias=dev(p.bias), row_mask=d.row_mask, rm=d.rm, ksplit=d.ksplit, part=pt, scale_a=None if scales[0] is None else word(scales[0]),
                    scale_b=None if scales[1] is None else word(scales[1]), cfg=cfg)
    torch.cuda.synchronize()
    if guard:
        G.check_all([ga, gb, gc])
    out = c.cpu().numpy()
    fails, fig = R.judge(ref, p.c0, out)
    print(f'FIG {tag} img {"bf16" if bf16 else "f16x2"} cfg={cfg} sharp={fig["sharp"]:.3g} honest={fig["honest"]:.3g} untouched={fig["untouched"]}')
    assert not fails, (tag, fails, fig)
    bf16_band('bf16' if bf16 else 'f16x2', d, fig, tag)
    if bits_of is not None:
        assert np.array_equal(out.view(np.uint32), bits_of.view(np.uint32)), (tag, 'bits differ')
    return out


def img_problem(M, N, K, layout, batch=1, **kw):
    """Image operands: bases 32-byte aligned, strides multiples of 8 elements."""
    ta, tb = LAYOUTS[layout]
    return problem(M, N, K, layout, batch=batch, ageom=kw.pop('ageom', None) or dense(K if ta else M, M if ta else K, batch, off=8, gap=16),
                   bgeom=kw.pop('bgeom', None) or dense(K if tb else N, N if tb else K, 1 if kw.get('shared_b') else batch, off=16, gap=24), **kw)


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('bf16', [False, True], ids=['f16x2', 'bf16'])
def test_img_layouts_and_tiles(E, bf16, layout):
    """cfg 0, 1 and 2 (256 x 256, 128 x 128, 256 x 128) on a shape with more than one tile and ragged edges, all four layouts, both forms;
    split-K 2 and 3 through the partial slabs, bias, accumulate, a batch with cstride."""
    K = 128 if bf16 else 96
    for cfg in (0, 1, 2, 3):                                # 3: 256 x 128 on two slots
        launch_img(E, img_problem(264, 136, K, layout, bias=True), bf16=bf16, cfg=cfg, tag=f'img {layout} 264x136x{K}')
        launch_img(E, img_problem(136, 264, K, layout, accum=True, c0='rand'), bf16=bf16, cfg=cfg, tag=f'img {layout} 136x264x{K} accum')
    for ks in (2, 3):
        p = img_problem(136, 136, 4 * K, layout, ksplit=ks, bias=True, c0='rand')
        first = launch_img(E, p, bf16=bf16, cfg=1, part=True, tag=f'img {layout} ks={ks} bias onto C0')
        launch_img(E, p, bf16=bf16, cfg=1, part=True, tag=f'img {layout} ks={ks} again', bits_of=first)
    launch_img(E, img_problem(136, 72, K, layout, batch=3, bias=True), bf16=bf16, cfg=1, tag=f'img {layout} batch 3')
    launch_img(E, img_problem(136, 72, K, layout, batch=3, shared_b=True), bf16=bf16, cfg=2, tag=f'img {layout} batch 3 shared B')
    launch_img(E, img_problem(136, 72, 4 * K, layout, batch=2, ksplit=2), bf16=bf16, cfg=1, part=True, tag=f'img {layout} batch 2 ks=2')


@pytest.mark.parametrize('bf16', [False, True], ids=['f16x2', 'bf16'])
def test_img_tn_partial_k_tile_through_zeros(E, bf16):
    for K in (72, 40, 8):
        for cfg in (0, 1, 2):
            launch_img(E, img_problem(136, 136, K, 'TN'), bf16=bf16, cfg=cfg, tag=f'img TN K={K} zeros')
    launch_img(E, img_problem(136, 136, 200, 'TN', ksplit=2), bf16=bf16, cfg=1, part=True, tag='img TN K=200 ks=2 zeros')


def test_img_scale_words(E):
    for layout in LAYOUTS:
        for sa, sb in ((4.0, 64.0), (64.0, 4.0), (None, 4.0)):
            launch_img(E, img_problem(136, 136, 96, layout), scales=(sa, sb), cfg=1, tag=f'img {layout} scales {sa} {sb}')


@pytest.mark.parametrize('bf16', [False, True], ids=['f16x2', 'bf16'])
def test_img_segments(E, bf16):
    """Segmented A for the convolution (K-contiguous, seglen = Ci, segstride = ld) and segmented columns of a reduction-major operand (the
    weight-gradient form), for A and for B."""
    for Ci in (64, 128):
        for cfg in (1, 2):
            launch_img(E, conv_problem(Ci, N=72, bias=True), bf16=bf16, cfg=cfg, tag=f'img conv Ci={Ci}')
        launch_img(E, conv_problem(Ci, N=72, pad=8), bf16=bf16, cfg=1, tag=f'img conv Ci={Ci} ld={Ci + 8}')
    if not bf16:
        launch_img(E, conv_problem(32, N=72), cfg=1, tag='img conv Ci=32')
    for Ci in (8, 32):
        launch_img(E, wgrad_problem(Ci, pad=8), bf16=bf16, cfg=1, tag=f'img wgrad Ci={Ci} (A columns segmented)')
        launch_img(E, wgrad_problem(Ci, ksplit=2), bf16=bf16, cfg=1, part=True, tag=f'img wgrad Ci={Ci} ks=2')
        # the same with the roles swapped: B reduction-major with segmented columns
        launch_img(E, problem(72, 5 * Ci, 128, 'TN', bgeom=(8, Ci + 8, 0, Ci, Ci + 8), slab_b=True), bf16=bf16, cfg=1, tag=f'img B columns segmented Ci={Ci}')


def same_data(base, other):
    """other's descriptor over base's buffers (the cached problems stay as they are)."""
    assert other.a.size == base.a.size and other.b.size == base.b.size and other.c0.size == base.c0.size
    q = Problem()
    q.d, q.a, q.b, q.c0, q.bias = other.d, base.a, base.b, base.c0, base.bias
    return q


@pytest.mark.parametrize('U', [4, 8])
@pytest.mark.parametrize('bf16', [False, True], ids=['f16x2', 'bf16'])
def test_img_row_map_equals_batch_and_row_mask(E, bf16, U):
    """rm_T = 36, rm_TP = 40 over 4 and 8 utterances (a 128-row and a 256-row cut inside an utterance), against the same contraction given as a
    batch of T rows and as a row mask over the slab: the written elements bit-identical, the halo rows untouched in all three."""
    T, TP, N, K = 36, 40, 72, 128
    lda, ldc = K + 8, N + 4
    ao, co = 8 + 2 * lda, 4 + 2 * ldc                        # the first real row of the first slab
    b_at = (16, K + 8, 0, 0, 0)
    for cfg in (0, 1, 2):
        base = problem(U * T, N, K, 'NT', ageom=(ao, lda, 0, 0, 0), bgeom=b_at, cgeom=(co, ldc, 0), rm=(T, TP), bias=True, seed=U)
        out = launch_img(E, base, bf16=bf16, cfg=cfg, tag=f'img rowmap U={U}')
        as_batch = problem(T, N, K, 'NT', batch=U, shared_b=True, ageom=(ao, lda, TP * lda, 0, 0), bgeom=b_at, cgeom=(co, ldc, TP * ldc), bias=True, seed=U)
        as_mask = problem(U * TP - 4, N, K, 'NT', ageom=(ao, lda, 0, 0, 0), bgeom=b_at, cgeom=(co, ldc, 0), row_mask=(TP, 0, 0, T), bias=True, seed=U)
        as_batch, as_mask = (same_data(base, other) for other in (as_batch, as_mask))
        launch_img(E, as_batch, bf16=bf16, cfg=cfg, tag=f'img rowmap U={U} as batch', bits_of=out)
        got = launch_img(E, as_mask, bf16=bf16, cfg=cfg, tag=f'img rowmap U={U} as row mask')
        assert np.array_equal(got.view(np.uint32), out.view(np.uint32))
    ks = problem(U * T, N, 4 * K, 'NT', ageom=(8 + 2 * (4 * K + 8), 4 * K + 8, 0, 0, 0), cgeom=(co, ldc, 0), rm=(T, TP), ksplit=3, bias=True)
    launch_img(E, ks, bf16=bf16, cfg=1, part=True, tag=f'img rowmap U={U} ks=3')


@pytest.mark.parametrize('bf16', [False, True], ids=['f16x2', 'bf16'])
def test_img_inside_guard_memory(E, bf16):
    K = 128 if bf16 else 96
    for tag, p, kw in (('layout', img_problem(264, 136, K, 'TN', bias=True), dict(cfg=2)), ('ta only', img_problem(136, 136, K, 'TA_only'), dict(cfg=1)),
                       ('split', img_problem(136, 136, 4 * K, 'NN_tb', ksplit=3), dict(cfg=1, part=True)), ('conv', conv_problem(64, N=72), dict(cfg=1)),
                       ('batch', img_problem(136, 72, K, 'NT', batch=3, shared_b=True), dict(cfg=1)),
                       ('rowmap', problem(4 * 36, 72, 128, 'NT', ageom=(8 + 2 * 136, 136, 0, 0, 0), cgeom=(4 + 2 * 76, 76, 0), rm=(36, 40)), dict(cfg=1))):
        launch_img(E, p, bf16=bf16, guard=True, tag=f'img guard {tag}', **kw)


def test_split_image_bytes(E):
    """ss_op_split_image against gemm_ref.pack_image byte for byte: scales 4, 16 and 64, a dense matrix and a row-strided view."""
    rng = np.random.default_rng(7)
    x = scaled(rng, 70, 96)
    x[0, :8] = [1.0, 1.0 + 2.0 ** -11, -1.0 - 3 * 2.0 ** -12, 0.0, 1e-7, 255.0, -0.3, 2.0 ** -14]
    xd = dev(x)
    for s in (4.0, 16.0, 64.0):
        want = R.pack_image(x.reshape(-1), s).view(F32).reshape(70, 96)
        got = E.split_image(xd, s).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), s
        wide = torch.full((70, 128), float('nan'), device='cuda')
        wide[:, 16:112] = xd
        out = torch.zeros(70, 136, device='cuda')
        got = E.split_image(wide[:, 16:112], s, out=out[:, 8:104]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s, 'strided')
