"""The re-layout and guard kernels of a training step -- conv_pack / _many / _dx, conv_unpack_grad[s] plain and accumulating, prep_run,
transpose2d, copy_rows with and without len, act_scales and param_guard -- each launched alone through its engine-free hook (ss_op_conv_pack
/ _many / _dx, ss_op_conv_unpack / _many, ss_op_prep, ss_op_transpose, ss_op_copy_rows, ss_op_act_scales, ss_op_param_guard) on guarded
buffers (tests/guarded.py: NaN guard bands, row strides above the width, odd offsets wherever the kernel allows them) and compared BIT FOR BIT
with tests/relayout_ref.py.  Every one of these kernels is exact, so the budget is zero differing bits; tests/test_relayout_ref_selftest.py
shows that bit equality tells the named wrong kernels from a right one.

  conv_pack      (Co, Ci, Cp) in (4,1,4) (8,3,4) (64,5,8) (512,80,80) (512,81,84): wf with its zero padding, wb with flipped taps, both images in
                 format v2 (equal to ss_op_split_image of the fp32 pack) and as bf16 (the rounding of the pack), wb == NULL, the many form
                 against the single one, conv_pack_dx against wb and on shapes no multiple of 4
  conv_unpack    the same shapes, padding columns of the pack holding NaN; plain, accumulating onto a non-zero arena, many
  prep           tasks on the float4 path and on the scalar path (n % 4 != 0; a misaligned operand), b null and given, -0.0, a NaN payload,
                 images in both formats, more than one sweep of the grid, a full table of 48 tasks
  transpose      R, C in {1, 31, 32, 33, 257}
  copy_rows      dense -> slab and slab -> dense, C in {1, 80, 83}, one shape beyond a sweep of the grid; len in {0, mid, T, above T, negative}
                 with NaN in the source rows behind it; halo rows keep their bits
  act_scales     C in {64, 100, 512}, the extreme in the last element; bounds exactly 2048, just above, huge, +inf and overflow (16 is kept),
                 NaN elements; an absent block (C = 0); T = 64 and 192
  param_guard    n in {4, 1024, 4 * 131072 + 4}; one bad element first / middle / last: NaN, +-inf, +-limit; just below the limit is good;
                 the other bits of the word stay; a clean arena leaves the word as it was

BUGS these tests exposed, fixed with them: (1) prep_kernel's scalar path copied as a + 0.f, which turns -0.0 into +0.0 while the float4 path
copies bits -- test_prep measured one differing element per -0.0 of every scalar-path copy; the scalar path now adds only when b is given.
(2) act_scale_kernel's comment said a non-finite bound keeps 16, its loop ran +inf down to 2^-20; the code now keeps 16 (see the header).

Each test prints `FIG <test> <case> <differing elements>` (budget 0)."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import relayout_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
HALO_FILL = -7.25
NAN = np.array([G.NAN32], np.uint32).view(F32)[0]
ODD = 67                                                    # an odd element offset: 4-byte alignment only


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def gin(a, name, ld=None, offset=64):
    a = np.ascontiguousarray(a)
    return G.inp(torch.from_numpy(a), 'cuda', ld=ld if ld is not None else a.shape[-1], name=name, offset=offset)


def gout(shape, name, ld=None, fill=None, dtype=torch.float32, offset=64):
    if isinstance(fill, np.ndarray):
        fill = torch.from_numpy(np.ascontiguousarray(fill))
    return G.Guarded(shape, ld=ld, role='out', dtype=dtype, device='cuda', fill=fill, name=name, offset=offset)


def host(g):
    t = g.t.contiguous().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def fig(test, case, n):
    print(f'FIG {test} {case} {n}')


def v2_image(E, flat_dev):
    """ss_op_split_image of a flat fp32 device tensor (n % 8 == 0) at scale 16, as bits"""
    n = flat_dev.numel()
    return E.split_image(flat_dev.contiguous().reshape(n // 8, 8)).reshape(-1).cpu().numpy()


def done(bufs):
    torch.cuda.synchronize()
    G.check_all([b for b in bufs if b is not None])


# ------------------------------------------------------------------------------------------------ conv_pack
def _pack_once(E, w, Cp, with_wb, img, many=False):
    """one launch into fresh guarded outputs; img in (None, 'v2', 'bf16'); returns (wf, wb, wf_img, wb_img) as host arrays (None where absent)"""
    Co, Ci, _ = w.shape
    nf, nb = Co * 5 * Cp, Ci * 5 * Co
    bf = img == 'bf16'
    gw = gin(w.reshape(-1), 'w', offset=ODD)
    gwf, gwb = gout((nf,), 'wf'), gout((nb,), 'wb') if with_wb else None
    idt = torch.bfloat16 if bf else torch.float32
    gfi = gout((nf,), 'wf_img', dtype=idt) if img else None
    gbi = gout((nb,), 'wb_img', dtype=idt) if img and with_wb and (bf or nb % 8 == 0) else None
    t = lambda g: g.t if g is not None else None            # noqa: E731
    wd = gw.t.reshape(Co, Ci, 5)
    if many:
        E.conv_pack_many([(wd, Cp, t(gwf), t(gwb), t(gfi), t(gbi))], img_bf16=bf)
    else:
        E.conv_pack(wd, Cp, t(gwf), t(gwb), t(gfi), t(gbi), img_bf16=bf)
    done((gw, gwf, gwb, gfi, gbi))
    out = [host(g) if g is not None else None for g in (gwf, gwb, gfi, gbi)]
    if img == 'v2':                                         # the device's own split of the fp32 packs
        out += [v2_image(E, gwf.t), v2_image(E, gwb.t) if gbi is not None else None]
    return out


@pytest.mark.parametrize('shape', R.CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv_pack(E, shape):
    Co, Ci, Cp = shape
    w = R.conv_weight(Co, Ci)
    rf, rb = R.conv_pack_ref(w, Cp)
    rf, rb = rf.reshape(-1), rb.reshape(-1)
    bad = 0
    wf, wb, _, _ = _pack_once(E, w, Cp, True, None)
    bad += R.n_diff(wf, rf) + R.n_diff(wb, rb)
    wf0, wb0, _, _ = _pack_once(E, w, Cp, False, None)                                       # wb == NULL
    assert wb0 is None
    bad += R.n_diff(wf0, rf)
    wf, wb, fi, bi, sf, sb = _pack_once(E, w, Cp, True, 'v2')
    bad += R.n_diff(wf, rf) + R.n_diff(wb, rb) + R.n_diff(fi, sf)
    assert (bi is None) == (Ci * 5 * Co % 8 != 0)
    if bi is not None:
        bad += R.n_diff(bi, sb)
    wf, wb, fi, bi = _pack_once(E, w, Cp, True, 'bf16')
    bad += R.n_diff(wf, rf) + R.n_diff(wb, rb) + R.n_diff(fi, R.bf16_bits(rf)) + R.n_diff(bi, R.bf16_bits(rb))
    wf, wb, fi, bi, sf, sb = _pack_once(E, w, Cp, True, 'v2', many=True)                     # a one-task table
    bad += R.n_diff(wf, rf) + R.n_diff(wb, rb) + R.n_diff(fi, sf)
    fig('conv_pack', f'{Co}x{Ci}x{Cp}', bad)
    assert bad == 0


def test_conv_pack_many_is_the_single_form(E):
    """all five shapes in one launch (blockIdx.y = task), images in both formats; one task without wb"""
    for img in ('v2', 'bf16'):
        bf = img == 'bf16'
        idt = torch.bfloat16 if bf else torch.float32
        tasks, bufs, refs = [], [], []
        for i, (Co, Ci, Cp) in enumerate(R.CONV_SHAPES):
            w = R.conv_weight(Co, Ci)
            nf, nb = Co * 5 * Cp, Ci * 5 * Co
            with_wb = i != 1
            gw = gin(w.reshape(-1), f'w{i}', offset=ODD)
            gwf, gwb = gout((nf,), f'wf{i}'), gout((nb,), f'wb{i}') if with_wb else None
            gfi = gout((nf,), f'wf_img{i}', dtype=idt)
            gbi = gout((nb,), f'wb_img{i}', dtype=idt) if with_wb and (bf or nb % 8 == 0) else None
            t = lambda g: g.t if g is not None else None    # noqa: E731
            tasks.append((gw.t.reshape(Co, Ci, 5), Cp, gwf.t, t(gwb), gfi.t, t(gbi)))
            bufs.append((gw, gwf, gwb, gfi, gbi))
            refs.append(_pack_once(E, w, Cp, with_wb, img))
        E.conv_pack_many(tasks, img_bf16=bf)
        bad = 0
        for i, (group, ref) in enumerate(zip(bufs, refs)):
            done(group)
            for g, r in zip(group[1:], ref[:4]):
                assert (g is None) == (r is None)
                if g is not None:
                    bad += R.n_diff(host(g), r)
        fig('conv_pack_many', img, bad)
        assert bad == 0


@pytest.mark.parametrize('shape', R.DX_SHAPES, ids=lambda s: 'x'.join(map(str, s[:2])))
def test_conv_pack_dx(E, shape):
    Co, Ci, _ = shape
    w = R.conv_weight(Co, Ci)
    gw, gwb = gin(w.reshape(-1), 'w', offset=ODD), gout((Ci * 5 * Co,), 'wb', offset=ODD + 2)
    E.conv_pack_dx(gw.t.reshape(Co, Ci, 5), gwb.t)
    done((gw, gwb))
    bad = R.n_diff(host(gwb), R.conv_pack_dx_ref(w).reshape(-1))
    if Co % 4 == 0:                                         # conv_pack's wb, on the device
        bad += R.n_diff(host(gwb), _pack_once(E, w, (Ci + 3) // 4 * 4, True, None)[1])
    fig('conv_pack_dx', f'{Co}x{Ci}', bad)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ conv_unpack
def _unpack_bufs(shape, acc, i=0):
    Co, Ci, Cp = shape
    gp = R.packed_grad(Co, Ci, Cp, NAN, seed=i)
    g0 = (R.conv_weight(Co, Ci, seed=3 + i) + F32(1)) if acc else None
    ggp = gin(gp.reshape(-1), f'gp{i}', offset=ODD)
    gg = gout((Co * Ci * 5,), f'g{i}', offset=ODD + 2, fill=g0.reshape(-1) if acc else None)
    return gp, g0, ggp, gg


@pytest.mark.parametrize('acc', (False, True), ids=('plain', 'acc'))
@pytest.mark.parametrize('shape', R.CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv_unpack(E, shape, acc):
    Co, Ci, Cp = shape
    gp, g0, ggp, gg = _unpack_bufs(shape, acc)
    E.conv_unpack(ggp.t, Co, Ci, Cp, gg.t, acc=acc)
    done((ggp, gg))
    got = host(gg)
    assert np.all(np.isfinite(got)), 'a padding column of the pack was read'
    bad = R.n_diff(got, R.conv_unpack_ref(gp, Ci, g0).reshape(-1))
    fig('conv_unpack', f'{Co}x{Ci}x{Cp}/{"acc" if acc else "plain"}', bad)
    assert bad == 0


@pytest.mark.parametrize('acc', (False, True), ids=('plain', 'acc'))
def test_conv_unpack_many(E, acc):
    sets = [_unpack_bufs(s, acc, i) for i, s in enumerate(R.CONV_SHAPES)]
    E.conv_unpack_many([(ggp.t, *s, gg.t) for s, (_, _, ggp, gg) in zip(R.CONV_SHAPES, sets)], acc=acc)
    bad = 0
    for (Co, Ci, Cp), (gp, g0, ggp, gg) in zip(R.CONV_SHAPES, sets):
        done((ggp, gg))
        bad += R.n_diff(host(gg), R.conv_unpack_ref(gp, Ci, g0).reshape(-1))
    fig('conv_unpack_many', 'acc' if acc else 'plain', bad)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ transpose
def test_transpose(E):
    bad = 0
    for Rr in R.TRANSPOSE_SIZES:
        for Cc in R.TRANSPOSE_SIZES:
            x = np.random.default_rng([15, Rr, Cc]).standard_normal((Rr, Cc)).astype(F32)
            gx, go = gin(x.reshape(-1), 'in', offset=ODD), gout((Rr * Cc,), 'out', offset=ODD + 2)
            E.transpose(gx.t.reshape(Rr, Cc), go.t)
            done((gx, go))
            d = R.n_diff(host(go), np.ascontiguousarray(x.T).reshape(-1))
            fig('transpose', f'{Rr}x{Cc}', d)
            bad += d
    assert bad == 0


# ------------------------------------------------------------------------------------------------ prep
PAYLOAD = np.array([0x7FC00123], np.uint32).view(F32)[0]


def _prep_task(i, n, with_b, img, a_off=64, b_off=64, d_off=64):
    """guarded operands of one task; offsets are in elements (64: 16-byte aligned and more; odd: the scalar path)"""
    rng = np.random.default_rng([16, i, n])
    a = R.signed_zeros(rng.standard_normal(n).astype(F32), rng)
    b = R.signed_zeros(rng.standard_normal(n).astype(F32), rng) if with_b else None
    if not with_b and not img and n > 5:
        a[5] = PAYLOAD                                      # a copy moves a NaN's payload too
    ga, gb = gin(a, f'a{i}', offset=a_off), gin(b, f'b{i}', offset=b_off) if with_b else None
    gd = gout((n,), f'dst{i}', offset=d_off)
    gi = gout((n,), f'img{i}', dtype=torch.bfloat16 if img == 'bf16' else torch.float32) if img else None
    vec = R.prep_takes_vec(n, ga.t.data_ptr(), gb.t.data_ptr() if with_b else 0, gd.t.data_ptr())
    return dict(a=a, b=b, ga=ga, gb=gb, gd=gd, gi=gi, n=n, vec=vec)


def _prep_run(E, tasks, bf16):
    E.prep([(t['ga'].t, t['gb'].t if t['gb'] else None, t['gd'].t, t['n'], t['gi'].t if t['gi'] else None) for t in tasks], img_bf16=bf16)
    bad = 0
    for t in tasks:
        done((t['ga'], t['gb'], t['gd'], t['gi']))
        ref = R.prep_ref(t['a'], t['b'])
        d = R.n_diff(host(t['gd']), ref)
        if t['gi'] is not None:
            d += R.n_diff(host(t['gi']), R.bf16_bits(ref) if bf16 else v2_image(E, t['gd'].t))
        t['bad'] = d
        bad += d
    return bad


@pytest.mark.parametrize('img', ('v2', 'bf16'))
def test_prep(E, img):
    """Before the fix, every scalar-path copy (b null) differed in exactly its -0.0 elements."""
    big_v, big_s = 4 * R.PREP_STRIDE + 4 * 1000, R.PREP_STRIDE + 3619                        # more than one sweep of the grid on either path
    spec = [  # n, with_b, image, offsets of a / b / dst
        (big_v, False, img, 64, 64, 64), (big_v, True, img, 64, 64, 64), (64, False, img, 64, 64, 64), (8, True, img, 64, 64, 64),
        (1024, False, None, 64, 64, 64), (1024, True, None, 64, 64, 64),
        (big_s, False, None, 64, 64, 64), (big_s, True, None, 64, 64, 64), (1023, False, None, 64, 64, 64), (1, False, None, 64, 64, 64),
        (2, True, None, 64, 64, 64), (1024, False, None, ODD, 64, 64), (1024, False, None, 64, 64, ODD), (1024, True, None, 64, ODD, 64),
        (1024, True, None, ODD, ODD, ODD), (257, False, None, 66, 64, 66)]
    tasks = [_prep_task(i, *s) for i, s in enumerate(spec)]
    assert [t['vec'] for t in tasks] == [True] * 6 + [False] * 10
    assert all(np.signbit(t['a'][t['a'] == 0]).any() for t in tasks if t['n'] >= 3)
    bad = _prep_run(E, tasks, img == 'bf16')
    for t, s in zip(tasks, spec):
        fig('prep', f'n={s[0]}/b={int(s[1])}/img={s[2]}/off={s[3]},{s[4]},{s[5]}/{"vec" if t["vec"] else "scalar"}', t['bad'])
    assert bad == 0


def test_prep_full_table(E):
    tasks = [_prep_task(100 + i, 4 * (i + 1) + (i % 3 == 0), i % 2 == 1, None, d_off=64 + (i % 5 == 2)) for i in range(48)]
    assert {t['vec'] for t in tasks} == {True, False}
    bad = _prep_run(E, tasks, False)
    fig('prep', '48-tasks', bad)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ copy_rows
def _slab_fill(B, T, C, real):
    s = np.full((B, T + 4, C), HALO_FILL, F32)
    s[:, 2:2 + T] = real
    return s


COPY_SHAPES = ((5, 9, 1), (5, 9, 80), (5, 9, 83), (2, 256, 80))                              # the last: 20480 elements, beyond one sweep (64 x 256)


@pytest.mark.parametrize('ragged', (False, True), ids=('plain', 'len'))
@pytest.mark.parametrize('shape', COPY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_copy_rows(E, shape, ragged):
    B, T, C = shape
    src = np.random.default_rng([17, B, T, C]).standard_normal((B, T, C)).astype(F32)
    src = R.signed_zeros(src, np.random.default_rng(1))
    lens = ([0, 4, T, T + 5, -3] if B == 5 else [T // 2 + 1, T + 1]) if ragged else None
    fed = src.copy()
    if ragged:
        for b, n in enumerate(lens):
            fed[b, R.ragged_len(n, T):] = NAN               # the rows behind len are never read
    ref = R.copy_rows_ref(src, lens)
    glen = gin(np.array(lens, np.int32), 'len', offset=ODD) if ragged else None
    lt = glen.t if ragged else None
    bad = 0
    # dense [B][T][C] (row stride above C) -> slab [B][T+4][ld]
    gs = gin(fed, 'dense', ld=C + 3, offset=ODD)
    gd = gout((B, T + 4, C), 'slab', ld=C + 5, offset=ODD + 2, fill=_slab_fill(B, T, C, NAN))
    E.copy_rows(gs.t, gd.t[:, 2:2 + T], lt)
    done((gs, gd, glen))
    got = host(gd)
    assert np.all(got[:, :2] == HALO_FILL) and np.all(got[:, 2 + T:] == HALO_FILL), 'a halo row changed'
    bad += R.n_diff(got[:, 2:2 + T], ref)
    # slab -> dense
    gs = gin(_slab_fill(B, T, C, fed), 'slab', ld=C + 5, offset=ODD)
    gs.t[:, :2] = float('nan')                              # the source's halo rows are not read either
    gs.t[:, 2 + T:] = float('nan')
    gd = gout((B, T, C), 'dense', ld=C + 3, offset=ODD + 2)
    E.copy_rows(gs.t[:, 2:2 + T], gd.t, lt)
    done((gs, gd, glen))
    bad += R.n_diff(host(gd), ref)
    fig('copy_rows', f'{B}x{T}x{C}/{"len" if ragged else "plain"}', bad)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ act_scales
@pytest.mark.parametrize('T', (64, 192))
def test_act_scales(E, T):
    cases = R.act_cases(T)
    bad = 0
    for C in R.ACT_C:
        for lo in range(0, len(cases), 7):                  # seven blocks and an absent one (C = 0) per launch
            chunk = cases[lo:lo + 7]
            blocks = [R.act_block(C, gm, bm, i) for i, (_, gm, bm) in enumerate(chunk)]
            gg = [gin(g, f'gamma{i}', offset=ODD) for i, (g, _) in enumerate(blocks)]
            gb = [gin(b, f'beta{i}', offset=ODD + 2) for i, (_, b) in enumerate(blocks)]
            aff = [(g.t, b.t) for g, b in zip(gg, gb)]
            aff.insert(3, (None, None))
            go = gout((len(aff),), 'scales', offset=ODD)
            E.act_scales(aff, T, go.t)
            done(gg + gb + [go])
            got = host(go)
            want = [R.act_scale_ref(R.act_bound(g, b, T)) for g, b in blocks]
            want.insert(3, F32(16))
            for (name, _, _), g, w in zip(chunk[:3] + (('absent', 0, 0),) + chunk[3:], got, want):
                d = R.n_diff(np.array([g], F32), np.array([w], F32))
                fig('act_scales', f'T={T}/C={C}/{name}', d)
                bad += d
    assert bad == 0


# ------------------------------------------------------------------------------------------------ param_guard
@pytest.mark.parametrize('n', R.GUARD_N)
def test_param_guard(E, n):
    limit = 2048.0
    clean = R.guard_arena(n)
    arena = gin(clean, 'arena')
    words = (0, 1, 0x80000003, 4)

    def run(word):
        gs = gout((1,), 'sticky', dtype=torch.int32, fill=word - (1 << 32) if word >= 1 << 31 else word)
        E.param_guard(arena.t, limit, gs.t)
        torch.cuda.synchronize()
        arena.check()
        gs.check(written=False)
        return int(gs.t.cpu().numpy().view(np.uint32)[0])
    bad = 0
    for word in words:                                      # a clean arena leaves the word as it was
        bad += run(word) != R.guard_ref(clean, limit, word) or run(word) != word
    fig('param_guard', f'n={n}/clean', bad)
    for name, v, is_bad in R.guard_values(limit):
        d = 0
        for pos in sorted({0, n // 2, n - 1}):
            keep = clean[pos]
            arena.t[pos] = float(v)
            p = clean.copy()
            p[pos] = v
            for word in words[:3]:
                want = R.guard_ref(p, limit, word)
                assert want == ((word | 4) if is_bad else word)
                d += run(word) != want
            arena.t[pos] = float(keep)
        fig('param_guard', f'n={n}/{name}', d)
        bad += d
    assert bad == 0
