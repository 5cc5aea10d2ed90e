"""The kernels between the heavy families of a training step -- mse_loss / ce_loss / finish_loss, the column sums, the decoder-input kernels with
their gradients and spk_grad -- each launched alone through its engine-free hook (ss_op_mse_loss, ss_op_ce_loss, ss_op_colsum, ss_op_dec_in /
_grad / _codes, ss_op_spk_grad) on guarded buffers (tests/guarded.py: row stride above the width, a non-zero offset, NaN guard bands, scratch
of exactly the stated size) and judged PER ELEMENT against the float64 references and worst-case rounding budgets of tests/step_ops_ref.py --
the budgets tests/test_step_ops_ref_selftest.py proves: each kernel's own operation order stays inside them, a subtly wrong kernel does not.

  MSE            (B, T, C) in (1,1,80) (3,8,80) (1,26,80) (2,256,80); normal, out == tgt (exact zeros), magnitudes 1e3 and 1e-20; grad_scale
                 1, 0.25, 1/3; repeat bits
  CE             C in {2, 63, 64, 65, 257} x (B, T) in {(1,1), (3,8)}; normal, all equal, target dominant by 60, another class dominant by 60,
                 offsets +-1000 (judged by the UNSHIFTED case's budget too: the kernel is shift-invariant), -inf in non-target classes; the
                 row gradient sums to zero within budget
  column sums    R in {1, 4, 15, 16, 17, 33, 520} x (257 columns one-direction; C in {4, 12, 32} two-direction; C = 2048 at R = 520); with and
                 without scratch, o1 / o3 NULL, a cancelling family; one counter buffer through three calls: all-zero after each, same bits
  decoder input  three source sets x T in {8, 16, 64} x B in {1, 3}, slab and compact forms; forward exact and bit-equal to the way through
                 dense codes; gradients bit-equal to the ascending fp32 chain and inside (f - 1) u sum|terms| of float64
  spk_grad       E in {1, 81, 256, 513, 1024} x H4 in {4, 2048} x rows in {1, 12, 260} x B in {1, 3}; repeat bits

What a kernel does not own keeps its bits: row gaps, bands, halo rows, padding columns, scratch beyond the stated size.  Each test prints
`FIG <test> <case> <worst error / budget>`."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import step_ops_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
HALO_FILL = -7.25                                           # what rows / elements a kernel does not own hold before and must hold after
NANBITS = G.NAN32 - (1 << 32) if G.NAN32 >= 1 << 31 else G.NAN32
NAN = np.array([G.NAN32], np.uint32).view(F32)[0]


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def gin(a, name, ld=None):
    a = np.ascontiguousarray(a)
    return G.inp(torch.from_numpy(a), 'cuda', ld=ld if ld is not None else a.shape[-1], name=name)


def gout(shape, name, ld=None, fill=None, dtype=torch.float32):
    if isinstance(fill, np.ndarray):
        fill = torch.from_numpy(np.ascontiguousarray(fill))
    return G.Guarded(shape, ld=ld, role='out', dtype=dtype, device='cuda', fill=fill, name=name)


def host(g):
    return g.t.contiguous().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def ratio(got, ref, budget):
    """worst |got - ref| / budget; every result finite; an element with budget 0 must be exact"""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), 'a result is not finite'
    err = np.abs(got - ref)
    b = np.asarray(budget, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


def fig(test, case, worst):
    print(f'FIG {test} {case} {worst:.4f}')


def haloed(real, halo=NAN):
    """[B, T, C] -> [B, T+4, C] with `halo` in the four halo rows"""
    B, T, C = real.shape
    s = np.full((B, T + 4, C), halo, F32)
    s[:, 2:2 + T] = real
    return s


# ------------------------------------------------------------------------------------------------ MSE
@pytest.mark.parametrize('shape', R.MSE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_mse_loss(E, shape):
    B, T, C = shape
    worst_l = worst_d = 0.0
    for fam in R.MSE_FAMILIES:
        o, y = R.mse_case(fam, B, T, C)
        go, gy = gin(o, 'out', ld=C + 8), gin(y, 'tgt', ld=C + 3)
        for gsc in R.GRAD_SCALES:
            runs = []
            for rep in range(2):
                gd, gp, gl = gout((B, T, C), 'd_out', ld=C + 5), gout((8 * B,), 'partials'), gout((1,), 'loss')
                E.mse_loss(go.t, gy.t, gd.t, gp.t, gl.t, grad_scale=gsc)
                torch.cuda.synchronize()
                G.check_all((go, gy, gd, gp, gl))
                runs.append((float(host(gl)[0]), host(gd)))
            assert runs[0][0] == runs[1][0] and same_bits(runs[0][1], runs[1][1]), 'a repeat differs'
            loss, d = runs[0]
            rl, rd = R.mse_ref(o, y, gsc)
            bl, bd = R.mse_budget(o, y, gsc)
            ql, qd = ratio(loss, rl, bl), ratio(d, rd, bd)
            fig('mse_loss', f'{B}x{T}x{C}/{fam}/gs={gsc:.4g}', max(ql, qd))
            worst_l, worst_d = max(worst_l, ql), max(worst_d, qd)
            if fam == 'equal':
                assert loss == 0.0 and not d.any(), 'out == tgt must give exact zeros'
    assert worst_l <= 1.0 and worst_d <= 1.0, (worst_l, worst_d)


# ------------------------------------------------------------------------------------------------ CE
@pytest.mark.parametrize('BT', R.CE_BT, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('C', R.CE_CLASSES)
def test_ce_loss(E, C, BT):
    """On the offset families the kernel's former order (lse = mx + logf(se), expf(x - lse)) measured 6.3 to 30.9 budgets here (every other
    family was inside); (x - mx) - logf(se) measures at most 0.85 on them.  The figures are in profiles/r05/step_ops/test_figures.txt."""
    B, T = BT
    failed = []
    for fam in R.CE_FAMILIES:
        x, y = R.ce_case(fam, B, T, C)
        gx, gy = gin(x, 'logits', ld=C + 3), gin(y, 'tgt')
        for gsc in (1.0, 1.0 / 3.0) if fam == 'normal' else (1.0,):
            gd, gp, gl = gout((B, T, C), 'd_out', ld=C + 5), gout((B * T,), 'partials'), gout((1,), 'loss')
            E.ce_loss(gx.t, gy.t, gd.t, gp.t, gl.t, grad_scale=gsc)
            torch.cuda.synchronize()
            G.check_all((gx, gy, gd, gp, gl))
            loss, row, d = float(host(gl)[0]), host(gp).reshape(B, T), host(gd)
            rl, rrow, rd = R.ce_ref(x, y, gsc)
            budgets = [R.ce_budget(x, y, gsc)]
            if fam.startswith('offset'):                    # the same budget as the unshifted case
                x0, y0 = R.ce_case('normal', B, T, C)
                assert np.array_equal(y0, y)
                budgets.append(R.ce_budget(x0, y0, gsc))
            q = 0.0
            for bl, brow, bd in budgets:
                q = max(q, ratio(loss, rl, bl), ratio(row, rrow, brow), ratio(d, rd, bd))
                q = max(q, float(np.max(np.abs(d.astype(np.float64).sum(axis=-1)) / bd.sum(axis=-1))))        # the row gradient sums to zero
            fig('ce_loss', f'{B}x{T}x{C}/{fam}/gs={gsc:.4g}', q)
            if not q <= 1.0:
                failed.append((fam, gsc, q))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ column sums
COLSUM_CONFIGS = (('one', 257), ('two', 4), ('two', 12), ('two', 32))


def _colsum_once(E, gx, v, two, Cc, pre, scratch, ctr, drop_pair=False):
    """one launch into fresh pre-filled outputs; returns the outputs' values (None where an output was not given)"""
    names = ('o0', 'o1', 'o2', 'o3') if two else ('o0',)
    outs = [None if drop_pair and n in ('o1', 'o3') else gout((Cc,), n, fill=pre[i]) for i, n in enumerate(names)]
    part = gout((R.colsum_scratch_doubles(v.shape[1]),), 'part', dtype=torch.float64) if scratch else None
    E.colsum(gx.t, [o.t if o is not None else None for o in outs], two_dir=two, part=part.t if scratch else None, ctr=ctr.t if scratch else None)
    torch.cuda.synchronize()
    G.check_all([gx] + [o for o in outs if o is not None])
    if scratch:
        part.check(written=False)                           # nothing outside part[0 .. scratch_doubles) changes
        ctr.check(written=False)
        assert not bool(ctr.t.any()), 'an arrival counter did not come back to zero'
    return [host(o) if o is not None else None for o in outs]


def _colsum_case(E, fam, Rr, two, Cc):
    cols = 2 * Cc if two else Cc
    v = R.colsum_case(fam, Rr, cols)
    gx = gin(v, 'in', ld=cols + 5)
    rng = np.random.default_rng([Rr, cols])
    pre = [(1.0 + rng.random(Cc)).astype(F32) * (-1) ** i for i in range(4 if two else 1)]
    ctr = gout((R.cdiv(cols, 64),), 'ctr', fill=0, dtype=torch.int32)

    def worst(outs):
        q = 0.0
        for i, o in enumerate(outs):
            if o is not None:
                ref, bud = R.colsum_ref(v[:, (i // 2) * Cc:(i // 2) * Cc + Cc] if two else v, pre[i])
                q = max(q, ratio(o, (v[:, (i // 2) * Cc:(i // 2) * Cc + Cc] if two else v).astype(np.float64).sum(0) + pre[i], bud))
                q = max(q, ratio(o, ref.astype(np.float64), bud))
        return q
    three = [_colsum_once(E, gx, v, two, Cc, pre, True, ctr) for _ in range(3)]            # the same counters, three calls
    for other in three[1:]:
        assert all(same_bits(a, b) for a, b in zip(three[0], other)), 'a repeat through the same counters differs'
    q = worst(three[0])
    plain = _colsum_once(E, gx, v, two, Cc, pre, False, None)
    q = max(q, worst(plain))
    if two:
        half = _colsum_once(E, gx, v, two, Cc, pre, True, ctr, drop_pair=True)
        assert same_bits(half[0], three[0][0]) and same_bits(half[2], three[0][2])
    fig('colsum', f'R={Rr}/{"two" if two else "one"}/C={Cc}/{fam}', q)
    return q


@pytest.mark.parametrize('Rr', R.COLSUM_R)
def test_colsum(E, Rr):
    worst = 0.0
    for kind, Cc in COLSUM_CONFIGS + ((('two', 2048),) if Rr == 520 else ()):
        worst = max(worst, _colsum_case(E, 'normal', Rr, kind == 'two', Cc))
        if Rr >= 4 and Cc in (257, 12):
            worst = max(worst, _colsum_case(E, 'cancelling', Rr, kind == 'two', Cc))
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ decoder input
def _dec_srcs(name):
    """the layout of step_ops_ref with guarded row strides: H = 3 keeps its ld of 8 (two padding columns), the others get four"""
    srcs, Ee, emb_col, ld = R.dec_layout(name)
    return [(H, fr, col, 8 if H == 3 else 2 * H + 4) for H, fr, col, _ in srcs], Ee, emb_col, ld


def _dec_dst(B, T, ld, f, name):
    if f:
        return gout((B, T // f, ld), name)
    fill = np.full((B, T + 4, ld), HALO_FILL, F32)
    fill[:, 2:2 + T] = NAN
    return gout((B, T + 4, ld), name, fill=fill)


def _dec_real(g, T, f):
    a = host(g)
    if f:
        return a
    assert np.all(a[:, :2] == HALO_FILL) and np.all(a[:, 2 + T:] == HALO_FILL), f'{g.name}: a halo row changed'
    return a[:, 2:2 + T]


@pytest.mark.parametrize('B', R.DEC_B)
@pytest.mark.parametrize('T', R.DEC_T)
@pytest.mark.parametrize('name', sorted(R.DEC_SETS))
def test_dec_in_forward(E, name, T, B):
    layout = _dec_srcs(name)
    srcs, Ee, emb_col, ld = layout
    rng = np.random.default_rng([1, T, B, len(srcs)])
    slabs = [haloed(rng.standard_normal((B, T, 2 * H)).astype(F32)) for H, *_ in srcs]
    emb = rng.standard_normal((B, Ee)).astype(F32) if Ee else None
    gs = [gin(s, f'o{i}', ld=sl[3]) for i, (s, sl) in enumerate(zip(slabs, srcs))]
    ge = gin(emb, 'emb') if Ee else None
    args = [(g.t, H, fr, col) for g, (H, fr, col, _) in zip(gs, srcs)]
    need = sum((B * (T // fr) * 2 * H + 3) // 4 * 4 for H, fr, _, _ in srcs)
    forms = [0] + ([srcs[0][1]] if len({fr for _, fr, _, _ in srcs}) == 1 else [])
    for f in forms:
        ref = R.dec_in_ref(slabs, layout, emb, B, T, f=f)
        assert not ref[:, :, emb_col + Ee:].any()                                           # the padding columns read zero
        d1, d2 = _dec_dst(B, T, ld, f, 'dst'), _dec_dst(B, T, ld, f, 'dst_via_codes')
        codes = gout((need,), 'codes')
        E.dec_in(args, ge.t if Ee else None, emb_col, d1.t, T, f=f)
        E.dec_in(args, ge.t if Ee else None, emb_col, d2.t, T, f=f, via_codes=codes.t)
        torch.cuda.synchronize()
        G.check_all(gs + ([ge] if Ee else []) + [d1, d2])
        codes.check(written=False)
        a1, a2 = _dec_real(d1, T, f), _dec_real(d2, T, f)
        assert same_bits(a1, ref), 'the decoder input differs from the index reference'
        assert same_bits(a2, a1), 'export_codes + dec_in_from_codes differs from build_dec_in'
        fig('dec_in_forward', f'{name}/T={T}/B={B}/f={f}', 0.0)


@pytest.mark.parametrize('B', R.DEC_B)
@pytest.mark.parametrize('T', R.DEC_T)
@pytest.mark.parametrize('name', sorted(R.DEC_SETS))
def test_dec_in_grad(E, name, T, B):
    layout = _dec_srcs(name)
    srcs, Ee, emb_col, ld = layout
    rng = np.random.default_rng([2, T, B, len(srcs)])

    def run(d_in_dev, f):
        fills = [haloed(np.full((B, T, 2 * H), NAN, F32), HALO_FILL) for H, *_ in srcs]
        gd = [gout((B, T + 4, 2 * sl[0]), f'd_o{i}', ld=sl[3], fill=fl) for i, (fl, sl) in enumerate(zip(fills, srcs))]
        E.dec_in_grad([(g.t, H, fr, col) for g, (H, fr, col, _) in zip(gd, srcs)], d_in_dev.t, T, f=f)
        torch.cuda.synchronize()
        G.check_all(gd + [d_in_dev])                        # the padding columns of d_o are guard: they keep their bits
        return [_dec_real(g, T, 0) for g in gd]
    t = np.arange(T)
    d_in = rng.standard_normal((B, T, ld)).astype(F32)
    got = run(gin(haloed(d_in), 'd_dec_in'), 0)
    worst = 0.0
    for g, (chain, r64, ra), (H, fr, col, _) in zip(got, R.dec_in_grad_chain(d_in, layout, B, T), srcs):
        assert not g[:, t % fr != fr - 1, :H].any() and not g[:, t % fr != 0, H:].any(), 'a non-zero at an unsampled frame'
        assert same_bits(g, chain), 'dec_in_grad is not the ascending fp32 chain over f frames'
        worst = max(worst, ratio(g, r64, (fr - 1) * R.U * ra))
    fig('dec_in_grad', f'{name}/T={T}/B={B}/slab', worst)
    assert worst <= 1.0
    if len({fr for _, fr, _, _ in srcs}) == 1:
        f = srcs[0][1]
        d_xc = rng.standard_normal((B, T // f, ld)).astype(F32)
        gotc = run(gin(d_xc, 'd_xc'), f)
        rep = np.repeat(d_xc / F32(f), f, axis=1).astype(F32)                               # the slab form fed the repeated rows (f a power of two)
        gots = run(gin(haloed(rep), 'd_dec_in_rep'), 0)
        worst = 0.0
        for g, gsl, (H, fr, col, _) in zip(gotc, gots, srcs):
            want = np.zeros((B, T, 2 * H), F32)
            want[:, fr - 1::fr, :H] = d_xc[:, :, col:col + H]
            want[:, 0::fr, H:] = d_xc[:, :, col + H:col + 2 * H]
            assert same_bits(g, want), 'dec_in_grad_compact: not the block sums at the sampled frames, zeros elsewhere'
            worst = max(worst, ratio(gsl, g.astype(np.float64), (fr - 1) * R.U * np.abs(g.astype(np.float64))))
        fig('dec_in_grad', f'{name}/T={T}/B={B}/compact', worst)
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ speaker gradient
@pytest.mark.parametrize('H4', R.SPK_H4)
@pytest.mark.parametrize('Ee', R.SPK_E)
def test_spk_grad(E, Ee, H4):
    col0, worst = 5, 0.0
    rng = np.random.default_rng([3, Ee, H4])
    w = rng.standard_normal((2 * H4, col0 + Ee)).astype(F32)
    w[:, :col0] = NAN                                       # the columns in front of col0 are never read
    gwf, gwr = gin(w[:H4], 'w_f', ld=col0 + Ee + 3), gin(w[H4:], 'w_r', ld=col0 + Ee + 3)
    for rows in R.SPK_ROWS:
        for B in (1, 3):
            dg = rng.standard_normal((B, rows, 2 * H4)).astype(F32)
            gdg = gin(dg, 'dg', ld=2 * H4 + 4)
            outs = []
            for rep in range(2):
                go = gout((B, Ee), 'out')
                E.spk_grad(gdg.t, gwf.t, gwr.t, col0, Ee, go.t)
                torch.cuda.synchronize()
                G.check_all((gdg, gwf, gwr, go))
                outs.append(host(go))
            assert same_bits(outs[0], outs[1]), 'a repeat differs'
            ref, bud = R.spk_ref(dg, w[:H4], w[H4:], col0, Ee)
            q = ratio(outs[0], ref, bud)
            fig('spk_grad', f'E={Ee}/H4={H4}/rows={rows}/B={B}', q)
            worst = max(worst, q)
    assert worst <= 1.0, worst
