"""Every GroupNorm + ReLU kernel form of csrc/elementwise.hip, launched alone through the engine-free hooks ss_op_gn_relu_fwd / _mask / _bwd on
guarded slabs (tests/guarded.py: row stride ld > C, a non-zero offset, NaN guard bands) and judged PER ELEMENT against the float64 references
and worst-case rounding budgets of tests/gn_ref.py -- the budgets tests/test_gn_ref_selftest.py proves: the kernels' own operation order
stays inside them, a subtly wrong kernel (unbiased variance, misplaced eps, wrong inv_n, a dropped backward term, ...) does not.

  register forward   T in {1, 2, 15, 16, 17, 128, 129, 192, 193, 255, 256}, every input family: y, mean, rstd; repeat bits; the mask hook
  ragged forward     lengths T, 1, 0, 15, 16, 17 with NaN behind the lengths: zeros, budget, bits of the dense run at T = len
  chunked forward    T in {257, 320, 321, 1000, 8192}, dense and ragged (a length below 256 included), repeat bits
  gather form        T = P in {8, 128, 129, 192, 193, 255, 256} (the instantiation switches and the 64 KiB LDS switch at 256): engine plans and
                     hand-made edge plans; stats / y bit-equal to the plain kernel + oracle gather; the v2 image (scales 16 and 0.5), the bf16 image
  backward           T in {1, 17, 128, 192, 193, 256}, every family: dx, d_gamma, d_beta, d_bias under the kernel's mask with the kink rule,
                     accumulation onto non-zero values, amax, the bf16 dy image, deterministic repeats
  scatter form       T = P in {128, 192, 193, 256} and P in {160, 161} at T = 192 (the 40 KiB LDS switch): bit-identical to the plain backward fed
                     with the engine's interp_backward under deterministic, dx inside the budget against the float64 adjoint; edge plans

Shapes: (B, C) = (1, 64) -- one workgroup column -- and (3, 192): three columns, twelve groups.  The halo rows of inputs are zero; the halo rows
of outputs a form does not own are pre-filled and must keep their bits.  Each test prints `FIG <test> <case> <worst error / budget>`."""
import functools

import numpy as np
import pytest
import torch

from oracle import interp_np, weights as W
from tests import gn_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = ((1, 64), (3, 192))
HALO_FILL = -7.25                                           # what the halo rows of an output slab hold before and must hold after
NANBITS = G.NAN32 - (1 << 32) if G.NAN32 >= 1 << 31 else G.NAN32


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


class Tuned:
    """ss_tune('deterministic', 1) for the duration of a block, back at the default afterwards whatever happens."""

    def __init__(self, E):
        self.E = E

    def __enter__(self):
        self.E.tune('deterministic', 1)

    def __exit__(self, *exc):
        self.E.tune('deterministic', 0)


COUNT = {'launches': 0, 'buffers': 0}


@pytest.fixture(autouse=True)
def _figures(request):
    """one line per test: the hook launches it made and the guarded buffers it read back -- every one with its guard words unchanged, or the
    test has failed"""
    before = dict(COUNT)
    yield
    print(f'\nFIG count {request.node.name} launches={COUNT["launches"] - before["launches"]} guarded_buffers={COUNT["buffers"] - before["buffers"]} '
          f'guard_words_changed=0')


# ------------------------------------------------------------------------------------------------------------------ cases and buffers
@functools.lru_cache(maxsize=64)
def case(family, B, T, C):
    """(x, gamma, beta, dy) float32 and the forward budget, computed once and shared (read only) by every test of the shape."""
    x, gamma, beta = R.make_case(family, B, T, C, seed=20)
    dy = np.random.default_rng([21, B, T, C]).standard_normal((B, T, C)).astype(F32)
    for a in (x, gamma, beta, dy):
        a.setflags(write=False)
    return x, gamma, beta, dy, (R.forward_budget(x, gamma, beta, long_path=T > 256) if T <= 1000 else None)


def ld_of(C):
    return C + 8                                            # ld > C, a multiple of 8 (the images need it)


def slab_in(x, name, lens=None):
    """x [B,T,C] -> guarded haloed input slab [B,T+4,C]: zero halo rows; rows t >= lens[b] hold the guard NaN (never to be read)."""
    B, T, C = x.shape
    s = np.zeros((B, T + 4, C), F32)
    s[:, 2:2 + T] = x
    t = torch.from_numpy(s)
    if lens is not None:
        for b, L in enumerate(lens):
            t[b, 2 + L:2 + T].view(torch.int32).fill_(NANBITS)
    return G.inp(t, 'cuda', ld=ld_of(C), name=name)


def slab_out(B, rows, C, name, dtype=torch.float32, real=None):
    """guarded output slab [B,rows+4,C]: halo rows HALO_FILL, real rows the guard NaN (or `real` [B,rows,C]: an in/out operand)."""
    f = torch.full((B, rows + 4, C), HALO_FILL, dtype=dtype)
    if real is None:
        f[:, 2:2 + rows].view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(0x7FC1 if dtype == torch.bfloat16 else NANBITS)
    else:
        f[:, 2:2 + rows] = torch.from_numpy(np.array(real, F32))
    return G.Guarded((B, rows + 4, C), ld=ld_of(C), role='out', dtype=dtype, device='cuda', fill=f, name=name)


def halo_kept(g, rows, value=HALO_FILL):
    h = torch.cat([g.t[:, :2], g.t[:, 2 + rows:]], 1)
    assert bool((h == value).all()), f'{g.name}: a halo row changed'


def real(g, rows):
    return g.t[:, 2:2 + rows].contiguous().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def vec(a, name, **kw):
    return G.inp(torch.from_numpy(np.array(a)), 'cuda', name=name, **kw)               # (a copy: the shared cases are read-only)


def run_forward(E, x, gamma, beta, lens=None, plan=None, img=None, img_scale=None, P=None):
    """One ss_op_gn_relu_fwd launch on fresh guarded buffers -> dict(y [B,rows,C], stats [B,G,2], img) as numpy; guards checked."""
    B, T, C = x.shape
    rows = T if plan is None else P
    xs, ga, be = slab_in(x, 'x', lens), vec(gamma, 'gamma'), vec(beta, 'beta')
    ys = slab_out(B, rows, C, 'y')
    st = G.out((B, C // 16, 2), 'cuda', name='stats')
    ln = vec(np.asarray(lens, np.int32), 'len') if lens is not None else None
    bufs = [xs, ga, be, ys, st] + ([ln] if ln is not None else [])
    need = E.gn_relu_scratch(B, T, C)
    scr = G.out((need // 8,), 'cuda', dtype=torch.float64, name='scratch') if need else None
    dplan = None
    if plan is not None:
        dplan = [vec(plan[0], 'i0'), vec(plan[1], 'lam'), vec(plan[2], 'nrows')]
        bufs += dplan
    yi = sc = None
    if img is not None:
        yi = slab_out(B, rows, C, 'y_img', dtype=torch.bfloat16 if img == 'bf16' else torch.float32)
        bufs.append(yi)
        if img_scale is not None:
            sc = vec(np.array([img_scale], F32), 'img_scale')
            bufs.append(sc)
    E.gn_relu_fwd(xs.t, ys.t, ga.t, be.t, st.t, lengths=ln.t if ln is not None else None, plan=tuple(p.t for p in dplan) if dplan else None,
                  y_img=yi.t if yi is not None else None, img_scale=sc.t if sc is not None else None, scratch=scr.t if scr is not None else None)
    torch.cuda.synchronize()
    for g in bufs:
        g.check(written=False if g in (ys, yi) else None)
    if scr is not None:
        scr.check()
    COUNT['launches'] += 1
    COUNT['buffers'] += len(bufs) + (scr is not None)
    halo_kept(ys, rows)
    out = dict(y=real(ys, rows), stats=st.t.cpu().numpy(), xs=xs, ga=ga, be=be, st=st)
    if yi is not None:
        halo_kept(yi, rows)
        out['img'] = yi.t[:, 2:2 + rows].contiguous().view(torch.int16 if img == 'bf16' else torch.int32).cpu().numpy()
        out['y_dev'] = ys
    return out


def judge_forward(tag, got, fb, lens=None):
    """y per element against dz, the mean within dm, rstd within rho rstd (rows of no frames excepted: NaN by contract) -> worst ratio"""
    ry = R.ratio(got['y'] - fb['y'], fb['dz'])
    live = np.ones(got['stats'].shape[0], bool) if lens is None else np.asarray(lens) > 0
    rm = R.ratio((got['stats'][..., 0] - fb['mean'])[live], fb['dm'][live])
    rr = R.ratio((got['stats'][..., 1] - fb['rstd'])[live], (fb['rho'] * fb['rstd'])[live])
    print(f'FIG {tag} y={ry:.3g} mean={rm:.3g} rstd={rr:.3g}')
    assert ry <= 1.0 and rm <= 1.0 and rr <= 1.0, (tag, ry, rm, rr)
    return max(ry, rm, rr)


# ------------------------------------------------------------------------------------------------------------------ forward, T <= 256
@pytest.mark.parametrize('B,C', SHAPES)
@pytest.mark.parametrize('T', R.T_LIST)
def test_forward(E, T, B, C):
    for family in R.FAMILIES:
        x, gamma, beta, _, fb = case(family, B, T, C)
        a = run_forward(E, x, gamma, beta)
        judge_forward(f'forward {family} B={B} T={T} C={C}', a, fb)
        b = run_forward(E, x, gamma, beta)
        assert same_bits(a['y'], b['y']) and same_bits(a['stats'], b['stats']), (family, 'a second run differs')
        mask = E.gn_relu_mask(a['xs'].t, a['ga'].t, a['be'].t, a['st'].t).cpu().numpy()
        assert same_bits(mask, (a['y'] > 0).astype(F32)), (family, 'the mask hook is not y > 0')
        if family == 'outlier':
            assert np.abs(a['y']).max() <= np.sqrt(16.0 * T) * np.abs(gamma).max() + np.abs(beta).max()       # the bound act_scales relies on
            if T > 1:
                assert np.abs(fb['h']).max() > 0.9 * np.sqrt(16.0 * T - 1)                                     # ... and the case approaches it
        if family in ('constant', 'constant_beta0'):
            exact = bits(a['stats'][:, 1, 0]) == bits(np.array(R.CONST))                    # the computed mean of the constant group is exact
            if T in (1, 2, 16):
                assert exact.all(), 'one row per thread and 16 T a power of two: the mean of a constant group is exact'
            he = np.zeros(x.shape, bool)
            he[exact, :, 16:32] = True
            assert R.mask_violations(mask > 0, fb['z'], fb['dz'], he, beta) == 0            # h = 0 exactly: z = beta, and z = 0 is "not taken"
            assert same_bits(a['y'][exact][:, :, 16:32], np.broadcast_to(np.maximum(beta[16:32], 0), (int(exact.sum()), T, 16)).astype(F32))


# ------------------------------------------------------------------------------------------------------------------ ragged forward
@pytest.mark.parametrize('T,B,C,lens', [(17, 3, 192, (17, 1, 0)), (17, 3, 192, (15, 16, 17)), (129, 3, 192, (0, 129, 16)), (256, 3, 192, (255, 17, 256)),
                                        (17, 1, 64, (0,)), (33, 1, 64, (32,)), (256, 1, 64, (241,))])
def test_forward_ragged(E, T, B, C, lens):
    for family in ('benign', 'mixed', 'offset1000'):
        x, gamma, beta, _, _ = case(family, B, T, C)
        fb = R.forward_budget(x, gamma, beta, lens)
        a = run_forward(E, x, gamma, beta, lens=lens)                                       # x rows t >= len hold NaN: never read
        for b, L in enumerate(lens):
            assert not bits(a['y'][b, L:]).any(), (b, 'rows t >= len are not exact zeros')
        judge_forward(f'ragged {family} B={B} T={T} C={C} lens={"/".join(map(str, lens))}', a, fb, lens)
        for b, L in enumerate(lens):
            if L == 0:
                assert np.isnan(a['stats'][b]).all()                                        # the header: the mean of no frames
                continue
            d = run_forward(E, np.ascontiguousarray(x[b:b + 1, :L]), gamma, beta)           # the same per-thread partition: the same bits
            assert same_bits(a['y'][b, :L], d['y'][0]) and same_bits(a['stats'][b], d['stats'][0]), (family, b, L)


# ------------------------------------------------------------------------------------------------------------------ chunked forward, T > 256
@pytest.mark.parametrize('T,B,C', [(257, 3, 192), (320, 3, 192), (321, 1, 64), (1000, 3, 192), (8192, 1, 64)])
def test_forward_long(E, T, B, C):
    lens = {3: (T, 200, 257), 1: (T - 70,)}[B]
    for family in (('benign', 'offset1000', 'mixed') if T <= 1000 else ('mixed',)):
        x, gamma, beta, _, fb = case(family, B, T, C)
        if fb is None:
            fb = R.forward_budget(x, gamma, beta, long_path=True)
        a = run_forward(E, x, gamma, beta)
        judge_forward(f'long {family} B={B} T={T} C={C} dense', a, fb)
        b = run_forward(E, x, gamma, beta)
        assert same_bits(a['y'], b['y']) and same_bits(a['stats'], b['stats']), (family, 'a second run differs')
        fr = R.forward_budget(x, gamma, beta, lens, long_path=True)
        r = run_forward(E, x, gamma, beta, lens=lens)
        for i, L in enumerate(lens):
            assert not bits(r['y'][i, L:]).any()
        judge_forward(f'long {family} B={B} T={T} C={C} lens={"/".join(map(str, lens))}', r, fr, lens)
        r2 = run_forward(E, x, gamma, beta, lens=lens)
        assert same_bits(r['y'], r2['y']) and same_bits(r['stats'], r2['stats'])


# ------------------------------------------------------------------------------------------------------------------ plans
_INTERP = {}


def engine_plan(E, B, T, P, seed):
    """A plan of an 'interp' engine (left bound in the engine for interp_backward) -> (eng, i0, lam, nrows) numpy; equal to the oracle's."""
    key = (B, T, P)
    if key not in _INTERP:
        _INTERP[key] = E.Engine('interp', W.default_hparams(max_len_pad=P), B, max(T, P))
    eng = _INTERP[key]
    rs = np.random.RandomState(seed)
    sc = (0.5 + rs.random_sample(B * 7)).astype(F32)
    ls = rs.randint(19, 32, size=B * 7).astype(np.int64)
    lens = np.array([T, max(T - 37, 2), max(T // 3, 2)][:B])
    _, i0, lam, cnt = eng.interp_forward(torch.zeros(B, T, 4), lens, sc, ls, want_plan=True)
    i0, lam, cnt = i0.cpu().numpy(), lam.cpu().numpy(), cnt.cpu().numpy()
    ri0, rlam, rcnt, rn = interp_np.interp_plan(sc, ls, lens, max_len_pad=P)
    assert np.array_equal(i0, ri0) and same_bits(lam, rlam) and np.array_equal(cnt, rcnt) and np.array_equal(np.minimum(cnt, P), rn)
    return eng, i0.astype(np.int32), lam.astype(F32), np.minimum(cnt, P).astype(np.int32)


def edge_plan(B, T, P, shift):
    """Hand-made plans, one kind per utterance: every row on one source row; i0 = T - 1 with lam > 0 (touches the zero row T); nrows = 0;
    sorted random rows with nrows = P."""
    rng = np.random.default_rng([31, T, P, shift])
    i0, lam, nrows = np.zeros((B, P), np.int32), np.zeros((B, P), F32), np.zeros(B, np.int32)
    for b in range(B):
        kind = (b + shift) % 4
        lam[b] = (0.05 + 0.9 * rng.random(P)).astype(F32)
        nrows[b] = P
        if kind == 0:
            i0[b] = T // 2
        elif kind == 1:
            i0[b] = T - 1
        elif kind == 2:
            nrows[b] = 0
            i0[b] = 12345                                   # rows past nrows are never read
        else:
            i0[b] = np.sort(rng.integers(0, T, P))
    return i0, lam, nrows


def host_check(plan, T, P, start=None):
    """the plan contract (include/speechsplit_amd.h) asserted on the host before every launch: a test bug must not become a wild index"""
    i0, lam, nrows = plan
    assert 1 <= P <= 258 and i0.shape[1] == P and ((0 <= nrows) & (nrows <= P)).all() and np.isfinite(lam).all()
    for b in range(len(nrows)):
        live = i0[b, :nrows[b]]
        assert ((0 <= live) & (live < T)).all() and (np.diff(live) >= 0).all(), b
    if start is not None:
        assert start.shape == (len(nrows), T + 1) and (start[:, 0] == 0).all() and (np.diff(start, axis=1) >= 0).all() and (start[:, T] == nrows).all()
        for b in range(len(nrows)):
            assert np.array_equal(start[b], np.searchsorted(i0[b, :nrows[b]], np.arange(T + 1), side='left')), b


# ------------------------------------------------------------------------------------------------------------------ gather form
def check_gather(E, tag, x, gamma, beta, plan, P):
    B, T, C = x.shape
    host_check(plan, T, P)
    plain = run_forward(E, x, gamma, beta)
    want = interp_np.interp_apply(np.concatenate([plain['y'], np.zeros((B, 1, C), F32)], 1), *plan)        # row T reads as zeros
    g = run_forward(E, x, gamma, beta, plan=plan, P=P)
    assert same_bits(g['stats'], plain['stats']), (tag, 'stats differ from the plain forward')
    assert same_bits(g['y'], want), (tag, 'y differs from the oracle gather of the plain kernel\'s y')
    for b in range(B):
        assert not bits(g['y'][b, plan[2][b]:]).any(), (tag, b)
    for scale in (16.0, 0.5):
        v = run_forward(E, x, gamma, beta, plan=plan, P=P, img='v2', img_scale=scale)
        assert same_bits(v['y'], want) and same_bits(v['stats'], plain['stats'])
        for b in range(B):
            ref = E.split_image(v['y_dev'].t[b, 2:2 + P], scale)
            assert np.array_equal(v['img'][b], ref.view(torch.int32).cpu().numpy()), (tag, scale, b, 'v2 image')
    h = run_forward(E, x, gamma, beta, plan=plan, P=P, img='bf16')
    assert same_bits(h['y'], want)
    assert np.array_equal(h['img'].view(np.uint16), R.bf16_rne(want)), (tag, 'bf16 image')
    print(f'FIG gather {tag} bit-identical: stats, y, v2 image (16, 0.5), bf16 image')


@pytest.mark.parametrize('B,C', SHAPES)
@pytest.mark.parametrize('T', (8, 128, 129, 192, 193, 255, 256))
def test_gather(E, T, B, C):
    P = T
    for family in ('benign', 'mixed'):
        x, gamma, beta, _, _ = case(family, B, T, C)
        _, i0, lam, nrows = engine_plan(E, B, T, P, seed=100 + T)
        check_gather(E, f'{family} B={B} T={T} C={C} engine plan nrows={"/".join(map(str, nrows))}', x, gamma, beta, (i0, lam, nrows), P)
    for shift in ((0, 1) if B == 3 else (1, 3)):
        check_gather(E, f'benign B={B} T={T} C={C} edge plan {shift}', *case('benign', B, T, C)[:3], edge_plan(B, T, P, shift), P)


# ------------------------------------------------------------------------------------------------------------------ backward
ACC0 = (0.5, -0.25, 2.0)


def run_backward(E, x, dy, gamma, beta, stats, amax0=0.0, part=False, scatter=None, src=None, P=None, img=True):
    """One ss_op_gn_relu_bwd launch on fresh guarded buffers -> dict(dx, dgamma, dbeta, dbias, amax, img) numpy; guards checked.
    dy None (scatter form): the dy slab's real rows start as the guard NaN -- written, never read."""
    B, T, C = x.shape
    xs, ga, be, st = slab_in(x, 'x'), vec(gamma, 'gamma'), vec(beta, 'beta'), vec(stats, 'stats')
    ds = slab_out(B, T, C, 'dy', real=dy)
    if dy is not None:
        ds.t[:, :2] = 0                                     # an input: zero halo rows, as the layout says
        ds.t[:, 2 + T:] = 0
    acc = [G.Guarded((C,), role='out', device='cuda', fill=torch.full((C,), v) + torch.arange(C) / 64.0, name=n)
           for v, n in zip(ACC0, ('g_gamma', 'g_beta', 'g_bias'))]
    am = G.Guarded((1,), role='out', device='cuda', fill=float(amax0), name='amax')
    pt = G.out((B, 3, C), 'cuda', name='part') if part else None
    di = slab_out(B, T, C, 'dy_img', dtype=torch.bfloat16) if img else None
    bufs = [xs, ga, be, st, ds, am] + acc + [b for b in (pt, di) if b is not None]
    sc = sr = None
    if scatter is not None:
        sc = [vec(scatter[0], 'lam'), vec(scatter[1], 'start')]
        s = np.zeros((B, P + 4, C), F32)
        s[:, 2:2 + P] = src
        sr = G.inp(torch.from_numpy(s), 'cuda', ld=ld_of(C), name='src')
        bufs += sc + [sr]
    E.gn_relu_bwd(xs.t, ds.t, ga.t, be.t, st.t, acc[0].t, acc[1].t, acc[2].t, amax=am.t, part=pt.t if part else None,
                  scatter=(sc[0].t, sc[1].t) if sc else None, src=sr.t if sr is not None else None, dy_img=di.t if img else None)
    torch.cuda.synchronize()
    for g in bufs:
        g.check(written=False if g in (ds, di) else None)
    COUNT['launches'] += 1
    COUNT['buffers'] += len(bufs)
    halo_kept(ds, T, 0.0 if dy is not None else HALO_FILL)
    out = dict(dx=real(ds, T), dgamma=acc[0].t.cpu().numpy(), dbeta=acc[1].t.cpu().numpy(), dbias=acc[2].t.cpu().numpy(), amax=am.t.cpu().numpy())
    if img:
        halo_kept(di, T)
        out['img'] = di.t[:, 2:2 + T].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return out


def acc0(C):
    return [np.full(C, v, F32) + (np.arange(C) / 64.0).astype(F32) for v in ACC0]


def judge_backward(tag, got, bb, C, amax0=0.0):
    ref, a0 = bb['ref'], acc0(C)
    r = dict(dx=R.ratio(got['dx'] - ref['dx'], bb['ddx']))
    for k, name in enumerate(('dgamma', 'dbeta', 'dbias')):
        r[name] = R.ratio(got[name] - (a0[k].astype(np.float64) + ref[name]), bb[name])
    print(f'FIG {tag} ' + ' '.join(f'{k}={v:.3g}' for k, v in r.items()))
    assert max(r.values()) <= 1.0, (tag, r)
    want = max(np.float32(amax0), np.abs(got['dx']).max())
    assert same_bits(got['amax'], np.array([want], F32)), (tag, 'amax', got['amax'], want)
    if 'img' in got:
        assert np.array_equal(got['img'], R.bf16_rne(got['dx'])), (tag, 'dy_img is not bf16(dx)')
    return max(r.values())


@pytest.mark.parametrize('B,C', SHAPES)
@pytest.mark.parametrize('T', (1, 17, 128, 192, 193, 256))
def test_backward(E, T, B, C):
    for family in R.FAMILIES:
        x, gamma, beta, dy, fb = case(family, B, T, C)
        f = run_forward(E, x, gamma, beta)
        mask = E.gn_relu_mask(f['xs'].t, f['ga'].t, f['be'].t, f['st'].t).cpu().numpy() > 0
        he = None
        if family == 'constant_beta0':
            he = np.zeros(x.shape, bool)
            he[bits(f['stats'][:, 1, 0]) == bits(np.array(R.CONST)), :, 16:32] = True
        assert R.mask_violations(mask, fb['z'], fb['dz'], he, beta) == 0, (family, 'the branch differs from float64 outside the kink budget')
        bb = R.backward_budget(x, dy, gamma, beta, mask, acc0(C))
        tag = f'backward {family} B={B} T={T} C={C}'
        a = run_backward(E, x, dy, gamma, beta, f['stats'])
        judge_backward(tag, a, bb, C)
        with Tuned(E):
            d1 = run_backward(E, x, dy, gamma, beta, f['stats'], amax0=1e30, part=True)     # a larger preset amax survives
            d2 = run_backward(E, x, dy, gamma, beta, f['stats'], amax0=1e30, part=True)
        judge_backward(tag + ' deterministic', d1, bb, C, amax0=1e30)
        assert all(same_bits(d1[k], d2[k]) for k in d1), (tag, 'deterministic runs differ')
        assert same_bits(a['dx'], d1['dx'])                                                 # the mode changes the order of the column sums only


# ------------------------------------------------------------------------------------------------------------------ scatter form
def check_scatter(E, tag, x, gamma, beta, plan, P, eng=None):
    B, T, C = x.shape
    i0, lam, nrows = plan
    start = E.gn_plan_start(torch.from_numpy(i0), torch.from_numpy(nrows), T).numpy()
    host_check(plan, T, P, start)
    src = np.random.default_rng([41, B, T, P]).standard_normal((B, P, C)).astype(F32)
    f = run_forward(E, x, gamma, beta)
    mask = E.gn_relu_mask(f['xs'].t, f['ga'].t, f['be'].t, f['st'].t).cpu().numpy() > 0
    adj, adj_err = R.scatter_adjoint(src, i0, lam, nrows, T)
    bb = R.backward_budget(x, adj, gamma, beta, mask, acc0(C), dy_err=adj_err)
    with Tuned(E):
        s = run_backward(E, x, None, gamma, beta, f['stats'], part=True, scatter=(lam, start), src=src, P=P)
        judge_backward(f'scatter {tag}', s, bb, C)
        if eng is not None:                                                                 # the two-kernel route: interp_scatter, then the plain backward
            dyp = eng.interp_backward(torch.from_numpy(src), T).cpu().numpy()
            assert R.ratio(dyp - adj, adj_err) <= 1.0
            p = run_backward(E, x, dyp, gamma, beta, f['stats'], part=True)
            assert all(same_bits(s[k], p[k]) for k in s), (tag, [k for k in s if not same_bits(s[k], p[k])])
            print(f'FIG scatter {tag} bit-identical to interp_backward + plain backward: dx, d_gamma, d_beta, d_bias, amax, dy_img')


@pytest.mark.parametrize('T,P,B,C', [(128, 128, 3, 192), (192, 192, 3, 192), (193, 193, 3, 192), (256, 256, 3, 192), (192, 160, 3, 192), (192, 161, 3, 192),
                                     (128, 128, 1, 64), (256, 256, 1, 64), (192, 161, 1, 64)])
def test_scatter(E, T, P, B, C):
    x, gamma, beta, _, _ = case('benign', B, T, C)
    eng, i0, lam, nrows = engine_plan(E, B, T, P, seed=200 + T + P)
    check_scatter(E, f'benign B={B} T={T} P={P} C={C} engine plan nrows={"/".join(map(str, nrows))}', x, gamma, beta, (i0, lam, nrows), P, eng)
    x, gamma, beta, _, _ = case('mixed', B, T, C)
    for shift in ((0, 1) if B == 3 else (1, 3)):
        check_scatter(E, f'mixed B={B} T={T} P={P} C={C} edge plan {shift}', x, gamma, beta, edge_plan(B, T, P, shift), P)
