"""The resampling kernels of csrc/interp.hip -- interp_plan, interp_gather, interp_quant, interp_scatter -- each launched alone through its
engine-free hook (ss_op_interp_plan / _gather / _quant / _scatter) on guarded buffers (tests/guarded.py) and judged against
oracle/interp_np.py: the plan, the gather and the quantiser BIT FOR BIT, the scatter per element against float64 with the budget
tests/test_interp_ref_selftest.py proves (n 2^-24 sum|terms|; exactly zero where no row contributes).

  plan       one launch of B = 512 utterances, S = 7, T = 224, for P in {8, 64, 192, 256, 512} at ncand = 64 and P = 192 at ncand = 38: the
             reference-range draws with lengths from 0 .. T, the stretched family, and hand-made rows (scales 0.5, 1.0, nextafter(1.5, 0),
             scales whose fp32 quotient is an integer while the float64 one is not; len_seg 1, 2, 32; len_seq 0, 1, 2, 3, T - 1, T); the batch's
             edge classes are asserted on the CPU first.  i0, lam, counts, nrows AND the inverse map start are the oracle's bits; entries
             beyond nrows are zero.  The len_seq_const form equals the array form.
  gather     C in {1, 3, 64, 81, 128, 256, 520}, dense views and haloed slabs; source rows at or beyond len_seq hold the guard NaN; -0.0 and
             operands whose products are subnormal; the image form at scales 16 and 0.5 equals ss_op_split_image of y
  quantiser  NOH = 257 in rows of 260 columns, CM in {1, 80, 129}: the 255 half-way values, 0, -0.0, the smallest subnormal, 1.0, 1.5, NaN on
             lam = 0 rows; -1e10 neighbours of voiced frames at lam in (0, 1); dead rows
  scatter    C in {1, 64, 130, 256} on plans with collisions and skipped frames; frames nobody contributes to and frames at or beyond
             len_seq exactly zero; repeat bits

Each test prints `FIG <test> <case> <differing elements, or worst error / budget>`."""
import numpy as np
import pytest
import torch

from oracle import interp_np as O
from tests import guarded as G
from tests import interp_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
HALO_FILL = -7.25
NAN = np.array([G.NAN32], np.uint32).view(F32)[0]
ODD = 67


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


@pytest.fixture(scope='module')
def batch():
    return R.plan_batch()


def gin(a, name, ld=None, offset=64):
    a = np.ascontiguousarray(a)
    return G.inp(torch.from_numpy(a), 'cuda', ld=ld if ld is not None else a.shape[-1], name=name, offset=offset)


def gout(shape, name, ld=None, fill=None, dtype=torch.float32, offset=64):
    if isinstance(fill, np.ndarray):
        fill = torch.from_numpy(np.ascontiguousarray(fill))
    return G.Guarded(shape, ld=ld, role='out', dtype=dtype, device='cuda', fill=fill, name=name, offset=offset)


def host(g):
    return g.t.contiguous().cpu().numpy()


def fig(test, case, v):
    print(f'FIG {test} {case} {v if isinstance(v, int) else format(v, ".4f")}')


def done(bufs):
    torch.cuda.synchronize()
    G.check_all([b for b in bufs if b is not None])


def plan_on_device(E, sc, ls, n, T, P, ncand=64):
    B = len(sc)
    const = isinstance(n, int)
    gs, gl, gn = gin(sc, 'scales', offset=ODD), gin(ls, 'len_seg', offset=ODD), None if const else gin(n, 'len_seq', offset=ODD)
    outs = [gout((B, P), 'i0', dtype=torch.int32, offset=ODD), gout((B, P), 'lam', offset=ODD), gout((B,), 'nrows', dtype=torch.int32, offset=ODD),
            gout((B,), 'counts', dtype=torch.int32, offset=ODD), gout((B, T + 1), 'start', dtype=torch.int32, offset=ODD)]
    E.interp_plan(gs.t, gl.t, n if const else gn.t, T, P, ncand, *[o.t for o in outs])
    done([gs, gl, gn] + outs)
    return [host(o) for o in outs]                          # i0, lam, nrows, counts, start


# ------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize('P,ncand', [(P, 64) for P in R.PLAN_P] + [(192, 38)], ids=lambda v: str(v))
def test_plan(E, batch, P, ncand):
    T = R.PLAN_T
    sc, ls, n, cls = batch
    assert len(R.integer_quotient_scales()) >= R.S and cls['integer-quotient']               # such scales were found, and are in the batch
    e = R.plan_edges(sc, ls, n, T, P, ncand)
    assert e['dead'] >= 5 and e['partial'] > 0 and e['lam=0 rows'] > 0, e
    if P <= 256 and ncand == 64:
        assert e['full'] > 0 and e['cut-mid-segment'] > 0, e
    ri0, rlam, rcounts, rnrows, rstart = R.plan_ref(sc, ls, n, T, P, ncand)
    i0, lam, nrows, counts, start = plan_on_device(E, sc, ls, n, T, P, ncand)
    bad = {'i0': R.n_diff(i0, ri0), 'lam': R.n_diff(lam, rlam), 'nrows': R.n_diff(nrows, rnrows), 'counts': R.n_diff(counts, rcounts),
           'start': R.n_diff(start, rstart)}
    beyond = np.arange(P)[None, :] >= nrows[:, None]
    bad['beyond-nrows'] = int(np.count_nonzero(i0[beyond])) + int(np.count_nonzero(R.bits(lam)[beyond]))
    for k, v in bad.items():
        fig('plan', f'P={P}/ncand={ncand}/{k}', v)
    assert not any(bad.values()), bad


def test_plan_constant_length(E, batch):
    """len_seq_dev NULL: every utterance has len_seq_const frames"""
    T, P = R.PLAN_T, 192
    sc, ls, _, _ = batch
    sc, ls = sc[:64], ls[:64]
    bad = 0
    for const in (0, 1, 100, T):
        ref = R.plan_ref(sc, ls, np.full(64, const, np.int32), T, P)
        got = plan_on_device(E, sc, ls, const, T, P)
        bad += sum(R.n_diff(g, r) for g, r in zip(got, (ref[0], ref[1], ref[3], ref[2], ref[4])))
    fig('plan', 'len_seq_const', bad)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ gather
GT, GP, GB = 64, 48, 8


def _plan_bufs(p):
    return (gin(p['i0'], 'i0', offset=ODD), gin(p['lam'], 'lam', offset=ODD), gin(p['nrows'], 'nrows', offset=ODD))


@pytest.mark.parametrize('C', R.GATHER_C)
def test_gather(E, C):
    p = R.small_plan(GT, GP, GB)
    x = R.gather_input(GB, GT, C, p['len_seq'], NAN)
    clean = R.gather_input(GB, GT, C, p['len_seq'], F32(0))
    ref = O.interp_apply(clean, p['i0'], p['lam'], p['nrows'])
    live = ref[np.arange(GP)[None, :] < p['nrows'][:, None]]
    assert np.isfinite(ref).all() and ((live != 0) & (np.abs(live) < np.finfo(F32).tiny)).any(), 'no subnormal result in the case'
    gi, gl, gn = _plan_bufs(p)
    # dense views, odd offsets, row strides above C
    gx, gy = gin(x, 'x', ld=C + 3, offset=ODD), gout((GB, GP, C), 'y', ld=C + 5, offset=ODD + 2)
    E.interp_gather(gi.t, gl.t, gn.t, gx.t, gy.t)
    done((gi, gl, gn, gx, gy))
    bad = R.n_diff(host(gy), ref)
    # haloed slabs: the views start at row 2; halo rows keep their bits
    xs = np.full((GB, GT + 4, C), NAN, F32)
    xs[:, 2:2 + GT] = x
    gx = gin(xs, 'x_slab', ld=C + 4, offset=ODD)
    gy = gout((GB, GP + 4, C), 'y_slab', ld=C + 7, offset=ODD, fill=np.full((GB, GP + 4, C), HALO_FILL, F32))
    gy.t[:, 2:2 + GP] = float('nan')
    E.interp_gather(gi.t, gl.t, gn.t, gx.t[:, 2:2 + GT], gy.t[:, 2:2 + GP])
    done((gi, gl, gn, gx, gy))
    got = host(gy)
    assert np.all(got[:, :2] == HALO_FILL) and np.all(got[:, 2 + GP:] == HALO_FILL), 'a halo row changed'
    bad += R.n_diff(got[:, 2:2 + GP], ref)
    fig('gather', f'C={C}', bad)
    assert bad == 0


@pytest.mark.parametrize('scale', (16.0, 0.5))
@pytest.mark.parametrize('C', R.GATHER_IMG_C)
def test_gather_image(E, C, scale):
    p = R.small_plan(GT, GP, GB)
    x = R.gather_input(GB, GT, C, p['len_seq'], NAN)
    ref = O.interp_apply(R.gather_input(GB, GT, C, p['len_seq'], F32(0)), p['i0'], p['lam'], p['nrows'])
    gi, gl, gn = _plan_bufs(p)
    gx = gin(x, 'x', ld=C + 4)
    gy, gimg = gout((GB, GP, C), 'y', ld=C + 8), gout((GB, GP, C), 'y_img', ld=C + 8)
    gsc = gin(np.array([scale], F32), 'img_scale', offset=ODD)
    E.interp_gather(gi.t, gl.t, gn.t, gx.t, gy.t, y_img=gimg.t, img_scale=gsc.t if scale != 16.0 else None)
    done((gi, gl, gn, gx, gy, gimg, gsc))
    bad = R.n_diff(host(gy), ref)
    want = E.split_image(gy.t.contiguous().reshape(GB * GP, C), scale).cpu().numpy().reshape(GB, GP, C)
    bad += R.n_diff(host(gimg), want)
    fig('gather_image', f'C={C}/scale={scale}', bad)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize('CM', R.QUANT_CM)
def test_quant(E, CM):
    P = T = 256
    yo_ld = 260
    c = R.quant_case(P, T, CM)
    rq, rmel, roh, _ = R.quant_ref(c, yo_ld)
    B = 3
    gi, gl, gn = _plan_bufs(c)
    gm, gf = gin(c['mel'].reshape(B * T, CM), 'mel', offset=ODD), gin(c['f0'], 'f0', offset=ODD)
    gym = gout((B, P, CM), 'ymel', ld=CM + 3, offset=ODD)
    goh = gout((B, P, yo_ld), 'onehot', offset=ODD)         # the kernel owns every column of the row stride: padding columns are written zero
    gq = gout((B, P), 'qidx', dtype=torch.int32, offset=ODD)
    E.interp_quant(gi.t, gl.t, gn.t, gm.t.reshape(B, T, CM), gf.t, gym.t, goh.t, R.NOH, gq.t)
    done((gi, gl, gn, gm, gf, gym, goh, gq))
    bad = {'qidx': R.n_diff(host(gq), rq), 'mel': R.n_diff(host(gym), rmel), 'onehot': R.n_diff(host(goh), roh)}
    for k, v in bad.items():
        fig('quant', f'CM={CM}/{k}', v)
    assert not any(bad.values()), bad


# ------------------------------------------------------------------------------------------------ scatter
def ratio(got, ref, budget):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), 'a result is not finite'
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


@pytest.mark.parametrize('C', R.SCATTER_C)
def test_scatter(E, C):
    p = R.small_plan(GT, GP, GB)
    dy = np.random.default_rng([25, C]).standard_normal((GB, GP, C)).astype(F32)
    ref, mag, cnt = R.scatter_ref(dy, p['i0'], p['lam'], p['nrows'], GT)
    fed = dy.copy()
    fed[np.arange(GP)[None, :] >= p['nrows'][:, None]] = NAN                                 # rows behind nrows are never read
    gl, gs = gin(p['lam'], 'lam', offset=ODD), gin(p['start'], 'start', offset=ODD)
    gdy = gin(fed, 'dy', ld=C + 3, offset=ODD)
    runs = []
    for rep in range(2):
        gdx = gout((GB, GT, C), 'dx', ld=C + 5, offset=ODD + 2)
        E.interp_scatter(gl.t, gs.t, gdy.t, gdx.t)
        done((gl, gs, gdy, gdx))
        runs.append(host(gdx))
    assert R.n_diff(runs[0], runs[1]) == 0, 'a repeat differs'
    got = runs[0]
    assert not R.bits(got)[cnt == 0].any(), 'a frame nobody contributes to is not +0.0'
    for b in range(GB):
        assert not R.bits(got[b, p['len_seq'][b]:]).any(), 'a frame at or beyond len_seq is not zero'
    q = ratio(got, ref, R.scatter_budget(mag, cnt))
    fig('scatter', f'C={C}', q)
    assert q <= 1.0
