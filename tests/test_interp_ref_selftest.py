"""tests/interp_ref.py and the oracle's inverse map proven on the CPU, without a GPU.

1. oracle.interp_np.interp_start is the inverse of the plan: through it the scatter visits exactly the (row, frame) pairs the oracle's
   interp_backward adds; the oracle's plan equals the reference's own formulation in torch on the batch's draws.
2. The plan batch holds every edge class at every P it is launched with, and scales whose fp32 quotient is an integer while the float64
   quotient is not were found; a plan from a float64 (or reciprocal) division differs on them.
3. The quantiser cases: the 255 half-way values multiply to exactly k + 0.5, their classes alternate by parity, the special values get the
   classes the issue names; a round-half-up or truncating quantiser, and one without the clamp, differ.
4. The scatter's budget: an emulation of the kernel's own order stays inside n u sum|terms|, and each named mutant -- neighbour weights
   swapped, start off by one, one contributing row dropped -- falls outside it."""
import numpy as np
import pytest
import torch

import interp_ref as R
from oracle import interp_np as O

F32 = np.float32


def ratio(got, ref, budget):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


# ------------------------------------------------------------------------------------------------ 1. the inverse map
def test_start_is_the_inverse_of_the_plan():
    T, P = 64, 48
    p = R.small_plan(T, P)
    st = p['start']
    assert st.shape == (8, T + 1) and st.dtype == np.int32 and not st[:, 0].any() and np.array_equal(st[:, T], p['nrows'])
    for b in range(8):
        pairs = set()
        for i in range(T):
            pairs |= {(r, i) for r in range(st[b, i], st[b, i + 1])}                         # rows with i0 == i
            if i > 0:
                pairs |= {(r, i) for r in range(st[b, i - 1], st[b, i])}                     # rows with i0 == i - 1
        want = set()
        for r in range(p['nrows'][b]):
            want |= {(r, int(p['i0'][b, r])), (r, int(p['i0'][b, r]) + 1)}
        assert pairs == want
    assert (np.diff(p['i0'][1, :p['nrows'][1]]) == 0).any(), 'no collision (two rows with one i0) in the plan'
    assert (np.diff(p['i0'][2, :p['nrows'][2]]) > 1).any(), 'no skipped frame in the plan'
    assert p['nrows'][0] == 0 and p['nrows'][3] == 0 and (p['counts'] > P).any() and ((p['nrows'] > 0) & (p['nrows'] < P)).any()


def test_oracle_plan_is_the_reference_formulation():
    """model.py:389-418 restated in torch on a slice of the batch (fp32 division, floor, masks as float comparisons)"""
    T = R.PLAN_T
    sc, ls, n, _ = R.plan_batch()
    pick = np.r_[0:80, 200:230]
    sc, ls, n = sc[pick], ls[pick], n[pick]
    B = len(n)
    i0, lam, counts, nrows, _ = R.plan_ref(sc, ls, n, T, 192)
    idx = torch.arange(64).unsqueeze(0).expand(B * R.S, -1)
    q = idx / torch.from_numpy(sc.reshape(-1, 1))
    fl = torch.floor(q)
    lm = q - fl
    seg = torch.from_numpy(ls.reshape(-1, 1)).long()
    m1 = fl < (seg - 1)
    off = torch.cumsum(seg.view(B, -1), dim=-1)
    off = torch.nn.functional.pad(off[:, :-1], (1, 0)).view(-1, 1)
    org = fl + off
    m2 = org < (torch.from_numpy(n).long().repeat_interleave(R.S).unsqueeze(-1) - 1)
    mask = m1 & m2
    assert np.array_equal(mask.view(B, -1).sum(1).numpy(), counts)
    for b in range(B):
        sel = mask.view(B, -1)[b]
        k = int(nrows[b])
        assert np.array_equal(org.view(B, -1)[b][sel][:k].long().numpy(), i0[b, :k]) and R.n_diff(lm.view(B, -1)[b][sel][:k].numpy(), lam[b, :k]) == 0


# ------------------------------------------------------------------------------------------------ 2. the plan batch
def test_integer_quotient_scales_exist_and_matter():
    found = R.integer_quotient_scales()
    assert len(found) >= R.S, len(found)
    differ = 0
    for sc, lane in found:
        q32 = F32(lane) / sc
        assert q32 == np.floor(q32) and 0.5 <= sc < 1.5
        q64 = float(lane) / float(sc)
        differ += np.floor(q64) != np.floor(q32) or (F32(lane) * (F32(1) / sc)) != q32
    assert differ > 0, 'on none of them would a float64 or a reciprocal division give another frame or lam'
    assert any(float(lane) / float(sc) < float(F32(lane) / sc) for sc, lane in found), 'none where the wider quotient floors one frame lower'


@pytest.mark.parametrize('P', R.PLAN_P)
def test_plan_batch_holds_every_edge(P):
    T = R.PLAN_T
    sc, ls, n, cls = R.plan_batch()
    assert sc.shape == (R.PLAN_B, R.S) and sc.dtype == F32 and ls.dtype == np.int32 and n.min() == 0 and n.max() == T
    for name in ('len_seq=0', 'len_seq=1', 'len_seq=2', 'len_seq=3', f'len_seq={T - 1}', f'len_seq={T}', 'scale=0.5', 'scale=1.0', 'scale=1.5-',
                 'integer-quotient', 'len_seg=1', 'len_seg=2', 'len_seg=32', 'len_seg-mixed', 'stretched', 'reference'):
        assert cls.get(name), name
    i0, lam, counts, nrows, start = R.plan_ref(sc, ls, n, T, P)
    e = R.plan_edges(sc, ls, n, T, P)
    assert e['dead'] >= 5 and e['partial'] > 0 and e['lam=0 rows'] > 0, e
    if P <= 256:
        assert e['full'] > 0 and e['truncated'] > 0 and e['cut-mid-segment'] > 0, e
    if P <= 192:
        assert (counts[cls['stretched']] > P).all()
    assert e['max count'] > 219
    for b in cls['scale=1.0']:
        assert nrows[b] > 0 and not lam[b].any()
    for b in cls['len_seg=1']:
        assert counts[b] == 0
    for b in cls['len_seg=2']:
        assert counts[b] > 0 and set(np.diff(i0[b, :nrows[b]])) <= {0, 2}                    # only candidate frame 0 of each segment
    for b in cls['integer-quotient'] if P == 512 else ():                                   # (untruncated)
        assert (lam[b, :nrows[b]] == 0).sum() > R.S                                          # more than the seven j = 0 candidates
    for b in range(R.PLAN_B):                                                               # entries beyond nrows are zero
        assert not i0[b, nrows[b]:].any() and not lam[b, nrows[b]:].any()
    live = np.arange(P)[None, :] < nrows[:, None]
    assert (i0[live] + 1 <= np.broadcast_to(n[:, None], i0.shape)[live] - 1).all(), 'a plan indexes a frame at or beyond len_seq'


def test_ncand_38_is_its_own_plan():
    T, P = R.PLAN_T, 192
    sc, ls, n, _ = R.plan_batch()
    a = R.plan_ref(sc, ls, n, T, P, ncand=38)
    b = R.plan_ref(sc, ls, n, T, P, ncand=64)
    assert (a[2] < b[2]).any() and (a[2] <= b[2]).all() and a[2].max() <= 38 * R.S


def test_wider_division_gives_another_plan():
    sc, ls, n, cls = R.plan_batch()
    rows = cls['integer-quotient']
    j = np.arange(64, dtype=np.float64)
    differ = 0
    for b in rows:
        for s in range(R.S):
            q64 = j / float(sc[b, s])
            q32 = (j.astype(F32) / sc[b, s]).astype(F32)
            differ += int((np.floor(q64) != np.floor(q32)).sum())
    assert differ > 0


# ------------------------------------------------------------------------------------------------ 3. the quantiser
def test_quantiser_cases():
    v = R.half_way_values()
    q = R.quant_class(v)
    assert np.array_equal(q, np.where(np.arange(255) % 2 == 0, np.arange(255), np.arange(255) + 1) + 1)     # ties to even
    half_up = np.floor((v * F32(255)).astype(np.float64) + 0.5).astype(np.int64) + 1
    assert (half_up != q).sum() == 128                                                       # round-half-up differs at every even k
    assert ((v * F32(255)).astype(np.int64) + 1 != q).any()                                  # truncation differs
    c = R.quant_case()
    want = {0.0: 0, 1.0: 256, 1.5: 256, 0.5: 129}          # (0.75 is the filler in front of the NaN: its row reads 0 * NaN)
    qr, ymel, oh, f = R.quant_ref(c, 260)
    seen = {}
    for (b, r), val in zip(c['rows'], c['vals']):
        assert c['lam'][b, r] == 0
        seen[repr(val)] = int(qr[b, r])
        if not np.isnan(val) and float(val) in want and not np.signbit(val):
            assert qr[b, r] == want[float(val)], val
    assert seen[repr(F32(-0.0))] == 0 and seen[repr(F32(1e-45))] == 1 and seen[repr(F32(np.nan))] == 0
    assert np.isnan(f).sum() == 2                                                            # the NaN frame's own row and the filler in front of it
    assert qr.max() == 256 and (np.rint(F32(1.5) * F32(255)) + 1 > 256)                      # 1.5 needs the clamp
    assert (oh.sum(-1) == 1).all() and not oh[..., R.NOH:].any() and oh.shape[-1] == 260
    dead = np.arange(qr.shape[1])[None, :] >= c['nrows'][:, None]
    assert dead.any() and not qr[dead].any() and not ymel[dead].any() and (oh[dead][:, 0] == 1).all()
    # utterance 2: a voiced frame beside an unvoiced one at lam in (0, 1) comes out negative: class 0
    b, n = 2, c['nrows'][2]
    i, l = c['i0'][b, :n], c['lam'][b, :n]
    mixed = (l > 0) & ((c['f0'][b, i] > 0) != (c['f0'][b, i + 1] > 0))
    assert mixed.sum() > 10 and not qr[b, :n][mixed].any() and (qr[b, :n] > 0).any()


# ------------------------------------------------------------------------------------------------ 4. the scatter's budget
@pytest.mark.parametrize('C', (1, 5))
def test_scatter_budget_and_mutants(C):
    T, P = 64, 48
    p = R.small_plan(T, P)
    i0, lam, nrows = p['i0'], p['lam'], p['nrows']
    dy = np.random.default_rng(C).standard_normal((8, P, C)).astype(F32)
    ref, mag, cnt = R.scatter_ref(dy, i0, lam, nrows, T)
    bud = R.scatter_budget(mag, cnt)
    back = O.interp_backward(dy, i0, lam, nrows, T)
    assert np.allclose(back, ref, rtol=1e-5, atol=1e-6)                                      # the same adjoint as the oracle's
    assert cnt.max() >= 3 and (cnt == 0).any()
    for b in range(8):
        assert not cnt[b, p['len_seq'][b]:].any()                                            # no term at or beyond len_seq
    got = R.scatter_emulated(dy, i0, lam, nrows, T)
    assert ratio(got, ref, bud) <= 1.0
    assert not got[cnt == 0].any()
    assert ratio(R.scatter_emulated(dy, i0, lam, nrows, T, swap=True), ref, bud) > 1.0, 'neighbour weights swapped'
    shifted = p['start'].copy()
    shifted[:, 1:] = np.minimum(shifted[:, 1:] + 1, nrows[:, None])
    assert ratio(R.scatter_emulated(dy, i0, lam, nrows, T, start=shifted), ref, bud) > 1.0, 'start off by one'
    b = 1
    r = int(np.argmax(np.abs(dy[b, :nrows[b]]).min(-1) * np.minimum(lam[b, :nrows[b]], 1 - lam[b, :nrows[b]])))
    assert ratio(R.scatter_emulated(dy, i0, lam, nrows, T, drop=(b, r)), ref, bud) > 1.0, 'one contributing row dropped'
