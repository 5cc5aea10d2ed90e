"""tests/step_ops_ref.py proven on the CPU, without a GPU.

1. The float64 references equal torch's float64 mse_loss, cross_entropy and autograd (losses, column sums, the decoder input's adjoint, the
   speaker contraction).
2. A numpy float32 EMULATION of each kernel's own operation order stays inside its budget on every case tests/test_gpu_step_ops.py runs -- for
   the cross-entropy that is the fixed order, (x - mx) - logf(se).
3. Each MUTANT -- a subtly wrong kernel -- exceeds a budget (ratio > 1): the cross-entropy in the former mx + logf(se) order on the offset
   family; the mean over B T C against B T; 2 / n dropped; a column sum that skips its last short chunk; a column sum in fp32 arrival order on
   a cancelling input; dec_in_grad over f - 1 frames; both halves of a code sampled at the same frame; spk_grad without its last slice of g.
4. K is what the module says it is: measure_k() on this CPU lies at or below K_MEASURED and above half of it."""
import numpy as np
import pytest
import torch

import step_ops_ref as R

F32 = np.float32


def ratio(got, ref, budget):
    """worst |got - ref| / budget; an element with budget 0 must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    b = np.asarray(budget, np.float64)
    assert np.all(np.isfinite(err)) and np.all(b >= 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


# ------------------------------------------------------------------------------------------------ 1. references against torch
@pytest.mark.parametrize('shape', R.MSE_SHAPES)
def test_mse_ref_is_torch(shape):
    o, y = R.mse_case('normal', *shape)
    to = torch.from_numpy(o).double().requires_grad_()
    loss = torch.nn.functional.mse_loss(to, torch.from_numpy(y).double())
    loss.backward()
    l, d = R.mse_ref(o, y, 0.25)
    assert abs(l - float(loss.detach())) <= 1e-14 * abs(l)
    np.testing.assert_allclose(d, 0.25 * to.grad.numpy(), rtol=1e-13, atol=0)


@pytest.mark.parametrize('C', R.CE_CLASSES)
@pytest.mark.parametrize('family', ('normal', 'offset+1000', 'neg_inf', 'target_dominant'))
def test_ce_ref_is_torch(family, C):
    B, T = 3, 8
    x, y = R.ce_case(family, B, T, C)
    tx = torch.from_numpy(x).double().requires_grad_()
    loss = torch.nn.functional.cross_entropy(tx.reshape(B * T, C), torch.from_numpy(y).long().reshape(-1))
    loss.backward()
    l, row, d = R.ce_ref(x, y, 1.0)
    assert abs(l - float(loss.detach())) <= 1e-13 * abs(l) + 1e-300
    assert abs(row.mean() - l) <= 1e-15 * abs(l)
    np.testing.assert_allclose(d, tx.grad.numpy() * (R.ce_gs(B, T, 1.0) * B * T), rtol=1e-12, atol=1e-30)


def test_targets_cover_both_ends():
    for fam, B, T, C in R.ce_cases():
        x, y = R.ce_case(fam, B, T, C)
        assert (y.reshape(-1)[0] == 0 or B * T == 1) and y.reshape(-1)[-1] == C - 1 and y.min() >= 0 and y.max() < C
        assert np.all(np.isfinite(np.take_along_axis(x, y[..., None].astype(np.int64), -1)))          # -inf is never the target
        assert np.all(np.isfinite(x).any(axis=-1))


def test_colsum_ref_is_torch_and_formula():
    v = R.colsum_case('normal', 33, 257)
    out0 = np.linspace(-1, 1, 257).astype(F32)
    ref, bud = R.colsum_ref(v, out0)
    t = (torch.from_numpy(v).double().sum(0).float() + torch.from_numpy(out0)).numpy()
    assert np.array_equal(ref, t) and np.all(bud > 0)
    for cols in (1, 64, 65, 257, 4096):
        nb = -(-cols // 64)
        assert R.colsum_scratch_doubles(cols) == (-(-1024 // nb) + 1) * nb * 64
    assert R.colsum_chunks(17, 257) == (2, 9) and R.colsum_chunks(520, 257) == (33, 16) and R.colsum_chunks(520, 257, scratch=False) == (1, 520)
    assert R.colsum_chunks(16, 8) == (1, 16) and R.colsum_chunks(33, 64)[0] == 3


@pytest.mark.parametrize('name', sorted(R.DEC_SETS))
def test_dec_in_ref_adjoint_is_autograd(name):
    B, T = 3, 16
    layout = R.dec_layout(name)
    srcs, E, emb_col, ld = layout
    rng = np.random.default_rng(5)
    slabs = [torch.from_numpy(rng.standard_normal((B, T + 4, 2 * H))).requires_grad_() for H, *_ in srcs]
    emb = rng.standard_normal((B, E))
    # the forward as torch indexing, so that autograd gives the adjoint
    cols = []
    for (H, fr, col, _), o in zip(srcs, slabs):
        blk = torch.arange(T) // fr
        cols += [o[:, blk * fr + fr - 1 + 2, :H], o[:, blk * fr + 2, H:]]
    full = torch.cat(cols + [torch.from_numpy(emb)[:, None, :].expand(B, T, E), torch.zeros(B, T, R.DEC_SETS[name][2], dtype=torch.float64)], dim=2)
    ref = R.dec_in_ref([s.detach().numpy().astype(F32) for s in slabs], layout, emb.astype(F32), B, T)
    np.testing.assert_array_equal(ref, full.detach().numpy().astype(F32))
    d_in = rng.standard_normal((B, T, ld))
    full.backward(torch.from_numpy(d_in))
    for (_, r64, _), s in zip(R.dec_in_grad_chain(d_in, layout, B, T), slabs):           # float64 in: r64 is the exact adjoint
        np.testing.assert_allclose(r64, s.grad.numpy()[:, 2:2 + T], rtol=1e-13, atol=1e-13)
        assert np.all(s.grad.numpy()[:, :2] == 0) and np.all(s.grad.numpy()[:, 2 + T:] == 0)
    if name == 'compact':
        f = 8
        np.testing.assert_array_equal(R.dec_in_ref([s.detach().numpy().astype(F32) for s in slabs], layout, emb.astype(F32), B, T, f=f), ref[:, ::f])


def test_spk_ref_is_autograd():
    rng = np.random.default_rng(7)
    B, rows, H4, E, col0 = 2, 12, 4, 81, 3
    dg = rng.standard_normal((B, rows, 2 * H4))
    w = torch.from_numpy(rng.standard_normal((2 * H4, col0 + E + 2)))
    emb = torch.zeros(B, E, dtype=torch.float64, requires_grad=True)
    x = torch.zeros(B, rows, col0 + E + 2, dtype=torch.float64)
    x = torch.cat([x[:, :, :col0], emb[:, None, :].expand(B, rows, E), x[:, :, col0 + E:]], dim=2)
    (x @ w.T).backward(torch.from_numpy(dg))
    ref, bud = R.spk_ref(dg, w.numpy()[:H4], w.numpy()[H4:], col0, E)
    np.testing.assert_allclose(ref, emb.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert R.spk_split(4, 81) == (12, 1) and R.spk_split(2048, 513) == (1, 4096) and R.spk_split(2048, 256) == (4, 1024)


# ------------------------------------------------------------------------------------------------ 2. emulations inside, 3. mutants outside
@pytest.mark.parametrize('shape', R.MSE_SHAPES)
def test_mse_emulation_inside_and_mutants_outside(shape):
    worst = 0.0
    for fam in R.MSE_FAMILIES:
        for gsc in R.GRAD_SCALES:
            o, y = R.mse_case(fam, *shape)
            l, d = R.mse_ref(o, y, gsc)
            bl, bd = R.mse_budget(o, y, gsc)
            el, ed = R.mse_emulate(o, y, gsc)
            worst = max(worst, ratio(el, l, bl), ratio(ed, d, bd))
            if fam == 'equal':
                assert el == 0.0 and not ed.any()
    assert worst <= 1.0, worst
    o, y = R.mse_case('normal', *shape)
    _, ed = R.mse_emulate(o, y, 1.0, drop_two_over_n=True)
    assert ratio(ed, R.mse_ref(o, y, 1.0)[1], R.mse_budget(o, y, 1.0)[1]) > 1.0


@pytest.mark.parametrize('BT', R.CE_BT)
@pytest.mark.parametrize('C', R.CE_CLASSES)
def test_ce_emulation_inside_and_mutants_outside(C, BT):
    B, T = BT
    for fam in R.CE_FAMILIES:
        x, y = R.ce_case(fam, B, T, C)
        for gsc in (1.0, 1.0 / 3.0):
            l, row, d = R.ce_ref(x, y, gsc)
            bl, brow, bd = R.ce_budget(x, y, gsc)
            el, erow, ed = R.ce_emulate(x, y, gsc)
            assert max(ratio(el, l, bl), ratio(erow, row, brow), ratio(ed, d, bd)) <= 1.0, (fam, gsc)
            assert abs(ed.astype(np.float64).sum(axis=-1)).max() <= bd.sum(axis=-1).max()
        if fam.startswith('offset'):
            # shift-invariant: the offset family's budget is the unshifted case's (up to the rounding of 1000 + x itself)
            x0, y0 = R.ce_case('normal', B, T, C)
            assert np.array_equal(y0, y)
            _, _, bd0 = R.ce_budget(x0, y0, 1.0)
            assert np.all(R.ce_budget(x, y, 1.0)[2] <= 1.001 * bd0 + 1e-30) and np.all(bd0 <= 1.001 * R.ce_budget(x, y, 1.0)[2] + 1e-30)
            # the former order, lse = mx + logf(se), is far outside it
            ml, mrow, md = R.ce_emulate(x, y, 1.0, order='lse')
            _, brow, bd = R.ce_budget(x, y, 1.0)
            assert ratio(md, R.ce_ref(x, y, 1.0)[2], bd) > 1.0 and ratio(mrow, R.ce_ref(x, y, 1.0)[1], brow) > 1.0, fam
    if B * T * C > B * T:
        x, y = R.ce_case('normal', B, T, C)
        ml, _, md = R.ce_emulate(x, y, 1.0, mean_over_btc=True)
        l, _, d = R.ce_ref(x, y, 1.0)
        bl, _, bd = R.ce_budget(x, y, 1.0)
        assert ratio(ml, l, bl) > 1.0 and ratio(md, d, bd) > 1.0


@pytest.mark.parametrize('Rr', R.COLSUM_R)
def test_colsum_emulation_inside_and_mutants_outside(Rr):
    for cols in (257, 8, 24, 64):
        for fam in ('normal', 'cancelling'):
            v = R.colsum_case(fam, Rr, cols)
            out0 = np.linspace(0.5, 1.5, cols).astype(F32)
            ref, bud = R.colsum_ref(v, out0)
            for scratch in (True, False):
                got = R.colsum_emulate(v, out0, scratch)
                assert ratio(got, ref.astype(np.float64), bud) <= 1.0
                assert ratio(got, v.astype(np.float64).sum(0) + out0, bud) <= 1.0
    chunks, rpc = R.colsum_chunks(Rr, 257)
    if chunks > 1:
        v = R.colsum_case('normal', Rr, 257)
        out0 = np.ones(257, F32)
        ref, bud = R.colsum_ref(v, out0)
        assert ratio(R.colsum_emulate(v, out0, skip_last_chunk=True), ref.astype(np.float64), bud) > 1.0
    if chunks > 2:
        v = R.colsum_case('cancelling', Rr, 257)
        out0 = np.zeros(257, F32)
        ref, bud = R.colsum_ref(v, out0)
        order = np.random.default_rng(1).permutation(chunks)
        assert ratio(R.colsum_emulate(v, out0, fp32_order=order), ref.astype(np.float64), bud) > 1.0


@pytest.mark.parametrize('T', R.DEC_T)
@pytest.mark.parametrize('name', sorted(R.DEC_SETS))
def test_dec_in_grad_chain_inside_and_mutants_outside(name, T):
    B = 3
    layout = R.dec_layout(name)
    srcs, E, emb_col, ld = layout
    rng = np.random.default_rng([T, len(srcs)])
    d_in = rng.standard_normal((B, T, ld)).astype(F32)
    for (g, r64, ra), (H, fr, col, _), (m, _, _) in zip(R.dec_in_grad_chain(d_in, layout, B, T), srcs,
                                                       R.dec_in_grad_chain(d_in, layout, B, T, frames=max(0, srcs[0][1] - 1))):
        assert ratio(g, r64, (fr - 1) * R.U * ra) <= 1.0
        t = np.arange(T)
        assert not g[:, t % fr != fr - 1, :H].any() and not g[:, t % fr != 0, H:].any()              # zeros exactly at the unsampled frames
        if fr > 1 and fr == srcs[0][1]:
            assert ratio(m, r64, (fr - 1) * R.U * ra) > 1.0                                           # f - 1 frames
    slabs = [rng.standard_normal((B, T + 4, 2 * H)).astype(F32) for H, *_ in srcs]
    emb = rng.standard_normal((B, E)).astype(F32)
    if any(fr > 1 for _, fr, _, _ in srcs):
        assert not np.array_equal(R.dec_in_ref(slabs, layout, emb, B, T), R.dec_in_ref(slabs, layout, emb, B, T, same_frame=True))


@pytest.mark.parametrize('E', R.SPK_E)
@pytest.mark.parametrize('H4', (4, 64))
def test_spk_emulation_inside_and_mutant_outside(E, H4):
    rng = np.random.default_rng([E, H4])
    for rows in (1, 12, 260):
        dg = rng.standard_normal((2, rows, 2 * H4)).astype(F32)
        w = rng.standard_normal((2 * H4, 5 + E + 3)).astype(F32)
        ref, bud = R.spk_ref(dg, w[:H4], w[H4:], 5, E)
        assert ratio(R.spk_emulate(dg, w[:H4], w[H4:], 5, E), ref, bud) <= 1.0
        assert ratio(R.spk_emulate(dg, w[:H4], w[H4:], 5, E, drop_last_slice=True), ref, bud) > 1.0


# ------------------------------------------------------------------------------------------------ 4. K
def test_k_is_measured_not_fitted():
    k = R.measure_k()
    assert 0.5 * R.K_MEASURED < k <= R.K_MEASURED, k
    assert R.K == 4 * R.K_MEASURED
