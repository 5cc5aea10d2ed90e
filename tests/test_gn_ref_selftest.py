"""tests/gn_ref.py proven on the CPU, without a GPU.

1. The float64 reference equals torch.nn.functional.group_norm + relu and its autograd in float64; the gather equals oracle/interp_np; the
   scatter adjoint is the transpose of the gather.
2. A numpy float32 EMULATION of the kernels' operation order (elementwise.hip: per-thread (a+b)+(c+d) chains, a float64 sum of the 64
   partials of a group, float(sum) * inv_n, the two-pass fused-multiply-add chain, 1 / sqrtf(var + eps), gn_h, gn_z; the backward's chains
   and its three column sums) stays inside the budgets on every input family and every T.
3. Each MUTANT -- a subtly wrong kernel -- exceeds a budget (ratio > 1) on at least one family at every T where it differs from the kernel:
   this is what shows that tests/test_gpu_gn_relu.py, which applies the same budgets to the HIP kernels, would fail for such a kernel.
   forward    unbiased variance; eps outside the square root; eps = 1e-6; inv_n over T rounded up to 16; the last row left out of the
              variance; the group index shifted by one; the one-pass variance E[x^2] - m^2
   backward   the m2 term dropped; m1 taken over padded rows; gamma missing from dxh; d_gamma formed from x instead of h; and the mask
              z >= 0 instead of z > 0, which the mask rule (gn_ref.mask_violations) catches where z is exactly zero
4. The budget is not vacuous: it never exceeds 1e-3 of max |z| on a family without a deliberate cancellation.
"""
import functools

import numpy as np
import pytest
import torch

import gn_ref as R
from oracle import interp_np

F32 = np.float32
C = 64
TS = (1, 2, 15, 16, 17, 129, 256)
FWD_MUTANTS = ('unbiased', 'eps_outside', 'eps_1e-6', 'inv_n_padded', 'last_row', 'group_shift', 'one_pass')
BWD_MUTANTS = ('no_m2', 'm1_padded', 'no_gamma', 'dgamma_from_x')


def _fma(a, b, c):
    """fused multiply-add on float32 arrays: the product of two float32 is exact in float64, the sum is rounded once more than the hardware
    does (double rounding: a difference of at most one unit in 2^29 cases, nothing an inequality test sees)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _thread_view(a, T):
    """[T, C] -> [nit, 16 (rg), C/4 (slot), 4] padded with zeros, and the row validity [nit, 16, 1]"""
    nit = (T + 15) // 16
    p = np.zeros((nit * 16, a.shape[1]), F32)
    p[:T] = a
    valid = (np.arange(nit * 16) < T).reshape(nit, 16, 1)
    return p.reshape(nit, 16, -1, 4), valid


def _group_sum(part):
    """[16 (rg), C/4] thread partials -> [C/16] float32(float64 sum of the 64 partials of each group)"""
    p = part.astype(np.float64).reshape(16, -1, 4)             # [rg, group, slot in group]
    return p.sum(axis=(0, 2)).astype(F32)


def emulate_forward(x, gamma, beta, mutant=None):
    """One utterance x [T, C] float32 -> (y, z, mean [G], rstd [G]) in the register kernel's order; mutant: one of FWD_MUTANTS."""
    T, Cc = x.shape
    v, valid = _thread_view(x, T)
    nit = v.shape[0]
    s = np.zeros((16, Cc // 4), F32)
    for it in range(nit):
        s = s + ((v[it, :, :, 0] + v[it, :, :, 1]) + (v[it, :, :, 2] + v[it, :, :, 3]))
    n = F32(16.0) * F32(16 * nit if mutant == 'inv_n_padded' else T)
    inv_n = F32(1.0) / n
    mean = _group_sum(s) * inv_n                              # [G]
    mslot = np.repeat(mean, 4)[None, :, None]                 # per slot
    ss = np.zeros((16, Cc // 4), F32)
    sq = np.zeros((16, Cc // 4), F32)
    for it in range(nit):
        ok = valid[it] & (not (mutant == 'last_row') or (np.arange(16)[:, None] + 16 * it < T - 1))
        for j in range(4):
            dlt = (v[it, :, :, j] - mslot[0, :, 0][None, :]).astype(F32)
            ss = np.where(ok, _fma(dlt, dlt, ss), ss)
            sq = np.where(ok, _fma(v[it, :, :, j], v[it, :, :, j], sq), sq)
    if mutant == 'one_pass':
        var = (_group_sum(sq) * inv_n - mean * mean).astype(F32)
    elif mutant == 'unbiased':
        var = _group_sum(ss) * (F32(1.0) / (n - F32(1.0)))
    else:
        var = _group_sum(ss) * inv_n
    with np.errstate(invalid='ignore', divide='ignore'):
        if mutant == 'eps_outside':
            rstd = F32(1.0) / (np.sqrt(var) + F32(1e-5))
        else:
            rstd = F32(1.0) / np.sqrt(var + F32(1e-6 if mutant == 'eps_1e-6' else 1e-5))
    rstd = rstd.astype(F32)
    if mutant == 'group_shift':                               # the statistics of the next group of the 64-channel block
        idx = (np.arange(Cc // 16) // 4) * 4 + (np.arange(Cc // 16) + 1) % 4
        mean, rstd = mean[idx], rstd[idx]
    mc, rc = np.repeat(mean, 16)[None, :], np.repeat(rstd, 16)[None, :]
    h = ((x - mc).astype(F32) * rc).astype(F32)
    z = _fma(h, gamma[None, :], beta[None, :])
    return np.maximum(z, F32(0)), z, mean, rstd


def emulate_backward(x, dy, gamma, beta, mean, rstd, acc0, mutant=None, mask_ge=False):
    """One utterance in gn_relu_bwd_kernel's order -> (dx [T,C], (dgamma, dbeta, dbias) [C] added to acc0, mask)."""
    T, Cc = x.shape
    mc, rc = np.repeat(mean, 16)[None, :], np.repeat(rstd, 16)[None, :]
    h = ((x - mc).astype(F32) * rc).astype(F32)
    z = _fma(h, gamma[None, :], beta[None, :])
    mask = (z >= 0) if mask_ge else (z > 0)
    dz = np.where(mask, dy, F32(0)).astype(F32)
    dxh = dz if mutant == 'no_gamma' else (dz * gamma[None, :]).astype(F32)
    hv, valid = _thread_view(h, T)
    gv, _ = _thread_view(dxh, T)
    nit = hv.shape[0]
    s1 = np.zeros((16, Cc // 4), F32)
    s2 = np.zeros((16, Cc // 4), F32)
    for it in range(nit):
        for j in range(4):
            s1 = s1 + gv[it, :, :, j]
            s2 = s2 + (gv[it, :, :, j] * hv[it, :, :, j]).astype(F32)
    inv_n = F32(1.0) / (F32(16.0) * F32(T))
    inv_n1 = F32(1.0) / (F32(16.0) * F32(16 * nit)) if mutant == 'm1_padded' else inv_n
    m1 = np.repeat(_group_sum(s1) * inv_n1, 16)[None, :]
    m2 = np.repeat(_group_sum(s2) * inv_n, 16)[None, :]
    if mutant == 'no_m2':
        m2 = np.zeros_like(m2)
    dx = (rc * ((dxh - m1).astype(F32) - (h * m2).astype(F32)).astype(F32)).astype(F32)

    def colsum(a, a0):                                        # thread chain over its rows, the 16 row groups in a chain, then the accumulator
        av, _ = _thread_view(a, T)                            # [nit, 16, C/4, 4]
        t = np.zeros(av.shape[1:], F32)
        for it in range(nit):
            t = t + av[it]
        s = np.zeros(av.shape[2:], F32)
        for rg in range(16):
            s = s + t[rg]
        return (a0 + s.reshape(-1)).astype(F32)
    terms = (dz * (x if mutant == 'dgamma_from_x' else h)).astype(F32)
    return dx, (colsum(terms, acc0[0]), colsum(dz, acc0[1]), colsum(dx, acc0[2])), mask


@functools.lru_cache(maxsize=None)
def case(family, T):
    x, gamma, beta = R.make_case(family, 1, T, C, seed=7)
    dy = np.random.default_rng([11, T]).standard_normal((1, T, C)).astype(F32)
    return x, gamma, beta, dy, R.forward_budget(x, gamma, beta)


def fwd_ratios(family, T, mutant=None):
    x, gamma, beta, _, fb = case(family, T)
    y, _, mean, rstd = emulate_forward(x[0], gamma, beta, mutant)
    with np.errstate(invalid='ignore'):
        return max(R.ratio(y[None] - fb['y'], fb['dz']), R.ratio(mean[None] - fb['mean'], fb['dm']),
                   R.ratio(rstd[None] - fb['rstd'], fb['rho'] * fb['rstd']))


def bwd_ratios(family, T, mutant=None):
    x, gamma, beta, dy, fb = case(family, T)
    _, _, mean, rstd = emulate_forward(x[0], gamma, beta)
    acc0 = (F32(0.5), F32(-0.25), F32(2.0))
    dx, sums, mask = emulate_backward(x[0], dy[0], gamma, beta, mean, rstd, acc0, mutant)
    assert R.mask_violations(mask[None], fb['z'], fb['dz']) == 0
    bb = R.backward_budget(x, dy, gamma, beta, mask[None], acc0)
    ref = bb['ref']
    return max(R.ratio(dx[None] - ref['dx'], bb['ddx']), R.ratio(sums[0] - (0.5 + ref['dgamma']), bb['dgamma']),
               R.ratio(sums[1] - (-0.25 + ref['dbeta']), bb['dbeta']), R.ratio(sums[2] - (2.0 + ref['dbias']), bb['dbias']))


# ---------------------------------------------------------------------------------------------------------------- 1. the reference itself
@pytest.mark.parametrize('T', (1, 17, 64))
def test_reference_equals_torch_float64(T):
    B, Cc = 3, 192
    x, gamma, beta = R.make_case('mixed', B, T, Cc, seed=3)
    dy = np.random.default_rng(5).standard_normal((B, T, Cc))
    xt = torch.tensor(x, dtype=torch.float64).permute(0, 2, 1).contiguous().requires_grad_(True)      # [B, C, T]
    g = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    zt = torch.nn.functional.group_norm(xt, Cc // 16, g, b, eps=1e-5)
    yt = torch.relu(zt)
    f = R.forward(x, gamma, beta)
    assert np.abs(f['y'] - yt.detach().permute(0, 2, 1).numpy()).max() < 1e-12 * max(1.0, np.abs(f['y']).max())
    yt.backward(torch.tensor(dy).permute(0, 2, 1))
    r = R.backward(x, dy, gamma, beta, f['z'] > 0)
    for got, want in ((r['dx'], xt.grad.permute(0, 2, 1).numpy()), (r['dgamma'], g.grad.numpy()), (r['dbeta'], b.grad.numpy())):
        assert np.abs(got - want).max() < 1e-10 * max(1.0, np.abs(want).max())
    assert np.abs(r['dbias'] - r['dx'].sum((0, 1))).max() == 0          # the conv bias sees dx summed over utterances and time


def test_ragged_reference_is_the_dense_one_per_row():
    x, gamma, beta = R.make_case('benign', 3, 20, C, seed=1)
    lens = [20, 7, 0]
    f = R.forward(x, gamma, beta, lens)
    for b, L in enumerate(lens):
        assert np.all(f['y'][b, L:] == 0)
        if L:
            assert np.array_equal(f['y'][b, :L], R.forward(x[b:b + 1, :L], gamma, beta)['y'][0])
    assert np.isnan(f['mean'][2]).all()


def test_gather_and_scatter_references():
    rng = np.random.default_rng(2)
    B, T, P = 2, 24, 24
    y = rng.standard_normal((B, T, C)).astype(F32)
    i0 = np.sort(rng.integers(0, T, (B, P)), axis=1).astype(np.int32)
    lam = rng.random((B, P)).astype(F32)
    nrows = np.array([P, 9], np.int32)
    want = interp_np.interp_apply(np.concatenate([y, np.zeros((B, 1, C), F32)], 1), i0, lam, nrows)      # row T reads as zeros
    got = R.gather(y, i0, lam, nrows)
    assert np.abs(got - want).max() <= 2 * R.U * np.abs(want).max()
    assert np.all(got[1, 9:] == 0)
    src = rng.standard_normal((B, P, C))
    adj, bud = R.scatter_adjoint(src, i0, lam, nrows, T)
    # <gather(y), src> == <y, adjoint(src)>: what falls on the zero row T is dropped on both sides
    assert abs((got * src).sum() - (y * adj).sum()) < 1e-9 * np.abs(got * src).sum() + 1e-9
    want = interp_np.interp_backward(src.astype(F32), i0, lam, nrows, T + 1)[:, :T]
    assert R.ratio(want - adj, bud + R.U * np.abs(adj)) <= 1.0


def test_bf16_rounding():
    a = np.array([1.0, 1.00390625, 1.01171875, -3.7, 1e-40, 65504.0, 0.0], F32)     # two ties: to even down, to even up
    assert np.array_equal(R.bf16_rne(a), torch.tensor(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ---------------------------------------------------------------------------------------------- 2. the faithful emulation is inside the budgets
@pytest.mark.parametrize('T', TS)
def test_emulated_kernel_order_is_inside_the_budgets(T):
    for family in R.FAMILIES:
        rf, rb = fwd_ratios(family, T), bwd_ratios(family, T)
        print(f'FIG selftest {family} T={T} forward {rf:.3g} backward {rb:.3g}')
        assert rf <= 1.0 and rb <= 1.0, (family, T, rf, rb)


def test_budget_is_not_vacuous():
    for T in TS:
        for family in ('benign', 'outlier', 'mixed', 'constant'):
            fb = case(family, T)[4]
            assert fb['dz'].max() <= 1e-3 * np.abs(fb['z']).max(), (family, T)


# ---------------------------------------------------------------------------------------------- 3. every mutant is outside
def _differs(a, b):
    return any(not np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@pytest.mark.parametrize('mutant', FWD_MUTANTS)
def test_forward_mutants_exceed_the_budget(mutant):
    for T in TS:
        differs, worst = False, {}
        for family in R.FAMILIES:
            x, gamma, beta = case(family, T)[:3]
            differs |= _differs(emulate_forward(x[0], gamma, beta, mutant), emulate_forward(x[0], gamma, beta))
            worst[family] = fwd_ratios(family, T, mutant)
        print(f'FIG selftest mutant {mutant} T={T} worst {max(worst.values()):.3g} ({max(worst, key=worst.get)})')
        if differs:
            assert max(worst.values()) > 1.0, (mutant, T, worst)
        else:
            assert mutant in ('inv_n_padded',) and T % 16 == 0, (mutant, T)      # the only mutant that coincides with the kernel somewhere


@pytest.mark.parametrize('mutant', BWD_MUTANTS)
def test_backward_mutants_exceed_the_budget(mutant):
    for T in TS:
        worst = {family: bwd_ratios(family, T, mutant) for family in R.FAMILIES}
        print(f'FIG selftest mutant {mutant} T={T} worst {max(worst.values()):.3g} ({max(worst, key=worst.get)})')
        if mutant == 'm1_padded' and T % 16 == 0:
            continue
        assert max(worst.values()) > 1.0, (mutant, T, worst)


def test_mask_rule_catches_greater_or_equal():
    """z >= 0 instead of z > 0 differs from the kernel only where z is exactly zero: the constant group with beta = 0 at the T where the
    computed mean is exact (one row per thread and 16 T a power of two).  There the mask rule refuses it and accepts the kernel's."""
    for T in (1, 2, 16):
        x, gamma, beta, dy, fb = case('constant_beta0', T)
        _, _, mean, rstd = emulate_forward(x[0], gamma, beta)
        assert mean[1] == R.CONST                                            # the check is live
        exact = (x == np.repeat(mean, 16)[None, None, :])
        for ge, bad in ((False, False), (True, True)):
            mask = emulate_backward(x[0], dy[0], gamma, beta, mean, rstd, (F32(0),) * 3, None, mask_ge=ge)[2]
            assert (R.mask_violations(mask[None], fb['z'], fb['dz'], exact, beta) > 0) == bad, (T, ge)
