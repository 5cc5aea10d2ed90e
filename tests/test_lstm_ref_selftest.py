"""The LSTM step checks of lstm_ref.py proven on the CPU, without a GPU: fp32 restatements of the recurrence go through exactly the checks
test_gpu_lstm_steps.py applies to the HIP kernels (all five scenarios, W_hh = 0, B = 3, H = 8 and 32, T = 48, d_out >= 0 and signed).

Accepted by every check: torch's own fp32 sigmoid / tanh (TorchF32) and csrc/common.h's formulas restated in fp32 (HeaderF32).
Reported -- WRONG below names the check(s) that must fail for each (the others may or may not):
    tanh(c) as 2 sigmoid(2x) - 1 (the round-3 form)           F2, B1        the |x| < 0.7 branch taken for all x            F2, B1
    tanh(c) + 3e-7                                            F2, B1        the branch threshold moved to 1.5              F2, B1
    sigmoid not clamped through inf (NaN at -300)             F1, F2, F3, B1 (scenario extreme)
    the g gate as a plain sigmoid                             F3 (g)        o and g pre-activations swapped                F3
    c_prev from the wrong neighbour in the reverse direction  B1            the f of the current frame in dc               B1
    1 - tc^2 from the saved h / o (0 / 0 where o underflows)  B1 (scenario extreme)
    d_f with c_t instead of c_prev                            B1
"""
import functools

import numpy as np
import pytest

import lstm_ref as R

B, T, HS = 3, 48, (8, 32)


class TanhAsGate(R.HeaderF32):
    tanh_c = staticmethod(R.HeaderF32.gate_g)


class TanhPlus3em7(R.HeaderF32):
    tanh_c = classmethod(lambda cls, x: (R.HeaderF32.tanh_c(x) + R.F32(3e-7)).astype(R.F32))


class SmallBranchAlways(R.HeaderF32):
    thresh = np.inf


class Threshold15(R.HeaderF32):
    thresh = 1.5


class SigmoidUnclamped(R.HeaderF32):
    @staticmethod
    def sigmoid(x):
        with np.errstate(all='ignore'):
            t = R._exp2(x * R.F32(-1.44269504))
            return (R.F32(1) - t / (R.F32(1) + t)).astype(R.F32)           # inf / inf at x = -300


class GateGSigmoid(R.HeaderF32):
    gate_g = staticmethod(R.HeaderF32.sigmoid)


class CprevWrongNeighbour(R.HeaderF32):
    cprev_wrong = True


class ForgetOfCurrentFrame(R.HeaderF32):
    f_current = True


class TcFromSavedH(R.HeaderF32):
    tc_from_h = True


class DfWithCt(R.HeaderF32):
    df_uses_c = True


class SwapOG(R.HeaderF32):
    swap_og = True


WRONG = {TanhAsGate: ('F2', 'B1'), TanhPlus3em7: ('F2', 'B1'), SmallBranchAlways: ('F2', 'B1'), Threshold15: ('F2', 'B1'),
         SigmoidUnclamped: ('F1', 'F2', 'F3_sigmoid', 'B1'), GateGSigmoid: ('F3_g',), CprevWrongNeighbour: ('B1',), ForgetOfCurrentFrame: ('B1',),
         TcFromSavedH: ('B1',), DfWithCt: ('B1',), SwapOG: ('F3_sigmoid', 'F3_g')}
BACKWARD_ONLY = (CprevWrongNeighbour, ForgetOfCurrentFrame, TcFromSavedH, DfWithCt)


@functools.lru_cache(None)
def inputs(H):
    return {sc: R.scenario(sc, B, T, H) for sc in R.SCENARIOS}, {s: R.d_out_for(B, T, H, s) for s in (False, True)}


def run_checks(fn, k=R.K_B1):
    """Worst ratio per check over all scenarios, both H and both d_out sign patterns."""
    worst = dict(F1=0.0, F2=0.0, F3_sigmoid=0.0, F3_g=0.0, B1=0.0)
    for H in HS:
        w0 = (np.zeros((4 * H, H), R.F32),) * 2
        pres, ds = inputs(H)
        for pre in pres.values():
            for signed, d in ds.items():
                r = R.layer32(pre, w0, d, fn)
                got = dict(B1=R.check_b1(r['act'], r['csave'], d, r['dgates'], k))
                if not signed:
                    got.update(F1=R.check_f1(r['act'], r['csave']), F2=R.check_f2(r['act'], r['csave'], r['out']))
                    got['F3_sigmoid'], got['F3_g'] = R.check_f3(pre, r['act'])
                for name, v in got.items():
                    worst[name] = max(worst[name], v)
    return worst


@pytest.mark.parametrize('fn', [R.TorchF32, R.HeaderF32], ids=lambda f: f.__name__)
def test_correct_restatements_pass_every_check(fn):
    w = run_checks(fn)
    print(fn.__name__, w)
    assert all(v <= 1.0 for v in w.values()), w


def test_documented_constants_hold():
    """The figures in lstm_ref.py's docstring: the header restatement's F1 .. F3 stay under MEASURED, both restatements' B1 ratios (k = 1)
    under B1_TORCH / B1_HEADER, and K_B1 is twice the larger, rounded up."""
    hdr, tor = run_checks(R.HeaderF32, k=1.0), run_checks(R.TorchF32, k=1.0)
    print('header', hdr, 'torch', tor)
    for name, bar in R.MEASURED.items():
        assert hdr[name] <= bar, (name, hdr[name], bar)
    assert hdr['B1'] <= R.B1_HEADER and tor['B1'] <= R.B1_TORCH, (hdr['B1'], tor['B1'])
    assert 2 * max(R.B1_HEADER, R.B1_TORCH) <= R.K_B1 <= 2 * max(R.B1_HEADER, R.B1_TORCH) + 0.01


@pytest.mark.parametrize('fn', list(WRONG), ids=lambda f: f.__name__)
def test_wrong_variants_are_reported(fn):
    w = run_checks(fn)
    print(fn.__name__, w)
    for name in WRONG[fn]:
        assert w[name] > 1.0, (fn.__name__, name, w)
    if fn in BACKWARD_ONLY:                                 # the forward is the correct one: only B1 may speak
        assert all(v <= 1.0 for n, v in w.items() if n != 'B1'), w


def test_scenario_conditions():
    """From the float64 reference alone: grow reaches max |c| >= 0.9 T with >= 90 % of the cells beyond 3, smallc puts >= 10 % of the cells on
    each side of |c| = 0.7 (and in both signs beyond it), every scenario's float64 result is finite, and the exact points are in extreme."""
    for H in HS:
        w0 = (np.zeros((4 * H, H)),) * 2
        pres, ds = inputs(H)
        for sc, pre in pres.items():
            r = R.layer64(pre, w0, ds[True])
            assert all(np.isfinite(v).all() for v in r.values()), sc
            c = r['csave']
            if sc == 'grow':
                assert np.abs(c).max() >= 0.9 * T and (np.abs(c) > 3).mean() >= 0.9
            if sc == 'smallc':
                assert (np.abs(c) < 0.7).mean() >= 0.1 and (c > 0.7).mean() >= 0.1 and (c < -0.7).mean() >= 0.1
                assert ((np.abs(c) > 0.01) & (np.abs(c) < 1)).mean() >= 0.75
            if sc == 'extreme':
                for v in (300.0, -300.0, 88.0, -88.0, 1e-40, -1e-40):
                    assert (pre == np.float32(v)).sum() >= 8, v
                assert (pre == 0).sum() >= 16 and np.signbit(pre[pre == 0]).any()
            if sc == 'sweep':
                assert np.abs(pre).max() > 30 and np.abs(pre).reshape(B, T, 2, 4, H)[:, :, 0, :, 0].max() <= 1e-3 * 1.0001


def test_layer64_is_torch_lstm_in_double():
    """layer64 (B2's reference) against torch.nn.LSTM in float64 with an identity-selecting W_ih, forward and autograd backward."""
    import torch
    H, Bq, Tq = 5, 2, 7
    pre, w, d = R.trained(Bq, Tq, H, 3)
    lstm = torch.nn.LSTM(8 * H, H, 1, batch_first=True, bidirectional=True).double()
    eye = torch.eye(8 * H, dtype=torch.float64)
    with torch.no_grad():
        for k, sfx in enumerate(('', '_reverse')):
            getattr(lstm, 'weight_ih_l0' + sfx).copy_(eye[k * 4 * H:(k + 1) * 4 * H])
            getattr(lstm, 'weight_hh_l0' + sfx).copy_(torch.from_numpy(w[k]).double())
            getattr(lstm, 'bias_ih_l0' + sfx).zero_()
            getattr(lstm, 'bias_hh_l0' + sfx).zero_()
    x = torch.from_numpy(pre).double().requires_grad_(True)
    y, _ = lstm(x)
    (y * torch.from_numpy(d).double()).sum().backward()
    r = R.layer64(pre, w, d)
    assert R.max_norm_error(r['out'], y.detach().numpy()) < 1e-13
    assert R.max_norm_error(r['dgates'], x.grad.numpy()) < 1e-13           # W_ih selects: d pre = d x
    for k, sfx in enumerate(('', '_reverse')):
        assert R.max_norm_error(r['dw_hh'][k], getattr(lstm, 'weight_hh_l0' + sfx).grad.numpy()) < 1e-12


def test_ragged_checks_and_b2_on_the_restatements():
    """The ragged forms of F1 / F2 (reverse direction from the zero state at len - 1, NaN behind the length ignored) accept a ragged
    restatement and report one whose reverse direction started at T - 1; B2 accepts the header restatement at both weight scales."""
    H, lens = 8, [T, T // 2, 1]
    pre = R.scenario('sweep', B, T, H)
    w = R.trained(B, T, H, 3)[1]
    r = R.layer32_ragged(pre, w, lens, R.HeaderF32)
    assert R.check_f1(r['act'], r['csave'], lens) <= 1 and R.check_f2(r['act'], r['csave'], r['out'], lens) <= 1
    assert R.tail_is_zero(r['out'], lens) and R.tail_is_zero(r['csave'], lens)
    full = R.layer32(pre, w, None, R.HeaderF32)
    assert R.check_f1(full['act'], full['csave'], lens) > 1                # row 1's reverse direction arrives at len - 1 with a state
    assert not R.tail_is_zero(full['out'], lens)
    for ws in (3, 6):
        pre, w, d = R.trained(B, T, H, ws)
        ref64, ref32 = R.layer64(pre, w, d), R.layer32(pre, w, d, R.TorchF32)
        res = R.check_b2(R.layer32(pre, w, d, R.HeaderF32), ref64, ref32)
        print(ws, res)
        assert all(v[2] <= 1 for v in res.values()), res
        bad = R.check_b2(R.layer32(pre, w, d, TanhPlus3em7), ref64, ref32)
        print(ws, 'tanh + 3e-7', bad)
