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
Further down: the recurrent products per step (F4, B3) on restatements with each kernel family's operand rounding and seven wrong products,
K_F4's measurement, check_b2_hi's figures, and the side-output references against float64 / torch with four wrong variants.
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


# ------------------------------------------------------------------------------------------------ F4, B3 and the side-output references
# F4 / B3 (the recurrent products per step) on fp32 restatements with each family's operand rounding.  Accepted: TorchF32 and HeaderF32 in
# the modes exact, f16x2 and f16hi, tagged and untagged.  Reported (OPERANDS_WRONG: the check that must speak and the modes it must speak in;
# the other check must stay silent, its half of the restatement being correct):
#     lo.hi product dropped                 F4, B3  f16x2          operand rounded to bf16 width            F4, B3  every mode
#     one k-chunk of 32 skipped             F4, B3  every mode     tag bit forced on odd k instead of even  F4      f16hi tagged (*)
#     h of the wrong neighbour              F4      every mode     W_hh not transposed in the backward      B3      every mode
#     da scaled per row, unscaled per block B3      f16x2, f16hi
# (*) in f16x2 the low piece absorbs the tag, so either parity represents h to the low piece's last bit, which F4's c_split admits by
# construction: the ratio is printed, not asserted.
MODES = [('exact', False), ('f16x2', False), ('f16x2', True), ('f16hi', False), ('f16hi', True)]
MODE_IDS = [m + ('_tagged' if t else '') for m, t in MODES]
PB, PT, PH = 3, 24, 64          # the smallest shape with two k-chunks of 32 per direction
K_F4_INPUTS = [(5, 40, 256), (3, 24, 64)]
B2_HI_INPUTS = [(5, 40, 256), (17, 40, 256), (16, 24, 512)]


def variant(**flags):
    return type('_'.join(flags), (R.Operands,), flags)


OPERANDS_WRONG = {
    'drop_lohi': (('F4', 'B3'), ('f16x2',)),
    'bf16_width': (('F4', 'B3'), ('exact', 'f16x2', 'f16hi')),
    'skip_chunk': (('F4', 'B3'), ('exact', 'f16x2', 'f16hi')),
    'tag_odd': (('F4',), ('f16hi',)),
    'w_untransposed': (('B3',), ('exact', 'f16x2', 'f16hi')),
    'da_row_scale': (('B3',), ('f16x2', 'f16hi')),
}


@functools.lru_cache(None)
def product_run(fn, mode, tagged, ws, flag=None):
    """(inputs, restatement, F4, B3): layer32 with the operand rounding (or its wrong variant `flag`) judged by the correct Operands."""
    pre, w, d = R.trained(PB, PT, PH, ws)
    ops = R.recurrent_operands(mode, tagged, PH)
    r = R.layer32(pre, w, d, fn, ops if flag is None else variant(**{flag: True})(mode, tagged, PH))
    return (pre, w, d), r, R.check_f4(pre, r['act'], r['out'], w, ops), R.check_b3(r['act'], r['csave'], d, r['dgates'], w, ops)


@pytest.mark.parametrize('mode,tagged', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('fn', [R.TorchF32, R.HeaderF32], ids=lambda f: f.__name__)
def test_f4_b3_accept_correct_restatements(fn, mode, tagged):
    for ws in (3, 6):
        _, _, f4, b3 = product_run(fn, mode, tagged, ws)
        print(fn.__name__, mode, tagged, ws, f'F4 {f4:.3f} B3 {b3:.3f}')
        assert f4 <= 1.0 and b3 <= 1.0, (ws, f4, b3)


@pytest.mark.parametrize('mode,tagged', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('flag', list(OPERANDS_WRONG))
def test_f4_b3_report_wrong_products(flag, mode, tagged):
    speaks, modes = OPERANDS_WRONG[flag]
    if flag == 'tag_odd' and not tagged:
        return                                              # without a tag the variant is the correct code
    for ws in (3, 6):
        _, _, f4, b3 = product_run(R.HeaderF32, mode, tagged, ws, flag)
        print(flag, mode, tagged, ws, f'F4 {f4:.3f} B3 {b3:.3f}')
        got = dict(F4=f4, B3=b3)
        for name in got:
            if name not in speaks:
                assert got[name] <= 1.0, (flag, mode, name, got)
            elif mode in modes:
                assert got[name] > 1.0, (flag, mode, name, got)


@pytest.mark.parametrize('mode,tagged', MODES, ids=MODE_IDS)
def test_f4_reports_h_of_the_wrong_neighbour(mode, tagged):
    """A forward whose gates of frame t were computed from h(t + 1) (t - 1 in the reverse direction): act rebuilt from a correct run's out."""
    (pre, w, _), r, _, _ = product_run(R.HeaderF32, mode, tagged, 3)
    ops = R.recurrent_operands(mode, tagged, PH)
    a = R.f4_reference(pre, r['out'], w, ops, wrong_neighbour=True)[0].astype(R.F32).reshape(PB, PT, 2, 4, PH)
    act = np.stack([R.HeaderF32.sigmoid(a[:, :, :, 0]), R.HeaderF32.sigmoid(a[:, :, :, 1]), R.HeaderF32.gate_g(a[:, :, :, 2]),
                    R.HeaderF32.sigmoid(a[:, :, :, 3])], 3).reshape(PB, PT, 8 * PH)
    assert R.check_f4(pre, act, r['out'], w, ops) > 1.0
    good = R.f4_reference(pre, r['out'], w, ops)[0].astype(R.F32).reshape(PB, PT, 2, 4, PH)       # the same rebuild from the right neighbour
    act = np.stack([R.HeaderF32.sigmoid(good[:, :, :, 0]), R.HeaderF32.sigmoid(good[:, :, :, 1]), R.HeaderF32.gate_g(good[:, :, :, 2]),
                    R.HeaderF32.sigmoid(good[:, :, :, 3])], 3).reshape(PB, PT, 8 * PH)
    assert R.check_f4(pre, act, r['out'], w, ops) <= 1.0


def test_k_f4_is_twice_the_sequential_restatement():
    """K_F4: the fp32 restatement that adds the exact products one after another (the least favourable order) on trained(B, T, H, ws),
    ws in {3, 6}, at (5, 40, 256) and (3, 24, 64), in every operand mode; its worst F4 ratio at k = 1 stays under F4_SEQUENTIAL and
    K_F4 is twice that.  The gate functions are the header's restated in numpy (HeaderF32), elementwise operations only, so that the
    recorded figure does not depend on a library's vectorised sigmoid."""
    worst = 0.0
    for Bq, Tq, H in K_F4_INPUTS:
        for ws in (3, 6):
            pre, w, _ = R.trained(Bq, Tq, H, ws)
            for mode, tagged in MODES:
                ops = R.recurrent_operands(mode, tagged, H)
                r = R.layer32(pre, w, None, R.HeaderF32, ops, sequential=True)
                q = R.check_f4(pre, r['act'], r['out'], w, ops, k=1.0)
                print(f'K_F4 ({Bq}, {Tq}, {H}) ws {ws} {mode} tagged {tagged}: {q:.3f}')
                assert R.check_f4(pre, r['act'], r['out'], w, ops) <= 1.0
                worst = max(worst, q)
    print(f'K_F4 worst sequential ratio {worst:.3f}')
    assert worst <= R.F4_SEQUENTIAL and 2 * R.F4_SEQUENTIAL <= R.K_F4 <= 2 * R.F4_SEQUENTIAL + 0.01
    assert worst >= 0.95 * R.F4_SEQUENTIAL                 # the recorded figure is this measurement, not a loose cap


@pytest.mark.parametrize('shape', B2_HI_INPUTS, ids=lambda s: 'b%d_t%d_h%d' % s)
def test_check_b2_hi_figures(shape):
    """check_b2_hi's cap must keep a correct kernel inside and a bf16-wide operand outside: with the exact emulation the tagged layer16
    is at most B2_HI_TAGGED x the untagged error and a bf16-wide operand more than B2_HI_BF16 x, per tensor, at both weight scales."""
    Bq, Tq, H = shape
    for ws in (3, 6):
        pre, w, d = R.trained(Bq, Tq, H, ws)
        r64, un, tg = R.layer64(pre, w, d), R.layer16(pre, w, d, False), R.layer16(pre, w, d, True)
        bf = R.layer16(pre, w, d, ops=variant(bf16_width=True)('f16hi', False, H))
        ok, bad = R.check_b2_hi(tg, r64, un), R.check_b2_hi(bf, r64, un)
        for n in ('out', 'dgates', 'dw_hh'):
            print(f'b2_hi {shape} ws {ws} {n}: untagged {ok[n][1]:.2e} tagged x{ok[n][0] / ok[n][1]:.2f} bf16-wide x{bad[n][0] / bad[n][1]:.2f}')
            assert ok[n][0] <= R.B2_HI_TAGGED * ok[n][1] and ok[n][2] <= 1.0, (n, ok[n])
            assert bad[n][0] > R.B2_HI_BF16 * bad[n][1] and bad[n][2] > 1.0, (n, bad[n])


def _dgates(Bq=5, Tq=16, H=32, seed=5):
    return (np.random.default_rng(seed).standard_normal((Bq, Tq, 8 * H)) * 1e-3).astype(R.F32)


def _walk_block_sums(dg, xf, close0):
    """The storing wave's loop (csrc/lstm_seq.hip) restated: per direction the steps in walking order, a running fp32 sum from zero, written
    and cleared when the close predicate holds.  close0(t, xf): the predicate of direction 0."""
    Bq, Tq, C = dg.shape
    res = np.full((Bq, Tq // xf, C), np.nan, R.F32)
    for d in range(2):
        col = slice(d * C // 2, (d + 1) * C // 2)
        acc = np.zeros((Bq, C // 2), R.F32)
        for t in (range(Tq - 1, -1, -1) if d == 0 else range(Tq)):
            acc = (acc + dg[:, t, col]).astype(R.F32)
            if close0(t, xf) if d == 0 else t % xf == xf - 1:
                res[:, t // xf, col] = acc
                acc = np.zeros_like(acc)
    return res


def test_block_sums_reference():
    dg = _dgates()
    for xf in (1, 8, 16):
        got = R.block_sums(dg, xf)
        ref = dg.astype(np.float64).reshape(5, 16 // xf, xf, -1)
        assert np.abs(got - ref.sum(2)).max() <= xf * 2.0 ** -24 * np.abs(ref).sum(2).max()
        assert np.array_equal(got, _walk_block_sums(dg, xf, lambda t, x: t % x == 0))
        if xf > 1:                                          # direction 0 closing at t % xf == xf - 1: one frame early
            bad = _walk_block_sums(dg, xf, lambda t, x: t % x == x - 1)
            assert not np.array_equal(got[:, :, :128], bad[:, :, :128], equal_nan=True) and np.array_equal(got[:, :, 128:], bad[:, :, 128:])
    assert np.array_equal(R.block_sums(dg, 1).view(np.uint32), dg.view(np.uint32))
    mz = np.full((1, 4, 2), -0.0, R.F32)                    # the sums start from +0: a block of -0 addends gives +0, also at xf = 1
    assert not np.signbit(R.block_sums(mz, 1)).any() and not np.signbit(R.block_sums(mz, 4)).any()
    order = np.array([1e8, 1.0, -1e8, 1.0], R.F32).reshape(1, 4, 1).repeat(2, 2)       # the order of the additions shows
    assert R.block_sums(order, 4)[0, 0].tolist() == [0.0, 1.0]         # descending ((1 - 1e8) + 1) + 1e8 = 0, ascending ((1e8 + 1) - 1e8) + 1 = 1


def test_bias_sums_and_check_gbias():
    import torch
    for Bq in (5, 17):
        nbt = (Bq + 15) // 16
        dg = _dgates(Bq)
        S = R.bias_sums(dg, nbt)
        assert S.shape == (nbt, 256) and np.allclose(S.sum(0), torch.from_numpy(dg).double().sum((0, 1)).numpy(), rtol=0, atol=1e-15)
        g0 = np.random.default_rng(6).standard_normal(256).astype(R.F32)
        got = g0.copy()
        for k in range(nbt):                                # one fp32 rounding per tile sum, one per atomic add
            got = (got + S[k].astype(R.F32)).astype(R.F32)
        assert R.check_gbias(got, g0, dg, nbt) <= 1.0
        pad = np.concatenate([dg, _dgates(16 * nbt - Bq, seed=7)])      # a sum over ceil16(B) rows: whatever the rows behind B hold
        assert R.check_gbias(g0 + pad.astype(np.float64).sum((0, 1)), g0, dg, nbt) > 1e3


def test_bf16_bits_and_amax_bits():
    import torch
    x = np.concatenate([_dgates().reshape(-1)[:4096], np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3.4e38, 1.00390625, 1.01171875,
                                                                 65280.0, -65281.0], R.F32)])
    ref = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], ref[~nan]) and np.isnan(R.bf16_value(got[nan])).all()
    assert np.array_equal(R.bf16_value(got[~nan]), torch.from_numpy(x).to(torch.bfloat16).float().numpy()[~nan])
    trunc = (x.view(np.uint32) >> 16).astype(np.uint16)     # bf16 by truncation
    assert (trunc[~nan] != got[~nan]).mean() > 0.3
    dg = _dgates()
    dg[1, 2, 3] = -7.0                                      # the largest magnitude is negative
    assert R.amax_bits(dg) == int(np.float32(7.0).view(np.uint32)) == int(torch.from_numpy(dg).abs().max().numpy().view(np.uint32))
    assert int(dg.max().view(np.uint32)) != R.amax_bits(dg)        # amax over signed values
    assert R.amax_bits(np.zeros((2, 3, 8), R.F32)) == 0


def test_operands_of_per_step_families_ignore_nw_and_g():
    """The per-step kernels multiply the fp32 words themselves whatever lstm_nw / lstm_g say; the persistent kernels' model is untouched by them."""
    for H in (64, 128, 256, 512):
        for nw in (4, 8, 16):
            for g in (0, 1, 2, 4, 8, 16):
                ops = R.operands_of(H, dict(persist=0, lstm_nw=nw, lstm_g=g), B=17)
                assert (ops.mode, ops.tagged) == ('exact', False), (H, nw, g)
    assert R.operands_of(128, dict(lstm_nw=4)).mode == 'exact'                      # no persistent kernel at H = 128
    for H in (256, 512):
        a, b = R.operands_of(H, dict(lstm_nw=4, lstm_g=2), B=5), R.operands_of(H, {}, B=5)
        assert (a.mode, a.tagged) == (b.mode, b.tagged) == ('f16x2', True)
