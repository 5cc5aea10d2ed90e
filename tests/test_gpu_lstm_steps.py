"""The LSTM recurrence kernels (csrc/lstm_small.hip, lstm_step.hip, lstm_seq.hip) step by step against float64 (pytest -m gpu): every
kernel family, at the smallest shapes that still select it, gets the caller's pre-activations through engine.blstm_recurrence and its own
saved state (activated gates, cell states, outputs, pre-activation gradients) goes through the checks of lstm_ref.py -- F1 .. F3 and B1 over
the five scenarios with W_hh = 0; F1, F2, the recurrent products per step F4 / B3 (each family's operand rounding, lstm_ref.operands_of) and
the chain budget B2 with trained-scale W_hh; F1 / F2 and the zero tails on a ragged forward with
NaN behind each row's length; bit-identical repeats of the `extreme` scenario.  The checks, their bars and where the bars come from are in
lstm_ref.py's docstring; test_lstm_ref_selftest.py proves on the CPU that they accept correct fp32 code and report the wrong variants.
Every test prints the ratios it measured before it asserts (a pass is <= 1)."""
import numpy as np
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DEFAULTS = dict(small_lds=1, persist=1, seq_tag=1)

# (id, H, B, T, knobs): the smallest shapes that select each family / path
FAMILIES = [(f'small_h{H}_lds{lds}', H, 3, 40, dict(small_lds=lds)) for H in (1, 5, 16, 32) for lds in (1, 2, 0)] + [
    ('step_h64', 64, 3, 24, {}),
    ('step_h256_per_step', 256, 3, 24, dict(persist=0)),
    ('seq_h256_b5_tagged', 256, 5, 40, dict(seq_tag=1)),          # a partial batch tile
    ('seq_h256_b5_flag_line', 256, 5, 40, dict(seq_tag=0)),
    ('seq_h256_b17_tagged', 256, 17, 40, dict(seq_tag=1)),        # a second tile
    ('seq_h256_b17_flag_line', 256, 17, 40, dict(seq_tag=0)),
    ('seq_h512_b16', 512, 16, 24, {}),
]
FAMILY_IDS = [f[0] for f in FAMILIES]


def run(fam, pre, w_hh, d_out=None, lengths=None):
    """engine.blstm_recurrence under the family's knobs, results as numpy: dict out, csave, act, dgates."""
    from speechsplit_amd import engine as E
    _, H, _, _, knobs = fam
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for k, v in knobs.items():
        E.tune(k, v)
    try:
        res = E.blstm_recurrence(dev(pre), tuple(dev(w) for w in w_hh), None if d_out is None else dev(d_out), lengths)
        torch.cuda.synchronize()
    finally:
        for k in knobs:
            E.tune(k, DEFAULTS[k])
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(('out', 'csave', 'act', 'dgates'), res)}


def zero_w(H):
    return (np.zeros((4 * H, H), R.F32),) * 2


@pytest.mark.parametrize('scenario', R.SCENARIOS)
@pytest.mark.parametrize('fam', FAMILIES, ids=FAMILY_IDS)
def test_steps_with_zero_whh(fam, scenario):
    """W_hh = 0: F1, F2, F3 on the forward's saved state and B1 (d_out >= 0, then signed) on the backward's gradients; all finite."""
    name, H, B, T, _ = fam
    pre = R.scenario(scenario, B, T, H)
    ratios = {}
    for signed in (False, True):
        d = R.d_out_for(B, T, H, signed)
        r = run(fam, pre, zero_w(H), d)
        assert all(np.isfinite(v).all() for v in r.values()), (name, scenario, 'non-finite output')
        if not signed:
            f3 = R.check_f3(pre, r['act'])
            ratios.update(F1=R.check_f1(r['act'], r['csave']), F2=R.check_f2(r['act'], r['csave'], r['out']), F3_sigmoid=f3[0], F3_g=f3[1])
        ratios['B1_signed' if signed else 'B1_pos'] = R.check_b1(r['act'], r['csave'], d, r['dgates'])
    print(f'lstm_steps {name} {scenario}: ' + ' '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (name, scenario, ratios)


@pytest.mark.parametrize('ws', [3, 6])
@pytest.mark.parametrize('fam', FAMILIES, ids=FAMILY_IDS)
def test_chain_budget_with_trained_scale_whh(fam, ws):
    """W_hh ~ U(+-ws / sqrt(H)): F1 and F2 still hold on the saved state, every step's recurrent product W_hh h(t-1) / da(t+1) W_hh is the
    family's (F4, B3), and out / dgates / dW_hh stay within B2 of float64."""
    name, H, B, T, knobs = fam
    pre, w, d = R.trained(B, T, H, ws)
    r = run(fam, pre, w, d)
    assert all(np.isfinite(v).all() for v in r.values()), (name, ws, 'non-finite output')
    f1, f2 = R.check_f1(r['act'], r['csave']), R.check_f2(r['act'], r['csave'], r['out'])
    ops = R.operands_of(H, knobs, B=B)
    f4, b3 = R.check_f4(pre, r['act'], r['out'], w, ops), R.check_b3(r['act'], r['csave'], d, r['dgates'], w, ops)
    r['dw_hh'] = R.dw_hh(r['dgates'], r['out'])
    b2 = R.check_b2(r, R.layer64(pre, w, d), R.layer32(pre, w, d, R.TorchF32))
    print(f'lstm_steps {name} ws {ws}: F1 {f1:.3f} F2 {f2:.3f} F4 {f4:.3f} B3 {b3:.3f} ({ops.mode}{" tagged" if ops.tagged else ""}) '
          'B2 (engine / fp32 error, ratio to bar) ' +
          ' '.join(f'{k} {e:.2e}/{e32:.2e} {q:.3f}' for k, (e, e32, q) in b2.items()))
    assert f1 <= 1.0 and f2 <= 1.0, (name, ws, f1, f2)
    assert f4 <= 1.0 and b3 <= 1.0, (name, ws, f4, b3)
    assert all(q <= 1.0 for _, _, q in b2.values()), (name, ws, b2)


@pytest.mark.parametrize('fam', FAMILIES, ids=FAMILY_IDS)
def test_ragged_forward_steps(fam):
    """Lengths T, T // 2, 1 (repeated over the batch), NaN pre-activations behind each length (the header permits them): F1 and F2 hold inside
    each row's length with the reverse direction starting at len - 1 from the zero state; out and csave are zero behind it."""
    name, H, B, T, _ = fam
    lens = [(T, T // 2, 1)[b % 3] for b in range(B)]
    pre, w, _ = R.trained(B, T, H, 3)
    for b, n in enumerate(lens):
        pre[b, n:] = np.nan
    r = run(fam, pre, w, None, lens)
    f1, f2 = R.check_f1(r['act'], r['csave'], lens), R.check_f2(r['act'], r['csave'], r['out'], lens)
    print(f'lstm_steps {name} ragged: F1 {f1:.3f} F2 {f2:.3f}')
    assert R.tail_is_zero(r['out'], lens) and R.tail_is_zero(r['csave'], lens), name
    assert all(np.isfinite(r[k][b, :n]).all() for k in ('out', 'csave', 'act') for b, n in enumerate(lens)), name
    assert f1 <= 1.0 and f2 <= 1.0, (name, f1, f2)
    # F1 / F2 see c and h of a step, not the h a step STARTED from: each row against its own run alone (the suite's 1e-4 bar for this hook,
    # test_gpu_ragged.py) shows that both directions started from h = 0 and read no padded frame
    ref = R.layer32_ragged(np.nan_to_num(pre), w, lens, R.HeaderF32)
    assert R.max_norm_error(r['out'], ref['out']) <= 1e-4, name


@pytest.mark.parametrize('fam', FAMILIES, ids=FAMILY_IDS)
def test_extreme_scenario_repeats_bit_identically(fam):
    name, H, B, T, _ = fam
    pre, d = R.scenario('extreme', B, T, H), R.d_out_for(B, T, H, True)
    a, b = run(fam, pre, zero_w(H), d), run(fam, pre, zero_w(H), d)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (name, k)
