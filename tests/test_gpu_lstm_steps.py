"""The LSTM recurrence kernels (csrc/lstm_small.hip, lstm_step.hip, lstm_seq.hip) step by step against float64 (pytest -m gpu): every
kernel family, at the smallest shapes that still select it, gets the caller's pre-activations through engine.blstm_recurrence and its own
saved state (activated gates, cell states, outputs, pre-activation gradients) goes through the checks of lstm_ref.py -- F1 .. F3 and B1 over
the five scenarios with W_hh = 0; F1, F2, the recurrent products per step F4 / B3 (each family's operand rounding, lstm_ref.operands_of) and
the chain budget B2 with trained-scale W_hh; F1 / F2 and the zero tails on a ragged forward with
NaN behind each row's length; bit-identical repeats of the `extreme` scenario.  The checks, their bars and where the bars come from are in
lstm_ref.py's docstring; test_lstm_ref_selftest.py proves on the CPU that they accept correct fp32 code and report the wrong variants.
Every test prints the ratios it measured before it asserts (a pass is <= 1).

Every instance <H, NW, G> of lstm_step.hip's two switches (lstm_step_fwd / lstm_step_bwd; ss_tune("lstm_nw"), ss_tune("lstm_g")) is a family
of its own, all under persist = 0 at B = 3, T = 24 (B = 17, a second batch tile, for one NW 8 and one NW 4 family of H = 512).  The family id
names the knobs, EXPECT the instance they must select -- forward and backward -- and run() asserts after every launch that this is the one
the launcher picked (ss_debug_last_variant, reset before the launch and read as the set of instances launched since: exactly the one expected
and no other, and none at all for the families that must not reach lstm_step.hip), so a key that silently falls back to the default fails here.  The operand model of all of them
is lstm_ref's `exact` one: NW and G only say which wave loads which 16-wide chunk of K and how many chunks a wave requests ahead; every
operand reaches v_mfma_f32_16x16x4_f32 as the fp32 value in memory in every instance (lstm_ref.operands_of ignores both keys).

Bit identity between instances, decided from the kernels:
  * same H and NW, different G -- IDENTICAL bits, asserted (test_group_size_does_not_change_the_bits).  A wave walks its chunks in ascending
    order whatever G is.  Forward: one accumulator per gate takes chunk c's four MFMAs (q = 0 .. 3) in that order.  Backward: chunk c goes to
    accumulator c & 1 (`i & 1` inside a group, and every G of the backward switch is even, so the parity inside the group is the chunk's) and
    the two are added once at the end.  G only moves the loads.
  * same H, different NW -- NOT identical, and not asserted: wave w sums the K range [w K / NW, (w + 1) K / NW) in its MFMA accumulator and
    the NW partial sums are then added in LDS order, so NW changes where the fp32 sum is cut and re-associated.  Those instances are held to
    the float64 bars (F4 / B3 per step, B2 over the chain) like every other family.
Worst error / bar over the 21 new families on an MI355X (profiles/r05/variant_knobs/test_figures.txt): F1 0.49, F2 0.69,
F3 0.46 (sigmoid) / 0.45 (g), B1 0.73, F4 0.41, B3 0.73, B2 0.14 (out) / 0.11 (dgates) / 0.14 (dW_hh); the 13 pairs of one (H, NW): 0 elements
whose bits differ in out, csave, act and dgates."""
import functools

import numpy as np
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DEFAULTS = dict(small_lds=1, persist=1, seq_tag=1, lstm_nw=16, lstm_g=0)

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

# id -> (forward instance, backward instance) as ss_debug_last_variant names them: "H NW G"
EXPECT = {'step_h64': ('64 4 1', '64 4 2'), 'step_h256_per_step': ('256 16 1', '256 16 4')}


def step_family(H, nw, g, fwd, bwd, B=3):
    """One per-step family under (lstm_nw, lstm_g) = (nw, g) and the <NW, G> its forward and backward must select."""
    name = f'step_h{H}_nw{nw}_g{g}_fwd{fwd[0]}x{fwd[1]}_bwd{bwd[0]}x{bwd[1]}' + (f'_b{B}' if B != 3 else '')
    EXPECT[name] = (f'{H} {fwd[0]} {fwd[1]}', f'{H} {bwd[0]} {bwd[1]}')
    return (name, H, B, 24, dict(persist=0, lstm_nw=nw, lstm_g=g))


# the first family of every (H, NW) is its lstm_g = 0 form: the one the others of that (H, NW) must equal bit for bit
STEP_GROUPS = {
    (128, 16): [step_family(128, 16, 0, (4, 2), (4, 4))],                                       # H = 128 has one instance, whatever the keys
    (256, 8): [step_family(256, 8, 0, (8, 2), (8, 4))],
    (256, 4): [step_family(256, 4, 0, (4, 4), (4, 8)), step_family(256, 4, 1, (4, 1), (4, 8)), step_family(256, 4, 2, (4, 2), (4, 8))],
    (512, 16): [step_family(512, 16, 0, (16, 2), (16, 8)), step_family(512, 16, 1, (16, 1), (16, 8)), step_family(512, 16, 4, (16, 2), (16, 4))],
    (512, 8): [step_family(512, 8, 0, (8, 4), (8, 8)), step_family(512, 8, 1, (8, 1), (8, 8)), step_family(512, 8, 2, (8, 2), (8, 8)),
               step_family(512, 8, 4, (8, 4), (8, 4)), step_family(512, 8, 16, (8, 4), (8, 16))],
    (512, 4): [step_family(512, 4, 0, (4, 4), (4, 8)), step_family(512, 4, 1, (4, 1), (4, 8)), step_family(512, 4, 2, (4, 2), (4, 8)),
               step_family(512, 4, 8, (4, 8), (4, 8)), step_family(512, 4, 4, (4, 4), (4, 4)), step_family(512, 4, 16, (4, 4), (4, 16))],
}
FAMILIES += [f for group in STEP_GROUPS.values() for f in group] + [step_family(512, 8, 2, (8, 2), (8, 8), B=17),
                                                                    step_family(512, 4, 16, (4, 4), (4, 16), B=17)]
FAMILY_IDS = [f[0] for f in FAMILIES]


def run(fam, pre, w_hh, d_out=None, lengths=None):
    """engine.blstm_recurrence under the family's knobs, results as numpy: dict out, csave, act, dgates."""
    from speechsplit_amd import engine as E
    _, H, _, _, knobs = fam
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for k, v in knobs.items():
        E.tune(k, v)
    try:
        E.reset_variants()                                # what is read below was written by THIS launch, not by an earlier test's
        res = E.blstm_recurrence(dev(pre), tuple(dev(w) for w in w_hh), None if d_out is None else dev(d_out), lengths)
        torch.cuda.synchronize()
        ran = (E.seen_variants('lstm_step_fwd'), E.seen_variants('lstm_step_bwd'))
        if fam[0] in EXPECT:                              # every step ran the one instance the knobs were meant to select, and nothing else
            want = ([EXPECT[fam[0]][0]], [EXPECT[fam[0]][1]] if d_out is not None else [])
            assert ran == want, (fam[0], 'launched', ran, 'expected', want)
        else:                                             # lstm_small / the persistent kernels: no per-step launch at all
            assert ran == ([], []), (fam[0], ran)
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


@functools.lru_cache(maxsize=None)
def _trained_run(name):
    """One trained-scale forward + backward of family `name`, made once and never changed."""
    fam = FAMILIES[FAMILY_IDS.index(name)]
    pre, w, d = R.trained(fam[2], fam[3], fam[1], 3)
    return run(fam, pre, w, d)


GROUP_PAIRS = [(g[0][0], f[0]) for g in STEP_GROUPS.values() for f in g[1:]]


@pytest.mark.parametrize('default,other', GROUP_PAIRS, ids=[o for _, o in GROUP_PAIRS])
def test_group_size_does_not_change_the_bits(default, other):
    """Instances of one (H, NW) add the same products into the same accumulators in the same order (this file's docstring): with trained-scale
    W_hh every saved array of the forward and the backward has the bits of that (H, NW)'s lstm_g = 0 instance."""
    a, b = _trained_run(default), _trained_run(other)
    diff = {k: int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()) for k in a}
    print(f'lstm_steps {other} against {default}: elements whose bits differ ' + ' '.join(f'{k} {v}' for k, v in diff.items()))
    assert all(np.isfinite(v).all() and v.any() for v in b.values()), other
    assert not any(diff.values()), (other, default, diff)
