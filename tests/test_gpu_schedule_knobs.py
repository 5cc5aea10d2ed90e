"""The engine's schedule knobs (ss_tune keys read by csrc/engine.hip) on one training step each (pytest -m gpu): a key that moves launches to
other streams or changes their enqueue order must not change ONE BIT of the loss, the output or any gradient; a key that changes tiles or
the order of a sum must keep every gradient inside the float64 oracle's bars.  One step with no_adam under ss_tune("deterministic", 1) --
split-K then goes through ordered partial slabs or is not split at all (gemm_on, launch_gemm), the bias sums through the ordered column
sum -- on inputs of oracle.gen_fixtures (synth_batch, draws_for), on the smallest shapes that keep every branch alive:

  A  Generator_3  B = 4,  T = 64   f32 and bf16   T % 64 == 0: lstm_input_grad's batched per-utterance form
  B  Generator_3  B = 5,  T = 72   f32            the other input-gradient path (whole haloed slab)
  C  Generator_6  B = 3,  T = 64   f32 and bf16
  D  Generator_3  B = 33, T = 64   f32            forward_core's `B > 32` side-stream projections (pw); overlap 1 and 0 only
  E  Generator_3  B = 8,  T = 64   f32            gemm_tr / gemm_ws only: the smallest shape at which the step launches 128 x 128 fp16 x 2 tiles

Class of every row, with the line of engine.hip that decides it:
  bits    overlap=0          `par = e->side2 && e->side3 && g_overlap` and its siblings only choose streams (b2 = b3 = s) and fork_joins;
                             LstmBlk::defers_weights turns false: the decoder's weight gradients follow each layer on the same stream --
                             same descriptors (lstm_weight_grads takes no stream-dependent split: pick_ksplit(M, N, K)).
  bits    prio_order=0       `prio = par && g_prio_order && ...`: enqueue order; `bw.wg_defer = prio` only says whether the encoder BLSTMs'
                             fused weight-gradient tasks go out in one lstm_small_wgrad launch or one per layer (a task's tiles and their
                             16 row groups do not depend on the table it sits in); Generator_6: dw_off needs prio, see conv_dw_off.
  bits    seq_prio=0         lstm_seq.hip: s_setprio of the persistent recurrences' waves, no arithmetic.
  bits    defer_dw=0         LstmBlk::defers_weights: when the decoder's weight gradients are enqueued (and so whether the tail split exists).
  bits    dec_tail_split=m   dec_tail_split(m, b2, b3) returns streams only (DwRoute.over_ih / over_hh, dec_late's ws / on_main).
                             FOUND by this file: m = 3 (layer 0 + head on the MAIN stream) passed the main stream's handle where a null handle
                             means "the side stream" -- and a caller on PyTorch's default stream has the null handle, so 3 ran 0's placement
                             (bits right, schedule not the one asked for).  dec_late now takes the main stream by pointer.
  bits    conv_dw_off=0|2|3  `dw_off = g_conv_dw_off == 1 && ... && !g3`: Generator_6's conv weight gradients on b2 reading a per-block copy of
                             the conv-output gradient (d_act_l) instead of d_act: same values, same GEMM.  Inert on Generator_3 (`!g3`).
  bits    own_streams=1, probe_queues=0   ss_bind: which hipStreams the engine creates / picks.  Read at bind time, so the variant is a
                             FRESH engine built under the key, compared with the default engine's step.
  bits    gemm_tr=0|2, gemm_ws=1|2        gemm_bf16x3.hip: how a tile's operands reach LDS and the MFMA fragments (transposing read or not,
                             staging waves or not): the same fp16 pieces (an image that is refused is split in the loop with the same scale
                             word), the same three MFMAs per fragment pair, k-tiles in ascending order (test_gpu_gemm_ws.py's docstring).
                             Config E ONLY.  Both keys act on 128-wide fp16 x 2 tiles, and at A, B and C the step launches none: the
                             decoder's weight gradients reduce over K = B (T + 4) <= 380 rows, pick_ksplit gives 1, 2048 x 1024 is 128
                             tiles against launch_layout's 256 and falls to 128 x 64 (CAN_TR / CAN_WS false); dX loses its split in
                             deterministic mode and the convolutions have 12 tiles: 64 x 64.  The 16-bit mode sets GEMM_BF16, which excludes
                             both paths.  There the keys are INERT and a row would compare the default with itself, so there is none.  At
                             E, K = 544: ksplit 2 through partial slabs, 256 tiles, 128 x 128 TN.  Each row asserts from
                             ss_debug_last_variant("gemm_seen") what the step launched: by default the decoder's W_ih gradients on
                             "128x128 TN f16x2 tr pipe"; under gemm_ws = 2 on "128x128 TN f16x2 tr ws" and no pipelined launch left (the
                             precedence the launcher gives it); under gemm_tr = 0 no launch with "tr", under gemm_tr = 2 none of TN (both:
                             "128x128 TN f16x2", the one-buffer loop, since the pipelined one needs the transposing-read image).  gemm_ws = 1
                             excludes TN, and TN is the only 128 x 128 launch of the step at E (measured: the record below), so that row
                             asserts that the step's launches are the default's -- inside the engine the key is inert at every shape an
                             oracle-sized test can afford; what it selects is tested alone in test_gpu_gemm_ws.py::test_ws1_heuristic.
  bits    overlap=0 + prio_order=0
  oracle  dx_batched=0|1     lstm_input_grad: the batch geometry of the input-gradient GEMM (per utterance without halo rows, or the whole
                             slab) and `g.want = g_dx_batched == 2 ? 512 : 0`, i.e. its TILE.  REACH at these shapes: the decoder's layers
                             take the `tiles < 512 && K >= 1024` split-K branch in front of the key (it needs B (T + 4) >= 4096 rows to get
                             past it, too large for a float64 oracle per row), so at A and C the key only reaches the encoder BLSTMs' input
                             gradients (K = 8 H <= 256), whose tile is 64 x 64 either way, and at B (T % 64 != 0) it reaches nothing.  The
                             rows' figures are equal to three digits for that reason; they show that the key is harmless here, not that
                             the decoder's batched form is right -- that is test_gpu_parity's dx_batched row at 4 x 128 and the 64 x 128
                             tests.  The rows print whether the variant's bits differ from the default's.
  oracle  lstm_nw=4 + persist=0   the decoder recurrences on the per-step kernels <512, 4, .> instead of the persistent ones: other operand
                             rounding (fp32 MFMA), other weight-gradient route (no measured amax: bf16 x 3).
bits rows: default schedule, variant, default schedule again on the same engine; the two default runs must agree bit for bit (the
comparison is reproducible) and the variant with them: loss, the `out` debug buffer, every tensor of grad_views().  oracle rows: every
gradient tensor against the float64 autograd oracle (tests/test_gpu_configs.py's Case: the oracle takes the ReLU branches of the DEFAULT
schedule's step) at that file's bars -- fp32 1e-4 of the tensor's maximum for every tensor (no tensor gets the kink allowance of
test_gpu_parity.grad_tolerances: at least as strict), Generator_6 also its per-tensor norms against the default schedule's at
test_g6_train_step's 2e-4, bf16 at BF16_BOUNDS of test_bf16_mode_against_fp32_oracle.  No tolerance is chosen here.

That the schedule under test is the one that ran (ss_profile_timeline, fp32 configs): overlap=0 puts every bracket on stream 0; for every
dec_tail_split m the twelve dec_dw brackets sit on the streams dec_tail_split's table gives (TAIL_STREAMS restates it; the tail split IS
active at B = 4, T = 64: the default m = 9 shows streams {1, 3}); conv_dw_off on Generator_6: conv_dw brackets on stream 2 with 1, none
there with 0 / 2 / 3.

Every test restores every key it touched through `Knobs` (one helper, in a finally): the keys are process-global.
Figures on an MI355X (profiles/r05/variant_knobs/test_figures.txt): all 91 bits rows 0 differing tensors (after the
dec_tail_split = 3 fix above; before it the bits agreed too and the timeline did not), default run twice 0 in every row; config E launches
64x64 NT / NN / TN, 128x64 TN and "128x128 TN f16x2 tr pipe", the last becoming "128x128 TN f16x2 tr ws" (gemm_ws 2) and "128x128 TN f16x2"
(gemm_tr 0, 2).  Oracle rows: worst gradient tensor 3.3e-6 of its maximum in fp32 (bar 1e-4; loss error <= 8.5e-8), 16-bit mode worst 2.2e-2,
median 5.3e-3 (bars 2e-1, 2e-2); dx_batched 0 / 1: 0 gradient tensors differ in bits from the default's (its reach, above), lstm_nw 4 +
persist 0: all of them."""
import numpy as np
import pytest
import torch

from oracle import weights as W
from tests.test_gpu_configs import BF16_BOUNDS, TOL, Case, rel, stack_draws

pytestmark = pytest.mark.gpu

DEFAULTS = dict(overlap=1, prio_order=1, seq_prio=1, defer_dw=1, dec_tail_split=9, conv_dw_off=1, own_streams=0, probe_queues=1, dx_batched=2,
                gemm_tr=1, gemm_ws=0, lstm_nw=16, lstm_g=0, persist=1, deterministic=0)
CONFIGS = {'A': ('G3', 4, 64), 'B': ('G3', 5, 72), 'C': ('G6', 3, 64), 'D': ('G3', 33, 64), 'E': ('G3', 8, 64)}
WSEED = {'G3': 9, 'G6': 4}


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


class Knobs:
    """ss_tune values for a block; EVERY key of DEFAULTS is put back afterwards, whatever happened and whichever were touched."""

    def __init__(self, E, **kv):
        assert set(kv) <= set(DEFAULTS), kv
        self.E, self.kv = E, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.E.tune(k, v)

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self.E.tune(k, v)


_CASES = {}


def case_of(E, cfg, precision):
    """One engine and one oracle state per (config, precision), made once; .oracle: dict of the float64 step, made on first use."""
    key = (cfg, precision)
    if key not in _CASES:
        kind, B, T = CONFIGS[cfg]
        c = Case(E, kind, B, T, 64, wseed=WSEED[kind], bseed=900 + B + T, precision=precision)
        c.cfg, c.oracle = cfg, None
        _CASES[key] = c
    return _CASES[key]


def step(c, eng=None, timeline=False):
    """One training step without the optimiser: (loss, out, {name: gradient}, timeline or None, {kind: kernel instances this step launched})."""
    eng = eng or c.eng
    eng.lib.ss_debug_last_variant(b'reset', None, 0)     # what `seen` holds below was launched by this step
    if timeline:
        eng.profile('timeline')
    d = stack_draws(c.draws(0))
    if c.kind == 'G3':
        loss = eng.g3_train_step(c.mel, c.f0, c.emb, c.lens, d, no_adam=True)
    else:
        loss = eng.g6_train_step(c.mel, c.onehot, c.qidx, d, no_adam=True)
    eng.check()
    assert eng.scratch_fallbacks() == 0
    from speechsplit_amd import engine as E_
    seen = {k: E_.seen_variants(k) for k in ('gemm', 'lstm_step_fwd', 'lstm_step_bwd')}
    tl = None
    if timeline:
        tl = eng.profile_timeline()
        eng.profile(False)
    return float(loss), eng.debug_buffer('out', c.B, c.T).clone(), {n: v.clone() for n, v in eng.grad_views().items()}, tl, seen


def worst_difference(a, b):
    """(tensor name, max |a - b| / max |b|) of the worst of out and the gradients; ('', 0.0) when every bit agrees."""
    worst = ('', 0.0)
    for n, x, y in [('out', a[1], b[1])] + [(n, a[2][n], g) for n, g in b[2].items()]:
        if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
            worst = max(worst, (n, max(rel(x, y), 1e-45)), key=lambda t: t[1])
    return worst


def assert_bits(E, c, knobs, tag, variant_engine=None, check_timeline=None, check_seen=None):
    """default, variant, default: the defaults agree (reproducible), the variant agrees with them.  check_timeline(timeline of the variant);
    check_seen(GEMM instances the default step launched, those the variant step launched)."""
    with Knobs(E, deterministic=1):
        first = step(c)
    with Knobs(E, deterministic=1, **knobs):
        got = step(c, variant_engine, timeline=check_timeline is not None)
    with Knobs(E, deterministic=1):
        again = step(c)
    repro, diff = worst_difference(first, again), worst_difference(got, first)
    print(f'[schedule {c.cfg} {c.eng_precision} {tag}] loss {got[0]!r} (default {first[0]!r}); worst tensor difference to '
          f'the default schedule: {diff[0] or "none"} {diff[1]:.2e}; default run twice: {repro[0] or "none"} {repro[1]:.2e}')
    assert first[0] == first[0] and any(bool(g.any()) for g in first[2].values()), 'the step computed nothing'
    assert first[0] == again[0] and repro == ('', 0.0), ('the default schedule is not bit-reproducible', tag, repro)
    assert got[0] == first[0] and diff == ('', 0.0), (tag, got[0], first[0], diff)
    if check_timeline is not None:
        check_timeline(got[3])
    if check_seen is not None:
        print(f'[schedule {c.cfg} {c.eng_precision} {tag}] GEMM instances of the step: default {first[4]["gemm"]}; variant {got[4]["gemm"]}')
        check_seen(first[4]['gemm'], got[4]['gemm'])


def oracle_of(E, c):
    """The float64 oracle's gradients for this case (ReLU branches of the default schedule's step), once; the engine's weights are put back."""
    if c.oracle is None:
        r = c.step(0, kink_bound=5e-2 if c.eng_precision == 'bf16' else 2e-5)
        c.oracle = dict(loss=r['loss_cpu'], grads=r['grads_cpu'], default={n: g.double().norm() for n, g in r['grads_gpu'].items()})
        c.eng.load_weights(W.make_weights(c.kind, c.hp, WSEED[c.kind]))          # step() ran Adam
        c.eng.adam_m.zero_()
        c.eng.adam_v.zero_()
    return c.oracle


def assert_oracle(E, c, knobs, tag):
    ref = oracle_of(E, c)
    with Knobs(E, deterministic=1):
        base = step(c)
    with Knobs(E, deterministic=1, **knobs):
        got = step(c)
    loss, grads, ran = got[0], got[2], (got[4]['lstm_step_fwd'], got[4]['lstm_step_bwd'])
    differ = sorted(n for n, g in grads.items() if not torch.equal(g.view(torch.int32), base[2][n].view(torch.int32)))
    print(f'[schedule {c.cfg} {c.eng_precision} {tag}] gradient tensors whose bits differ from the default schedule\'s: {len(differ)} of {len(grads)}')
    el = abs(loss - ref['loss']) / abs(ref['loss'])
    eg = {n: rel(grads[n], g) for n, g in ref['grads'].items()}
    worst = max(eg.items(), key=lambda x: x[1])
    med = float(np.median(list(eg.values())))
    print(f'[schedule {c.cfg} {c.eng_precision} {tag}] loss error {el:.2e}; gradients against the float64 oracle: worst {worst[0]} {worst[1]:.2e}, median {med:.2e}')
    if c.eng_precision == 'bf16':
        assert el < BF16_BOUNDS['loss'] and worst[1] < BF16_BOUNDS['grad'] and med < BF16_BOUNDS['grad_median'], (tag, el, worst, med)
        return ran
    assert el <= 1e-5, (tag, loss, ref['loss'])
    assert worst[1] < TOL, (tag, worst)
    if c.kind == 'G6':                                   # test_g6_train_step's bar on the per-tensor norms, against the default schedule's
        for n, l2 in ref['default'].items():
            assert abs(float(grads[n].double().norm()) - float(l2)) <= 2e-4 * float(l2) + 1e-12, (tag, n)
    return ran


def get(E, cfg, precision):
    c = case_of(E, cfg, precision)
    c.eng_precision = precision
    return c


# ---- what the timeline must show -------------------------------------------------------------------------------------------------------------
SIDE, PITCH, THIRD, MAIN = 1, 2, 3, 0


def TAIL_STREAMS(m):
    """dec_tail_split(m, ...) restated: the streams of the twelve dec_dw brackets in enqueue order -- layer 2, 1, 0; per layer forward dW_ih,
    dW_hh, reverse dW_ih, dW_hh.  0: everything on the side stream."""
    l1 = {4: THIRD, 5: THIRD, 6: PITCH}.get(m, SIDE)
    l0 = {1: PITCH, 5: PITCH, 2: THIRD, 6: THIRD, 3: MAIN}.get(m, THIRD if m >= 7 else SIDE)
    l1_ih = THIRD if m in (7, 8) else l1
    l1_hh = PITCH if m == 7 else (THIRD if m in (8, 9, 10) else l1)
    l2_hh = THIRD if m == 10 else SIDE
    return [SIDE, SIDE, SIDE, l2_hh, l1, l1, l1_ih, l1_hh] + [l0] * 4


def tail_check(m):
    def check(tl):
        got = [st for k, _, _, st in tl if k == 'dec_dw']
        assert got == TAIL_STREAMS(m), (m, got, TAIL_STREAMS(m))
    return check


def all_on_main(tl):
    assert len(tl) >= 20 and {st for *_, st in tl} == {MAIN}, sorted({(k, st) for k, _, _, st in tl if st != MAIN})


def conv_dw_on_pitch_stream(expected):
    def check(tl):
        on = {st for k, _, _, st in tl if k == 'conv_dw'}
        assert on and ((PITCH in on) == expected), (expected, on)
    return check


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
F32_CONFIGS = [('A', 'f32'), ('B', 'f32'), ('C', 'f32')]
BOTH = F32_CONFIGS + [('A', 'bf16'), ('C', 'bf16')]
ids = lambda cs: [f'{c}_{p}' for c, p in cs]

BITS_ROWS = [dict(overlap=0), dict(prio_order=0), dict(seq_prio=0), dict(defer_dw=0), dict(overlap=0, prio_order=0)]


def row_id(kn):
    return '+'.join(f'{k}={v}' for k, v in kn.items())


@pytest.mark.parametrize('knobs', BITS_ROWS, ids=[row_id(k) for k in BITS_ROWS])
@pytest.mark.parametrize('cfg,precision', BOTH, ids=ids(BOTH))
def test_stream_and_order_knobs_keep_every_bit(E, cfg, precision, knobs):
    c = get(E, cfg, precision)
    check = all_on_main if knobs.get('overlap') == 0 and precision == 'f32' else None
    assert_bits(E, c, knobs, row_id(knobs), check_timeline=check)


@pytest.mark.parametrize('overlap', (1, 0))
def test_side_stream_forward_branch_above_32_utterances(E, overlap):
    """Config D (B = 33): forward_core's `pw = e->side3 && g_overlap && !compact && B > 32` -- the default schedule against itself and overlap=0."""
    c = get(E, 'D', 'f32')
    assert_bits(E, c, dict(overlap=overlap), f'overlap={overlap}', check_timeline=all_on_main if overlap == 0 else None)


@pytest.mark.parametrize('m', range(11))
@pytest.mark.parametrize('cfg,precision', [('A', 'f32'), ('B', 'f32'), ('A', 'bf16')], ids=['A_f32', 'B_f32', 'A_bf16'])
def test_dec_tail_split_values(E, cfg, precision, m):
    """Every value of the tail-split table: the decoder's weight gradients on the streams the table names (fp32), every bit as with the default."""
    c = get(E, cfg, precision)
    assert_bits(E, c, dict(dec_tail_split=m), f'dec_tail_split={m}', check_timeline=tail_check(m) if precision == 'f32' else None)


@pytest.mark.parametrize('v', (0, 1, 2, 3))
@pytest.mark.parametrize('cfg,precision', [('C', 'f32'), ('C', 'bf16'), ('A', 'f32')], ids=['C_f32', 'C_bf16', 'A_f32_inert'])
def test_conv_dw_off_values(E, cfg, precision, v):
    """Generator_6: only 1 takes the conv weight gradients off the trunk's chain (stream 2); 0, 2 and 3 leave them on it.  Generator_3: inert."""
    c = get(E, cfg, precision)
    check = conv_dw_on_pitch_stream(v == 1) if (cfg, precision) == ('C', 'f32') else None
    assert_bits(E, c, dict(conv_dw_off=v), f'conv_dw_off={v}', check_timeline=check)


@pytest.mark.parametrize('knobs', [dict(own_streams=1), dict(probe_queues=0), dict(own_streams=1, probe_queues=0)], ids=row_id)
@pytest.mark.parametrize('cfg,precision', BOTH, ids=ids(BOTH))
def test_bind_time_stream_knobs(E, cfg, precision, knobs):
    """own_streams / probe_queues are read by ss_bind: a fresh engine built under the key against the default engine, bit for bit."""
    c = get(E, cfg, precision)
    with Knobs(E, **knobs):
        eng = E.Engine(c.kind, c.hp, c.B, c.T)
        eng.set_precision(precision)
        eng.load_weights(W.make_weights(c.kind, c.hp, WSEED[c.kind]))
    assert_bits(E, c, knobs, row_id(knobs) + ' (fresh engine)', variant_engine=eng)


ORACLE_ROWS = [dict(dx_batched=0), dict(dx_batched=1), dict(dx_batched=2), dict(lstm_nw=4, persist=0)]


@pytest.mark.parametrize('knobs', ORACLE_ROWS, ids=[row_id(k) for k in ORACLE_ROWS])
@pytest.mark.parametrize('cfg,precision', BOTH, ids=ids(BOTH))
def test_tile_and_kernel_knobs_against_the_float64_oracle(E, cfg, precision, knobs):
    """dx_batched = 2 is the default: the same bars on the schedule every other row is compared with."""
    c = get(E, cfg, precision)
    ran = assert_oracle(E, c, knobs, row_id(knobs))
    H = '512' if c.kind == 'G3' else '256'
    if 'lstm_nw' in knobs:                                  # THIS step ran the decoder's recurrences (H = 512, Generator_6: 256) step by step on 4 waves, and no other instance
        assert [[r.split()[:2] for r in kind] for kind in ran] == [[[H, '4']], [[H, '4']]], ran
    else:                                                   # persistent kernels: no per-step launch
        assert ran == ([], []), ran


# ---- gemm_tr / gemm_ws inside the engine: config E, where the step launches 128 x 128 fp16 x 2 tiles ----------------------------------------------
def big(seen):
    return [v for v in seen if v.startswith('128x128 ') and ' f16x2' in v]


def gemm_rule(knobs):
    """What the step's GEMM launches must look like under the key (launch_cfg's rules, restated), given what the default step launched."""
    def check(default, variant):
        assert any(v.startswith('128x128 TN f16x2 tr pipe') for v in default), ('the default step has no pipelined 128 x 128 TN launch: the shape is too small for this test', default)
        assert [v for v in variant if not v.startswith('128x128 ')] == [v for v in default if not v.startswith('128x128 ')], 'other tiles are not the keys\' business'
        tn = [v for v in big(variant) if ' TN ' in v]
        assert tn, variant
        if knobs.get('gemm_ws') == 2:       # every 128 x 128 fp16 x 2 launch wave-specialised, the pipelined loop's included
            assert all(v.endswith(' ws') for v in big(variant)) and '128x128 TN f16x2 tr ws' in variant and not any('pipe' in v for v in variant), variant
        if knobs.get('gemm_ws') == 1:       # never for TN; for the others where the grid has at most 320 workgroups
            assert not any(v.endswith(' ws') for v in tn) and big(variant) != [] and tn == [v for v in big(default) if ' TN ' in v], variant
        if knobs.get('gemm_tr') == 0:       # no transposing read anywhere, hence no pipelined loop (it needs B's transposing-read image)
            assert not any(' tr' in v for v in variant) and '128x128 TN f16x2' in variant, variant
        if knobs.get('gemm_tr') == 2:       # not for TN
            assert not any(' tr' in v for v in tn) and '128x128 TN f16x2' in variant, variant
            assert [v for v in big(variant) if ' TN ' not in v] == [v for v in big(default) if ' TN ' not in v], variant
    return check


GEMM_ROWS = [dict(gemm_tr=0), dict(gemm_tr=2), dict(gemm_ws=1), dict(gemm_ws=2)]


@pytest.mark.parametrize('knobs', GEMM_ROWS, ids=[row_id(k) for k in GEMM_ROWS])
def test_gemm_form_knobs_keep_every_bit_where_they_act(E, knobs):
    """Config E: the keys change the kernels the step launches (asserted from the record of the step's launches) and not one bit of it."""
    c = get(E, 'E', 'f32')
    assert_bits(E, c, knobs, row_id(knobs), check_seen=gemm_rule(knobs))
