"""Engine-level containment (pytest -m gpu): a whole engine bound to guarded memory, the zero-at-rest invariants of its slabs, and the
independence of a step from whatever the engine ran before.

Guarded binding.  The four arenas, the workspace, the loss word, every input, the draws and every output are carved out of guarded
allocations (tests/guarded.py).  The workspace is 256-byte aligned, EXACTLY ss_workspace_bytes() long (ss_plan_bytes(1, T) after a move) and
filled with the quiet-NaN pattern before ss_bind: the bind zeroes the planned part only, so the never-zeroed scratch behind it (engine.hip
part_floats: split-K partial slabs, column sums, fused encoder weight gradients) starts as NaN and any read-before-write of it shows in
the results.  After every run: all guards bit for bit, ss_check, finite results, ss_scratch_fallbacks() == 0, and agreement with the same
run on an ordinary Engine at the bar the existing test of that path uses -- 1e-4 (the suite's TOL) on outputs, losses and per-tensor
gradients, conftest.assert_same_trajectory on stepped parameters (test_gpu_buckets_dp.py), test_gpu_configs.BF16_BOUNDS in the 16-bit mode,
bit identity under ss_tune("deterministic", 1) (test_deterministic_mode_is_bit_reproducible).  The status slot (last four floats of the
gradient arena) lies inside the arena and is not guard."""
import numpy as np
import pytest
import torch

from conftest import assert_same_trajectory
from oracle import interp_np, weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from tests import guarded as G
from tests.test_capi_bottleneck_widths import hparams_of
from tests.test_gpu_configs import BF16_BOUNDS

pytestmark = pytest.mark.gpu
TOL = 1e-4
LR = 1e-4
DEV = 'cuda'
WSEED = {'G3': 3, 'G6': 4}


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def stack_draws(draws):
    return np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])


class Bound:
    """An Engine whose every device buffer comes from a guarded allocation (Engine's `alloc` provider)."""

    def __init__(self, E, kind, hp, B, T, precision='f32'):
        self.keep, self.outs, self.ins = [], [], []
        self.eng = E.Engine(kind, hp, B, T, alloc=self.alloc)
        assert self.ws.t.numel() == self.eng.lib.ss_workspace_bytes(self.eng.h)
        self.eng.set_precision(precision)
        self.eng.load_weights(W.make_weights(kind, hp, WSEED[kind]))
        self.eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)

    def alloc(self, name, shape, dtype):
        if name in ('params', 'grads', 'adam_m', 'adam_v'):
            g = G.out(shape, DEV, fill=0.0, offset=64, name=name)               # header ss_bind: "All four arenas hold ss_arena_numel floats"
        elif name == 'ws':
            g = G.out(shape, DEV, dtype=torch.uint8, offset=256, name='ws')      # the pattern everywhere: scratch behind the plan starts as NaN
            assert g.t.data_ptr() % 256 == 0                                     # header ss_set_workspace: "256-byte aligned"
            self.ws = g
        elif name == 'loss':
            g = G.out(shape, DEV, offset=3, name='loss')
        else:
            g = G.out(shape, DEV, offset=(1, 64, 3)[len(self.outs) % 3], name=name)
            self.outs.append(g)
            return g.t
        self.keep.append(g)
        return g.t

    def inp(self, t, name, dtype=None):
        t = torch.as_tensor(t)
        g = G.inp(t.to(dtype) if dtype else t, DEV, offset=(3, 64, 1, 5)[len(self.ins) % 4], name=name)
        self.ins.append(g)
        return g.t

    def draws(self, d):
        return self.inp(d[0], 'scales', torch.float32), self.inp(d[1], 'len_seg', torch.int32)

    def check(self, tag):
        self.eng.check()
        for g in self.keep + self.ins:
            g.check(written=False)
        for g in self.outs:
            g.check()                                                            # fresh outputs: fully written as well
            assert bool(torch.isfinite(g.t).all()), (tag, g.name)
        self.outs.clear()
        self.ins.clear()
        assert self.eng.scratch_fallbacks() == 0, tag
        assert bool(torch.isfinite(self.eng.params).all()) and bool(torch.isfinite(self.eng.grads).all()), tag


def plain(E, kind, hp, B, T, precision='f32'):
    e = E.Engine(kind, hp, B, T)
    e.set_precision(precision)
    e.load_weights(W.make_weights(kind, hp, WSEED[kind]))
    e.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    return e


def g3_batch(seed, B, T):
    mel, f0, emb, lens = synth_batch(seed, B, T, 64 if T <= 128 else 96)
    return mel, f0, emb, lens, stack_draws(draws_for(seed + 100, B, 4))


def g6_batch(seed, B, T):
    mel, f0, _, _ = synth_batch(seed, B, T, 96 if T > 128 else 64)
    qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
    return mel, torch.nn.functional.one_hot(qidx, 257).float(), qidx, stack_draws(draws_for(seed + 100, B, 3))


def g3_step(b, batch, **kw):
    """A Generator_3 train step on a Bound (guarded inputs) or on an ordinary Engine."""
    mel, f0, emb, lens, d = batch
    if isinstance(b, Bound):
        return b.eng.g3_train_step(b.inp(mel, 'mel'), b.inp(f0, 'f0'), b.inp(emb, 'emb'), b.inp(lens, 'len_org', torch.int32), b.draws(d), **kw)
    return b.g3_train_step(mel, f0, emb, lens, d, **kw)


def g6_step(b, batch, **kw):
    mel, onehot, qidx, d = batch
    if isinstance(b, Bound):
        return b.eng.g6_train_step(b.inp(mel, 'mel'), b.inp(onehot, 'f0_onehot'), b.inp(qidx, 'target_idx', torch.int32), b.draws(d), **kw)
    return b.g6_train_step(mel, onehot, qidx, d, **kw)


def same_grads(a, b, tol, tag, median=None):
    ga, gb = a.grad_views(), b.grad_views()
    errs = []
    for n in ga:
        errs.append(G.assert_close(ga[n], gb[n], tol, (tag, n)))
    if median is not None:
        assert float(np.median(errs)) < median, tag


def compare_step(tag, b, ref, la, lb, steps, bf16=False, exact=False):
    la, lb = float(la), float(lb)
    assert np.isfinite(la), tag
    if exact:
        assert la == lb and torch.equal(b.eng.grads, ref.grads) and torch.equal(b.eng.params, ref.params), tag
        return
    assert abs(la - lb) <= (BF16_BOUNDS['loss'] if bf16 else TOL) * abs(lb), (tag, la, lb)
    same_grads(b.eng, ref, BF16_BOUNDS['grad'] if bf16 else TOL, tag, BF16_BOUNDS['grad_median'] if bf16 else None)
    assert_same_trajectory(b.eng.params, ref.params, LR, steps, tag)


# --------------------------------------------------------------------------------------------- guarded binding
@pytest.mark.parametrize('B,T', [(16, 128), (64, 128), (16, 256)])
def test_guarded_g3_train_step_buckets_and_back(E, B, T):
    """Generator_3 train step at (max_batch, max_frames), then the same engine at a smaller bucket (SS_STEP_BUCKET, 5 x 96) and back.
    Each compared step starts both engines from the same weights and a fresh Adam state: in the default (atomic split-K) mode two identical
    runs already differ by up to lr in single weights after one step (conftest.assert_same_trajectory), which a later step's ReLU kinks
    amplify beyond 1e-4 -- that is run-to-run noise, not what this test is after; what carries over is the engine's workspace history."""
    hp = W.default_hparams(max_len_pad=T)
    b, ref = Bound(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
    w = W.make_weights('G3', hp, WSEED['G3'])
    full, small = g3_batch(11 + B, B, T), g3_batch(12 + B, 5, 96)
    for k, (batch, kw) in enumerate([(full, {}), (small, dict(bucket=True)), (full, {})]):
        for e in (b.eng, ref):
            e.load_weights(w)
            e.adam_m.zero_()
            e.adam_v.zero_()
            e.set_adam(LR, 0.9, 0.999, 1e-8, 0)
        la, lb = g3_step(b, batch, **kw), g3_step(ref, batch, **kw)
        b.check((B, T, k))
        compare_step((B, T, k), b, ref, la, lb, 1)


@pytest.mark.parametrize('training', [True, False], ids=['training', 'eval'])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_guarded_g3_forward_backward_input_gradients(E, training, precision):
    """g3_forward + g3_backward with all three input gradients, training and eval mode, both precisions."""
    B, T = 4, 128
    hp = W.default_hparams(max_len_pad=T)
    bf16 = precision == 'bf16'
    b, ref = Bound(E, 'G3', hp, 8, T, precision), plain(E, 'G3', hp, 8, T, precision)
    mel, onehot, _, d3 = g6_batch(21, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    emb = torch.nn.functional.one_hot(torch.arange(B) % hp.dim_spk_emb, hp.dim_spk_emb).float()
    d_out = torch.randn(B, T, hp.dim_freq, generator=torch.Generator().manual_seed(5)) * 0.1
    out = b.eng.g3_forward(b.inp(x_f0, 'x_f0'), b.inp(mel, 'x_org'), b.inp(emb, 'c_trg'), b.draws(d3) if training else None, training=training)
    dx = b.eng.g3_backward(b.inp(d_out, 'd_out'), inputs=E.Engine.G3_INPUTS)
    out_r = ref.g3_forward(x_f0, mel, emb, d3 if training else None, training=training)
    dx_r = ref.g3_backward(d_out, inputs=E.Engine.G3_INPUTS)
    G.assert_close(out, out_r, BF16_BOUNDS['out'] if bf16 else TOL, 'out')
    for n, a, r in zip(E.Engine.G3_INPUTS, dx, dx_r):
        G.assert_close(a, r, BF16_BOUNDS['grad'] if bf16 else TOL, 'd' + n)
    same_grads(b.eng, ref, BF16_BOUNDS['grad'] if bf16 else TOL, (training, precision))
    b.check((training, precision))


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_guarded_g6_train_step_and_input_gradients(E, precision):
    """Generator_6 at 32 x 192: a train step, then a training forward + backward with both input gradients."""
    B, T = 32, 192
    hp = W.default_hparams(max_len_pad=T)
    bf16 = precision == 'bf16'
    b, ref = Bound(E, 'G6', hp, B, T, precision), plain(E, 'G6', hp, B, T, precision)
    batch = g6_batch(31, B, T)
    la, lb = g6_step(b, batch), g6_step(ref, batch)
    b.check(('g6 step', precision))
    compare_step(('g6 step', precision), b, ref, la, lb, 1, bf16)
    mel, onehot, _, d3 = batch
    d_out = torch.randn(B, T, hp.dim_f0, generator=torch.Generator().manual_seed(6)) * 0.1
    out = b.eng.g6_forward(b.inp(mel, 'x_org'), b.inp(onehot, 'f0_trg'), b.draws(d3), training=True)
    dx = b.eng.g6_backward(b.inp(d_out, 'd_out'), inputs=E.Engine.G6_INPUTS)
    out_r = ref.g6_forward(mel, onehot, d3, training=True)
    dx_r = ref.g6_backward(d_out, inputs=E.Engine.G6_INPUTS)
    G.assert_close(out, out_r, BF16_BOUNDS['out'] if bf16 else TOL, 'logits')
    for n, a, r in zip(E.Engine.G6_INPUTS, dx, dx_r):
        G.assert_close(a, r, BF16_BOUNDS['grad'] if bf16 else TOL, 'd' + n)
    b.check(('g6 input gradients', precision))


def test_guarded_g3_bf16_train_step(E):
    """set_precision('bf16'): Generator_3 train step at 16 x 128 on guarded memory."""
    B, T = 16, 128
    hp = W.default_hparams(max_len_pad=T)
    b, ref = Bound(E, 'G3', hp, B, T, 'bf16'), plain(E, 'G3', hp, B, T, 'bf16')
    batch = g3_batch(41, B, T)
    la, lb = g3_step(b, batch), g3_step(ref, batch)
    b.check('bf16')
    compare_step('bf16', b, ref, la, lb, 1, bf16=True)


def test_guarded_deterministic_mode_is_bit_identical(E):
    """ss_tune("deterministic", 1): two train steps on guarded memory are bit-identical to the same steps on an ordinary engine (the
    ordered partial-slab split-K and column sums live in the never-zeroed scratch, here pre-filled with NaN)."""
    B, T = 16, 128
    hp = W.default_hparams(max_len_pad=T)
    E.tune('deterministic', 1)
    try:
        b, ref = Bound(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
        for k in range(2):
            batch = g3_batch(51 + k, B, T)
            la, lb = g3_step(b, batch), g3_step(ref, batch)
            b.check(('deterministic', k))
            compare_step(('deterministic', k), b, ref, la, lb, k + 1, exact=True)
    finally:
        E.tune('deterministic', 0)


def test_guarded_width_config_w_mix(E):
    """A non-default width configuration (tests/test_gpu_bottleneck_widths.py W_mix: widths 12 / 3 / 24, factors 4 / 16 / 8; padded row strides)."""
    B, T = 16, 192
    hp = hparams_of('W_mix', T)
    b, ref = Bound(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
    batch = g3_batch(61, B, T)
    la, lb = g3_step(b, batch), g3_step(ref, batch)
    b.check('W_mix')
    compare_step('W_mix', b, ref, la, lb, 1)


def test_guarded_native_data_parallel_step_one_rank(E):
    """ss_g3_dp_train_step on a one-rank communicator equals the plain step (test_gpu_buckets_dp.py), on guarded memory."""
    B, T = 8, 128
    hp = W.default_hparams(max_len_pad=T)
    b, ref = Bound(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
    b.eng.comm_init(0, 1)
    mel, f0, emb, lens, d = g3_batch(71, B, T)
    la = b.eng.dp_train_step_native(b.inp(mel, 'mel'), b.inp(f0, 'f0'), b.inp(emb, 'emb'), b.inp(lens, 'len_org', torch.int32), b.draws(d))
    lb = ref.g3_train_step(mel, f0, emb, lens, d)
    b.check('dp')
    compare_step('dp', b, ref, la, lb, 1)
    b.eng.lib.ss_comm_destroy(b.eng.h)


def test_guarded_eval_forward_2000_frames_on_a_16x192_workspace(E):
    """The header's own example: "a 16 x 192 Generator_3 workspace holds a 1 x 2000 forward" -- no growth, guarded, against an ordinary engine."""
    hp = W.default_hparams(max_len_pad=192)
    b, ref = Bound(E, 'G3', hp, 16, 192), plain(E, 'G3', hp, 16, 192)
    ws = b.ws
    assert b.eng.plan_bytes(1, 2000) <= ws.t.numel()
    mel, onehot, _, _ = g6_batch(81, 1, 2000)
    x_f0 = torch.cat((mel, onehot), -1)
    emb = torch.nn.functional.one_hot(torch.tensor([3]), hp.dim_spk_emb).float()
    out = b.eng.g3_forward(b.inp(x_f0, 'x_f0'), b.inp(mel, 'x_org'), b.inp(emb, 'c_trg'))
    assert b.ws is ws
    G.assert_close(out, ref.g3_forward(x_f0, mel, emb), TOL, 'out')
    b.check('1x2000')


def test_guarded_long_eval_forward_moves_the_workspace(E):
    """A 1 x 4096 eval forward on an 8 x 192 engine: ss_plan_bytes(1, T) > ss_workspace_bytes(), so the engine moves (ss_set_workspace) to a
    guarded, NaN-pre-filled workspace of exactly ss_plan_bytes(1, T) bytes; then a train step at the engine's own shape on the new workspace."""
    hp = W.default_hparams(max_len_pad=192)
    b, ref = Bound(E, 'G3', hp, 8, 192), plain(E, 'G3', hp, 8, 192)
    T = 4096
    need = b.eng.plan_bytes(1, T)
    assert need > b.ws.t.numel()
    mel, onehot, _, _ = g6_batch(91, 1, T)
    x_f0 = torch.cat((mel, onehot), -1)
    emb = torch.nn.functional.one_hot(torch.tensor([5]), hp.dim_spk_emb).float()
    out = b.eng.g3_forward(b.inp(x_f0, 'x_f0'), b.inp(mel, 'x_org'), b.inp(emb, 'c_trg'))
    assert b.ws.t.numel() == need and b.eng.ws.data_ptr() == b.ws.t.data_ptr()
    G.assert_close(out, ref.g3_forward(x_f0, mel, emb), TOL, 'out')
    b.check('1x4096')
    batch = g3_batch(92, 8, 192)
    la, lb = g3_step(b, batch), g3_step(ref, batch)
    b.check('step after the move')
    compare_step('step after the move', b, ref, la, lb, 1)


# --------------------------------------------------------------------------------------------- zero-at-rest invariants
def _small_widths(hp):
    """Name (without the layer digit) of the slabs whose rows are lstm_small_ld(H) floats apart -- a small BLSTM's out / csave / dmid and
    its output-gradient slab -- -> the 2H columns that carry data; everything past them is padding."""
    n1, n2, n3 = 2 * hp.dim_neck, 2 * hp.dim_neck_2, 2 * hp.dim_neck_3
    return {'enc1.lstm1.out': n1, 'enc1.lstm1.c': n1, 'enc1.lstm1.dmid': n1, 'enc1.d_o': n1,
            'enc1.lstm2.out': n3, 'enc1.lstm2.c': n3, 'enc3.lstm.out': n3, 'enc3.lstm.c': n3, 'enc.d_o': n3,
            'enc2.lstm.out': n2, 'enc2.lstm.c': n2, 'enc2.d_ot': n2}


# Slabs kernels.h declares zero-haloed ("two all-zero rows on either side of every utterance"; lstm_small_ld: "The padding columns are never
# written: zero, like the halo rows"): conv-block inputs and outputs, BLSTM out / csave, and their gradient slabs.  They must be among the
# engine's named slabs (ss_debug_names).  NO name is left out of the assertion: the remaining named slabs -- the conv outputs before the
# GroupNorm "*.conv", the gate slabs "*.gates<l>" (kernels.h WgradTask: "pre-activation gradients [R][8H] (halo rows zero)"), "dec.in",
# "dec.d_in", "out" and "d_out" (engine.hip: "gradient of the loss w.r.t. the head output is in d_out_slab (halo rows zero)") -- are
# written by contractions whose "rows computed for halo positions are never stored" (engine.hip flatten_rows) or per utterance from row
# HALO on, and no sentence in the source lets their halo be non-zero; so their halo rows are asserted zero like the others.
ZERO_HALO = ('in.mel', 'in.f0', 'in.org', 'enc.xf0', 'enc.xf1', 'enc.xf2', 'enc.act', 'enc2.act', 'enc.d_act', 'enc2.d_act', 'enc.d_xf',
             'enc1.d_o1', 'enc.d_o2', 'enc2.d_ot', 'dec.d_top')
ZERO_HALO_SUFFIX = ('.out0', '.out1', '.out2', '.c0', '.c1', '.c2', '.dmid0', '.dmid1')


@pytest.mark.parametrize('kind,name', [('G3', None), ('G3', 'W_mix'), ('G6', None)], ids=['g3', 'g3_w_mix', 'g6'])
def test_zero_at_rest_after_a_step_that_followed_a_larger_one(E, kind, name):
    """After a full train step at (B, T) that followed a step at a LARGER (B, T) on the same engine, EVERY named slab (ss_debug_names; the
    ones listed above must be among them) has exactly zero halo rows, and the small BLSTMs' output-shaped ones exactly zero lstm_small_ld
    padding columns, read whole through ss_debug_buffer (Engine.debug_buffer(halo=True))."""
    Bm, Tm, B, T = 16, 192, 6, 128
    hp = hparams_of(name, Tm) if name else W.default_hparams(max_len_pad=Tm)
    eng = plain(E, kind, hp, Bm, Tm)
    step = g3_step if kind == 'G3' else g6_step
    mk = g3_batch if kind == 'G3' else g6_batch
    step(eng, mk(101, Bm, Tm))
    step(eng, mk(102, B, T), bucket=True)
    eng.check()
    names = eng.debug_names()
    listed = [n for n in names if n in ZERO_HALO or (n.endswith(ZERO_HALO_SUFFIX) and '.lstm' in n)]
    assert len(listed) >= 12, listed
    widths = _small_widths(eng.hp)
    padded = 0
    for n in names:
        s = eng.debug_buffer(n, B, T, halo=True)
        sb = s.view(torch.int32)
        assert not bool(sb[:, :2].any()) and not bool(sb[:, T + 2:].any()), (n, 'halo rows not zero', int(sb[:, :2].count_nonzero() + sb[:, T + 2:].count_nonzero()))
        w = widths.get(n.rstrip('0123456789'))
        if w is not None and w < s.shape[2]:
            padded += 1
            assert not bool(sb[:, :, w:].any()), (n, 'padding columns not zero')
    if name == 'W_mix':
        assert padded >= 3, padded                                 # dim_neck_2 = 3: rows of 6 floats padded to 8 (out, c, enc2.d_ot)


# --------------------------------------------------------------------------------------------- history independence
@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_history_independence_is_bit_exact_in_deterministic_mode(E, kind):
    """ss_tune("deterministic", 1): a fresh engine A and an engine B that has first run a larger bucket, a bf16 step (then back to f32), an
    input-gradient backward and a long eval forward that moved its workspace -- then weights reloaded, Adam moments zeroed, step counter 0 --
    run the same three train steps at a (B, T) below the maximum: losses and parameter arenas bit-identical.  The split-K choice of a
    contraction is a function of its shape alone (engine.hip pick_ksplit), not of the workspace size, so A keeps its ordinary workspace.
    Every switch of precision or call kind here coincides with a change of (B, T), which re-zeroes the workspace (engine.hip geometry):
    history at an UNCHANGED shape is what tests/test_gpu_same_shape_history.py holds."""
    Bm, Tm, B, T = 12, 192, 6, 128
    hp = W.default_hparams(max_len_pad=Tm)
    step = g3_step if kind == 'G3' else g6_step
    mk = g3_batch if kind == 'G3' else g6_batch
    w = W.make_weights(kind, hp, WSEED[kind])
    E.tune('deterministic', 1)
    try:
        a, b = plain(E, kind, hp, Bm, Tm), plain(E, kind, hp, Bm, Tm)
        step(b, mk(201, Bm, Tm))                                   # the larger bucket
        b.set_precision('bf16')
        step(b, mk(202, 5, 96), bucket=True)
        b.set_precision('f32')
        Tb = 96                                                    # a train-mode forward runs at the current max_len_pad: the last bucket
        mel, onehot, _, d3 = g6_batch(203, 3, Tb)
        if kind == 'G3':
            emb = torch.nn.functional.one_hot(torch.arange(3), hp.dim_spk_emb).float()
            b.g3_forward(torch.cat((mel, onehot), -1), mel, emb, d3, training=True)
            b.g3_backward(torch.ones(3, Tb, hp.dim_freq) * 0.1, inputs=E.Engine.G3_INPUTS)
            ml, ol, _, _ = g6_batch(204, 1, 4096)
            assert b.plan_bytes(1, 4096) > b.ws.numel()
            b.g3_forward(torch.cat((ml, ol), -1), ml, emb[:1])
        else:
            b.g6_forward(mel, onehot, d3, training=True)
            b.g6_backward(torch.ones(3, Tb, hp.dim_f0) * 0.1, inputs=E.Engine.G6_INPUTS)
            ml, ol, _, _ = g6_batch(204, 1, 4096)
            assert b.plan_bytes(1, 4096) > b.ws.numel()
            b.g6_forward(ml, ol)
        b.check()
        b.load_weights(w)
        b.adam_m.zero_()
        b.adam_v.zero_()
        b.set_adam(LR, 0.9, 0.999, 1e-8, 0)
        for k in range(3):
            batch = mk(210 + k, B, T)
            la, lb = float(step(a, batch, bucket=True)), float(step(b, batch, bucket=True))
            assert la == lb, (kind, k, la, lb)
        a.check()
        b.check()
        assert torch.equal(a.params, b.params), kind
    finally:
        E.tune('deterministic', 0)


def test_input_gradient_targets_die_with_their_call(E):
    """A train-mode forward + ss_g3_backward_inputs into three caller buffers, then, on the same engine, another forward + plain
    ss_g3_backward of a DIFFERENT batch and output gradient (a target that outlived its call would be written again, with other values):
    the second pass's gradient arena is bit-identical to the same forward + backward on a fresh engine, and the three buffers keep the bits
    the first call gave them.  Deterministic mode, fp32, 2 x 128."""
    B, T = 2, 128
    hp = W.default_hparams(max_len_pad=T)
    emb = torch.nn.functional.one_hot(torch.arange(B), hp.dim_spk_emb).float()

    def pass_inputs(seed):
        mel, onehot, _, d3 = g6_batch(seed, B, T)
        d_out = torch.randn(B, T, hp.dim_freq, generator=torch.Generator().manual_seed(seed)) * 0.1
        return torch.cat((mel, onehot), -1), mel, d3, d_out

    x1, org1, draws1, dout1 = pass_inputs(301)
    x2, org2, draws2, dout2 = pass_inputs(302)
    E.tune('deterministic', 1)
    try:
        fresh, used = plain(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
        used.g3_forward(x1, org1, emb, draws1, training=True)
        dx = used.g3_backward(dout1, inputs=E.Engine.G3_INPUTS)
        used.check()
        kept = [t.clone() for t in dx]
        assert all(bool(torch.isfinite(t).all()) and bool(t.any()) for t in kept)
        for e in (used, fresh):
            e.g3_forward(x2, org2, emb.flip(0), draws2, training=True)
            assert e.g3_backward(dout2) is None
            e.check()
        assert torch.equal(used.grads.view(torch.int32), fresh.grads.view(torch.int32))
        assert bool(fresh.grads.any())
        for n, t, k in zip(E.Engine.G3_INPUTS, dx, kept):
            assert torch.equal(t.view(torch.int32), k.view(torch.int32)), n
    finally:
        E.tune('deterministic', 0)
