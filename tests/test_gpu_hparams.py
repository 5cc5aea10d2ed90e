"""Every ss_hparams field beyond the bottleneck widths at non-default values (pytest -m gpu): conv widths, the mel, speaker and F0 widths and
the InterpLnr segment fields, through eval forwards, rhythm codes, two training steps, input gradients, the resampling op, guarded memory,
the 16-bit mode and the default (non-deterministic) mode.  The float64 / fp32 oracle takes every field from hp, so each comparison is
against it at the suite's bars, imported and not restated: check_fp32_step, check_adam and BF16_BOUNDS of tests/test_gpu_configs.py,
TOL = 1e-4, the kink bound 2e-5 of Case.step, compare_step of tests/test_gpu_engine_containment.py.

The configurations (tests/test_capi_hparams.py CONFIGS; RUNNING here, the refused ones have their test there):
  H_narrow  dim_freq 36, speaker 81, conv widths 192 / 64 / 64: layer-0 blocks without weight images (Cp % 8 == 4), head N = 36, an odd
            163-wide decoder input, one-tile GroupNorms, CE = 256
  H_wide    dim_freq 100, speaker 256, conv widths 576 / 192 / 320: blocks wider than 512, CE = 896, four slices in the speaker gradient
  H_spk1    speaker width 1: 1024 one-column slices in the speaker gradient, an 83-wide decoder input
  H_segs10  segments of 10..23 frames, S = 10, 48 candidates;  H_segs3: S = 3 segments of 31 frames (T = 128: dead rows in every slab)
  P_narrow  Generator_6 at dim_freq 36, conv widths 64 / 64, S = 10;  P_f0_65: Generator_6 over 65 F0 classes (f0p = 72)
Speaker embeddings are dense random rows, so every column of the speaker gradient carries a value of its own."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import interp_np, ref_model, weights as W
from oracle.gen_fixtures import synth_batch
from tests import guarded as G
from tests.test_capi_hparams import CONFIGS, RUNNING, TRAIN_T, draws_of, hparams_of, nseg, train_seeds
from tests.test_gpu_configs import BF16_BOUNDS, LR, Case, check_adam, check_fp32_step, stack_draws
from tests.test_gpu_engine_containment import Bound, compare_step, g3_step, g6_step, plain
from tests.test_gpu_input_grads import engine_branches, masks_of

pytestmark = pytest.mark.gpu
TOL = 1e-4
WSEED = {'G3': 3, 'G6': 4}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def p64(w):
    return {k: torch.from_numpy(np.array(v, dtype=np.float64)) for k, v in w.items()}


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def batch_of(hp, seed, B, T, len_lo):
    """oracle.gen_fixtures.synth_batch at hp's widths, the speaker rows dense."""
    mel, f0, _, lens = synth_batch(seed, B, T, len_lo, dim_freq=hp.dim_freq, dim_spk_emb=hp.dim_spk_emb)
    emb = torch.rand(B, hp.dim_spk_emb, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
    return mel, f0, emb, lens


def f0_inputs(hp, seed, B, T, f0=None):
    """Generator_6's one-hot input and target classes: the quantised F0 track at the reference's 257 classes, else random classes."""
    if hp.dim_f0 == 257 and f0 is not None:
        qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
        return torch.nn.functional.one_hot(qidx, 257).float(), qidx
    g = torch.Generator().manual_seed(seed + 2)
    onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (B, T), generator=g), hp.dim_f0).float()
    return onehot, torch.randint(0, hp.dim_f0, (B, T), generator=g)


def eval_inputs(hp, seed, B, T):
    mel, f0, emb, _ = batch_of(hp, seed, B, T, T)
    return mel, f0_inputs(hp, seed, B, T)[0], emb


class HCase(Case):
    """tests/test_gpu_configs.Case with the hparams of a configuration: batch widths, draws and segment count follow hp."""

    def __init__(self, E, name, B, T, len_lo, bseed, dseed, precision='f32'):
        kind = CONFIGS[name][0]
        self.kind, self.B, self.T = kind, B, T
        self.hp = hp = hparams_of(name, T)
        w = W.make_weights(kind, hp, WSEED[kind])
        self.eng = E.Engine(kind, hp, B, T)
        self.eng.set_precision(precision)
        self.eng.load_weights(w)
        self.eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
        self.st = ref_model.TrainState(w, LR)
        self.mel, self.f0, self.emb, self.lens = batch_of(hp, bseed, B, T, len_lo)
        self.ncalls = 4 if kind == 'G3' else 3
        if kind == 'G6':
            self.onehot, self.qidx = f0_inputs(hp, bseed, B, T, self.f0)
        self.dseed = dseed

    def draws(self, it):
        return draws_of(self.hp, self.dseed + it, self.B, self.ncalls)


# --------------------------------------------------------------------------------------------- 1: eval forwards and rhythm codes
@pytest.mark.parametrize('name', RUNNING)
def test_eval_forward_and_codes(E, name):
    B, T = 3, 64
    kind = CONFIGS[name][0]
    hp = hparams_of(name, T)
    w = W.make_weights(kind, hp, WSEED[kind])
    P = p64(w)
    e = plain(E, kind, hp, B, T)
    mel, onehot, emb = eval_inputs(hp, 10 + len(name), B, T)
    with torch.no_grad():
        if kind == 'G3':
            x_f0 = torch.cat((mel, onehot), -1)
            out = e.g3_forward(x_f0, mel, emb)
            ref = ref_model.generator_3(P, hp, x_f0.double(), mel.double(), emb.double())
        else:
            out = e.g6_forward(mel, onehot)
            ref = ref_model.generator_6(P, hp, mel.double(), onehot.double())
    e.check()
    assert out.shape == ref.shape == (B, T, hp.dim_freq if kind == 'G3' else hp.dim_f0)
    err = rel(out, ref)
    print(f'[{name} eval {B}x{T}] rel {err:.2e}')
    assert err < TOL
    if kind == 'G3':
        codes = e.g3_rhythm(mel)
        with torch.no_grad():
            ref_c = ref_model.encoder_t(mel.double().transpose(1, 2), P, hp)
        assert codes.shape == ref_c.shape == (B, T // hp.freq_2, 2 * hp.dim_neck_2)
        assert rel(codes, ref_c) < TOL


# --------------------------------------------------------------------------------------------- 2: two training steps
def _train_steps(E, name, B):
    T = TRAIN_T[name]
    bseed, dseed = train_seeds(name, B)
    c = HCase(E, name, B, T, T // 2, bseed, dseed)
    hp, S = c.hp, nseg(c.hp)
    for it in range(2):                       # the second step runs on the first one's update
        draws = c.draws(it)
        assert draws[0][0].shape == (B * S,)
        if name.startswith('H_segs'):          # what the configuration is for, asserted before the engine runs (tests/test_capi_hparams.py)
            counts = np.stack([interp_np.interp_plan(d[0], d[1], np.full(B, T), hp.max_len_seg, T)[2] for d in draws[1:]])
            assert bool((counts < T).all()) if name == 'H_segs3' else bool((counts >= T).any()), counts
        r = c.step(it)
        check_fp32_step(r, f'{name} {B}x{T} step {it}')
        check_adam(r, f'{name} {B}x{T} step {it}', it)
        assert c.eng.scratch_fallbacks() == 0
        # every resampled slab: rows behind the utterance's row count are zeros
        for i, d in enumerate(draws[-3:]):
            nrows = interp_np.interp_plan(d[0], d[1], np.full(B, T), hp.max_len_seg, T)[3]
            xf = c.eng.debug_buffer(f'enc.xf{i}', B, T).cpu()
            for b in range(B):
                assert not bool(xf[b, int(nrows[b]):].any()), (name, i, b)
                assert bool(xf[b, :int(nrows[b])].any()), (name, i, b)
        if c.kind == 'G3':                    # the outer call: resampled mel bit-exact, F0 classes those of the reference's quantiser
            xi = ref_model.interp(torch.cat((c.mel, c.f0), -1), c.lens.numpy(), draws[0], hp)
            assert np.array_equal(c.eng.debug_buffer('in.mel', B, T).cpu().numpy(), xi[:, :, :hp.dim_freq].numpy())
            f0s = c.eng.debug_buffer('in.f0', B, T).cpu()
            assert np.array_equal(f0s[:, :, :hp.dim_f0].argmax(-1).numpy(), interp_np.quantize_f0(xi[:, :, -1].numpy()))
            assert bool((f0s.sum(-1) == 1).all())                      # one class per row, nothing in the padding columns


@pytest.mark.parametrize('name', RUNNING)
def test_train_steps_against_oracle(E, name):
    _train_steps(E, name, 3)


def test_train_steps_partial_second_batch_tile(E):
    """B = 17: one full 16-utterance tile and one with a single row."""
    _train_steps(E, 'H_narrow', 17)


# --------------------------------------------------------------------------------------------- 3: input gradients
@pytest.mark.parametrize('name', ['H_narrow', 'H_wide', 'H_spk1', 'P_narrow'])
def test_input_gradients_against_oracle(E, name):
    """ss_g3_backward_inputs / ss_g6_backward_inputs of a training forward against the oracle's autograd in float64, with the decoder's
    layer 0 in its compact form and in the full one (ss_tune("compact0")): dc_trg is spk_grad_kernel at E = 81, 256 and 1."""
    B, T = 3, 64
    kind = CONFIGS[name][0]
    hp = hparams_of(name, T)
    w = W.make_weights(kind, hp, 7)
    mel, onehot, emb = eval_inputs(hp, 50 + len(name), B, T)
    draws = draws_of(hp, 550 + len(name), B, 3)
    wout = torch.randn(B, T, hp.dim_freq if kind == 'G3' else hp.dim_f0, generator=torch.Generator().manual_seed(5))
    xs_in = (torch.cat((mel, onehot), -1), mel, emb) if kind == 'G3' else (mel, onehot)
    names = E.Engine.G3_INPUTS if kind == 'G3' else E.Engine.G6_INPUTS
    ref = None
    for compact in (1, 0):
        E.tune('compact0', compact)
        try:
            eng = E.Engine(kind, hp, B, T)
            eng.load_weights(w)
            if kind == 'G3':
                eng.g3_forward(*xs_in, stack_draws(draws), training=True)
            else:
                eng.g6_forward(*xs_in, stack_draws(draws), training=True)
            masks = masks_of(eng, B, T)
            got = (eng.g3_backward if kind == 'G3' else eng.g6_backward)(wout.cuda(), inputs=names)
            eng.check()
        finally:
            E.tune('compact0', 1)
        if ref is None:                       # the oracle once: the conv trunk, and so its ReLU branches, does not depend on the decoder's form
            xs = [x.double().requires_grad_() for x in xs_in]
            with engine_branches(masks):
                out = (ref_model.generator_3 if kind == 'G3' else ref_model.generator_6)(p64(w), hp, *xs, draws, True)
            (out * wout.double()).sum().backward()
            ref = [x.grad for x in xs]
        for n, a, r in zip(names, got, ref):
            assert a.shape == r.shape
            err = rel(a, r)
            print(f'[{name} compact0={compact}] d{n} rel {err:.2e}')
            assert err < TOL, (n, compact, err)


# --------------------------------------------------------------------------------------------- 4: the resampling op
@pytest.mark.parametrize('segs', ['H_segs10', 'H_segs3'])
@pytest.mark.parametrize('C_', [36, 81])
def test_interp_op_other_segment_counts(E, segs, C_):
    """ss_interp_forward / ss_interp_backward on an SS_INTERP_ONLY engine at S = 10 / 48 candidates and S = 3 / 64 candidates: the plan and
    the values bit-exact against oracle/interp_np.py, the adjoint at the 1e-6 of test_interp_bit_exact_against_reference."""
    B, T = 3, 128
    hp = hparams_of(segs, T)
    eng = E.Engine('interp', hp, B, T)
    lens = np.array([128, 101, 64])
    x = torch.randn(B, T, C_, generator=torch.Generator().manual_seed(C_))
    (sc, ls), = draws_of(hp, 70 + C_, B, 1)
    y, i0, lam, cnt = eng.interp_forward(x, lens, sc, ls, want_plan=True)
    ri0, rlam, rcnt, rn = interp_np.interp_plan(sc, ls, lens, hp.max_len_seg, T)
    assert np.array_equal(i0.cpu().numpy(), ri0) and np.array_equal(cnt.cpu().numpy(), rcnt)
    assert np.array_equal(lam.cpu().numpy(), rlam)
    assert np.array_equal(y.cpu().numpy(), interp_np.interp_apply(x.numpy(), ri0, rlam, rn))
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    dx = eng.interp_backward(dy, T)
    assert rel(dx, interp_np.interp_backward(dy.numpy(), ri0, rlam, rn, T)) < 1e-6


# --------------------------------------------------------------------------------------------- 5: guarded memory
@pytest.mark.parametrize('name', [n for n in ('H_narrow', 'H_oddmel', 'P_narrow') if n in RUNNING])
def test_guarded_step_and_input_gradients(E, name):
    """One train step and one training forward + backward with every input gradient on guarded, NaN-surrounded memory
    (tests/test_gpu_engine_containment.py): guards intact, everything finite, and in deterministic mode bit-identical to an ordinary engine."""
    B, T = 3, 64
    kind = CONFIGS[name][0]
    hp = hparams_of(name, T)
    mel, f0, emb, lens = batch_of(hp, 80 + len(name), B, T, T // 2)
    onehot, qidx = f0_inputs(hp, 80, B, T, f0)
    E.tune('deterministic', 1)
    try:
        b, ref = Bound(E, kind, hp, B, T), plain(E, kind, hp, B, T)
        d = stack_draws(draws_of(hp, 180, B, 4 if kind == 'G3' else 3))
        if kind == 'G3':
            batch = (mel, f0, emb, lens, d)
            la, lb = g3_step(b, batch), g3_step(ref, batch)
        else:
            batch = (mel, onehot, qidx, d)
            la, lb = g6_step(b, batch), g6_step(ref, batch)
        b.check((name, 'step'))
        compare_step((name, 'step'), b, ref, la, lb, 1, exact=True)
        d3 = stack_draws(draws_of(hp, 181, B, 3))
        if kind == 'G3':
            x_f0 = torch.cat((mel, onehot), -1)
            d_out = torch.randn(B, T, hp.dim_freq, generator=torch.Generator().manual_seed(5)) * 0.1
            out = b.eng.g3_forward(b.inp(x_f0, 'x_f0'), b.inp(mel, 'x_org'), b.inp(emb, 'c_trg'), b.draws(d3), training=True)
            dx = b.eng.g3_backward(b.inp(d_out, 'd_out'), inputs=E.Engine.G3_INPUTS)
            out_r = ref.g3_forward(x_f0, mel, emb, d3, training=True)
            dx_r = ref.g3_backward(d_out, inputs=E.Engine.G3_INPUTS)
        else:
            d_out = torch.randn(B, T, hp.dim_f0, generator=torch.Generator().manual_seed(6)) * 0.1
            out = b.eng.g6_forward(b.inp(mel, 'x_org'), b.inp(onehot, 'f0_trg'), b.draws(d3), training=True)
            dx = b.eng.g6_backward(b.inp(d_out, 'd_out'), inputs=E.Engine.G6_INPUTS)
            out_r = ref.g6_forward(mel, onehot, d3, training=True)
            dx_r = ref.g6_backward(d_out, inputs=E.Engine.G6_INPUTS)
        ref.check()
        assert torch.equal(out, out_r)
        for a, r in zip(dx, dx_r):
            assert torch.equal(a, r) and bool(a.any())
        assert torch.equal(b.eng.grads, ref.grads)
        b.check((name, 'input gradients'))
    finally:
        E.tune('deterministic', 0)


# --------------------------------------------------------------------------------------------- 6: 16-bit mode
@pytest.mark.parametrize('name', ['H_narrow', 'H_wide'])
def test_bf16_mode_against_fp32_oracle(E, name):
    B, T = 3, 64
    bseed, dseed = train_seeds(name, B)
    c = HCase(E, name, B, T, T // 2, bseed + 1000, dseed + 1000, precision='bf16')
    r = c.step(0, kink_bound=5e-2)            # as tests/test_gpu_configs.py: a bf16-product GroupNorm output may sit 1e-2 from the oracle's
    el = abs(r['loss_gpu'] - r['loss_cpu']) / abs(r['loss_cpu'])
    eo = rel(r['out_gpu'], r['out_cpu'])
    eg = {n: rel(r['grads_gpu'][n], g) for n, g in r['grads_cpu'].items()}
    worst = max(eg.items(), key=lambda x: x[1])
    med = float(np.median(list(eg.values())))
    print(f'[bf16 {name} {B}x{T}] loss {el:.2e}  output {eo:.2e}  gradients: worst {worst[0]} {worst[1]:.2e}, median {med:.2e}')
    assert el < BF16_BOUNDS['loss'] and eo < BF16_BOUNDS['out']
    assert worst[1] < BF16_BOUNDS['grad'] and med < BF16_BOUNDS['grad_median']
    assert worst[1] > 1e-4                    # really the reduced-precision arithmetic
    assert c.eng.scratch_fallbacks() == 0


# --------------------------------------------------------------------------------------------- 7: default (non-deterministic) mode
def test_default_mode_two_fresh_engines_agree(E):
    """The train step of H_wide twice, on two fresh engines in the default mode (split-K sums meet in arrival order): losses, every gradient
    tensor and the stepped parameters agree at compare_step's engine-against-engine bar."""
    name, B, T = 'H_wide', 3, 64
    hp = hparams_of(name, T)
    mel, f0, emb, lens = batch_of(hp, 91, B, T, T // 2)
    batch = (mel, f0, emb, lens, stack_draws(draws_of(hp, 191, B, 4)))
    a, b = plain(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
    la, lb = g3_step(a, batch), g3_step(b, batch)
    a.check()
    b.check()
    assert bool(a.grads.any())
    compare_step(name, SimpleNamespace(eng=a), b, la, lb, 1)
