"""The differentiable decode on the GPU (pytest -m gpu): ss_*_decode_train / ss_*_decode_backward / ss_adam_step_decoder /
ss_g3_decode_train_step, the kernel behind the code gradients alone (ss_op_dec_in_codes_grad), and the Python surface on top
(Generator_3.decode_grad / Generator_6.decode_grad, convert.adapt_speaker).

The reference is tests/decode_grad_ref.py, float64 torch autograd over the oracle's decoder (checked against finite differences and on
wrong variants by tests/test_decode_grad_ref_selftest.py).  The bar is the project's 1e-4 relative max-norm per tensor
(tests/test_gpu_parity.py).  Codes and speaker rows are N(0, 0.25): the scale of real codes, stated in decode_grad_ref's docstring and
printed from the engine's own encode by test_consistency_with_the_full_path.

Shapes (B x T): 2 x 8 (one code row per utterance: the block is the whole row), 3 x 16 (two blocks), 17 x 16 (two batch tiles), 2 x 64,
2 x 256 (the largest frame count), both generators; W_mix (tests/test_capi_bottleneck_widths.py: factors 4 / 16 / 8, widths 12 / 3 / 24,
the slab form of the decoder input, where the kernel really sums) at 3 x 32 and H_narrow (tests/test_capi_hparams.py: dim_freq 36, 81
speaker columns) at 3 x 16.

Measured on MI355X (fp32 mode, worst over the shapes above; the tests print every figure): see DESIGN.md section 8, "Differentiable
decode"."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import adam_ref as A, codes_ref, decode_grad_ref as R, guarded as G
from tests.test_capi_bottleneck_widths import hparams_of as widths_hparams
from tests.test_capi_hparams import hparams_of as hparams_hparams
from tests.test_gpu_configs import BF16_BOUNDS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MAXB, MAXT = 17, 256
CONFIGS = {'default': W.default_hparams(max_len_pad=64), 'W_mix': widths_hparams('W_mix', 64), 'H_narrow': hparams_hparams('H_narrow', 64)}
SHAPES = [(2, 8), (3, 16), (17, 16), (2, 64), (2, 256)]
CASES = [(k, 'default', B, T) for k in ('G3', 'G6') for B, T in SHAPES] + [('G3', 'W_mix', 3, 32), ('G3', 'H_narrow', 3, 16)]
IDS = [f'{k.lower()}_{c}_{B}x{T}' for k, c, B, T in CASES]
WSEED = {'G3': codes_ref.SEED_G3, 'G6': codes_ref.SEED_G6}


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


_ENGINES = {}


def get_engine(E, kind, cfg='default', precision='f32'):
    """one engine per generator, configuration and precision for the module, at 17 x 256; reset() before every use"""
    key = (kind, cfg, precision)
    if key not in _ENGINES:
        eng = E.Engine(kind, CONFIGS[cfg], MAXB, MAXT)
        eng.set_precision(precision)
        _ENGINES[key] = eng
    return reset(_ENGINES[key], kind, cfg)


def reset(eng, kind, cfg='default'):
    eng.load_weights(W.make_weights(kind, CONFIGS[cfg], WSEED[kind]))
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
    eng.zero_grads()
    return eng


@functools.lru_cache(maxsize=None)
def reference(kind, cfg, B, T, seed=5):
    """(codes, emb, d_out, float64 reference) of a case, computed once and shared"""
    hp = CONFIGS[cfg]
    codes, emb, d_out = R.make_inputs(kind, hp, B, T, seed)
    return codes, emb, d_out, R.decode_grad(kind, R.p64(kind, hp, WSEED[kind]), hp, codes, emb, d_out)


def run_decode(eng, kind, codes, emb, d_out, accumulate=False):
    """decode_train + decode_backward with every gradient asked for -> (out, [code gradients], dc_trg or None)"""
    if kind == 'G3':
        out = eng.g3_decode_train(*codes, emb)
        *dc, de = eng.g3_decode_backward(d_out, want=('x', 'r', 'f0', 'c_trg'), accumulate=accumulate)
        return out, dc, de
    out = eng.g6_decode_train(*codes)
    return out, list(eng.g6_decode_backward(d_out, want=('r', 'f0'), accumulate=accumulate)), None


def dec_names(eng):
    return [n for n, off, _ in eng.table if off >= eng.grad_split]


# ------------------------------------------------------------------------------------------------ parity with the float64 restatement
@pytest.mark.parametrize('kind,cfg,B,T', CASES, ids=IDS)
def test_parity_with_float64(E, kind, cfg, B, T):
    eng = get_engine(E, kind, cfg)
    codes, emb, d_out, ref = reference(kind, cfg, B, T)
    out, dcodes, dc = run_decode(eng, kind, codes, emb, d_out)
    eng.check()
    fig = {'out': R.rel(out, ref['out'])}
    gv = eng.grad_views()
    names = dec_names(eng)
    assert set(names) == set(ref['grads']) and all(n.startswith('decoder.') for n in names)
    for n in names:
        fig[n] = R.rel(gv[n], ref['grads'][n])
    for (cn, _, _), g, r in zip(R.factors(kind, CONFIGS[cfg]), dcodes, ref['d_codes']):
        assert tuple(g.shape) == tuple(r.shape)
        fig['d_codes_' + cn] = R.rel(g, r)
    if kind == 'G3':
        assert tuple(dc.shape) == (B, CONFIGS[cfg].dim_spk_emb)
        fig['dc_trg'] = R.rel(dc, ref['dc_trg'])
    worst = max(fig.items(), key=lambda x: x[1])
    grads = [fig[n] for n in names]
    print(f'[{kind} {cfg} {B}x{T}] out {fig["out"]:.2e}  decoder/head gradients worst {max(grads):.2e} median {float(np.median(grads)):.2e}  '
          + '  '.join(f'{k} {v:.2e}' for k, v in fig.items() if k[:2] in ('d_', 'dc')) + f'  (worst: {worst[0]})')
    for k, v in fig.items():
        assert v < R.BAR, (k, v)
    # arena rule: a non-accumulating backward leaves exact zeros below ss_grad_split
    assert int(torch.count_nonzero(eng.grads[:eng.grad_split])) == 0
    assert eng.grad_accum_count == 1


def test_code_gradients_have_the_same_bits_on_every_run(E):
    """the kernel adds in one fixed order without atomics: from the same decoder-input gradient it gives the same bits (deterministic mode
    pins the GEMMs in front of it as well, so whole calls can be compared)"""
    kind, cfg, B, T = 'G3', 'W_mix', 3, 32
    E.tune('deterministic', 1)
    try:
        eng = get_engine(E, kind, cfg)
        codes, emb, d_out, _ = reference(kind, cfg, B, T)
        _, a, da = run_decode(eng, kind, codes, emb, d_out)
        _, b, db = run_decode(eng, kind, codes, emb, d_out)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(da, db)
    finally:
        E.tune('deterministic', 0)


def test_null_outputs_give_parameter_gradients_only(E):
    kind, cfg, B, T = 'G3', 'default', 3, 16
    eng = get_engine(E, kind, cfg)
    codes, emb, d_out, ref = reference(kind, cfg, B, T)
    eng.g3_decode_train(*codes, emb)
    assert eng.g3_decode_backward(d_out) == (None, None, None, None)
    gv = eng.grad_views()
    for n in dec_names(eng):
        assert R.rel(gv[n], ref['grads'][n]) < R.BAR, n
    eng.g3_decode_train(*codes, emb)
    dx, dr, df, dc = eng.g3_decode_backward(d_out, want=('r',))
    assert dx is None and df is None and dc is None and R.rel(dr, ref['d_codes'][1]) < R.BAR


# ------------------------------------------------------------------------------------------------ no encoder launch
def test_no_encoder_launch_in_either_call(E):
    eng = get_engine(E, 'G3')
    codes, emb, d_out, _ = reference('G3', 'default', 3, 16)
    eng.g3_decode_train(*codes, emb)                      # (the geometry's memset is out of the way)
    eng.profile('timeline')
    try:
        run_decode(eng, 'G3', codes, emb, d_out)
        eng.g3_decode_train_step(*codes, emb, torch.zeros(3, 16, 80), no_adam=True)
        torch.cuda.synchronize()
        names = [t[0] for t in eng.profile_timeline()]
    finally:
        eng.profile(False)
    print('[profile] classes launched:', {n: names.count(n) for n in sorted(set(names))})
    for banned in ('conv_fwd', 'conv_dw', 'conv_dx', 'gn', 'enc_rec', 'enc_lstm', 'wgrad'):
        assert banned not in names, banned
    for needed in ('rec_fwd', 'rec_bwd', 'head', 'dec_dw'):
        assert needed in names, needed


# ------------------------------------------------------------------------------------------------ consistency with the full path
def test_consistency_with_the_full_path(E):
    """codes from ss_g3_encode(x), d_out from the same MSE: decode_train + decode_backward against an eval-mode ss_g3_forward +
    ss_g3_backward_inputs on x -- the decoder-range gradients and dc_trg, at the 1e-4 bar; whether they are in fact bit-equal is printed."""
    B, T = 4, 64
    eng = get_engine(E, 'G3')
    hp = CONFIGS['default']
    mel, onehot, emb = codes_ref.inputs(codes_ref.SEED_IN, B, T, hp)
    x_f0 = torch.cat((mel, onehot), -1)
    codes = eng.g3_encode(x_f0, mel)
    print('[scale] standard deviation of the codes of ss_g3_encode on the test weights: '
          + ', '.join(f'{n} {float(c.std()):.3f}' for n, c in zip(('content', 'rhythm', 'pitch'), codes)) + f'  (test inputs: N(0, {R.SCALE}))')
    out_full = eng.g3_forward(x_f0, mel, emb).clone()
    d_out = (2.0 / out_full.numel()) * (out_full - mel.to(DEV))
    _, _, dc_full = eng.g3_backward(d_out, inputs=('c_trg',))
    g_full = eng.grads.clone()
    out_dec = eng.g3_decode_train(*codes, emb)
    assert torch.equal(out_dec, out_full)                 # decode(encode(x)) is the forward, bit for bit
    _, _, _, dc_dec = eng.g3_decode_backward(d_out, want=('c_trg',))
    lo = eng.grad_split
    full, dec = eng.views(g_full), eng.grad_views()
    worst = 0.0
    for n in dec_names(eng):
        worst = max(worst, R.rel(dec[n], full[n]))
        assert R.rel(dec[n], full[n]) < R.BAR, n
    e_dc = R.rel(dc_dec, dc_full)
    print(f'[full path] decoder-range gradients worst {worst:.2e}, dc_trg {e_dc:.2e}; bit-equal: gradients '
          f'{bool(torch.equal(eng.grads[lo:], g_full[lo:]))}, dc_trg {bool(torch.equal(dc_dec, dc_full))}')
    assert e_dc < R.BAR
    assert int(torch.count_nonzero(eng.grads[:lo])) == 0 and int(torch.count_nonzero(g_full[:lo])) > 0


# ------------------------------------------------------------------------------------------------ arena rules
def test_accumulating_backward_adds_to_a_full_step(E):
    from tests.test_gpu_engine_containment import g3_batch
    B, T = 3, 64
    eng = get_engine(E, 'G3')
    codes, emb, d_out, _ = reference('G3', 'default', B, T)
    run_decode(eng, 'G3', codes, emb, d_out)
    g_dec = eng.grads.clone()
    mel, f0, spk, lens, draws = g3_batch(41, B, T)
    eng.g3_train_step(mel, f0, spk, lens, draws, no_adam=True)
    g_full = eng.grads.clone()
    assert eng.grad_accum_count == 1
    run_decode(eng, 'G3', codes, emb, d_out, accumulate=True)
    assert eng.grad_accum_count == 2
    lo = eng.grad_split
    assert torch.equal(eng.grads[:lo], g_full[:lo])       # the encoder range is not touched
    want, got = eng.views(g_full.double() + g_dec.double()), eng.grad_views()
    for n in dec_names(eng):                              # per element, against the per-tensor scale
        err = float((got[n].double() - want[n]).abs().max() / want[n].abs().max())
        assert err < R.BAR, (n, err)
    assert not torch.equal(eng.grads[lo:], g_full[lo:])


# ------------------------------------------------------------------------------------------------ ss_adam_step_decoder
@pytest.mark.parametrize('kind', ['G3', 'G6'])
@pytest.mark.parametrize('clip', [False, True], ids=['noclip', 'clip_inf'])
def test_adam_step_decoder(E, kind, clip):
    """adam_ref's case default_t7_gs1 (one of the cases its bars were measured on): controlled gradients and restored moments over the
    whole arena, so an update of the encoder range would move every element there.  The decoder range against float64 at adam_ref's bars
    (step 8), the encoder range of the parameters and both moments bit-unchanged, and the following full ss_adam_step at step 9.
    clip_inf: the clipping route (max_norm = inf: coefficient 1, the same update)."""
    from tests.test_gpu_optimizer import fill
    eng = get_engine(E, kind)
    (_, hp, restored, gs), n, dev = A.CASES[-1], eng.params.numel(), eng.device
    assert A.CASES[-1][0] == 'default_t7_gs1'
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    for _, off, shape in eng.table:
        mask[off:off + int(np.prod(shape))] = True
    cls, lo = A.classes(n, dev), eng.grad_split
    fill(eng, eng.params, A.make_params(n, dev))
    m0, v0 = A.make_moments(n, restored, hp['eps'], gs, dev)
    fill(eng, eng.adam_m, m0)
    fill(eng, eng.adam_v, v0)
    eng.set_adam(hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], restored)
    g1 = A.make_grad(n, 1, hp['eps'], dev)
    if clip:
        g1 = torch.where(cls == 3, torch.zeros_like(g1), g1)      # without the 'large' class, whose squares overflow fp32's norm
        eng.set_grad_clip(float('inf'))
    try:
        fill(eng, eng.grads, g1)
        before = (eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone())
        eng.adam_step_decoder(gs)
        got = (eng.params, eng.adam_m, eng.adam_v)
        for a, b in zip(got, before):
            assert A.bits_equal(a[:lo], b[:lo]), 'the encoder range changed'
        want = A.adam_f64(before[0], eng.grads, before[1], before[2], t=restored + 1, grad_scale=gs, **hp)
        rep = A.compare([x[lo:] for x in got], [x[lo:] for x in want], [x[lo:] for x in before], cls[lo:], mask[lo:])
        assert not A.excess(rep), (A.excess(rep), rep['worst'])
        print(f'[{kind} adam_step_decoder{" clip" if clip else ""}] decoder range against float64:\n{A.table(rep)}')
        assert int((got[0][lo:] != before[0][lo:]).sum()) > 0.5 * int(mask[lo:].sum())
        # the following full step applies step restored + 2
        fill(eng, eng.grads, torch.where(cls == 3, torch.zeros_like(g1), A.make_grad(n, 2, hp['eps'], dev)) if clip else A.make_grad(n, 2, hp['eps'], dev))
        before = (eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone())
        eng.adam_step(gs)
        want = A.adam_f64(before[0], eng.grads, before[1], before[2], t=restored + 2, grad_scale=gs, **hp)
        rep = A.compare((eng.params, eng.adam_m, eng.adam_v), want, before, cls, mask)
        assert not A.excess(rep), ('full step after the decoder step', A.excess(rep), rep['worst'])
        eng.check()
    finally:
        if clip:
            eng.set_grad_clip(0.0)


# ------------------------------------------------------------------------------------------------ the fused step
def test_fused_step_against_float64_adam_on_the_decoder(E):
    kind, cfg, B, T = 'G3', 'default', 3, 16
    eng = get_engine(E, kind, cfg)
    hp = CONFIGS[cfg]
    codes, emb, _, ref = reference(kind, cfg, B, T)
    target = (ref['out'] + 0.1 * torch.randn(ref['out'].shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)).float()
    p0 = eng.params.clone()
    # SS_STEP_NO_ADAM: nothing moves, and the speaker gradient comes back
    loss, dc = eng.g3_decode_train_step(*codes, emb, target, no_adam=True, want_dc_trg=True)
    loss0 = float(loss)
    assert A.bits_equal(eng.params, p0) and int(torch.count_nonzero(eng.adam_m)) == 0 and int(torch.count_nonzero(eng.adam_v)) == 0
    r0 = R.decode_grad(kind, R.p64(kind, hp, WSEED[kind]), hp, codes, emb, target=target)
    assert abs(loss0 - r0['loss']) <= 1e-5 * abs(r0['loss']), (loss0, r0['loss'])
    assert R.rel(dc, r0['dc_trg']) < R.BAR
    # three steps against float64 torch Adam over the decoder + head parameters
    losses = [float(eng.g3_decode_train_step(*codes, emb, target)) for _ in range(3)]
    eng.check()
    want_l, want_p = R.train_decoder_f64(kind, R.p64(kind, hp, WSEED[kind]), hp, codes, emb, target, 3)
    pv = eng.param_views()
    fig = {n: R.rel(pv[n], want_p[n]) for n in dec_names(eng)}
    el = max(abs(a - b) / abs(b) for a, b in zip(losses, want_l))
    print(f'[fused step 3x16] loss step 0 {loss0:.6f} (oracle {r0["loss"]:.6f}); three steps: loss rel {el:.2e}, parameters worst {max(fig.values()):.2e}')
    assert abs(losses[0] - want_l[0]) <= 1e-5 * abs(want_l[0]) and el < R.BAR, (losses, want_l)
    assert max(fig.values()) < R.BAR, max(fig.items(), key=lambda x: x[1])
    lo = eng.grad_split
    assert A.bits_equal(eng.params[:lo], p0[:lo]) and not A.bits_equal(eng.params[lo:], p0[lo:])
    assert int(torch.count_nonzero(eng.adam_m[:lo])) == 0


# ------------------------------------------------------------------------------------------------ the kernel alone, on guarded slabs
HOOK_CASES = {
    # name: (B, T, [(H, freq)], ld, f)
    'slab_mixed_factors': (3, 32, [(12, 4), (3, 16), (24, 8)], 176, 0),         # W_mix's decoder input: sums of 4, 16 and 8 frames
    'slab_default': (17, 16, [(8, 8), (1, 8), (32, 8)], 164, 0),                # the default widths when layer 0 is not compact
    'slab_one_block': (2, 8, [(8, 8), (1, 8), (32, 8)], 164, 0),
    'compact_default': (3, 64, [(8, 8), (1, 8), (32, 8)], 164, 8),              # the compact form: the block sums are there, a copy
    'slab_g6': (2, 256, [(1, 8), (32, 8)], 72, 0),
}


@pytest.mark.parametrize('name', list(HOOK_CASES))
def test_kernel_alone_on_guarded_slabs(E, name):
    """ss_op_dec_in_codes_grad: the input's halo rows, the columns of no code and the memory around it are NaN, the outputs are guarded;
    every element against the float64 sum within the rounding of a freq-term float32 sum in the kernel's order (sum_order_budget: zero
    for the compact form, where the result must be the input's bits)."""
    B, T, codes, ld, f = HOOK_CASES[name]
    g = torch.Generator().manual_seed(21)
    rows = T // f if f else T + 4
    width = sum(2 * H for H, _ in codes)
    data = torch.full((B, rows, width + 3), float('nan'))                        # three columns of no code behind the codes'
    live = slice(0, rows) if f else slice(2, 2 + T)
    data[:, live, :width] = torch.randn(B, T // f if f else T, width, generator=g)
    d_in = G.inp(data, DEV, ld=ld, name='d_in')
    outs, args, col = [], [], 0
    for i, (H, fr) in enumerate(codes):
        o = G.out((B, T // fr, 2 * H), DEV, name=f'd_code{i}', offset=64 + 4 * i)
        outs.append(o)
        args.append((o.t, H, fr, col))
        col += 2 * H
    E.dec_in_codes_grad(args, d_in.t, T, f)
    torch.cuda.synchronize()
    d_in.check()
    G.check_all(outs)
    col = 0
    x = data[:, live, :width].double()
    for o, (H, fr) in zip(outs, codes):
        k = 1 if f else fr
        blocks = x[:, :, col:col + 2 * H].reshape(B, -1, k, 2 * H)
        col += 2 * H
        want, budget = blocks.sum(2), R.sum_order_budget(blocks.abs().sum(2), k)
        err = (o.t.double().cpu() - want).abs()
        over = err > budget
        assert not bool(over.any()), (name, int(over.sum()), float((err - budget).max()))
        if k == 1:
            assert torch.equal(o.t.cpu(), blocks[:, :, 0].float())
        print(f'[{name}] code {2 * H} wide, {k}-term sums: worst error / budget {float((err / budget.clamp(min=1e-300)).max()) if k > 1 else 0.0:.2f}')


# ------------------------------------------------------------------------------------------------ state and history
def test_mixed_up_calls_are_refused_and_the_engine_works_afterwards(E):
    eng = get_engine(E, 'G3')
    B, T = 3, 16
    codes, emb, d_out, ref = reference('G3', 'default', B, T)
    hp = CONFIGS['default']
    mel, onehot, spk = codes_ref.inputs(5, B, T, hp)
    eng.g3_decode_train(*codes, emb)
    for call in (lambda: eng.g3_backward(d_out), lambda: eng.lib.ss_g3_backward_inputs(eng.h, None, None, None, None, None),
                 lambda: eng.train_finish()):
        with pytest.raises(RuntimeError, match='was a decode'):
            r = call()
            if isinstance(r, int) and r != 0:
                raise RuntimeError(eng.lib.ss_last_error().decode())
    _, _, _, dc = eng.g3_decode_backward(d_out, want=('c_trg',))      # ... and the decode's own backward still follows
    assert R.rel(dc, ref['dc_trg']) < R.BAR
    eng.g3_forward(torch.cat((mel, onehot), -1), mel, spk)
    with pytest.raises(RuntimeError, match='full forward'):
        eng.g3_decode_backward(d_out)
    eng.g3_decode(*codes, emb)
    with pytest.raises(RuntimeError, match='without a preceding'):
        eng.g3_decode_backward(d_out)
    fresh = E.Engine('G3', hp, 2, 64)
    with pytest.raises(RuntimeError, match='without a preceding'):
        fresh.g3_decode_backward(torch.zeros(2, 16, 80))
    # shapes outside the rules, flags outside the set: refused by name, nothing enqueued
    big = [torch.zeros(1, 512 // f, w) for _, f, w in R.factors('G3', hp)]
    with pytest.raises(RuntimeError, match='ss_g3_decode_train: T outside 1 .. max_frames'):
        eng.g3_decode_train(*big, torch.zeros(1, hp.dim_spk_emb))
    with pytest.raises(RuntimeError, match='ss_g3_decode_train: batch outside'):
        eng.g3_decode_train(*[torch.zeros(MAXB + 1, 1, w) for _, _, w in R.factors('G3', hp)], torch.zeros(MAXB + 1, hp.dim_spk_emb))
    p = codes[0].to(DEV)
    for flags in (2, 4, 16, 32):
        assert eng.lib.ss_g3_decode_train_step(eng.h, p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), B, T, 1.0, flags,
                                               p.data_ptr(), None, None) != 0
        assert 'ss_g3_decode_train_step: flags' in eng.lib.ss_last_error().decode()
    eng.g3_decode_train(*codes, emb)
    assert eng.lib.ss_g3_decode_backward(eng.h, p.data_ptr(), None, None, None, None, 1, None) != 0
    assert 'ss_g3_decode_backward: flags' in eng.lib.ss_last_error().decode()
    assert eng.lib.ss_g3_decode_backward(eng.h, None, None, None, None, None, 0, None) != 0
    assert 'null pointer' in eng.lib.ss_last_error().decode()
    # the engine works afterwards
    out, dcodes, dc = run_decode(eng, 'G3', codes, emb, d_out)
    eng.check()
    assert R.rel(out, ref['out']) < R.BAR and R.rel(dcodes[0], ref['d_codes'][0]) < R.BAR
    e6 = get_engine(E, 'G6')
    c6, _, d6, r6 = reference('G6', 'default', B, T)
    e6.g6_decode_train(*c6)
    with pytest.raises(RuntimeError, match='was a decode'):
        e6.g6_backward(d6)
    dr, df = e6.g6_decode_backward(d6, want=('r', 'f0'))
    assert R.rel(dr, r6['d_codes'][0]) < R.BAR and R.rel(df, r6['d_codes'][1]) < R.BAR


def test_a_train_step_after_decode_steps_has_a_fresh_engines_bits(E):
    """in the manner of tests/test_gpu_same_shape_history.py: deterministic mode, engines created at exactly the shape they run, the dirty
    one reset as that file resets; the plain ss_g3_train_step afterwards gives the loss, gradient and parameter bits of a fresh engine"""
    from tests.test_gpu_engine_containment import g3_batch, g3_step, plain
    B, T = 3, 64
    hp = W.default_hparams(max_len_pad=T)
    codes, emb, d_out, _ = reference('G3', 'default', B, T)
    batch = g3_batch(77, B, T)
    E.tune('deterministic', 1)
    try:
        dirty = plain(E, 'G3', hp, B, T)
        run_decode(dirty, 'G3', codes, emb, d_out)
        dirty.g3_decode_train_step(*codes, emb, torch.zeros(B, T, hp.dim_freq))
        dirty.g3_decode_train_step(*codes, emb, torch.zeros(B, T, hp.dim_freq), no_adam=True, accumulate=True)
        dirty.g3_decode_train(*codes, emb)                # a decode left without its backward
        dirty.load_weights(W.make_weights('G3', hp, 3))
        dirty.adam_m.zero_()
        dirty.adam_v.zero_()
        dirty.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
        dirty.zero_grads()
        fresh = plain(E, 'G3', hp, B, T)
        la, lb = float(g3_step(dirty, batch)), float(g3_step(fresh, batch))
        dirty.check()
        fresh.check()
        assert la == lb and torch.equal(dirty.grads, fresh.grads) and torch.equal(dirty.params, fresh.params)
        assert dirty.scratch_fallbacks() == 0
    finally:
        E.tune('deterministic', 0)


# ------------------------------------------------------------------------------------------------ 16-bit mode
def test_bf16_mode_against_the_fp32_oracle(E):
    """one 4 x 64 run in the 16-bit mode: out and the decoder / head gradients under tests/test_gpu_configs.py's BF16_BOUNDS (out 4e-2,
    gradients worst 2e-1, median 2e-2), the code gradients and dc_trg under the same relative gradient bound"""
    kind, cfg, B, T = 'G3', 'default', 4, 64
    eng = get_engine(E, kind, cfg, 'bf16')
    codes, emb, d_out, ref = reference(kind, cfg, B, T)
    out, dcodes, dc = run_decode(eng, kind, codes, emb, d_out)
    eng.check()
    gv = eng.grad_views()
    eg = {n: R.rel(gv[n], ref['grads'][n]) for n in dec_names(eng)}
    ec = [R.rel(g, r) for g, r in zip(dcodes, ref['d_codes'])] + [R.rel(dc, ref['dc_trg'])]
    eo, worst, med = R.rel(out, ref['out']), max(eg.items(), key=lambda x: x[1]), float(np.median(list(eg.values())))
    print(f'[bf16 decode {B}x{T}] output {eo:.2e}  gradients: worst {worst[0]} {worst[1]:.2e}, median {med:.2e}  '
          f'code gradients x / r / f0 {ec[0]:.2e} / {ec[1]:.2e} / {ec[2]:.2e}  dc_trg {ec[3]:.2e}')
    assert eo < BF16_BOUNDS['out'] and worst[1] < BF16_BOUNDS['grad'] and med < BF16_BOUNDS['grad_median']
    assert max(ec) < BF16_BOUNDS['grad']
    assert int(torch.count_nonzero(eng.grads[:eng.grad_split])) == 0


# ------------------------------------------------------------------------------------------------ Python: modules and adapt_speaker
@functools.lru_cache(maxsize=None)
def module(kind):
    from speechsplit_amd import model
    hp = CONFIGS['default']
    M = (model.Generator_3 if kind == 'G3' else model.Generator_6)(hp, max_batch=4)
    M.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_weights(kind, hp, WSEED[kind]).items()}, strict=False)
    return M.to(DEV)


@pytest.mark.parametrize('want', ['c_trg', 'codes_2', 'all'])
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_module_decode_grad_under_autograd(want, mode):
    B, T = 3, 16
    M = module('G3')
    M.train(mode == 'train')
    codes, emb, d_out, ref = reference('G3', 'default', B, T)
    names = ('codes_x', 'codes_2', 'codes_f0', 'c_trg')
    ins = [t.to(DEV).clone().requires_grad_(want == 'all' or want == n) for n, t in zip(names, (*codes, emb))]
    M.zero_grad(set_to_none=True)
    out = M.decode_grad(*ins)
    assert out.requires_grad and R.rel(out, ref['out']) < R.BAR
    (out * d_out.to(DEV)).sum().backward()
    wanted = dict(zip(names, (*ref['d_codes'], ref['dc_trg'])))
    for n, t in zip(names, ins):
        if t.requires_grad:
            assert R.rel(t.grad, wanted[n]) < R.BAR, n
        else:
            assert t.grad is None, n
    for n, p in M.named_parameters():
        if n.startswith('decoder.'):
            assert R.rel(p.grad, ref['grads'][n]) < R.BAR, n
        else:
            assert p.grad is None, n                    # the encoders get no gradient from this call: None, not zeros
    # a broadcast speaker row gets the sum over the batch
    if want == 'c_trg':
        row = emb[:1].to(DEV).clone().requires_grad_()
        M.decode_grad(*[c.to(DEV) for c in codes], row).sum().backward()
        assert tuple(row.grad.shape) == (1, emb.shape[1])
    # decode keeps its refusals
    M.eval()
    with pytest.raises(RuntimeError, match='not autograd-connected'):
        M.decode(*[t.detach() for t in ins[:3]], ins[3].detach().requires_grad_())
    M.train()
    with pytest.raises(RuntimeError, match='eval-mode only'):
        M.decode(*[t.detach() for t in ins])


def test_module_decode_grad_generator_6():
    B, T = 3, 16
    M = module('G6')
    codes, _, d_out, ref = reference('G6', 'default', B, T)
    ins = [c.to(DEV).clone().requires_grad_() for c in codes]
    M.zero_grad(set_to_none=True)
    out = M.decode_grad(*ins)
    (out * d_out.to(DEV)).sum().backward()
    assert R.rel(out, ref['out']) < R.BAR
    for t, r in zip(ins, ref['d_codes']):
        assert R.rel(t.grad, r) < R.BAR
    for n, p in M.named_parameters():
        assert (R.rel(p.grad, ref['grads'][n]) < R.BAR) if n.startswith('decoder.') else p.grad is None, n


def test_adapt_speaker_on_two_demo_entries():
    from speechsplit_amd import convert, model
    z = np.load(os.path.join(GOLD, 'demo_config1.npz'))
    hp = W.default_hparams()
    G3 = model.Generator_3(hp, max_batch=2).eval()
    G3.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_weights('G3', hp, int(z['seed_g3'])).items()}, strict=False)
    G3 = G3.to(DEV)
    ent = []
    for n in range(2):
        L = int(z[f'u{n}_len'])
        ent.append([f'p{n}', z[f'u{n}_emb'], (z[f'u{n}_mel_pad'][0, :L], z[f'u{n}_f0_pad'][:L], L, f'utt{n}')])
    before = {n: p.detach().clone() for n, p in G3.named_parameters()}
    # only the row learns: every model parameter keeps its bits (the rate is the row's own: the point here is the direction)
    row, losses = convert.adapt_speaker(G3, ent, 21, lr=1e-2, train_decoder=False)
    print(f'[adapt_speaker row only] loss {losses[0]:.6f} -> {losses[20]:.6f} after 20 steps')
    assert tuple(row.shape) == (1, hp.dim_spk_emb) and len(losses) == 21 and all(np.isfinite(losses))
    assert losses[20] < losses[0]
    for n, p in G3.named_parameters():
        assert A.bits_equal(p.detach(), before[n]), n
    assert not G3.training
    # decoder and row
    row2, losses2 = convert.adapt_speaker(G3, ent, 21, lr=1e-4, train_decoder=True, emb0=row)
    print(f'[adapt_speaker decoder + row] loss {losses2[0]:.6f} -> {losses2[20]:.6f} after 20 steps')
    assert losses2[20] < losses2[0]
    changed = {n for n, p in G3.named_parameters() if not A.bits_equal(p.detach(), before[n])}
    assert changed and all(n.startswith('decoder.') for n in changed)
    G3._eng.check()
