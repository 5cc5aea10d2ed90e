"""Gradients with respect to the model INPUTS (ss_g3_backward_inputs / ss_g6_backward_inputs and the autograd path of
Generator_3 / Generator_6) against the oracle run in float64 with its inputs set to require grad.  Runs on the GPU box: pytest -m gpu.

Bar: relative max-norm <= 1e-4 per tensor (the suite's).  Input gradients sit below every ReLU of the trunk, and a GroupNorm output
within rounding of 0 takes either branch in two correct implementations (kink note of test_gpu_parity.py; at these sizes such an
element exists in most cases), so the oracle is handed the branch the engine took (ss_debug_relu_mask -> ref_model.MASK) and the
test checks that the override only ever acted at the kink, as tests/test_gpu_configs.py does."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import ref_model, weights as W
from oracle.gen_fixtures import draws_for

pytestmark = pytest.mark.gpu
TOL = 1e-4
BF16_GRAD = 2e-2            # tests/test_gpu_configs.py BF16_BOUNDS['grad_median']: a dense, non-cancelling gradient tensor


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def p64(w):
    return {k: torch.from_numpy(np.array(v, dtype=np.float64)) for k, v in w.items()}


def stack(draws):
    return np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])


def g3_inputs(seed, B, T):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, 80, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 257, (B, T), generator=g), 257).float()
    c_trg = torch.nn.functional.one_hot(torch.randint(0, 82, (B,), generator=g), 82).float()
    return torch.cat((mel, onehot), -1), mel, c_trg


def train_draws(seed, B, T):
    """The three encoder draws of a training forward.  Above 192 frames the stretching ones of tests/test_gpu_frame_range.py, under which
    every row of the resampled slabs is live (asserted here, on the CPU); the reference's own below."""
    if T <= 192:
        return draws_for(seed, B, 3)
    from tests.test_gpu_frame_range import all_rows_live, stretch_draws
    draws = stretch_draws(seed, B, 3)
    for d in draws:
        all_rows_live(d, np.full(B, T), T)
    return draws


def g3_case(w, hp, B, T, training, seed):
    x_f0, x_org, c_trg = g3_inputs(seed, B, T)
    return x_f0, x_org, c_trg, train_draws(seed + 500, B, T) if training else None


def g6_case(w, hp, B, T, training, seed):
    _, x_org, _ = g3_inputs(seed, B, T)
    g = torch.Generator().manual_seed(seed + 1000)
    f0_trg = torch.nn.functional.one_hot(torch.randint(0, 257, (B, T), generator=g), 257).float()
    return x_org, f0_trg, train_draws(seed + 500, B, T) if training else None


def masks_of(eng, B, T):
    """The ReLU branches the engine took in its last forward (read before the backward)."""
    return {k: v.cpu() for k, v in eng.relu_masks(B, T).items()}


@contextlib.contextmanager
def engine_branches(masks, kink_bound=1e-4):
    """The oracle takes the engine's ReLU branches; on exit: it only had to where its own pre-activation was within kink_bound of 0."""
    ref_model.MASK, ref_model.MASK_STATS = masks, {}
    try:
        yield
        stats = ref_model.MASK_STATS
    finally:
        ref_model.MASK, ref_model.MASK_STATS = None, None
    assert set(stats) == set(masks), (sorted(stats), sorted(masks))
    for k, (n, zmax) in stats.items():
        assert zmax < kink_bound, (k, n, zmax)


def oracle_grads(kind, w, hp, inputs, draws, training, wout, masks, kink_bound=1e-4):
    """Input gradients of sum(G(inputs) * wout) in float64, on the engine's ReLU branches."""
    P = p64(w)
    xs = [x.detach().double().requires_grad_() for x in inputs]
    fn = ref_model.generator_3 if kind == 'G3' else ref_model.generator_6
    with engine_branches(masks, kink_bound):
        out = fn(P, hp, *xs, draws, training)
    (out * wout.double()).sum().backward()
    return [x.grad for x in xs]


_MODS = {}


def module(kind, T, w):
    """One Generator module per (kind, T) for the whole file (each owns an engine); weights reloaded per test."""
    from speechsplit_amd import model
    hp = W.default_hparams(max_len_pad=T, batch_size=4)
    key = (kind, T)
    if key not in _MODS:
        _MODS[key] = (model.Generator_3 if kind == 'G3' else model.Generator_6)(hp).to('cuda:0')
    G = _MODS[key]
    enc = 'encoder_1' if kind == 'G3' else 'encoder_3'
    G.load_state_dict({**{k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, enc + '.len_org': torch.tensor(T)})
    G.zero_grad(set_to_none=True)
    return G, hp


def cuda_leaf(x):
    return x.cuda().requires_grad_()


# --------------------------------------------------------------------------------------------- 1, 2: Generator_3 module
@pytest.mark.parametrize('B,T,training', [(2, 128, False), (3, 192, False), (2, 128, True), (2, 256, True), (2, 200, True)])
def test_g3_module_input_grads(B, T, training):
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G3', hp, 7)
    x_f0, x_org, c_trg, draws = g3_case(w, hp, B, T, training, 11 + B)
    G, _ = module('G3', T, w)
    G.train(training)
    wout = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(5))
    xs = [cuda_leaf(x) for x in (x_f0, x_org, c_trg)]
    out = G(*xs, draws=stack(draws) if training else None)
    masks = masks_of(G._eng, B, T)
    (out * wout.cuda()).sum().backward()
    ref = oracle_grads('G3', w, hp, (x_f0, x_org, c_trg), draws, training, wout, masks)
    for name, x, r in zip(('x_f0', 'x_org', 'c_trg'), xs, ref):
        assert x.grad is not None, name
        assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.device == x.device, name
        assert rel(x.grad, r) < TOL, (name, rel(x.grad, r))
    # the two stacks' columns of x_f0 separately (content 0..79, pitch 80..336)
    assert rel(xs[0].grad[..., :80], ref[0][..., :80]) < TOL
    assert rel(xs[0].grad[..., 80:], ref[0][..., 80:]) < TOL


def test_g3_module_only_requested_inputs_and_dtype():
    """Only x_org requires grad (float64 input): the others stay None, the gradient comes back as float64."""
    B, T = 2, 128
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G3', hp, 7)
    x_f0, x_org, c_trg, _ = g3_case(w, hp, B, T, False, 13)
    G, _ = module('G3', T, w)
    G.eval()
    wout = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(5))
    xo = x_org.double().cuda().requires_grad_()
    xf = x_f0.cuda()
    out = G(xf, xo, c_trg.cuda())
    masks = masks_of(G._eng, B, T)
    (out * wout.cuda()).sum().backward()
    assert xo.grad.dtype == torch.float64 and xf.grad is None
    ref = oracle_grads('G3', w, hp, (x_f0, x_org, c_trg), None, False, wout, masks)
    assert rel(xo.grad, ref[1]) < TOL


# --------------------------------------------------------------------------------------------- 3: Generator_6 module
@pytest.mark.parametrize('training,T', [(False, 128), (True, 128), (True, 256)], ids=['False', 'True', 'True-256'])
def test_g6_module_input_grads(training, T):
    B = 2
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G6', hp, 8)
    x_org, f0_trg, draws = g6_case(w, hp, B, T, training, 21)
    G, _ = module('G6', T, w)
    G.train(training)
    wout = torch.randn(B, T, 257, generator=torch.Generator().manual_seed(6))
    xs = [cuda_leaf(x) for x in (x_org, f0_trg)]
    out = G(*xs, draws=stack(draws) if training else None)
    masks = masks_of(G._eng, B, T)
    (out * wout.cuda()).sum().backward()
    ref = oracle_grads('G6', w, hp, (x_org, f0_trg), draws, training, wout, masks)
    for name, x, r in zip(('x_org', 'f0_trg'), xs, ref):
        assert x.grad is not None, name
        assert rel(x.grad, r) < TOL, (name, rel(x.grad, r))


# --------------------------------------------------------------------------------------------- 4: learned speaker table
def test_learned_speaker_embedding_trains():
    B, T, n_spk = 3, 128, 5
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G3', hp, 9)
    x_f0, x_org, _, _ = g3_case(w, hp, B, T, False, 31)
    ids = torch.tensor([3, 0, 3])
    table0 = torch.randn(n_spk, 82, generator=torch.Generator().manual_seed(2)) * 0.1
    target = torch.rand(B, T, 80, generator=torch.Generator().manual_seed(4))
    G, _ = module('G3', T, w)
    G.eval()
    emb = torch.nn.Embedding(n_spk, 82).cuda()
    with torch.no_grad():
        emb.weight.copy_(table0)
    # the oracle: the same in float64
    P = p64(w)
    ref_tab = table0.double().clone().requires_grad_()
    opt = opt_ref = None
    for step in range(2):
        out = G(x_f0.cuda(), x_org.cuda(), emb(ids.cuda()))
        masks = masks_of(G._eng, B, T)
        emb.weight.grad = None
        torch.nn.functional.mse_loss(out, target.cuda()).backward()
        ref_tab.grad = None
        with engine_branches(masks):
            ro = ref_model.generator_3(P, hp, x_f0.double(), x_org.double(), ref_tab[ids], None, False)
        torch.nn.functional.mse_loss(ro, target.double()).backward()
        if step == 0:
            assert emb.weight.grad is not None
            assert rel(emb.weight.grad, ref_tab.grad) < TOL, rel(emb.weight.grad, ref_tab.grad)
            assert float(emb.weight.grad[[1, 2, 4]].abs().max()) == 0.0      # speakers not in the batch
            eps = 0.1 * float(ref_tab.grad.abs().max())      # Adam's update smooth in the gradient: no sign flips of near-zero elements
            opt = torch.optim.Adam(emb.parameters(), lr=1e-3, eps=eps)
            opt_ref = torch.optim.Adam([ref_tab], lr=1e-3, eps=eps)
        opt.step()
        opt_ref.step()
    moved = emb.weight.detach().cpu().double() - table0.double()
    moved_ref = ref_tab.detach() - table0.double()
    assert float(moved_ref.abs().max()) > 1e-4
    assert rel(moved, moved_ref) < 1e-3, rel(moved, moved_ref)


# --------------------------------------------------------------------------------------------- 5: chained behind InterpLnr
def test_chain_through_interp_module():
    from speechsplit_amd import model
    B, T = 2, 128
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G3', hp, 7)
    G, _ = module('G3', T, w)
    G.eval()
    interp = model.InterpLnr(hp).train()
    lens = torch.tensor([128, 112])
    _, mel, c_trg = g3_inputs(41, B, T)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 257, (B, T), generator=torch.Generator().manual_seed(42)), 257).float()
    draw = draws_for(43, B, 1)[0]
    wout = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(5))
    m = cuda_leaf(mel)
    y = interp(torch.cat((m, onehot.cuda()), -1), lens, draws=draw)
    out = G(y, m, c_trg.cuda())
    masks = masks_of(G._eng, B, T)
    (out * wout.cuda()).sum().backward()
    m64 = mel.double().requires_grad_()
    xi64 = ref_model.interp(torch.cat((m64, onehot.double()), -1), lens.numpy(), draw, hp)
    with engine_branches(masks):
        ro = ref_model.generator_3(p64(w), hp, xi64, m64, c_trg.double())
    (ro * wout.double()).sum().backward()
    assert m.grad is not None
    assert rel(m.grad, m64.grad) < TOL, rel(m.grad, m64.grad)


# --------------------------------------------------------------------------------------------- 6: broadcast speaker row
def test_broadcast_speaker_row_gets_the_batch_sum():
    B, T = 3, 128
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G3', hp, 7)
    x_f0, x_org, c_all, _ = g3_case(w, hp, B, T, False, 51)
    c1 = c_all[:1]
    G, _ = module('G3', T, w)
    G.eval()
    wout = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(5))
    c = cuda_leaf(c1)
    out = G(x_f0.cuda(), x_org.cuda(), c)
    masks = masks_of(G._eng, B, T)
    (out * wout.cuda()).sum().backward()
    assert c.grad.shape == (1, 82)
    rows = c1.expand(B, -1).clone().cuda().requires_grad_()
    (G(x_f0.cuda(), x_org.cuda(), rows) * wout.cuda()).sum().backward()
    assert rel(c.grad, rows.grad.sum(0, keepdim=True)) < 1e-5
    c64 = c1.double().requires_grad_()
    with engine_branches(masks):
        out = ref_model.generator_3(p64(w), hp, x_f0.double(), x_org.double(), c64.expand(B, -1), None, False)
    (out * wout.double()).sum().backward()
    assert rel(c.grad, c64.grad) < TOL, rel(c.grad, c64.grad)


# --------------------------------------------------------------------------------------------- 7 - 9: engine level
_ENG = {}


def engine(kind, T, precision='f32', B=4):
    from speechsplit_amd.engine import Engine
    key = (kind, T, precision)
    if key not in _ENG:
        _ENG[key] = Engine(kind, W.default_hparams(max_len_pad=T), B, T)
        _ENG[key].set_precision(precision)
    return _ENG[key]


@pytest.mark.parametrize('kind,training', [('G3', False), ('G3', True), ('G6', True)])
def test_parameter_gradients_unchanged(kind, training):
    B, T = 4, 128
    hp = W.default_hparams(max_len_pad=T)
    eng = engine(kind, T)
    eng.load_weights(W.make_weights(kind, hp, 3))
    x_f0, x_org, c_trg = g3_inputs(61, B, T)
    d = stack(draws_for(62, B, 3)) if training else None
    d_out = torch.randn(B, T, 80 if kind == 'G3' else 257, generator=torch.Generator().manual_seed(63)).cuda()

    def run(inputs):
        if kind == 'G3':
            eng.g3_forward(x_f0, x_org, c_trg, d, training=training)
            r = eng.g3_backward(d_out, inputs=inputs)
        else:
            eng.g6_forward(x_org, x_f0[..., 80:], d, training=training)
            r = eng.g6_backward(d_out, inputs=inputs)
        torch.cuda.synchronize()
        return r, eng.grads.clone()

    r0, ref = run(())
    assert r0 is None
    names = eng.G3_INPUTS if kind == 'G3' else eng.G6_INPUTS
    r1, got = run(names)
    assert all(t is not None and bool(torch.isfinite(t).all()) for t in r1)
    assert rel(got, ref) < 1e-5, rel(got, ref)
    assert eng.scratch_fallbacks() == 0


def test_speaker_gradient_both_decoder_forms_and_deterministic():
    from speechsplit_amd.engine import tune
    B, T = 4, 128
    hp = W.default_hparams(max_len_pad=T)
    eng = engine('G3', T)
    eng.load_weights(W.make_weights('G3', hp, 3))
    x_f0, x_org, c_trg = g3_inputs(71, B, T)
    d_out = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(72)).cuda()

    def dc():
        eng.g3_forward(x_f0, x_org, c_trg)
        return eng.g3_backward(d_out, inputs=('c_trg',))[2].clone()

    try:
        tune('compact0', 0)
        full = dc()
        tune('compact0', 1)
        compact = dc()
        # bit-identical repeats: the speaker kernel's sums have a fixed order; what feeds it (split-K input gradients of the decoder
        # layers above) is bit-reproducible in the deterministic mode
        tune('deterministic', 1)
        once, again = dc(), dc()
    finally:
        tune('compact0', 1)
        tune('deterministic', 0)
    assert rel(full, compact) < 1e-5, rel(full, compact)
    assert torch.equal(once, again)
    assert rel(once, compact) < 1e-5
    assert float(compact.abs().max()) > 0


@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_bf16_engine_input_grads(kind):
    B, T = 2, 128
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights(kind, hp, 7)
    eng = engine(kind, T, 'bf16')
    eng.load_weights(w)
    if kind == 'G3':
        x_f0, x_org, c_trg, _ = g3_case(w, hp, B, T, False, 81)
        inputs = (x_f0, x_org, c_trg)
        wout = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(5))
        eng.g3_forward(x_f0, x_org, c_trg)
        masks = masks_of(eng, B, T)
        got = eng.g3_backward(wout.cuda(), inputs=eng.G3_INPUTS)
    else:
        x_org, f0_trg, _ = g6_case(w, hp, B, T, False, 81)
        inputs = (x_org, f0_trg)
        wout = torch.randn(B, T, 257, generator=torch.Generator().manual_seed(6))
        eng.g6_forward(x_org, f0_trg)
        masks = masks_of(eng, B, T)
        got = eng.g6_backward(wout.cuda(), inputs=eng.G6_INPUTS)
    # a bf16-product GroupNorm output may sit ~1e-2 from the oracle's: the override may act up to there (tests/test_gpu_configs.py)
    ref = oracle_grads(kind, w, hp, inputs, None, False, wout, masks, kink_bound=5e-2)
    errs = [rel(g, r) for g, r in zip(got, ref)]
    print(f'[bf16 {kind}] input gradients, relative max-norm error: {errs}')
    for g, e in zip(got, errs):
        assert bool(torch.isfinite(g).all())
        assert e < BF16_GRAD, errs
