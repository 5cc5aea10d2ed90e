"""Bottleneck widths other than the defaults (pytest -m gpu): dim_neck, dim_neck_2 and dim_neck_3 anywhere in 1..32 and down-sampling
factors that differ from each other, through every path -- the recurrence kernels and the fused weight gradients at the op level, eval
forwards (long ones included), rhythm codes, training steps, input gradients, the 16-bit mode, the modules, the solver and the
data-parallel step.  The float64 oracle takes the widths and factors from hp, so every comparison is against it at the suite's bars.

The configurations (tests/test_capi_bottleneck_widths.py CONFIGS): W_odd (3, 2, 5) -- odd widths, padded slabs, a 102-wide decoder input;
W_mix (12, 3, 24) with factors (4, 16, 8) -- fused-wgrad blocks that straddle both directions, the non-compact decoder input; W_top
(31, 1, 17) -- the top of the range; P_mix, Generator_6 with (3, 20) and factors (8, 4)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import interp_np, ref_model, weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from tests.test_capi_bottleneck_widths import CONFIGS, hparams_of
from tests.test_gpu_configs import BF16_BOUNDS, LR, Case, check_adam, check_fp32_step
from tests.test_gpu_input_grads import engine_branches, masks_of

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def inputs(hp, seed, B, T):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, hp.dim_freq, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, hp.dim_f0, (B, T), generator=g), hp.dim_f0).float()
    emb = torch.nn.functional.one_hot(torch.randint(0, hp.dim_spk_emb, (B,), generator=g), hp.dim_spk_emb).float()
    return mel, onehot, emb


# --------------------------------------------------------------------------------------------- 1: one BLSTM layer at odd widths
def _torch_blstm(B, T, H, In, seed):
    g = torch.Generator().manual_seed(seed)
    ref = torch.nn.LSTM(In, H, 1, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1)      # O(1) weights: saturating and linear gates both
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    d_out = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64) * 0.1
    return ref, x, d_out


@pytest.mark.parametrize('H,T', [(3, 136), (5, 136), (12, 136), (17, 136), (24, 136), (31, 136), (31, 400)])
def test_small_blstm_layer_against_torch(E, H, T):
    """The encoder recurrences (LDS-staged, single-wave for 4H <= 64; T = 400 at H = 31 is past the LDS budget: the streaming kernels)
    against torch.nn.LSTM in float64: output, input gradient and every weight / bias gradient, per direction."""
    B, In = 4, 96
    ref, x, d_out = _torch_blstm(B, T, H, In, 40 + H + T)
    xr = x.clone().requires_grad_(True)
    y_ref, _ = ref(xr)
    y_ref.backward(d_out)
    f = lambda n: getattr(ref, n).detach().float().cuda()
    y, dx, grads = E.blstm_layer(x.float().cuda(), (f('weight_ih_l0'), f('weight_ih_l0_reverse')), (f('weight_hh_l0'), f('weight_hh_l0_reverse')),
                                 (f('bias_ih_l0'), f('bias_ih_l0_reverse')), (f('bias_hh_l0'), f('bias_hh_l0_reverse')), d_out.float().cuda())
    assert y.shape == (B, T, 2 * H)
    assert rel(y, y_ref.detach()) < TOL
    assert rel(dx, xr.grad) < TOL
    for d, sfx in enumerate(('', '_reverse')):
        gw_ih, gw_hh, gb = grads[d]
        assert rel(gw_ih, getattr(ref, 'weight_ih_l0' + sfx).grad) < TOL, sfx
        assert rel(gw_hh, getattr(ref, 'weight_hh_l0' + sfx).grad) < TOL, sfx
        assert rel(gb, getattr(ref, 'bias_ih_l0' + sfx).grad) < TOL, sfx


# --------------------------------------------------------------------------------------------- 2: fused weight gradients
@pytest.mark.parametrize('H', [3, 12, 17, 24, 31])
def test_fused_wgrad_any_width(E, H):
    """csrc/lstm_wgrad.hip for widths whose 64-row blocks hold both directions (H = 3, 12) or straddle the boundary at row 4H
    (H = 17 .. 31): every dW_hh and bias row of both directions, against float64, bit-identical when run twice."""
    In, R = 200, 8 * 132 + 3
    g = torch.Generator().manual_seed(5 + H)
    dg = torch.randn(R, 8 * H, generator=g) * 1e-3
    dg[0] = 0
    dg[-1] = 0
    x = torch.randn(R, In, generator=g)
    hout = torch.tanh(torch.randn(R, 2 * H, generator=g))
    hout[0] = 0
    hout[-1] = 0
    gwih, gwhh, gb = E.lstm_wgrad(dg.cuda(), x.cuda(), hout.cuda())
    d64, x64, h64 = dg.double(), x.double(), hout.double()
    for d in range(2):
        dd = d64[:, d * 4 * H:(d + 1) * 4 * H]
        assert rel(gwih[d], dd.t() @ x64) < 2e-6, d
        ref_hh = dd[1:].t() @ h64[:-1, :H] if d == 0 else dd[:-1].t() @ h64[1:, H:]
        assert rel(gwhh[d], ref_hh) < 2e-6, d
        assert rel(gb[d, 0], dd.sum(0)) < 2e-6 and torch.equal(gb[d, 0], gb[d, 1])
    again = E.lstm_wgrad(dg.cuda(), x.cuda(), hout.cuda())
    assert all(torch.equal(a, b) for a, b in zip((gwih, gwhh, gb), again))


# --------------------------------------------------------------------------------------------- 3: eval forwards and rhythm codes
_ENG = {}


def eval_engine(E, name, precision='f32'):
    key = (name, precision)
    if key not in _ENG:
        kind = CONFIGS[name][0]
        hp = hparams_of(name, 192)
        e = E.Engine(kind, hp, 4, 192)
        e.set_precision(precision)
        e.load_weights(W.make_weights(kind, hp, WSEED[kind]))
        _ENG[key] = e
    return _ENG[key]


def _eval_check(E, name, B, T):
    kind = CONFIGS[name][0]
    hp = hparams_of(name, 192)
    P = p64(W.make_weights(kind, hp, WSEED[kind]))
    e = eval_engine(E, name)
    mel, onehot, emb = inputs(hp, 10 + T + B, B, T)
    with torch.no_grad():
        if kind == 'G3':
            x_f0 = torch.cat((mel, onehot), -1)
            out = e.g3_forward(x_f0, mel, emb)
            ref = ref_model.generator_3(P, hp, x_f0.double(), mel.double(), emb.double())
        else:
            out = e.g6_forward(mel, onehot)
            ref = ref_model.generator_6(P, hp, mel.double(), onehot.double())
    e.check()
    err = rel(out, ref)
    print(f'[{name} eval {B}x{T}] rel {err:.2e}')
    assert err < TOL
    if kind == 'G3':
        codes = e.g3_rhythm(mel)
        with torch.no_grad():
            ref_c = ref_model.encoder_t(mel.double().transpose(1, 2), P, hp)
        assert codes.shape == ref_c.shape == (B, T // hp.freq_2, 2 * hp.dim_neck_2)
        assert rel(codes, ref_c) < TOL


@pytest.mark.parametrize('name', list(CONFIGS))
def test_eval_forward_and_codes(E, name):
    _eval_check(E, name, 3, 192)


@pytest.mark.parametrize('name,T', [('W_top', 1024), ('P_mix', 2048)])
def test_eval_forward_long(E, name, T):
    _eval_check(E, name, 1, T)


# --------------------------------------------------------------------------------------------- 4: training parity
class WCase(Case):
    """tests/test_gpu_configs.Case with the hparams of a width configuration."""

    def __init__(self, E, name, B, T, len_lo, bseed, precision='f32', max_T=None):
        kind = CONFIGS[name][0]
        self.kind, self.B, self.T = kind, B, T
        self.hp = hparams_of(name, T)
        w = W.make_weights(kind, self.hp, WSEED[kind])
        self.eng = E.Engine(kind, hparams_of(name, max_T or T), B, max_T or T)
        self.eng.set_precision(precision)
        self.eng.load_weights(w)
        self.eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
        self.st = ref_model.TrainState(w, LR)
        self.mel, self.f0, self.emb, self.lens = synth_batch(bseed, B, T, len_lo)
        self.ncalls = 4 if kind == 'G3' else 3
        if kind == 'G6':
            self.qidx = torch.from_numpy(interp_np.quantize_f0(self.f0[:, :, 0].numpy()))
            self.onehot = torch.nn.functional.one_hot(self.qidx, 257).float()
        self.dseed = bseed + 100


TRAIN = {'W_odd': (16, 128), 'W_mix': (16, 192), 'W_top': (16, 128), 'P_mix': (8, 192)}


@pytest.mark.parametrize('name', list(TRAIN))
def test_train_steps_against_oracle(E, name):
    B, T = TRAIN[name]
    c = WCase(E, name, B, T, T // 2, bseed=300 + B + T)
    for it in range(2):
        r = c.step(it)
        check_fp32_step(r, f'{name} step {it}')
        check_adam(r, f'{name} step {it}', it)


def test_bucketed_train_step_against_oracle(E):
    """SS_STEP_BUCKET at a T below the engine's max_len_pad, for W_mix (every factor divides 128)."""
    B, T = 8, 128
    c = WCase(E, 'W_mix', B, T, 64, bseed=411, max_T=192)
    draws = draws_for(c.dseed, B, 4)
    d = (np.stack([x[0] for x in draws]), np.stack([x[1] for x in draws]))
    loss = float(c.eng.g3_train_step(c.mel, c.f0, c.emb, c.lens, d, no_adam=True, bucket=True))
    c.eng.check()
    grads = {n: v.clone().cpu() for n, v in c.eng.grad_views().items()}
    masks = {k: v.cpu() for k, v in c.eng.relu_masks(B, T).items()}
    with engine_branches(masks, 2e-5):
        lo, _ = c.st.step_g3(c.hp, c.mel, c.f0, c.emb, c.lens.numpy(), draws)
    assert abs(loss - float(lo)) <= 1e-5 * abs(float(lo)), (loss, float(lo))
    for n, p in c.st.P.items():
        assert rel(grads[n], p.grad) < TOL, n


# --------------------------------------------------------------------------------------------- 5: input gradients
def test_g3_input_grads_w_mix(E):
    name, B, T = 'W_mix', 2, 128
    hp = hparams_of(name, T)
    w = W.make_weights('G3', hp, 7)
    eng = E.Engine('G3', hp, B, T)
    eng.load_weights(w)
    mel, onehot, emb = inputs(hp, 51, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    wout = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(5))
    eng.g3_forward(x_f0, mel, emb)
    masks = masks_of(eng, B, T)
    got = eng.g3_backward(wout.cuda(), inputs=('x_f0', 'x_org', 'c_trg'))
    eng.check()
    xs = [x.double().requires_grad_() for x in (x_f0, mel, emb)]
    with engine_branches(masks):
        out = ref_model.generator_3(p64(w), hp, *xs)
    (out * wout.double()).sum().backward()
    for n, a, x in zip(('x_f0', 'x_org', 'c_trg'), got, xs):
        assert rel(a, x.grad) < TOL, (n, rel(a, x.grad))


def test_g6_input_grads_p_mix(E):
    name, B, T = 'P_mix', 2, 128
    hp = hparams_of(name, T)
    w = W.make_weights('G6', hp, 8)
    eng = E.Engine('G6', hp, B, T)
    eng.load_weights(w)
    mel, onehot, _ = inputs(hp, 52, B, T)
    wout = torch.randn(B, T, 257, generator=torch.Generator().manual_seed(6))
    eng.g6_forward(mel, onehot)
    masks = masks_of(eng, B, T)
    got = eng.g6_backward(wout.cuda(), inputs=('x_org', 'f0_trg'))
    eng.check()
    xs = [x.double().requires_grad_() for x in (mel, onehot)]
    with engine_branches(masks):
        out = ref_model.generator_6(p64(w), hp, *xs)
    (out * wout.double()).sum().backward()
    for n, a, x in zip(('x_org', 'f0_trg'), got, xs):
        assert rel(a, x.grad) < TOL, (n, rel(a, x.grad))


# --------------------------------------------------------------------------------------------- 6: 16-bit mode
@pytest.mark.parametrize('name', ['W_mix', 'P_mix'])
def test_bf16_mode_against_fp32_oracle(E, name):
    B, T = 16, 192
    c = WCase(E, name, B, T, 96, bseed=700 + B, precision='bf16')
    r = c.step(0, kink_bound=5e-2)
    el = abs(r['loss_gpu'] - r['loss_cpu']) / abs(r['loss_cpu'])
    eo = rel(r['out_gpu'], r['out_cpu'])
    eg = {n: rel(r['grads_gpu'][n], g) for n, g in r['grads_cpu'].items()}
    worst = max(eg.items(), key=lambda x: x[1])
    med = float(np.median(list(eg.values())))
    print(f'[bf16 {name}] loss {el:.2e}  output {eo:.2e}  gradients: worst {worst[0]} {worst[1]:.2e}, median {med:.2e}')
    assert el < BF16_BOUNDS['loss'] and eo < BF16_BOUNDS['out']
    assert worst[1] < BF16_BOUNDS['grad'] and med < BF16_BOUNDS['grad_median']


# --------------------------------------------------------------------------------------------- 7: module, solver, data parallel
def test_module_solver_and_checkpoint(tmp_path):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, model, solver
    _, (n1, n2, n3), (f1, f2, f3) = CONFIGS['W_odd']
    hp = HP.default_hparams(batch_size=4, max_len_pad=128, dim_neck=n1, dim_neck_2=n2, dim_neck_3=n3, freq=f1, freq_2=f2, freq_3=f3)
    # the module loads a state_dict keyed and shaped as the reference's for these hparams
    G = model.Generator_3(hp).to('cuda:0')
    w = W.make_weights('G3', hp, 3)
    G.load_state_dict({**{k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, 'encoder_1.len_org': torch.tensor(128)})
    sd = G.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items() if k != 'encoder_1.len_org'] == [(n, tuple(s)) for n, s in W.param_spec('G3', hp)]
    for k, v in w.items():
        assert torch.equal(sd[k].cpu(), torch.from_numpy(np.asarray(v))), k
    del G
    np.random.seed(0)
    torch.manual_seed(0)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(8, seed=2))
    cfg = SimpleNamespace(num_iters=1, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False, device_id=0,
                          log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path), log_step=1, sample_step=1000,
                          model_save_step=1)
    s = solver.Solver(loader, cfg, hp)
    batch = next(iter(loader))
    loss = float(s.train_on_batch(batch))
    s.eng.check()
    assert np.isfinite(loss) and loss > 0
    s.save_model(1)
    s2 = solver.Solver(loader, SimpleNamespace(**{**vars(cfg), 'resume_iters': 1}), hp)
    s2.restore_model(1)
    for (n, a), (_, b) in zip(s.G.state_dict().items(), s2.G.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), n
    assert torch.equal(s.eng.adam_v, s2.eng.adam_v)


def _free_port():
    so = socket.socket()
    so.bind(('127.0.0.1', 0))
    p = so.getsockname()[1]
    so.close()
    return p


def _dp_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    from speechsplit_amd import dist as D
    from speechsplit_amd.engine import Engine
    from tests.test_capi_bottleneck_widths import hparams_of as hpo
    dist.init_process_group('gloo', rank=rank, world_size=world)
    Bg, T = 8, 128
    hp = hpo('W_mix', T)
    w = W.make_weights('G3', hp, 3)
    mel, f0, emb, lens = synth_batch(33, Bg, T, 64)
    dr = draws_for(43, Bg, 4)
    sc, ls = torch.from_numpy(np.stack([d[0] for d in dr])), torch.from_numpy(np.stack([d[1] for d in dr]))
    eng = Engine('G3', hp, Bg // world, T, device='cuda:0')
    eng.load_weights(w)
    eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    melr, embr, f0r, lenr = D.shard_batch((mel, emb, f0, lens), rank, world)
    loss = float(eng.dp_train_step(melr, f0r, embr, lenr, D.shard_draws(sc, ls, Bg, rank, world), world))
    eng.check()
    torch.cuda.synchronize()
    q.put((rank, loss, eng.params.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_step_two_ranks_w_mix(E):
    """Two ranks (gloo, one GPU) at the W_mix widths end with the parameters of one process stepping on the global batch."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (lo, prm)) for r, lo, prm in (q.get(timeout=600) for _ in procs))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    Bg, T = 8, 128
    hp = hparams_of('W_mix', T)
    eng = E.Engine('G3', hp, Bg, T)
    eng.load_weights(W.make_weights('G3', hp, 3))
    eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    mel, f0, emb, lens = synth_batch(33, Bg, T, 64)
    dr = draws_for(43, Bg, 4)
    loss = float(eng.g3_train_step(mel, f0, emb, lens, (np.stack([d[0] for d in dr]), np.stack([d[1] for d in dr]))))
    eng.check()
    ref = eng.params.cpu().numpy()
    assert np.array_equal(res[0][1], res[1][1])                      # replicas stay bit-identical
    assert abs((res[0][0] + res[1][0]) / 2 - loss) <= 2e-5 * abs(loss), (res[0][0], res[1][0], loss)
    assert float(np.abs(res[0][1] - ref).max()) <= 2.1 * LR, float(np.abs(res[0][1] - ref).max())
