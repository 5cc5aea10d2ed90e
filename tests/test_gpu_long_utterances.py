"""Eval-mode inference of utterances longer than 256 frames (ss_plan_bytes / ss_set_workspace, the chunked GroupNorm forward) against
the float64 oracle, and the refusals of everything that trains or differentiates at such lengths.  Runs on the GPU box: pytest -m gpu.

Bars: relative max-norm 1e-4 in f32 mode, as the suite's eval-forward tests (test_gpu_parity.py); 4e-2 in 16-bit mode
(test_gpu_configs.py BF16_BOUNDS['out'])."""
import numpy as np
import pytest
import torch

from oracle import ref_model, weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-4
BF16_OUT = 4e-2


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def p64(w):
    return {k: torch.from_numpy(np.array(v, dtype=np.float64)) for k, v in w.items()}


HP = W.default_hparams()
WEIGHTS = {'G3': W.make_weights('G3', HP, 3), 'G6': W.make_weights('G6', HP, 4)}


def inputs(seed, B, T):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, HP.dim_freq, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, HP.dim_f0, (B, T), generator=g), HP.dim_f0).float()
    emb = torch.nn.functional.one_hot(torch.randint(0, HP.dim_spk_emb, (B,), generator=g), HP.dim_spk_emb).float()
    return mel, onehot, emb


def oracle_g3(x_f0, mel, emb, P=None):
    with torch.no_grad():
        return ref_model.generator_3(P or p64(WEIGHTS['G3']), HP, x_f0.double(), mel.double(), emb.double())


def oracle_g6(mel, onehot):
    with torch.no_grad():
        return ref_model.generator_6(p64(WEIGHTS['G6']), HP, mel.double(), onehot.double())


_ENG = {}


def engine(kind, precision='f32', B=8):
    """One engine per (kind, precision), created for 8 x 192 like an ordinary one: long shapes grow its workspace (Engine.reserve)."""
    key = (kind, precision)
    if key not in _ENG:
        from speechsplit_amd.engine import Engine
        e = Engine(kind, HP, B, 192)
        e.set_precision(precision)
        e.load_weights(WEIGHTS[kind])
        _ENG[key] = e
    return _ENG[key]


# --------------------------------------------------------------------------------------------- the GroupNorm kernel (ss_op_conv_block)
@pytest.mark.parametrize('T', [264, 1000, 4096])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('Co', [256, 512])
def test_conv_block_forward_long(T, B, Co):
    from speechsplit_amd.engine import conv_block
    g = torch.Generator().manual_seed(T + 7 * B + Co)
    Ci = 80
    x = torch.rand(B, T, Ci, generator=g) * 2 - 1 + 0.3          # a non-zero mean: the two-pass variance matters
    w = torch.randn(Co, Ci, 5, generator=g) * 0.1
    bias = torch.randn(Co, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(Co, generator=g)
    beta = 0.1 * torch.randn(Co, generator=g)
    dev = torch.device('cuda:0')
    y1 = conv_block(x.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), beta.to(dev))
    y2 = conv_block(x.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), beta.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)                                   # fixed-order float64 reductions: identical bits
    P = {'b.0.conv.weight': w.double(), 'b.0.conv.bias': bias.double(), 'b.1.weight': gamma.double(), 'b.1.bias': beta.double()}
    ref = ref_model.conv_gn_relu(x.double().transpose(1, 2), P, 'b').transpose(1, 2)
    assert rel(y1, ref) < TOL


def test_conv_block_long_backward_is_refused():
    from speechsplit_amd.engine import conv_block
    dev = torch.device('cuda:0')
    x = torch.rand(1, 512, 80, device=dev)
    w, v = torch.randn(256, 80, 5, device=dev) * 0.1, torch.ones(256, device=dev)
    with pytest.raises(RuntimeError, match='forward only'):
        conv_block(x, w, v, v, v, dy=torch.ones(1, 512, 256, device=dev))


# --------------------------------------------------------------------------------------------- whole models, eval mode
@pytest.mark.parametrize('B,T', [(1, 264), (2, 1024), (1, 4096)])
def test_g3_eval_forward_long(B, T):
    e = engine('G3')
    mel, onehot, emb = inputs(10 + T + B, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    out = e.g3_forward(x_f0, mel, emb)
    e.check()
    assert out.shape == (B, T, HP.dim_freq)
    err = rel(out, oracle_g3(x_f0, mel, emb))
    print(f'[G3 {B}x{T}] rel {err:.2e}')
    assert err < TOL


@pytest.mark.parametrize('B,T', [(1, 1024), (1, 8192)])
def test_g6_eval_forward_long(B, T):
    e = engine('G6')
    mel, onehot, _ = inputs(20 + T, B, T)
    out = e.g6_forward(mel, onehot)
    e.check()
    ref = oracle_g6(mel, onehot)
    err = rel(out, ref)
    print(f'[G6 {B}x{T}] rel {err:.2e}')
    assert err < TOL
    top2 = ref.topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > 1e-3
    assert torch.equal(out.argmax(-1).cpu()[sure], ref.argmax(-1)[sure])


def test_g3_rhythm_long():
    e = engine('G3')
    mel, _, _ = inputs(31, 1, 2048)
    codes = e.g3_rhythm(mel)
    with torch.no_grad():
        ref = ref_model.encoder_t(mel.double().transpose(1, 2), p64(WEIGHTS['G3']), HP)
    assert codes.shape == ref.shape
    assert rel(codes, ref) < TOL


def test_g3_bf16_long():
    e = engine('G3', 'bf16')
    mel, onehot, emb = inputs(41, 3, 1024)
    x_f0 = torch.cat((mel, onehot), -1)
    out = e.g3_forward(x_f0, mel, emb)
    e.check()
    err = rel(out, oracle_g3(x_f0, mel, emb))
    print(f'[G3 bf16 3x1024] rel {err:.2e}')
    assert err < BF16_OUT


def test_workspace_grows_and_never_shrinks():
    from speechsplit_amd.engine import Engine
    e = Engine('G6', HP, 2, 192)
    e.load_weights(WEIGHTS['G6'])
    n0 = e.ws.numel()
    assert e.plan_bytes(2, 192) == n0
    assert not e.reserve(1, 256)
    assert e.reserve(1, 4096) and e.ws.numel() == e.plan_bytes(1, 4096) > n0
    n1 = e.ws.numel()
    assert not e.reserve(1, 1024) and e.ws.numel() == n1
    mel, onehot, _ = inputs(51, 2, 192)                      # the ordinary shapes still run, on the grown workspace
    assert rel(e.g6_forward(mel, onehot), oracle_g6(mel, onehot)) < TOL
    with pytest.raises(RuntimeError, match='multiple'):
        e.plan_bytes(1, 1020)


# --------------------------------------------------------------------------------------------- modules and the conversion
def test_module_long_input_keeps_engine_and_adam_state():
    """Generator_3 (batch 16) in eval mode on 1 x 2000 (fits the bound workspace) and 1 x 4096 (grows it): same engine object, and
    a train step afterwards matches a fresh engine's -- the Adam state crossed ss_set_workspace, the re-plan left nothing stale."""
    from conftest import assert_same_trajectory
    from oracle.gen_fixtures import draws_for, synth_batch
    from speechsplit_amd import model
    from speechsplit_amd.engine import Engine
    G = model.Generator_3(HP, max_batch=16)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in WEIGHTS['G3'].items()}, strict=False)
    G = G.eval().cuda()
    eng = G._eng
    ref = Engine('G3', HP, 16, 192)
    ref.load_weights(WEIGHTS['G3'])
    B = 4
    mel, f0, emb, lens = synth_batch(61, B, 192, 64)
    dr = [draws_for(71 + s, B, 4) for s in range(2)]
    st = lambda d: (np.stack([x[0] for x in d]), np.stack([x[1] for x in d]))
    for e in (eng, ref):
        e.set_adam(lr=1e-4)
        e.g3_train_step(mel, f0, emb, lens, st(dr[0]))
    n0 = eng.ws.numel()
    P = {n: v.detach().cpu().double() for n, v in eng.param_views().items()}      # the weights after the first step
    for T in (2000, 4096):
        m, oh, em = inputs(80 + T, 1, T)
        x_f0 = torch.cat((m, oh), -1).cuda()
        with torch.no_grad():
            out = G(x_f0, m.cuda(), em.cuda())
        assert G._eng is eng
        assert (eng.ws.numel() == n0) == (T == 2000)         # 16 x 192 holds a 2000-frame utterance; 4096 frames grow it
        assert rel(out, oracle_g3(x_f0.cpu(), m, em, P)) < TOL
    assert G._eng is eng and G._plist[0].data.data_ptr() == eng.param_views()[G._names[0]].data_ptr()
    for e in (eng, ref):
        e.g3_train_step(mel, f0, emb, lens, st(dr[1]))
    eng.check()
    ref.check()
    assert_same_trajectory(eng.params, ref.params, lr=1e-4, steps=2, tag='after long eval forwards')


def _entry(name, seed, L):
    g = np.random.default_rng(seed)
    mel = g.random((L, HP.dim_freq)).astype(np.float32)
    f0 = g.random(L)
    f0[g.random(L) < 0.3] = 0.0                              # unvoiced frames
    emb = np.zeros((1, HP.dim_spk_emb), np.float32)
    emb[0, seed % HP.dim_spk_emb] = 1.0
    return [name, emb, (mel, f0, L, f'{name}_utt')]


def test_demo_conversion_long_pair():
    from speechsplit_amd import convert, model
    from speechsplit_amd.utils import pad_seq_to_2, quantize_f0_numpy
    G, P = model.Generator_3(HP).eval(), model.Generator_6(HP).eval()
    G.load_state_dict({k: torch.from_numpy(v) for k, v in WEIGHTS['G3'].items()}, strict=False)
    P.load_state_dict({k: torch.from_numpy(v) for k, v in WEIGHTS['G6'].items()}, strict=False)
    G, P = G.to('cuda:0'), P.to('cuda:0')
    ei, ej = _entry('p0', 5, 500), _entry('p1', 6, 430)
    res = convert.demo_conversion(G, P, ei, ej)
    T = convert.conversion_frames((500, 430))
    assert T == 504

    # the oracle: demo.ipynb's steps at the common padded T, in float64
    def prep(ent):
        mel, f0, L, _ = ent[2]
        mel_pad, _ = pad_seq_to_2(mel[None], T)
        oh = quantize_f0_numpy(np.pad(f0, (0, T - L)))[0][None]
        return torch.from_numpy(mel_pad).double(), torch.from_numpy(oh).double(), torch.from_numpy(ent[1]).double(), L
    x_org, oh_org, emb_org, len_org = prep(ei)
    x_trg, oh_trg, emb_trg, len_trg = prep(ej)
    logits = oracle_g6(x_org, oh_trg)[0]
    _, idx = convert.convert_f0(P, x_org.float().cuda(), oh_trg.float().cuda())
    top2 = logits.topk(2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(idx.cpu()[sure], logits.argmax(-1)[sure])
    # the seven conditions from the engine's F0 decision (a class within 1e-3 of a tie may go either way in any fp32 implementation)
    oh_con = torch.nn.functional.one_hot(idx.cpu(), HP.dim_f0).double()[None]
    xf_org, xf_trg = torch.cat((x_org, oh_org), -1), torch.cat((x_org, oh_con), -1)
    cs = convert.CONDITIONS
    x_f0 = torch.cat([xf_trg if 'F' in c else xf_org for c in cs])
    x_rh = torch.cat([x_trg if 'R' in c else x_org for c in cs])
    emb = torch.cat([emb_trg if 'U' in c else emb_org for c in cs])
    ref = oracle_g3(x_f0, x_rh, emb)
    assert [r[0] for r in res] == [f'p0_p1_p0_utt_{c}' for c in cs]
    for n, ((name, mel), c) in enumerate(zip(res, cs)):
        keep = len_trg if 'R' in c else len_org
        assert mel.shape == (keep, HP.dim_freq)
        assert rel(mel, ref[n, :keep]) < TOL, c


# --------------------------------------------------------------------------------------------- refusals
def test_backward_after_long_forward_is_refused():
    e = engine('G3')
    mel, onehot, emb = inputs(91, 1, 512)
    x_f0 = torch.cat((mel, onehot), -1)
    out = e.g3_forward(x_f0, mel, emb)
    for call in (lambda: e.g3_backward(torch.ones_like(out)), lambda: e.g3_backward(torch.ones_like(out), inputs=('x_org',))):
        with pytest.raises(RuntimeError, match='eval-only'):
            call()
    e.check()
    # usable afterwards: an ordinary forward + backward
    m, oh, em = inputs(92, 2, 192)
    x = torch.cat((m, oh), -1)
    assert rel(e.g3_forward(x, m, em), oracle_g3(x, m, em)) < TOL
    e.g3_backward(torch.ones(2, 192, HP.dim_freq))
    e.check()


def test_module_autograd_through_long_forward_raises():
    from speechsplit_amd import model
    P = model.Generator_6(HP).eval()
    P.load_state_dict({k: torch.from_numpy(v) for k, v in WEIGHTS['G6'].items()}, strict=False)
    P = P.cuda()
    mel, onehot, _ = inputs(93, 1, 512)
    out = P(mel.cuda(), onehot.cuda())
    assert out.requires_grad
    with pytest.raises(RuntimeError, match='eval-only'):
        out.sum().backward()
    P._eng.check()


def test_training_at_long_frames_is_refused():
    from oracle.gen_fixtures import draws_for, synth_batch
    from speechsplit_amd.engine import Engine, draw_interp
    e = Engine('G3', HP, 2, 192)
    e.load_weights(WEIGHTS['G3'])
    assert e.reserve(1, 1024)                                # grown to hold 1024 frames: training still may not use them
    mel, onehot, emb = inputs(94, 1, 1024)
    x_f0 = torch.cat((mel, onehot), -1)
    with pytest.raises(RuntimeError, match='eval mode only'):
        e.g3_forward(x_f0, mel, emb, draw_interp(1, 3, HP), training=True)
    m, f0, em, lens = synth_batch(95, 1, 512, 300)
    dr = draws_for(96, 1, 4)
    st = (np.stack([x[0] for x in dr]), np.stack([x[1] for x in dr]))
    for bucket in (False, True):
        with pytest.raises(RuntimeError, match='max_frames'):
            e.g3_train_step(m, f0, em, lens, st, bucket=bucket)
    e.check()
    # usable afterwards: an ordinary step and an eval forward at the grown length
    m, f0, em, lens = synth_batch(97, 2, 192, 64)
    dr = draws_for(98, 2, 4)
    loss = float(e.g3_train_step(m, f0, em, lens, (np.stack([x[0] for x in dr]), np.stack([x[1] for x in dr]))))
    assert np.isfinite(loss)
    out = e.g3_forward(x_f0, mel, emb)
    e.check()
    assert bool(torch.isfinite(out).all())


def test_interp_above_max_frames_is_refused():
    from speechsplit_amd.engine import Engine, draw_interp
    e = Engine('interp', HP, 2, 192)
    sc, ls = draw_interp(2, 1, HP)
    x = torch.rand(2, 512, 20, device='cuda')
    with pytest.raises(RuntimeError, match='max_frames'):
        e.interp_forward(x, [512, 400], sc[0], ls[0])
    y = e.interp_forward(x[:, :128], [128, 100], sc[0], ls[0])          # usable afterwards
    with pytest.raises(RuntimeError, match='max_frames'):
        e.interp_backward(torch.ones_like(y), 512)
    dx = e.interp_backward(torch.ones_like(y), 128)
    e.check()
    assert dx.shape == (2, 128, 20)
