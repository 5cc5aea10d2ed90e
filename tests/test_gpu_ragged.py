"""Ragged eval-mode batches (ss_g3_forward_ragged / ss_g6_forward_ragged / ss_g3_rhythm_ragged and the two ragged test hooks): rows of
different lengths in one batch, each compared with the float64 oracle run on that row ALONE at its own length -- never with a second engine
call.  Runs on the GPU box: pytest -m gpu.

Bars: relative max-norm per row 1e-4 in f32 mode (the suite's eval-forward bar, tests/test_gpu_long_utterances.py; hook-level BLSTM
comparisons use the same 1e-4 that tests/test_gpu_parity.py uses for those hooks); 4e-2 in 16-bit mode (test_gpu_configs.py
BF16_BOUNDS['out']).  The padded frames of every input hold NaN unless a test says otherwise, and every output must be exactly zero
behind each row's end.  On the length sets used here the float64 oracle run on the zero-padded batch misses the oracle run per row by more
than 0.25, so a predicate left out of any one kernel cannot pass."""
import numpy as np
import pytest
import torch

from oracle import ref_model, weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-4
BF16_OUT = 4e-2
DEV = 'cuda:0'
HP = W.default_hparams()
WEIGHTS = {'G3': W.make_weights('G3', HP, 3), 'G6': W.make_weights('G6', HP, 4)}
_P64 = {}
NAN = float('nan')

MIXED17 = [16 if b % 2 == 0 else 8 for b in range(16)] + [8]        # two batch tiles, lengths differing inside and across tiles


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def p64(kind):
    if kind not in _P64:
        _P64[kind] = {k: torch.from_numpy(np.array(v, dtype=np.float64)) for k, v in WEIGHTS[kind].items()}
    return _P64[kind]


def inputs(seed, B, T):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, HP.dim_freq, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, HP.dim_f0, (B, T), generator=g), HP.dim_f0).float()
    emb = torch.nn.functional.one_hot(torch.randint(0, HP.dim_spk_emb, (B,), generator=g), HP.dim_spk_emb).float()
    return mel, onehot, emb


def padded(x, lens, value):
    """copy of x [B, T, C] with frames t >= lens[b] of row b set to `value`"""
    y = x.clone()
    for b, n in enumerate(lens):
        y[b, n:] = value
    return y


def check_rows(out, lens, ref_of_row, bar, tag):
    """every row: zeros behind its end, and its own frames within `bar` of the oracle's run of that row alone; returns the worst row"""
    out = out.detach().cpu()
    worst = 0.0
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == 0).all()), (tag, b, 'padding is not zero')
        assert bool(torch.isfinite(out[b, :n]).all()), (tag, b)
        worst = max(worst, rel(out[b, :n], ref_of_row(b, n)))
    print(f'[{tag}] worst row rel {worst:.2e}')
    assert worst < bar, (tag, worst)
    return worst


_ENG = {}


def engine(kind, precision='f32'):
    """one engine per (kind, precision), 17 x 192: long shapes grow its workspace (Engine.reserve)"""
    key = (kind, precision)
    if key not in _ENG:
        from speechsplit_amd.engine import Engine
        e = Engine(kind, HP, 17, 192)
        e.set_precision(precision)
        e.load_weights(WEIGHTS[kind])
        _ENG[key] = e
    return _ENG[key]


def oracle_g3_row(x_f0, mel, emb):
    def f(b, n):
        with torch.no_grad():
            return ref_model.generator_3(p64('G3'), HP, x_f0[b:b + 1, :n].double(), mel[b:b + 1, :n].double(), emb[b:b + 1].double())[0]
    return f


def oracle_g6_row(mel, onehot):
    def f(b, n):
        with torch.no_grad():
            return ref_model.generator_6(p64('G6'), HP, mel[b:b + 1, :n].double(), onehot[b:b + 1, :n].double())[0]
    return f


# --------------------------------------------------------------------------------------------- 1. GroupNorm through the conv-block hook
@pytest.mark.parametrize('B,T,lens', [(3, 40, [40, 8, 24]), (3, 256, [256, 248, 16]), (3, 264, [264, 200, 8]), (3, 520, [520, 264, 64])],
                         ids=['reg_t40', 'reg_t256', 'chunked_t264', 'chunked_t520'])
@pytest.mark.parametrize('Co', [256, 512])
def test_conv_block_ragged(B, T, lens, Co):
    """The register kernel (T <= 256) and the three chunked launches: a partial last chunk, a length of exactly one chunk (64), rows whose
    chunks are empty from the second on (8), and lengths <= 256 on the long kernels."""
    from speechsplit_amd.engine import conv_block
    g = torch.Generator().manual_seed(T + Co)
    Ci = 80
    x = torch.rand(B, T, Ci, generator=g) * 2 - 1 + 0.3
    w = torch.randn(Co, Ci, 5, generator=g) * 0.1
    bias = torch.randn(Co, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(Co, generator=g)
    beta = 0.1 * torch.randn(Co, generator=g)
    xn = padded(x, lens, NAN).to(DEV)
    args = (w.to(DEV), bias.to(DEV), gamma.to(DEV), beta.to(DEV))
    y1 = conv_block(xn, *args, lengths=lens)
    y2 = conv_block(xn, *args, lengths=torch.tensor(lens, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)                                   # fixed-order reductions, empty chunks contribute 0.0: identical bits
    P = {'b.0.conv.weight': w.double(), 'b.0.conv.bias': bias.double(), 'b.1.weight': gamma.double(), 'b.1.bias': beta.double()}

    def ref(b, n):
        return ref_model.conv_gn_relu(x[b:b + 1, :n].double().transpose(1, 2), P, 'b').transpose(1, 2)[0]
    check_rows(y1, lens, ref, TOL, f'conv block {B}x{T} Co {Co}')


# --------------------------------------------------------------------------------------------- 2. recurrences through the BLSTM hook
def _blstm_case(H, B, T, lens, In=24):
    from speechsplit_amd.engine import blstm_layer
    g = torch.Generator().manual_seed(1000 + 7 * H + B + T)
    k = 1.0 / np.sqrt(H)
    u = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k           # torch.nn.LSTM's initialiser
    P = {}
    for sfx in ('', '_reverse'):
        P['l.weight_ih_l0' + sfx], P['l.weight_hh_l0' + sfx] = u(4 * H, In), u(4 * H, H)
        P['l.bias_ih_l0' + sfx], P['l.bias_hh_l0' + sfx] = u(4 * H), u(4 * H)
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    f = lambda n: P[n].float().to(DEV)
    y = blstm_layer(padded(x, lens, NAN).float().to(DEV), (f('l.weight_ih_l0'), f('l.weight_ih_l0_reverse')),
                    (f('l.weight_hh_l0'), f('l.weight_hh_l0_reverse')), (f('l.bias_ih_l0'), f('l.bias_ih_l0_reverse')),
                    (f('l.bias_hh_l0'), f('l.bias_hh_l0_reverse')), lengths=lens)
    torch.cuda.synchronize()

    def ref(b, n):
        with torch.no_grad():
            return ref_model.blstm(x[b:b + 1, :n], P, 'l', 1)[0]
    return y, ref


@pytest.mark.parametrize('small_lds', [1, 2, 0], ids=['wave_or_lds', 'lds', 'streaming'])
@pytest.mark.parametrize('H', [1, 5, 8, 32])
def test_small_recurrences_ragged(H, small_lds):
    """the three kernels of lstm_small.hip (single-wave, LDS-staged, streaming)"""
    from speechsplit_amd.engine import tune
    lens = [24, 8, 16]
    tune('small_lds', small_lds)
    try:
        y, ref = _blstm_case(H, 3, 24, lens)
    finally:
        tune('small_lds', 1)
    check_rows(y, lens, ref, TOL, f'small H {H} small_lds {small_lds}')


def test_small_recurrence_past_lds_budget_ragged():
    """H = 32 at 520 frames: 266 KB of pre-activations per (utterance, direction), so the streaming kernel runs by itself"""
    lens = [520, 328]
    y, ref = _blstm_case(32, 2, 520, lens)
    check_rows(y, lens, ref, TOL, 'small H 32 T 520')


@pytest.mark.parametrize('seq_tag', [1, 0], ids=['tagged', 'flag_line'])
@pytest.mark.parametrize('H', [256, 512])
def test_persistent_recurrence_ragged(H, seq_tag):
    from speechsplit_amd.engine import tune
    lens = [24, 8, 16]
    tune('seq_tag', seq_tag)
    try:
        y, ref = _blstm_case(H, 3, 24, lens, In=96)
    finally:
        tune('seq_tag', 1)
    check_rows(y, lens, ref, TOL, f'persistent H {H} seq_tag {seq_tag}')


@pytest.mark.parametrize('H', [256, 512])
def test_persistent_recurrence_ragged_two_batch_tiles(H):
    y, ref = _blstm_case(H, 17, 16, MIXED17, In=96)
    check_rows(y, MIXED17, ref, TOL, f'persistent H {H} 17 x 16')


@pytest.mark.parametrize('H,persist', [(512, 0), (64, 1), (128, 1)], ids=['h512_per_step', 'h64', 'h128'])
def test_per_step_recurrence_ragged(H, persist):
    from speechsplit_amd.engine import tune
    lens = [24, 8, 16]
    tune('persist', persist)
    try:
        y, ref = _blstm_case(H, 3, 24, lens, In=96)
    finally:
        tune('persist', 1)
    check_rows(y, lens, ref, TOL, f'per-step H {H}')


# --------------------------------------------------------------------------------------------- 3. whole models
SHAPES = [(4, 64, [64, 8, 40, 24]), (17, 16, MIXED17)]


@pytest.mark.parametrize('B,T,lens', SHAPES, ids=['4x64', '17x16'])
def test_g3_ragged(B, T, lens):
    e = engine('G3')
    mel, onehot, emb = inputs(100 + B, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    out_nan = e.g3_forward(padded(x_f0, lens, NAN), padded(mel, lens, NAN), emb, lengths=lens)
    out_zero = e.g3_forward(padded(x_f0, lens, 0.0), padded(mel, lens, 0.0), emb, lengths=torch.tensor(lens, device=DEV))
    e.check()
    assert torch.equal(out_nan, out_zero)                        # the padded input frames are never used
    check_rows(out_nan, lens, oracle_g3_row(x_f0, mel, emb), TOL, f'G3 ragged {B}x{T}')


@pytest.mark.parametrize('B,T,lens', SHAPES, ids=['4x64', '17x16'])
def test_g6_ragged(B, T, lens):
    e = engine('G6')
    mel, onehot, _ = inputs(200 + B, B, T)
    out_nan = e.g6_forward(padded(mel, lens, NAN), padded(onehot, lens, NAN), lengths=lens)
    out_zero = e.g6_forward(padded(mel, lens, 0.0), padded(onehot, lens, 0.0), lengths=np.asarray(lens))
    e.check()
    assert torch.equal(out_nan, out_zero)
    check_rows(out_nan, lens, oracle_g6_row(mel, onehot), TOL, f'G6 ragged {B}x{T}')


@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_full_lengths_and_none_are_the_plain_forward(kind):
    """every length equal to T: the predicates select nothing, the bits are the plain forward's; lengths=None IS the plain call"""
    e = engine(kind)
    B, T = 4, 64
    mel, onehot, emb = inputs(300, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    if kind == 'G3':
        codes = (e.g3_rhythm(mel), e.g3_rhythm(mel, lengths=[T] * B), e.g3_rhythm(mel, lengths=None))
        assert torch.equal(codes[0], codes[1]) and torch.equal(codes[0], codes[2])
        plain, full, none = e.g3_forward(x_f0, mel, emb), e.g3_forward(x_f0, mel, emb, lengths=[T] * B), e.g3_forward(x_f0, mel, emb, lengths=None)
    else:
        plain, full, none = e.g6_forward(mel, onehot), e.g6_forward(mel, onehot, lengths=[T] * B), e.g6_forward(mel, onehot, lengths=None)
    e.check()
    assert torch.equal(plain, full)
    assert torch.equal(plain, none)
    assert e._fwd_bt == (B, T)                                   # a plain forward again: differentiable
    (e.g3_backward if kind == 'G3' else e.g6_backward)(torch.ones_like(plain))
    e.check()


def test_g3_rhythm_ragged():
    e = engine('G3')
    B, T, lens = SHAPES[0]
    mel, _, _ = inputs(400, B, T)
    codes = e.g3_rhythm(padded(mel, lens, NAN), lengths=lens)
    e.check()
    assert codes.shape == (B, T // HP.freq_2, 2 * HP.dim_neck_2)

    def ref(b, n):
        with torch.no_grad():
            return ref_model.encoder_t(mel[b:b + 1, :n * HP.freq_2].double().transpose(1, 2), p64('G3'), HP)[0]
    check_rows(codes, [n // HP.freq_2 for n in lens], ref, TOL, 'G3 rhythm ragged 4x64')


@pytest.mark.parametrize('T,lens', [(520, [520, 264]), (1280, [1280, 640])], ids=['520', '1280_streaming_encoder'])
def test_g3_ragged_long(T, lens):
    """chunked GroupNorm, and at 1280 frames the H = 8 encoder recurrence on its streaming kernel (its LDS budget holds 1264 frames)"""
    e = engine('G3')
    mel, onehot, emb = inputs(500 + T, 2, T)
    x_f0 = torch.cat((mel, onehot), -1)
    out = e.g3_forward(padded(x_f0, lens, NAN), padded(mel, lens, NAN), emb, lengths=lens)
    e.check()
    check_rows(out, lens, oracle_g3_row(x_f0, mel, emb), TOL, f'G3 ragged 2x{T}')


def test_g6_ragged_long():
    e = engine('G6')
    T, lens = 520, [520, 264]
    mel, onehot, _ = inputs(600, 2, T)
    out = e.g6_forward(padded(mel, lens, NAN), padded(onehot, lens, NAN), lengths=lens)
    e.check()
    check_rows(out, lens, oracle_g6_row(mel, onehot), TOL, 'G6 ragged 2x520')


@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_ragged_bf16(kind):
    e = engine(kind, 'bf16')
    B, T, lens = SHAPES[0]
    mel, onehot, emb = inputs(700, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    if kind == 'G3':
        out = e.g3_forward(padded(x_f0, lens, NAN), padded(mel, lens, NAN), emb, lengths=lens)
        ref = oracle_g3_row(x_f0, mel, emb)
    else:
        out = e.g6_forward(padded(mel, lens, NAN), padded(onehot, lens, NAN), lengths=lens)
        ref = oracle_g6_row(mel, onehot)
    e.check()
    check_rows(out, lens, ref, BF16_OUT, f'{kind} ragged bf16 4x64')


# --------------------------------------------------------------------------------------------- 4. one engine on guarded memory
def test_guarded_g3_ragged():
    """Inputs, lengths and output in guarded buffers (tests/guarded.py), the engine's arenas and workspace as well: nothing outside `out` is
    written, every element of `out` is, and the NaN all round the inputs -- and inside them, behind each row's end -- changes nothing."""
    from speechsplit_amd import engine as E
    from tests.test_gpu_engine_containment import Bound, plain
    B, T, lens = SHAPES[0]
    hp = W.default_hparams(max_len_pad=T)
    b, ref_eng = Bound(E, 'G3', hp, B, T), plain(E, 'G3', hp, B, T)
    mel, onehot, emb = inputs(800, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    out = b.eng.g3_forward(b.inp(padded(x_f0, lens, NAN), 'x_f0'), b.inp(padded(mel, lens, NAN), 'x_org'), b.inp(emb, 'c_trg'),
                           lengths=b.inp(torch.tensor(lens), 'lengths', torch.int32))
    out = out.clone()
    b.check('ragged G3 4x64')
    assert torch.equal(out, ref_eng.g3_forward(padded(x_f0, lens, 0.0), padded(mel, lens, 0.0), emb, lengths=lens))
    check_rows(out, lens, oracle_g3_row(x_f0, mel, emb), TOL, 'guarded G3 ragged 4x64')


# --------------------------------------------------------------------------------------------- 5. refusals
def _ordinary_forward_backward(e):
    """the engine is usable afterwards: an ordinary forward within the bar, and its backward"""
    m, oh, em = inputs(92, 2, 192)
    x = torch.cat((m, oh), -1)
    with torch.no_grad():
        ref = ref_model.generator_3(p64('G3'), HP, x.double(), m.double(), em.double())
    assert rel(e.g3_forward(x, m, em), ref) < TOL
    e.g3_backward(torch.ones(2, 192, HP.dim_freq))
    e.check()


def test_c_entry_point_refuses_training_with_lengths():
    from speechsplit_amd.engine import _ptr, _stream
    e = engine('G3')
    B, T = 2, 192
    mel, onehot, emb = inputs(900, B, T)
    x_f0, mel, emb = torch.cat((mel, onehot), -1).to(DEV), mel.to(DEV), emb.to(DEV)
    ln = torch.tensor([192, 64], dtype=torch.int32, device=DEV)
    out = torch.full((B, T, HP.dim_freq), 7.0, device=DEV)
    rc = e.lib.ss_g3_forward_ragged(e.h, _ptr(x_f0), _ptr(mel), _ptr(emb), _ptr(ln), B, T, 1, _ptr(out), _stream())
    assert rc != 0 and b'eval-only' in e.lib.ss_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                              # nothing was enqueued
    with pytest.raises(ValueError, match='eval-mode'):
        e.g3_forward(x_f0, mel, emb, training=True, lengths=[192, 64])
    _ordinary_forward_backward(e)


def test_backward_after_ragged_forward_is_refused():
    e = engine('G3')
    mel, onehot, emb = inputs(901, 2, 64)
    x_f0 = torch.cat((mel, onehot), -1)
    out = e.g3_forward(x_f0, mel, emb, lengths=[64, 24])
    for call in (lambda: e.g3_backward(torch.ones_like(out)), lambda: e.g3_backward(torch.ones_like(out), inputs=('x_org',))):
        with pytest.raises(RuntimeError, match='eval-only'):
            call()
    e.check()
    _ordinary_forward_backward(e)
    e6 = engine('G6')
    out = e6.g6_forward(mel, onehot, lengths=[64, 24])
    with pytest.raises(RuntimeError, match='eval-only'):
        e6.g6_backward(torch.ones_like(out))
    e6.check()


def _module(kind):
    from speechsplit_amd import model
    M = (model.Generator_3 if kind == 'G3' else model.Generator_6)(HP)
    M.load_state_dict({k: torch.from_numpy(v) for k, v in WEIGHTS[kind].items()}, strict=False)
    return M.to(DEV)


def test_module_refusals():
    """.train() with lengths raises before anything runs; autograd through a ragged eval forward raises the eval-only error; the module
    then trains an ordinary batch"""
    G = _module('G3')
    mel, onehot, emb = inputs(902, 2, 64)
    x_f0, mel_d, emb_d = torch.cat((mel, onehot), -1).to(DEV), mel.to(DEV), emb.to(DEV)
    G.train()
    with pytest.raises(ValueError, match='eval mode'):
        G(x_f0, mel_d, emb_d, lengths=[64, 24])
    with pytest.raises(ValueError, match='eval mode'):
        G.rhythm(mel_d, lengths=[64, 24])
    G.eval()
    out = G(x_f0, mel_d, emb_d, lengths=[64, 24])
    assert out.requires_grad and bool((out[1, 24:] == 0).all())
    with pytest.raises(RuntimeError, match='eval-only'):
        out.sum().backward()
    G._eng.check()
    # usable afterwards: an ordinary eval forward within the bar and autograd through it
    m, oh, em = inputs(903, 2, 192)
    x = torch.cat((m, oh), -1)
    out = G(x.to(DEV), m.to(DEV), em.to(DEV))
    with torch.no_grad():
        ref = ref_model.generator_3(p64('G3'), HP, x.double(), m.double(), em.double())
    assert rel(out, ref) < TOL
    out.sum().backward()
    G._eng.check()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in G.parameters())


# --------------------------------------------------------------------------------------------- 6. convert_batch
def _entry(name, seed, L):
    g = np.random.default_rng(seed)
    mel = g.random((L, HP.dim_freq)).astype(np.float32)
    f0 = g.random(L)
    f0[g.random(L) < 0.3] = 0.0                              # unvoiced frames
    emb = np.zeros((1, HP.dim_spk_emb), np.float32)
    emb[0, seed % HP.dim_spk_emb] = 1.0
    return [name, emb, (mel, f0, L, f'{name}_utt')]


def test_convert_batch():
    """Three pairs with their own conversion_frames() (192, 504, 200) against the float64 oracle at each pair's own length, exactly as
    test_demo_conversion_long_pair compares one pair: the engine's F0 decision, classes within 1e-3 of a tie left out of the argmax check."""
    from speechsplit_amd import convert
    from speechsplit_amd.utils import pad_seq_to_2, quantize_f0_numpy
    G, P = _module('G3').eval(), _module('G6').eval()
    pairs = [(_entry('a0', 5, 40), _entry('a1', 6, 64)), (_entry('b0', 7, 500), _entry('b1', 8, 430)), (_entry('c0', 9, 200), _entry('c1', 10, 120))]
    res = convert.convert_batch(G, P, pairs, max_rows=8)
    assert len(res) == len(pairs)
    cs = convert.CONDITIONS
    worst = 0.0
    for (ei, ej), got in zip(pairs, res):
        T = convert.conversion_frames((ei[2][2], ej[2][2]))

        def prep(ent):
            mel, f0, L, _ = ent[2]
            mel_pad, _ = pad_seq_to_2(mel[None], T)
            oh = quantize_f0_numpy(np.pad(f0, (0, T - L)))[0][None]
            return torch.from_numpy(mel_pad).double(), torch.from_numpy(oh).double(), torch.from_numpy(ent[1]).double(), L
        x_org, oh_org, emb_org, len_org = prep(ei)
        x_trg, oh_trg, emb_trg, len_trg = prep(ej)
        with torch.no_grad():
            logits = ref_model.generator_6(p64('G6'), HP, x_org, oh_trg)[0]
        _, idx = convert.convert_f0(P, x_org.float().to(DEV), oh_trg.float().to(DEV))      # the engine's F0 decision (batch 1)
        top2 = logits.topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > 1e-3
        assert torch.equal(idx.cpu()[sure], logits.argmax(-1)[sure])
        oh_con = torch.nn.functional.one_hot(idx.cpu(), HP.dim_f0).double()[None]
        xf_org, xf_trg = torch.cat((x_org, oh_org), -1), torch.cat((x_org, oh_con), -1)
        x_f0 = torch.cat([xf_trg if 'F' in c else xf_org for c in cs])
        x_rh = torch.cat([x_trg if 'R' in c else x_org for c in cs])
        emb = torch.cat([emb_trg if 'U' in c else emb_org for c in cs])
        with torch.no_grad():
            ref = ref_model.generator_3(p64('G3'), HP, x_f0, x_rh, emb)
        assert [r[0] for r in got] == [f'{ei[0]}_{ej[0]}_{ei[0]}_utt_{c}' for c in cs]
        for n, ((name, mel), c) in enumerate(zip(got, cs)):
            keep = len_trg if 'R' in c else len_org
            assert mel.shape == (keep, HP.dim_freq)
            err = rel(mel, ref[n, :keep])
            worst = max(worst, err)
            assert err < TOL, (name, err)
    print(f'[convert_batch] worst rel {worst:.2e}')
    # names and shapes are demo_conversion's
    one = convert.demo_conversion(G, P, *pairs[2])
    assert [(n, m.shape) for n, m in one] == [(n, m.shape) for n, m in res[2]]
