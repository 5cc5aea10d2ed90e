"""Parity of the HIP engine (through the C ABI) against the CPU oracle and the reference-generated golden vectors.
Runs on the GPU box: pytest -m gpu.

Tolerances: index path bit-exact; fp32 values within 1e-4 relative (max-norm per tensor), the bar BASELINE.json's
north_star states for the mel reconstruction, applied here to outputs, losses, gradients and updated weights.

ReLU kink note: a GroupNorm output that lands within fp32 rounding (~1e-6) of 0 can take the other ReLU branch
than the oracle's (any two fp32 implementations disagree there), which moves the gradients of that channel and of
the conv layers below it in the same stream by O(1/T).  At B*T*C ~ 1e6 pre-activations such an element exists in
roughly every other case.  Element-wise gradient tests therefore (a) run on a small shape with seeded inputs whose
closest pre-activation is >= 1e-5 from the kink (the oracle reports the margin), and (b) at larger shapes hold every
tensor to 1e-4 except conv-trunk tensors at or below a layer where the oracle reports an ambiguous element.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import interp_np, ref_model, weights as W
from oracle.gen_fixtures import draws_for, load_train_rec, synth_batch, train_len_lo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = 1e-4


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


_ENGINES = {}


def get_engine(E, kind, T, B=8):
    key = (kind, T)
    if key not in _ENGINES or _ENGINES[key].max_batch < B:
        _ENGINES[key] = E.Engine(kind, W.default_hparams(max_len_pad=T), B, T)
    return _ENGINES[key]


def stack_draws(draws):
    return np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])


def kink_margins(P, hp, mel, f0, emb, lens, draws):
    ref_model.TAP = {}
    with torch.no_grad():
        ref_model.g3_loss(P, hp, mel, f0, emb, lens.numpy(), draws)
    tap, ref_model.TAP = ref_model.TAP, None
    return {k[5:]: v for k, v in tap.items() if k.startswith('zmin:')}


def kink_safe_case(hp, weights, B, T, first_seed, tries=100, margin=1e-5):
    """Seeded batch + draws whose GroupNorm outputs all keep >= margin distance from the ReLU kink in the oracle."""
    P = ref_model.as_params(weights, False)
    for seed in range(first_seed, first_seed + tries):
        mel, f0, emb, lens = synth_batch(seed, B, T, 64 if T <= 128 else 96)
        draws = draws_for(seed + 100, B, 4)
        if min(kink_margins(P, hp, mel, f0, emb, lens, draws).values()) >= margin:
            return mel, f0, emb, lens, draws
    raise AssertionError('no kink-safe seed found')


def grad_tolerances(names, margins, loose=3e-2, margin=1e-5):
    """Per-parameter tolerance: TOL everywhere, `loose` only for conv-trunk tensors at or below an ambiguous layer."""
    tol = {}
    for n in names:
        t = TOL
        for stream, pre in (('c1', 'encoder_1.convolutions_1.'), ('c2', 'encoder_1.convolutions_2.')):
            if n.startswith(pre):
                layer = int(n[len(pre)])
                if any(margins.get(f'enc1.{stream}_{i}.conv', 1.0) < margin for i in range(layer, 3)):
                    t = loose
        if n.startswith('encoder_2.convolutions.') and margins.get('enc2.c.conv', 1.0) < margin:
            t = loose
        tol[n] = t
    return tol


# --------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('shape', [(128, 128, 64), (256, 512, 400), (100, 80, 164), (333, 257, 66), (1024, 512, 2560)])
@pytest.mark.parametrize('layout', [(False, False), (False, True), (True, True)])
def test_gemm_layouts(E, shape, layout):
    M, N, K = shape
    ta, tb = layout
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    Bm = torch.randn((K, N) if tb else (N, K), generator=g)
    bias = torch.randn(N, generator=g)
    ref = (A.t() if ta else A).double() @ (Bm if tb else Bm.t()).double() + bias.double()
    for ks in (1, 4):
        c = E.gemm(A.cuda(), Bm.cuda(), bias.cuda(), ta, tb, ks)
        assert rel(c, ref) < 5e-6, (shape, layout, ks)


def test_interp_bit_exact_against_reference(E):
    z = np.load(os.path.join(GOLD, 'interp.npz'))
    for i in range(int(z['n'])):
        pad = int(z[f'c{i}_max_len_pad'])
        eng = get_engine(E, 'interp', pad, 16)
        x = torch.from_numpy(z[f'c{i}_x'])
        y, i0, lam, cnt = eng.interp_forward(x, z[f'c{i}_len_seq'], z[f'c{i}_scales'], z[f'c{i}_len_seg'], want_plan=True)
        ri0, rlam, rcnt, rn = interp_np.interp_plan(z[f'c{i}_scales'], z[f'c{i}_len_seg'], z[f'c{i}_len_seq'], max_len_pad=pad)
        assert np.array_equal(y.cpu().numpy(), z[f'c{i}_y']), i            # values: bit-exact vs the reference's output
        assert np.array_equal(i0.cpu().numpy(), ri0) and np.array_equal(cnt.cpu().numpy(), rcnt)
        assert np.array_equal(lam.cpu().numpy(), rlam)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(i))
        dx = eng.interp_backward(dy, x.shape[1])
        assert rel(dx, interp_np.interp_backward(dy.numpy(), ri0, rlam, rn, x.shape[1])) < 1e-6


def test_interp_module_autograd(E):
    from speechsplit_amd import model
    hp = W.default_hparams(max_len_pad=128)
    m = model.InterpLnr(hp).train()
    x = torch.randn(3, 128, 20, device='cuda', requires_grad=True)
    lens = torch.tensor([128, 100, 64])
    sc, ls = draws_for(5, 3, 1)[0]
    y = m(x, lens, draws=(sc, ls))
    ref = interp_np.interp_forward(x.detach().cpu().numpy(), lens.numpy(), sc, ls, max_len_pad=128)
    assert np.array_equal(y.detach().cpu().numpy(), ref)
    (y * y).sum().backward()
    i0, lam, _, nrows = interp_np.interp_plan(sc, ls, lens.numpy(), max_len_pad=128)
    assert rel(x.grad, interp_np.interp_backward(2 * ref, i0, lam, nrows, 128)) < 1e-6
    assert m.eval()(x, lens) is x                                         # model.py:382-383


# --------------------------------------------------------------------------------------------- config 1 (demo.pkl)
def test_config1_demo_eval_forward(E):
    z = np.load(os.path.join(GOLD, 'demo_config1.npz'))
    hp = W.default_hparams()
    e3, e6 = get_engine(E, 'G3', 192), get_engine(E, 'G6', 192)
    e3.load_weights(W.make_weights('G3', hp, int(z['seed_g3'])))
    e6.load_weights(W.make_weights('G6', hp, int(z['seed_g6'])))
    for n in range(2):
        mel = torch.from_numpy(z[f'u{n}_mel_pad'])
        onehot = torch.from_numpy(interp_np.onehot(z[f'u{n}_qidx'].astype(np.int64)))[None]
        emb = torch.from_numpy(z[f'u{n}_emb'])
        out3 = e3.g3_forward(torch.cat((mel, onehot), -1), mel, emb)
        assert rel(out3, z[f'u{n}_out3']) < TOL
        assert rel(e3.g3_rhythm(mel), z[f'u{n}_rhythm']) < TOL
        assert rel(e6.g6_forward(mel, onehot), z[f'u{n}_out6']) < TOL


def test_demo_conversion_seven_conditions(E):
    """demo.ipynb cell 0 through the drop-in modules: Generator_6 F0 conversion (argmax classes identical to the reference's)
    and the seven conversion conditions as one batch-7 forward, against the reference's seven batch-1 outputs."""
    from speechsplit_amd import convert, model
    z, c = np.load(os.path.join(GOLD, 'demo_config1.npz')), np.load(os.path.join(GOLD, 'demo_conversion.npz'))
    hp = W.default_hparams()
    G, P = model.Generator_3(hp).eval(), model.Generator_6(hp).eval()
    G.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_weights('G3', hp, int(z['seed_g3'])).items()}, strict=False)
    P.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_weights('G6', hp, int(z['seed_g6'])).items()}, strict=False)
    G, P = G.to('cuda:0'), P.to('cuda:0')
    ent = []
    for n in range(2):
        L = int(z[f'u{n}_len'])
        ent.append([f'p{n}', z[f'u{n}_emb'], (z[f'u{n}_mel_pad'][0, :L], z[f'u{n}_f0_pad'][:L], L, f'utt{n}')])
    x_org = torch.from_numpy(z['u0_mel_pad']).cuda()
    oh_trg = torch.from_numpy(interp_np.onehot(z['u1_qidx'].astype(np.int64)))[None].cuda()
    _, idx = convert.convert_f0(P, x_org, oh_trg)
    assert np.array_equal(idx.cpu().numpy(), c['f0_pred_idx'].astype(np.int64))
    res = convert.demo_conversion(G, P, ent[0], ent[1])
    assert [r[0] for r in res] == [f'p0_p1_utt0_{cond}' for cond in convert.CONDITIONS]
    for (name, mel), cond in zip(res, convert.CONDITIONS):
        assert mel.shape == c[f'out_{cond}'].shape
        assert rel(mel, c[f'out_{cond}']) < TOL, cond


def test_device_batcher_equals_host_collator(E):
    """batches assembled on the GPU from an HBM-resident corpus (ss_collate) are bit-identical to the host
    collator's (reference data_loader.py:101-128 semantics) under the same generator state, incl. utterances shorter than
    the drawn crop."""
    from speechsplit_amd import data_loader as DL, hparams as HPM
    hp = HPM.default_hparams(batch_size=12)
    ds = DL.SyntheticUtterances(40, seed=3)
    ds.items[5] = (ds.items[5][0][:70], ds.items[5][1], ds.items[5][2][:70])      # shorter than most crops
    ds.items[9] = (ds.items[9][0][:64] * 3 - 1, ds.items[9][1], ds.items[9][2][:64])   # values outside [0,1]: clip
    corpus = DL.DeviceCorpus(ds, 'cuda')
    batcher = DL.DeviceBatcher(hp, corpus)
    coll = DL.MyCollator(hp)
    for trial, idx in enumerate(([5, 9, 0, 1, 2, 3, 4, 6, 7, 8, 10, 11], [39, 5, 5, 9, 20, 21, 22, 23, 24, 25, 26, 27])):
        np.random.seed(100 + trial)
        host = coll([ds[i] for i in idx])
        np.random.seed(100 + trial)
        dev = batcher.assemble(idx)
        for h, d in zip(host, dev):
            assert h.shape == d.shape and h.dtype == d.dtype
            assert torch.equal(h, d.cpu())
    np.random.seed(7)
    n = sum(1 for _ in batcher)
    assert n == len(batcher) == len(ds) * hp.samplier // hp.batch_size


def test_device_batcher_against_reference_collator_fixture(E):
    """The batch ss_collate assembles from the HBM-resident corpus equals the REFERENCE collator's batch (tests/golden/collate.npz)
    for the same items under the same numpy seed."""
    from speechsplit_amd import data_loader as DL, hparams as HPM
    z = np.load(os.path.join(GOLD, 'collate.npz'))
    ds = DL.SyntheticUtterances(int(z['corpus_n']), seed=int(z['corpus_seed']))
    batcher = DL.DeviceBatcher(HPM.default_hparams(batch_size=6), DL.DeviceCorpus(ds, 'cuda'))
    np.random.seed(int(z['np_seed']))
    mel, emb, f0, ln = batcher.assemble([int(i) for i in z['items']])
    assert np.array_equal(mel.cpu().numpy(), z['mel']) and np.array_equal(emb.cpu().numpy(), z['emb'])
    assert np.array_equal(f0.cpu().numpy(), z['f0']) and np.array_equal(ln.cpu().numpy(), z['len_org'])


def test_mel_spectrogram_and_f0_normalisation_against_reference_fixture(E):
    """SURVEY.md section 8(f) row N4, device half (csrc/features.hip): STFT magnitude -> mel -> dB -> [0, 1] scaling and the F0
    normalisation against what the REFERENCE's pySTFT / speaker_normalization produced (tests/golden/features.npz).  float64
    arithmetic on both sides, float32 results: agreement to float32 rounding (stated: 2e-6 absolute on values of order 1)."""
    from speechsplit_amd import features as F
    z = np.load(os.path.join(GOLD, 'features.npz'))
    for u in range(2):
        S = F.melspectrogram(z[f'u{u}_wav'], z['mel_basis']).cpu().numpy()
        assert S.shape == z[f'u{u}_S'].shape and S.dtype == np.float32
        assert float(np.abs(S - z[f'u{u}_S']).max()) <= 2e-6, u
        fn = F.normalize_f0(z[f'u{u}_f0']).cpu().numpy()
        ref = z[f'u{u}_f0norm']
        assert np.array_equal(fn == -1e10, ref == -1e10)
        assert float(np.abs(fn - ref)[ref != -1e10].max()) <= 2e-7, u


def test_eval_forward_ragged_batch(E):
    """B not a multiple of the 16-utterance LSTM tile, T below max_len_pad (eval works at any T % 8 == 0)."""
    hp = W.default_hparams()
    w = W.make_weights('G3', hp, 5)
    eng = get_engine(E, 'G3', 192)
    eng.load_weights(w)
    P = ref_model.as_params(w, False)
    g = torch.Generator().manual_seed(3)
    B, T = 3, 64
    mel = torch.rand(B, T, 80, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 257, (B, T), generator=g), 257).float()
    emb = torch.nn.functional.one_hot(torch.tensor([1, 5, 80]), 82).float()
    x_f0 = torch.cat((mel, onehot), -1)
    with torch.no_grad():
        ref = ref_model.generator_3(P, hp, x_f0, mel, emb)
    assert rel(eng.g3_forward(x_f0, mel, emb), ref) < TOL
    # the ablation inputs of solver.py:245-251: zeroed pitch / zeroed content are not one-hot rows
    x0 = torch.cat((mel, torch.zeros_like(onehot)), -1)
    with torch.no_grad():
        ref0 = ref_model.generator_3(P, hp, x0, mel, emb)
    assert rel(eng.g3_forward(x0, mel, emb), ref0) < TOL


# --------------------------------------------------------------------------------------------- module-level boundary (B1)
def test_module_train_step_with_torch_adam(E):
    """Reference-style usage (solver.py:57-66, 157-172): optimizer built before .to(device), G.train(), G(...),
    mse_loss, backward, Adam.step -- compared with the oracle doing the same on CPU."""
    from speechsplit_amd import model
    B, T = 2, 64                    # small on purpose (kink note above); max_len_pad=64 also exercises the truncation
    hp = W.default_hparams(max_len_pad=T, batch_size=B)
    w = W.make_weights('G3', hp, 3)
    mel, f0, emb, lens, draws = kink_safe_case(hp, w, B, T, 41)
    G = model.Generator_3(hp)
    G.load_state_dict({**{k: torch.from_numpy(v) for k, v in w.items()}, 'encoder_1.len_org': torch.tensor(T)})
    opt = torch.optim.Adam(G.parameters(), 1e-4, [0.9, 0.999])
    G.to('cuda:0')
    assert G.train() is G
    st = ref_model.TrainState(w)
    xi = ref_model.interp(torch.cat((mel, f0), -1), lens.numpy(), draws[0], hp)
    onehot, _ = ref_model.quantize_f0(xi[:, :, -1])
    x_in = torch.cat((xi[:, :, :-1], onehot), -1)
    out = G(x_in.cuda(), mel.cuda(), emb.cuda(), draws=stack_draws(draws[1:4]))
    loss = torch.nn.functional.mse_loss(mel.cuda(), out, reduction='mean')
    opt.zero_grad()
    loss.backward()
    lo, ro = st.step_g3(hp, mel, f0, emb, lens.numpy(), draws)       # oracle: loss, backward, Adam
    assert rel(out, ro) < TOL and abs(float(loss) - float(lo)) < 1e-5 * float(lo)
    for n, p in G.named_parameters():
        assert rel(p.grad, st.P[n].grad) < TOL, n
    opt.step()
    for n, p in G.named_parameters():
        assert rel(p, st.P[n]) < TOL, n
    sd = G.state_dict()
    assert list(sd.keys())[0] == 'encoder_1.len_org' and sd['decoder.lstm.weight_hh_l2_reverse'].shape == (2048, 512)
    # eval mode: identity resampling, no draws needed
    with torch.no_grad():
        oe = G.eval()(x_in.cuda(), mel.cuda(), emb.cuda())
        re_ = ref_model.generator_3(st.P, hp, x_in, mel, emb)
    assert rel(oe, re_) < TOL


# --------------------------------------------------------------------------------------------- fused training step (B2)
def test_gemm_bf16_mode(E):
    """GEMM_BF16: operands rounded to bf16 (nearest-even) inside the kernel, fp32 accumulation.  Against an fp64 product of
    the bf16-rounded operands the result is fp32-accurate; against the fp32 product it shows bf16's ~2e-3."""
    g = torch.Generator().manual_seed(5)
    for M, N, K, ta, tb in [(256, 512, 400, False, False), (384, 256, 1024, False, True), (1024, 512, 2560, True, True)]:
        A = torch.randn((K, M) if ta else (M, K), generator=g)
        Bm = torch.randn((K, N) if tb else (N, K), generator=g)
        Ab, Bb = A.bfloat16().double(), Bm.bfloat16().double()
        ref = (Ab.t() if ta else Ab) @ (Bb if tb else Bb.t())
        ref32 = (A.t() if ta else A).double() @ (Bm if tb else Bm.t()).double()
        for ks in (1, 4):
            c = E.gemm(A.cuda(), Bm.cuda(), None, ta, tb, ks, bf16=True)
            assert rel(c, ref) < 5e-6, (M, N, K, ta, tb, ks)
            assert 1e-4 < rel(c, ref32) < 1e-2


def test_gemm_fp16x2_mode(E):
    """GEMM_F16X2 (forward contractions, and gradient contractions with a measured scale): fp16 x 2 split, 3 MFMAs, fp32
    accumulation.  fp32-grade against fp64 also when one reduction mixes magnitudes from 2e-8 to 250."""
    g = torch.Generator().manual_seed(6)
    for M, N, K, ta, tb in [(256, 512, 400, False, False), (384, 256, 1024, False, True), (1024, 512, 2560, True, True)]:
        A = torch.randn((K, M) if ta else (M, K), generator=g)
        Bm = torch.randn((K, N) if tb else (N, K), generator=g) * 0.05
        A.view(-1)[:7] = torch.tensor([1e-3, 3e-5, 1e-6, 2e-8, 100.0, -250.0, 0.0])
        ref = (A.t() if ta else A).double() @ (Bm if tb else Bm.t()).double()
        for ks in (1, 4):
            c = E.gemm(A.cuda(), Bm.cuda(), None, ta, tb, ks, f16x2=True)
            assert rel(c, ref) < 5e-6, (M, N, K, ta, tb, ks)


def test_gradient_scale_invariance_of_fp16x2(E):
    """The gradient GEMMs scale their gradient operand by the power of two measured by the producing kernel, so the size of
    the incoming gradient must not matter: backward of d_out * 2^-30 and of d_out * 2^20, divided back, equals backward of d_out
    (a fixed fp16 scale would flush the first to zero and overflow the second)."""
    B, T = 4, 192
    hp = W.default_hparams(max_len_pad=T)
    eng = get_engine(E, 'G3', T, 8)
    eng.load_weights(W.make_weights('G3', hp, 2))
    mel, f0, emb, lens = synth_batch(19, B, T, 96)
    onehot = torch.from_numpy(interp_np.onehot(interp_np.quantize_f0(f0[:, :, 0].numpy())))
    x_f0 = torch.cat((mel, onehot), -1)
    draws = stack_draws(draws_for(20, B, 3))
    d_out = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(3))
    got = {}
    for gs in (1.0, 2.0 ** -30, 2.0 ** 20):
        eng.g3_forward(x_f0, mel, emb, draws, training=True)
        eng.g3_backward(d_out * gs)
        got[gs] = {n: v.double().cpu() / gs for n, v in eng.grad_views().items()}
    eng.check()
    for gs in (2.0 ** -30, 2.0 ** 20):
        for n, v in got[1.0].items():
            assert torch.isfinite(got[gs][n]).all(), (gs, n)
            assert rel(got[gs][n], v) < 1e-5, (gs, n)


def test_bf16_precision_train_step(E):
    """BASELINE configs 2-4 name bf16.  ss_set_precision(BF16) rounds the operands of every contraction to bf16 (fp32
    accumulate, fp32 storage / recurrent state / GroupNorm / Adam).  Stated bounds against the fp32 reference fixture and
    the fp32 engine: loss 1e-3, mel reconstruction 1e-2, every gradient tensor 1e-1 (max-norm relative); the resampling
    index path stays bit-exact because it never touches the GEMMs."""
    tag = 'b8_t128'
    rec = json.load(open(os.path.join(GOLD, 'train_steps.json')))[tag]
    B, T = rec['B'], rec['T']
    hp = W.default_hparams(max_len_pad=T)
    mel, f0, emb, lens = synth_batch(rec['bseed'], B, T, 64)
    nsteps = len(rec['losses'])
    draws = draws_for(rec['dseed'], B, 4 * nsteps)
    got = {}
    for prec in ('f32', 'bf16'):
        eng = E.Engine('G3', hp, B, T)
        eng.set_precision(prec)
        eng.load_weights(W.make_weights('G3', hp, rec['wseed']))
        eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
        loss = eng.g3_train_step(mel, f0, emb, lens, stack_draws(draws[:4]), no_adam=True)
        got[prec] = dict(loss=float(loss), out=eng.debug_buffer('out', B, T).cpu(), mel=eng.debug_buffer('in.mel', B, T).cpu(),
                         f0=eng.debug_buffer('in.f0', B, T).cpu(), grads={n: v.clone().cpu() for n, v in eng.grad_views().items()})
        eng.adam_step()
        losses = [float(loss)]
        for it in range(1, nsteps):
            losses.append(float(eng.g3_train_step(mel, f0, emb, lens, stack_draws(draws[4 * it:4 * it + 4]))))
        got[prec]['losses'] = losses
        eng.check()
    b = got['bf16']
    for it in range(nsteps):
        assert abs(b['losses'][it] - rec['losses'][it]) <= 1e-3 * rec['losses'][it], (it, b['losses'])
    assert rel(b['out'], np.load(os.path.join(GOLD, f'train_{tag}_out.npy'))) < 1e-2
    assert np.array_equal(b['mel'].numpy(), np.load(os.path.join(GOLD, f'train_{tag}_xin_mel.npy')))        # bit-exact
    assert torch.equal(b['f0'], got['f32']['f0'])
    worst = max(rel(b['grads'][n], got['f32']['grads'][n]) for n in b['grads'])
    assert 1e-4 < worst < 1e-1, worst        # really a different arithmetic, and within the stated bound


@pytest.mark.parametrize('tag', ['b2_t128', 'b2_t192', 'b8_t128', 'b2_t256', 'b2_t8'])
def test_fused_train_step_against_reference_fixture(E, tag):
    rec = load_train_rec(tag, GOLD)
    B, T = rec['B'], rec['T']
    hp = W.default_hparams(max_len_pad=T)
    eng = get_engine(E, 'G3', T, B)
    eng.load_weights(W.make_weights('G3', hp, rec['wseed']))
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
    mel, f0, emb, lens = synth_batch(rec['bseed'], B, T, train_len_lo(T))
    nsteps = len(rec['losses'])
    draws = draws_for(rec['dseed'], B, 4 * nsteps)
    for it in range(nsteps):
        loss = eng.g3_train_step(mel, f0, emb, lens, stack_draws(draws[4 * it:4 * it + 4]))
        assert abs(float(loss) - rec['losses'][it]) <= 2e-5 * rec['losses'][it], (it, float(loss))
        if it == 0:
            out = eng.debug_buffer('out', B, T)
            assert rel(out, np.load(os.path.join(GOLD, f'train_{tag}_out.npy'))) < TOL
            # index path and resampled values of the outer InterpLnr call: bit-exact
            assert np.array_equal(eng.debug_buffer('in.mel', B, T).cpu().numpy(), np.load(os.path.join(GOLD, f'train_{tag}_xin_mel.npy')))
            cls = eng.debug_buffer('in.f0', B, T)[:, :, :257].argmax(-1).cpu().numpy()
            assert np.array_equal(cls, np.load(os.path.join(GOLD, f'train_{tag}_xin_f0idx.npy')).astype(np.int64))
            pv = eng.param_views()
            for n, s in rec['params_after'].items():
                flat = pv[n].reshape(-1).cpu()
                for p, v in zip(s['pos'], s['val']):
                    assert abs(float(flat[p]) - v) <= TOL * s['amax'] + 1e-9, (n, p)


@pytest.mark.parametrize('case', [(2, 64, 9, 46, True, 1), (4, 128, 9, 61, False, 1), (5, 192, 4, 70, False, 1),
                                  (4, 128, 9, 61, False, 0), (3, 64, 9, 46, False, 0), (1, 128, 5, 33, False, 1), (17, 64, 2, 80, False, 1)])
def test_fused_train_step_full_gradients(E, case):
    """Every element of all 86 gradients against the oracle's autograd.  The last field selects the decoder recurrence
    schedule: 1 = persistent kernels (default), 0 = one launch per time step.  (Round 2's third schedule -- the per-step launches
    captured in a hipGraph -- left the product library in round 3 and the source in round 4: no gain, and a crash inside the
    runtime's graph launch.)"""
    B, T, wseed, bseed, want_safe, sched = case
    E.tune('persist', 1 if sched == 1 else 0)
    try:
        _full_gradients(E, B, T, wseed, bseed, want_safe)
    finally:
        E.tune('persist', 1)
    with pytest.raises(RuntimeError, match='unknown key'):
        E.tune('graph', 1)


def _full_gradients(E, B, T, wseed, bseed, want_safe):
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G3', hp, wseed)
    if want_safe:
        mel, f0, emb, lens, draws = kink_safe_case(hp, w, B, T, bseed)
    else:
        mel, f0, emb, lens = synth_batch(bseed, B, T, 64 if T <= 128 else 96)
        draws = draws_for(bseed + 100, B, 4)
    eng = get_engine(E, 'G3', T, max(8, B))
    eng.load_weights(w)
    loss = eng.g3_train_step(mel, f0, emb, lens, stack_draws(draws), no_adam=True)
    eng.check()                       # no persistent kernel gave up
    P = ref_model.as_params(w)
    margins = kink_margins(P, hp, mel, f0, emb, lens, draws)
    lo, _ = ref_model.g3_loss(P, hp, mel, f0, emb, lens.numpy(), draws)
    lo.backward()
    assert abs(float(loss) - float(lo)) <= 1e-5 * float(lo)
    gv = eng.grad_views()
    tol = grad_tolerances(list(P), margins)
    if want_safe:
        assert all(t == TOL for t in tol.values())
    for n, p in P.items():
        assert rel(gv[n], p.grad) < tol[n], (n, tol[n])


@pytest.mark.parametrize('knob', ['small_lds', 'defer_dw', 'dx_batched', 'gemm_tr=2', 'gemm_tr=0'])
def test_schedule_knobs_do_not_change_gradients(E, knob):
    """The LDS-staged small recurrences vs. the streaming fallback, the deferred vs. co-scheduled decoder weight
    gradients, the per-utterance vs. whole-slab input-gradient GEMMs and the two LDS images of reduction-major GEMM
    operands (transposing reads not for TN / nowhere; default: everywhere) are alternative schedules of the same arithmetic: the oracle parity of the variant that is off by default must hold as well."""
    name, _, val = knob.partition('=')
    E.tune(name, int(val or 0))
    try:
        _full_gradients(E, 4, 128, 9, 61, False)
    finally:
        E.tune(name, 2 if name == 'dx_batched' else 1)


def test_g6_train_step(E):
    rec = json.load(open(os.path.join(GOLD, 'g6_train.json')))
    B, T = rec['B'], rec['T']
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights('G6', hp, rec['wseed'])
    eng = get_engine(E, 'G6', T)
    eng.load_weights(w)
    mel, f0, emb, lens = synth_batch(rec['bseed'], B, T, 96)
    qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
    onehot = torch.nn.functional.one_hot(qidx, 257).float()
    draws = draws_for(rec['dseed'], B, 3)
    out = eng.g6_forward(mel, onehot, stack_draws(draws), training=True)
    assert rel(out, np.load(os.path.join(GOLD, 'g6_train_logits.npy'))) < TOL
    loss = eng.g6_train_step(mel, onehot, qidx, stack_draws(draws), no_adam=True)
    assert abs(float(loss) - rec['loss']) <= 1e-5 * rec['loss']
    gv = eng.grad_views()
    for n, s in rec['grads'].items():
        assert abs(float(gv[n].double().norm()) - s['l2']) <= 2e-4 * s['l2'] + 1e-12, n


# --------------------------------------------------------------------------------------------- full size (B=64, T=128): properties
def test_full_size_data_parallel_linearity_and_descent(E):
    """BASELINE config at full size, where the oracle is too slow to be the checker: (1) the gradient of the
    64-utterance batch equals the mean of the gradients of its two 32-utterance shards given the matching slices of
    the draws (the N-rank == 1-rank identity data parallelism relies on); (2) identical draws -> bit-identical
    resampled inputs; (3) a few Adam steps on a fixed batch reduce the loss."""
    from speechsplit_amd import dist as D
    B, T = 64, 128
    hp = W.default_hparams(max_len_pad=T)
    eng = get_engine(E, 'G3', T, B)
    w = W.make_weights('G3', hp, 0)
    eng.load_weights(w)
    mel, f0, emb, lens = synth_batch(7, B, T, 64)
    sc, ls = stack_draws(draws_for(8, B, 4))
    sc, ls = torch.from_numpy(sc), torch.from_numpy(ls)
    l_full = float(eng.g3_train_step(mel, f0, emb, lens, (sc, ls), no_adam=True))
    g_full = eng.grads.clone()
    xin = eng.debug_buffer('in.mel', B, T)
    acc = torch.zeros_like(g_full)
    l_sh = 0.0
    for r in range(2):
        b = D.shard_batch((mel, emb, f0, lens), r, 2)
        d = D.shard_draws(sc, ls, B, r, 2)
        l_sh += float(eng.g3_train_step(b[0], b[2], b[1], b[3], d, no_adam=True)) / 2
        acc += eng.grads / 2
        lo, hi = D.shard_range(B, r, 2)
        assert torch.equal(eng.debug_buffer('in.mel', B // 2, T), xin[lo:hi])
    assert abs(l_sh - l_full) <= 1e-5 * l_full
    gv_f, gv_s = eng.views(g_full), eng.views(acc)
    for n in gv_f:
        assert rel(gv_s[n], gv_f[n]) < TOL, n
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
    losses = [float(eng.g3_train_step(mel, f0, emb, lens, (sc, ls))) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def _shard_linearity(E, kind, B, T, len_lo, parts, wseed=0, bseed=11, descent=True, precision='f32', tol=TOL):
    """Gradient of a B-utterance batch == mean of the gradients of its `parts` equal shards given the matching draw slices,
    and a few Adam steps on the fixed batch reduce the loss.  The shards may run a different recurrence schedule than the
    whole batch (persistent kernels, XCD-local or not, or one launch per time step), which this cross-checks at full size."""
    from speechsplit_amd import dist as D
    hp = W.default_hparams(max_len_pad=T)
    eng = E.Engine(kind, hp, B, T)
    eng.set_precision(precision)
    eng.load_weights(W.make_weights(kind, hp, wseed))
    mel, f0, emb, lens = synth_batch(bseed, B, T, len_lo)
    ncalls = 4 if kind == 'G3' else 3
    sc, ls = stack_draws(draws_for(bseed + 1, B, ncalls))
    sc, ls = torch.from_numpy(sc), torch.from_numpy(ls)
    if kind == 'G6':
        qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
        onehot = torch.nn.functional.one_hot(qidx, 257).float()

    def step(lo, hi, draws, **kw):
        if kind == 'G3':
            return eng.g3_train_step(mel[lo:hi], f0[lo:hi], emb[lo:hi], lens[lo:hi], draws, **kw)
        return eng.g6_train_step(mel[lo:hi], onehot[lo:hi], qidx[lo:hi], draws, **kw)

    l_full = float(step(0, B, (sc, ls), no_adam=True))
    g_full = eng.grads.clone()
    eng.check()
    acc = torch.zeros_like(g_full)
    l_sh = 0.0
    for r in range(parts):
        lo, hi = D.shard_range(B, r, parts)
        l_sh += float(step(lo, hi, D.shard_draws(sc, ls, B, r, parts), no_adam=True)) / parts
        acc += eng.grads / parts
    eng.check()
    assert abs(l_sh - l_full) <= 1e-5 * abs(l_full), (l_sh, l_full)
    gv_f, gv_s = eng.views(g_full), eng.views(acc)
    for n in gv_f:
        assert rel(gv_s[n], gv_f[n]) < tol, n
    if descent:
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.set_adam(1e-3, 0.9, 0.999, 1e-8, 0)
        losses = [float(step(0, B, (sc, ls))) for _ in range(5)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_full_size_generator6_config(E):
    """BASELINE config 3's per-GPU shape: Generator_6 (Encoder_6 pitch path, CE loss), 32 utterances x 192 frames.
    The whole batch runs the H=256 persistent recurrences with 4 groups (spanning XCDs: write-through hand-off), the two
    16-utterance shards with 2 groups."""
    _shard_linearity(E, 'G6', 32, 192, 96, 2)


def test_full_size_192_frames(E):
    """BASELINE config 4's frame count: Generator_3, 64 utterances x 192 frames, lengths 96..192 (padded, as the
    reference does); shards of 32 run the persistent recurrences with groups that span XCDs."""
    _shard_linearity(E, 'G3', 64, 192, 96, 2)


@pytest.mark.parametrize('case', [('G3', 64, 128, 64), ('G6', 64, 192, 96)], ids=['config3_g3_2x32x128', 'config4_g6_2x32x192'])
def test_bf16_configs_data_parallel_linearity(E, case):
    """BASELINE configs 3 and 4 name bf16 arithmetic at 32 utterances per GPU: in the bf16 product mode the gradient of a 64-utterance
    batch equals the mean of its two 32-utterance shards' gradients given the matching draw slices (the N-rank == 1-rank identity; operand
    rounding is per element, so the summation order differs -- and, for the 64-utterance Generator_3 batch, the last bit of the hidden
    state's fp16 x 2 pieces, which carries the step tag of the forward hand-off only when every group sits on one XCD; a bf16 rounding
    that flips on that bit moves a small-gradient tensor by a few 1e-4), and a few Adam steps reduce the loss."""
    kind, B, T, len_lo = case
    _shard_linearity(E, kind, B, T, len_lo, 2, wseed=0 if kind == 'G3' else 4, precision='bf16', tol=1e-3)


@pytest.mark.parametrize('case', [(64, 128, 512, 1), (50, 37, 512, 1), (16, 8, 512, 1), (33, 5, 256, 1), (64, 3, 256, 1), (7, 1, 256, 1), (64, 40, 512, 0)],
                         ids=['b64_t128_h512_tagged_both', 'b50_t37_h512_partial_tile', 'b16_t8_h512_one_group_pair', 'b33_t5_h256', 'b64_t3_h256',
                              'b7_t1_h256_single_step', 'b64_t40_h512_flag_forward'])
def test_persistent_blstm_layer_against_torch(E, case):
    """One decoder-sized BLSTM layer through the persistent recurrence kernels (tagged hand-off, memory waves, LDS-DMA operand ring:
    sequences shorter than the ring, odd lengths, a batch tile that is not full, groups on one XCD and across XCDs, and the forward's
    flag-line form) against torch.nn.LSTM in float64: output, input gradient and every weight / bias gradient."""
    B, T, H, tag = case
    E.tune('seq_tag', tag)
    try:
        In = 96
        g = torch.Generator().manual_seed(100 + B + T)
        ref = torch.nn.LSTM(In, H, 1, batch_first=True, bidirectional=True).double()
        x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
        d_out = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64) * 0.1
        xr = x.clone().requires_grad_(True)
        y_ref, _ = ref(xr)
        y_ref.backward(d_out)
        f = lambda n: getattr(ref, n).detach().float().cuda()
        y, dx, grads = E.blstm_layer(x.float().cuda(), (f('weight_ih_l0'), f('weight_ih_l0_reverse')), (f('weight_hh_l0'), f('weight_hh_l0_reverse')),
                                     (f('bias_ih_l0'), f('bias_ih_l0_reverse')), (f('bias_hh_l0'), f('bias_hh_l0_reverse')), d_out.float().cuda())
        assert rel(y, y_ref.detach()) < TOL
        assert rel(dx, xr.grad) < TOL
        for d, sfx in enumerate(('', '_reverse')):
            gw_ih, gw_hh, gb = grads[d]
            assert rel(gw_ih, getattr(ref, 'weight_ih_l0' + sfx).grad) < TOL, sfx
            assert rel(gw_hh, getattr(ref, 'weight_hh_l0' + sfx).grad) < TOL, sfx
            assert rel(gb, getattr(ref, 'bias_ih_l0' + sfx).grad) < TOL, sfx
    finally:
        E.tune('seq_tag', 1)


@pytest.mark.parametrize('shape', [(64, 128, 512), (33, 19, 256)], ids=['b64_t128_h512', 'b33_t19_h256'])
def test_backward_recurrence_warmup_forms_are_bit_identical(E, shape):
    """The backward recurrence's warm-up reads only move lines into the L2 (ss_tune("seq_var"): 2 one dword per 128-byte line -- the default --,
    4 one per 64 bytes, 0 whole 1 KB runs): whichever form runs, every result of the layer is the same bit for bit."""
    B, T, H = shape
    In = 64
    g = torch.Generator().manual_seed(7 + B)
    x = torch.randn(B, T, In, generator=g).cuda()
    d_out = (torch.randn(B, T, 2 * H, generator=g) * 0.1).cuda()
    w = lambda *sz: ((torch.rand(*sz, generator=g) * 2 - 1) / H ** 0.5).cuda()
    wih, whh = (w(4 * H, In), w(4 * H, In)), (w(4 * H, H), w(4 * H, H))
    bih, bhh = (w(4 * H), w(4 * H)), (w(4 * H), w(4 * H))
    res = {}
    try:
        for form in (2, 0, 4):
            E.tune('seq_var', form)
            y, dx, grads = E.blstm_layer(x, wih, whh, bih, bhh, d_out)
            res[form] = [y.clone(), dx.clone()] + [t.clone() for d in grads for t in d]
    finally:
        E.tune('seq_var', 2)
    for form in (0, 4):
        for a, b in zip(res[2], res[form]):
            assert torch.equal(a, b), form


def test_batch_beyond_one_workgroup_per_cu(E):
    """128 utterances per GPU do not fit the persistent recurrence (one workgroup per CU): the decoder falls back to one
    launch per time step.  Its gradients must equal the mean over two 64-utterance shards, which run the persistent kernels."""
    _shard_linearity(E, 'G3', 128, 128, 64, 2, descent=False)


def test_solver_trains_and_checkpoints(E, tmp_path):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver
    hp = HP.default_hparams(batch_size=4, max_len_pad=128)
    np.random.seed(0)
    torch.manual_seed(0)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = SimpleNamespace(num_iters=3, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False,
                          device_id=0, log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path),
                          log_step=1, sample_step=1000, model_save_step=3)
    s = solver.Solver(loader, cfg, hp)
    s.train()
    ck = torch.load(os.path.join(str(tmp_path), '3-G.ckpt'), weights_only=False)
    ref_keys = json.load(open(os.path.join(GOLD, 'keys_G3.json')))['keys']
    assert list(ck['model'].keys()) == ref_keys
    assert len(ck['optimizer']['state']) == 86 and float(ck['optimizer']['state'][0]['step']) == 3.0
    # the optimizer half loads into a stock torch.optim.Adam over the reference's parameter list
    plist = [torch.nn.Parameter(ck['model'][k].clone()) for k in ref_keys if k != 'encoder_1.len_org']
    torch.optim.Adam(plist, 1e-4).load_state_dict(ck['optimizer'])
    cfg2 = SimpleNamespace(**{**vars(cfg), 'resume_iters': 3, 'num_iters': 1})
    s2 = solver.Solver(loader, cfg2, hp)
    s2.restore_model(3)
    assert s2.step_count == 3
    for (n, a), (_, b) in zip(s.G.state_dict().items(), s2.G.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), n
    assert torch.equal(s.eng.adam_v, s2.eng.adam_v)


def test_split_backward_equals_fused(E):
    """SS_STEP_SPLIT_BACKWARD + ss_train_finish (the data-parallel schedule) produces the same gradients as the one-call
    step, and the decoder range is already final when the first call returns."""
    B, T = 4, 128
    hp = W.default_hparams(max_len_pad=T)
    eng = get_engine(E, 'G3', T, 8)
    eng.load_weights(W.make_weights('G3', hp, 2))
    mel, f0, emb, lens = synth_batch(17, B, T, 64)
    d = stack_draws(draws_for(18, B, 4))
    eng.g3_train_step(mel, f0, emb, lens, d, no_adam=True)
    ref = eng.grads.clone()
    eng.g3_train_step(mel, f0, emb, lens, d, no_adam=True, split_backward=True)
    k = eng.grad_split
    names = [n for n, o, s in eng.table if o >= k]
    assert names[0] == 'decoder.lstm.weight_ih_l0' and names[-1].endswith('linear_layer.bias')
    assert rel(eng.grads[k:], ref[k:]) < 1e-5
    assert float(eng.grads[:k].abs().max()) == 0.0            # encoder gradients not produced yet
    eng.train_finish(no_adam=True)
    assert rel(eng.grads[:k], ref[:k]) < 1e-5


def test_dp_step_on_a_one_rank_rccl_group(E):
    """The three data-parallel schedules end to end (two async RCCL all-reduces behind the step / overlapped from a
    communication stream / after a joined split; Adam with the mean folded in) on a world of one: each must equal
    the plain fused step."""
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda:0'))
    try:
        B, T = 4, 128
        hp = W.default_hparams(max_len_pad=T)
        w = W.make_weights('G3', hp, 6)
        mel, f0, emb, lens = synth_batch(27, B, T, 64)
        d = stack_draws(draws_for(28, B, 4))
        res = []
        for dp in (None, 'overlap', 'after', 'join'):
            eng = get_engine(E, 'G3', T, 8)
            eng.load_weights(w)
            eng.adam_m.zero_()
            eng.adam_v.zero_()
            eng.set_adam(1e-4, 0.9, 0.999, 1e-8, 0)
            for _ in range(2):          # two steps: the second one runs on the first one's update
                loss = eng.dp_train_step(mel, f0, emb, lens, d, 1, schedule=dp) if dp else eng.g3_train_step(mel, f0, emb, lens, d)
            torch.cuda.synchronize()
            res.append((float(loss), eng.params.clone()))
        for r in res[1:]:
            assert r[0] == res[0][0]
            assert rel(r[1], res[0][1]) < 1e-6
    finally:
        dist.destroy_process_group()


def test_solver_validation_path_and_prefetcher(E, tmp_path):
    """Solver.validate reproduces solver.py:206-227 on demo.pkl-shaped entries (built from the committed config-1 vectors):
    the sum-reduced MSE equals the one computed from the reference's own outputs; the ablation forwards run."""
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver, staging
    z = np.load(os.path.join(GOLD, 'demo_config1.npz'))
    hp = HP.default_hparams(batch_size=2)
    cfg = SimpleNamespace(num_iters=1, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False, device_id=0,
                          log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path), log_step=1,
                          sample_step=1, model_save_step=100)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(8, seed=3))
    s = solver.Solver(loader, cfg, hp)
    s.G.load_state_dict({**{k: torch.from_numpy(v) for k, v in W.make_weights('G3', hp, int(z['seed_g3'])).items()},
                         'encoder_1.len_org': torch.tensor(192)})
    val = []
    for n in range(2):
        L = int(z[f'u{n}_len'])
        val.append([f'u{n}', z[f'u{n}_emb'], (z[f'u{n}_mel_pad'][0, :L], z[f'u{n}_f0_pad'][:L], L, 'x')])
    loss, outs = s.validate(val, ablations=True)
    ref = np.mean([float(((z[f'u{n}_mel_pad'] - z[f'u{n}_out3']) ** 2).sum()) for n in range(2)])
    assert abs(loss - ref) <= 1e-4 * ref
    for n in range(2):
        assert rel(outs[f'u{n}']['out'], z[f'u{n}_out3']) < TOL
        assert set(outs[f'u{n}']) == {'out', 'woF', 'woR', 'woC'}
    pf = staging.DevicePrefetcher(loader, 'cuda:0')
    mel, emb, f0, ln = next(pf)
    assert mel.is_cuda and mel.shape == (2, 192, 80) and ln.dtype == torch.int64
    s.validation_pt = val
    s.train()                       # one iteration + validation print through the prefetcher


@pytest.fixture
def img_queue(E, request):
    """ss_tune("img_xcc"): 0 = one workgroup per tile; 255 = work-queue form on every XCD; 0xF0 = work-queue form on XCDs 4-7 only (the
    workgroups that land on XCDs 0-3 leave: the form that runs beside a persistent recurrence holding those XCDs)."""
    E.tune('img_xcc', request.param)
    yield request.param
    E.tune('img_xcc', 0)


@pytest.mark.parametrize('img_queue', [0, 255, 0xF0], indirect=True, ids=['grid', 'queue', 'queue_xcd4to7'])
@pytest.mark.parametrize('cfg', [0, 1, 2])
@pytest.mark.parametrize('layout', [(False, False), (False, True), (True, True)])
def test_image_gemm_against_fp64(E, layout, cfg, img_queue):
    """gemm_img.hip (operand images, LDS-DMA ring, deterministic split-K): fp32-grade results against fp64 in every layout and tile
    configuration, with ragged M / N (multiples of 8 / 4 only), K tails of a reduction-major pair, bias, accumulation and split-K --
    as a plain grid and in the work-queue form (all XCDs / half of them)."""
    ta, tb = layout
    g = torch.Generator().manual_seed(11 + cfg)
    shapes = [(264, 200, 96, 1), (1000, 520, 1024, 1), (512, 512, 4096, 4), (2048, 1024, 2112, 8)]
    if ta and tb:
        shapes += [(512, 264, 1027, 3), (256, 256, 8447, 8), (136, 128, 31, 1)]
    for M, N, K, ks in shapes:
        A = torch.randn(M, K, generator=g).cuda()
        Bm = (torch.randn(N, K, generator=g) * 0.05).cuda()
        bias = torch.randn(N, generator=g).cuda()
        c0 = torch.randn(M, N, generator=g).cuda()
        ref = A.double() @ Bm.double().t() + bias.double() + c0.double()
        ai = E.split_image(A.t().contiguous() if ta else A)
        bi = E.split_image(Bm.t().contiguous() if tb else Bm)
        c = E.gemm_img(ai, bi, ta, tb, bias, ks, cfg, out=c0.clone(), accumulate=True)
        assert rel(c, ref) < 5e-6, (M, N, K, ks, layout, cfg)
        # bit-identical on a second run (partial slabs are added in a fixed order)
        c2 = E.gemm_img(ai, bi, ta, tb, bias, ks, cfg, out=c0.clone(), accumulate=True)
        assert torch.equal(c, c2)


def test_image_gemm_conv_windows_and_scales(E):
    """The segmented K axis (a k=5 convolution read as one GEMM over overlapping rows of a haloed slab) and images split with other
    power-of-two scales."""
    g = torch.Generator().manual_seed(5)
    B, T, Ci, Co = 3, 40, 64, 128
    TP = T + 4
    x = torch.zeros(B, TP, Ci)
    x[:, 2:2 + T] = torch.randn(B, T, Ci, generator=g)
    w = torch.randn(Co, 5, Ci, generator=g) * 0.05                 # [Co][tap][ci]: K-contiguous pack
    xs = x.reshape(B * TP, Ci).cuda()
    rows = B * TP - 4
    ref = torch.zeros(rows, Co, dtype=torch.float64)
    for tap in range(5):
        ref += xs[tap:tap + rows].double().cpu() @ w[:, tap].double().t()
    for cfg in (0, 1, 2):
        c = E.gemm_img(E.split_image(xs, 4.0), E.split_image(w.reshape(Co, 5 * Ci).cuda(), 64.0), cfg=cfg, scale_a=4.0, scale_b=64.0,
                       a_seg=(Ci, Ci), M=rows, K=5 * Ci)
        assert rel(c, ref) < 5e-6, cfg


@pytest.mark.parametrize('cfg', [0, 1, 2])
@pytest.mark.parametrize('layout', [(False, False), (False, True), (True, True), (True, False)])
def test_image_gemm_bf16_single_piece(E, layout, cfg):
    """The single-piece form of gemm_img.hip (round 4, the 16-bit data path of SS_PRECISION_BF16): operands are plain bf16 matrices, one
    v_mfma_f32_32x32x16_bf16 per k16-step, k-tiles of 64.  A bf16 x bf16 product is exact in fp32 and the accumulation is fp32, so against
    float64 on the SAME bf16 operands the result is fp32-grade -- every layout and tile configuration, ragged M / N, K tails of a
    reduction-major pair, bias, accumulation, split-K, and the conv window (segmented K) over a haloed slab."""
    ta, tb = layout
    g = torch.Generator().manual_seed(23 + cfg)
    shapes = [(264, 200, 128, 1), (1000, 520, 1024, 1), (512, 512, 4096, 4), (2048, 1024, 2112 if (ta and tb) else 2176, 8)]
    if ta and tb:
        shapes += [(512, 264, 1027, 3), (256, 256, 8447, 8), (136, 128, 31, 1)]
    for M, N, K, ks in shapes:
        A = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
        Bm = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).cuda()
        bias = torch.randn(N, generator=g).cuda()
        c0 = torch.randn(M, N, generator=g).cuda()
        ref = A.double() @ Bm.double().t() + bias.double() + c0.double()
        ai = A.t().contiguous() if ta else A
        bi = Bm.t().contiguous() if tb else Bm
        c = E.gemm_img(ai, bi, ta, tb, bias, ks, cfg, out=c0.clone(), accumulate=True)
        assert rel(c, ref) < 5e-6, (M, N, K, ks, layout, cfg)
        c2 = E.gemm_img(ai, bi, ta, tb, bias, ks, cfg, out=c0.clone(), accumulate=True)
        assert torch.equal(c, c2)
    if not ta and not tb:
        B, T, Ci, Co = 3, 40, 64, 128
        TP = T + 4
        x = torch.zeros(B, TP, Ci)
        x[:, 2:2 + T] = torch.randn(B, T, Ci, generator=g)
        w = (torch.randn(Co, 5, Ci, generator=g) * 0.05).to(torch.bfloat16)
        xs = x.reshape(B * TP, Ci).to(torch.bfloat16).cuda()
        rows = B * TP - 4
        ref = torch.zeros(rows, Co, dtype=torch.float64)
        for tap in range(5):
            ref += xs[tap:tap + rows].double().cpu() @ w[:, tap].double().t()
        c = E.gemm_img(xs, w.reshape(Co, 5 * Ci).cuda(), cfg=cfg, a_seg=(Ci, Ci), M=rows, K=5 * Ci)
        assert rel(c, ref) < 5e-6, cfg


@pytest.mark.parametrize('shape', [(1, 128, 4 * 132), (8, 512, 8 * 132 + 3), (8, 16, 5 * 196), (32, 256, 6 * 196), (32, 100, 1000)],
                         ids=['h1_in128', 'h8_in512', 'h8_in16', 'h32_in256', 'h32_in100_ragged'])
def test_fused_encoder_blstm_weight_gradients(E, shape):
    """csrc/lstm_wgrad.hip: dW_ih, dW_hh (h(t-1) = one slab row earlier / later per direction) and both bias gradients of an encoder BLSTM
    layer in one fp32 launch, against float64 -- including an input that is a column view of a wider slab and row counts that are not
    multiples of the chunk; run twice: the ordered float64 reduction makes it bit-reproducible."""
    H, In, R = shape
    g = torch.Generator().manual_seed(3 + H + In)
    dg = torch.randn(R, 8 * H, generator=g) * 1e-3
    dg[0] = 0
    dg[-1] = 0                       # halo rows of a gradient slab are zero
    wide = torch.randn(R, In + 24, generator=g)
    hout = torch.tanh(torch.randn(R, 2 * H, generator=g))
    hout[0] = 0
    hout[-1] = 0
    xd = wide.cuda()[:, 8:8 + In] if In % 4 == 0 else wide.cuda()[:, 3:3 + In]
    x = wide[:, 8:8 + In] if In % 4 == 0 else wide[:, 3:3 + In]
    gwih, gwhh, gb = E.lstm_wgrad(dg.cuda(), xd, hout.cuda())
    d64, x64, h64 = dg.double(), x.double(), hout.double()
    for d in range(2):
        dd = d64[:, d * 4 * H:(d + 1) * 4 * H]
        assert rel(gwih[d], dd.t() @ x64) < 2e-6, (shape, d)
        ref_hh = dd[1:].t() @ h64[:-1, :H] if d == 0 else dd[:-1].t() @ h64[1:, H:]
        assert rel(gwhh[d], ref_hh) < 2e-6, (shape, d)
        assert rel(gb[d, 0], dd.sum(0)) < 2e-6 and torch.equal(gb[d, 0], gb[d, 1])
    again = E.lstm_wgrad(dg.cuda(), xd, hout.cuda())
    assert all(torch.equal(a, b) for a, b in zip((gwih, gwhh, gb), again))
