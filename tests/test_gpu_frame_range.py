"""The frame axis end to end (pytest -m gpu): training, gradients and the resampling at 200 and 256 frames -- the third of the documented
range 8 <= T <= 256 above the 192 frames of BASELINE's configs -- and at the minimum, 8 frames.

What only runs up there (csrc/elementwise.hip): gn_relu_bwd_kernel<16> and gn_relu_gather_kernel<16> replace the <12> forms at T > 192; the
backward's P * 256 bytes of dynamic LDS beside its 15.4 KB of static LDS pass 64 KB at P = 200; the gather's (T + 1) * 256 bytes pass 64 KB
at T = 256 only; s_start / s_lam hold 258 entries and T = 256 uses 257 of them; flatten_rows (engine.hip) rewrites the per-utterance
contractions at T % 128 != 0, so 200 runs the flattened form at a new row period and 256 the batched one at a new M.

Stretching draws.  With draws as the reference makes them (rand + 0.5, randint(19, 32)) a resampled slab of 256 rows has 150-195 live
rows, so rows 192..255 of the gather's output and of the backward's source tile would stay zero even at T = 256.  stretch_draws() stays
inside the reference's ranges at their stretching end (scales in [1.3, 1.5), len_seg in 28..31): a full-length utterance then selects more
than P positions, every one of the P rows is live and the count is truncated at P.  Every test that uses them asserts that on the CPU
(all_rows_live) before anything runs on the GPU.

Bars: none is new.  Whole steps: loss 1e-5, output and every gradient tensor 1e-4, check_adam, ReLU hand-over acting below 2e-5 only
(tests/test_gpu_configs.py).  Conv block: 1e-4 (test_conv_block_against_reference_vectors, same hook).  Resampling: bit-exact forward,
1e-6 backward (test_interp_bit_exact_against_reference).  Engine against engine: compare_step of tests/test_gpu_engine_containment.py."""
import types

import numpy as np
import pytest
import torch

from oracle import interp_np, ref_model, weights as W
from tests.test_gpu_configs import Case, check_adam, check_fp32_step, rel
from tests.test_gpu_engine_containment import LR, WSEED, compare_step, g3_batch, g3_step, plain

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINK = 2e-5


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def stretch_draws(seed, B, ncalls, nseg=7):
    """[(scales f32[B*7], len_seg int64[B*7])] * ncalls at the stretching end of the reference's own ranges (model.py:392-393, 399-402):
    scales in [1.3, 1.5) where the reference draws [0.5, 1.5), len_seg in 28..31 where it draws 19..31."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(ncalls):
        sc = np.minimum((1.3 + 0.2 * rs.random_sample(B * nseg)).astype(np.float32), np.float32(1.4999))
        ls = rs.randint(28, 32, size=B * nseg).astype(np.int64)
        out.append((sc, ls))
    return out


def all_rows_live(draw, len_seq, P):
    """The precondition of the stretching draws, checked on the CPU: every utterance of full length selects at least P positions, so all
    P rows of its resampled slab are live.  Returns the plan's (counts, nrows)."""
    len_seq = np.asarray(len_seq)
    _, _, counts, nrows = interp_np.interp_plan(draw[0], draw[1], len_seq, max_len_pad=P)
    assert (len_seq == P).any()
    for b in range(len(len_seq)):
        if len_seq[b] == P:
            assert counts[b] >= P and nrows[b] == P, (b, int(counts[b]), P)
    return counts, nrows


def set_lengths(c, lens):
    """Give a Case's batch (synthesised at full length) the stated utterance lengths, padded as synth_batch pads: mel 0, F0 -1e10."""
    B, T = c.B, c.T
    assert int(c.lens.min()) == T and len(lens) == B
    c.lens = torch.tensor(lens)
    pad = torch.arange(T)[None, :, None] >= c.lens[:, None, None]
    c.mel = torch.where(pad, torch.zeros_like(c.mel), c.mel)
    c.f0 = torch.where(pad, torch.full_like(c.f0, -1e10), c.f0)


# --------------------------------------------------------------------------------------------- 1: whole steps against the oracle
#                kind  B   T   draws      lens (None: synth_batch's, from len_lo)   len_lo
STEP_CASES = [('G3', 2, 200, 'ref', None, 96),              # first T on the <16> kernels; backward LDS past 64 KB; T % 16 == 8; flattened rows
              ('G3', 2, 200, 'stretch', [200, 163], 200),   # rows up to P live, count truncated at P
              ('G3', 2, 256, 'stretch', [256, 219], 256),   # the maximum: the gather's > 64 KB branch, all 256 rows live, 257 index entries
              ('G3', 3, 256, 'ref', None, 96),              # odd batch, short live range: rows past nrows must be zero
              ('G6', 2, 256, 'stretch', None, 256),         # Encoder_6 / Decoder_4 (H = 256), cross-entropy loss
              ('G3', 3, 8, 'ref', None, 8),                 # the minimum: one code frame, nit = 1, half of a workgroup's row lanes idle
              ('G3', 1, 8, 'ref', None, 8),
              ('G6', 2, 8, 'ref', None, 8)]


@pytest.mark.parametrize('case', STEP_CASES, ids=[f'{k.lower()}_{B}x{T}_{d}' for k, B, T, d, _, _ in STEP_CASES])
def test_train_steps_against_oracle(E, case):
    """Two train steps, the second on the first one's update, engine against oracle at the standing bars."""
    kind, B, T, how, lens, len_lo = case
    stretch = how == 'stretch'
    c = Case(E, kind, B, T, len_lo, wseed=0 if kind == 'G3' else 4, bseed=1700 + 7 * B + T, draws_fn=stretch_draws if stretch else None)
    if lens is not None:
        set_lengths(c, lens)
    if stretch:
        for it in range(2):
            draws = stretch_draws(c.dseed + it, B, c.ncalls)
            if kind == 'G3':
                all_rows_live(draws[0], c.lens.numpy(), T)           # the outer call resamples each utterance at its own length
            for d in draws[1 if kind == 'G3' else 0:]:
                all_rows_live(d, np.full(B, T), T)                   # the encoders' calls: len_seq = max_len_pad
    tag = f'{kind} {B}x{T} {how} draws'
    for it in range(2):
        r = c.step(it, kink_bound=KINK)
        check_fp32_step(r, f'{tag} step {it}')
        check_adam(r, f'{tag} step {it}', it)
    assert c.eng.scratch_fallbacks() == 0
    if kind != 'G3':
        return
    # resampled inputs of the last step: bit-exact against the oracle's index path, rows past the live ones zero
    draws = c.draws(1)
    xi = ref_model.interp(torch.cat((c.mel, c.f0), -1), c.lens.numpy(), draws[0], c.hp)
    got = c.eng.debug_buffer('in.mel', B, T).cpu().numpy()
    assert np.array_equal(got, xi[:, :, :80].numpy())
    cls = c.eng.debug_buffer('in.f0', B, T)[:, :, :257].argmax(-1).cpu().numpy()
    assert np.array_equal(cls, interp_np.quantize_f0(xi[:, :, -1].numpy()))
    _, nrows = interp_np.interp_plan(draws[0][0], draws[0][1], c.lens.numpy(), max_len_pad=T)[2:]
    for b in range(B):
        assert not got[b, nrows[b]:].any(), (b, int(nrows[b]))
    if how == 'ref' and T == 256:
        assert int(nrows.max()) < T                                  # the short live range this case is there for


# --------------------------------------------------------------------------------------------- 4: one conv block against float64
def conv_block_f64(x, w, bias, gamma, beta, dy, mask):
    """conv1d(padding 2) -> group_norm(C / 16 groups, eps 1e-5) -> relu in float64 on the CPU, gradients by autograd.  mask [B, T, Co]:
    the ReLU branch to take (the engine's); returns (z, y, dx, gw, gb, ggamma, gbeta) with z the GroupNorm output, all [B, T, C] layout."""
    p = [t.double().requires_grad_() for t in (x, w, bias, gamma, beta)]
    x64, w64, b64, ga64, be64 = p
    z = torch.nn.functional.group_norm(torch.nn.functional.conv1d(x64.transpose(1, 2), w64, b64, padding=2), w.shape[0] // 16, ga64, be64, eps=1e-5)
    z = z.transpose(1, 2)
    y = torch.where(mask, z, torch.zeros_like(z))
    y.backward(dy.double())
    return (z.detach(), y.detach()) + tuple(t.grad for t in p)


@pytest.mark.parametrize('shape', [(2, 200, 80, 128), (2, 256, 80, 512), (1, 256, 512, 512), (3, 200, 512, 256), (2, 8, 80, 128), (1, 8, 256, 256)],
                         ids=lambda s: 'b%d_t%d_%dto%d' % s)
def test_conv_block_against_float64(E, shape):
    """ss_op_conv_block forward and backward (the GroupNorm backward WITHOUT the fused scatter) at the ends of the frame range.  The
    engine's arithmetic is fp16 x 2: the bar is the 1e-4 the reference-vector test applies to the same hook."""
    B, T, Ci, Co = shape
    g = torch.Generator().manual_seed(31 * T + Ci + Co + B)
    x = torch.randn(B, T, Ci, generator=g)
    w = torch.randn(Co, Ci, 5, generator=g) * 0.05
    bias = torch.randn(Co, generator=g) * 0.05
    gamma = 1.0 + 0.1 * torch.randn(Co, generator=g)
    beta = 0.1 * torch.randn(Co, generator=g)
    dy = torch.randn(B, T, Co, generator=g)
    got = [t.cpu() for t in E.conv_block(x.cuda(), w.cuda(), bias.cuda(), gamma.cuda(), beta.cuda(), dy.cuda())]
    torch.cuda.synchronize()
    mask = got[0] > 0                                              # the branch the engine took
    z, *ref = conv_block_f64(x, w, bias, gamma, beta, dy, mask)
    dis = mask != (z > 0)
    zmax = float(z.abs()[dis].max()) if bool(dis.any()) else 0.0
    assert zmax < KINK, (int(dis.sum()), zmax)                     # the hand-over only ever acted at the kink
    errs = {n: rel(a, r) for n, a, r in zip(('y', 'dx', 'gw', 'gb', 'ggamma', 'gbeta'), got, ref)}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f'[conv block {B}x{T} {Ci}->{Co}] ' + '  '.join(f'{n} {e:.2e}' for n, e in errs.items()) + f'  worst {worst[0]} {worst[1]:.2e}'
          f'  (branches handed over at the kink: {int(dis.sum())})')
    for n, e in errs.items():
        assert e < TOL, (shape, n, e)


# --------------------------------------------------------------------------------------------- 5: the resampling alone
_INTERP = {}


@pytest.mark.parametrize('C', [81, 8, 337, 512])
@pytest.mark.parametrize('T', [200, 256, 8])
def test_interp_all_rows_live(E, T, C):
    """ss_interp_forward / ss_interp_backward at P = T with every row of the full-length utterance live and its count truncated at P.
    C: the scalar path (81, 337), the vector path (8, 512) and the threads-per-row switches at 128 and 256 of interp_gather / interp_scatter.
    Lengths [T, T - 37, 20]; at 8 frames, where those do not exist, [8, 5, 2]."""
    B = 3
    lens = np.array([T, T - 37, 20] if T > 37 else [8, 5, 2])
    assert int(lens.max()) == T and int(lens.min()) >= 2
    sc, ls = stretch_draws(4000 + T, B, 1)[0]
    counts, _ = all_rows_live((sc, ls), lens, T)
    assert counts[0] > T                                           # truncated, not just full
    if T not in _INTERP:
        _INTERP[T] = E.Engine('interp', W.default_hparams(max_len_pad=T), B, T)
    eng = _INTERP[T]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(T + C))
    y, i0, lam, cnt = (t.cpu().numpy() for t in eng.interp_forward(x, lens, sc, ls, want_plan=True))
    ri0, rlam, rcnt, rn = interp_np.interp_plan(sc, ls, lens, max_len_pad=T)
    assert np.array_equal(i0, ri0) and np.array_equal(lam, rlam) and np.array_equal(cnt, rcnt)
    assert np.array_equal(y, interp_np.interp_apply(x.numpy(), ri0, rlam, rn))
    for b in range(B):
        assert not y[b, rn[b]:].any(), b                           # rows >= nrows exactly zero
    assert rn[0] == T and bool(y[0, T - 1].any())                  # ... and the last row of the full-length one is live
    dy = torch.randn(B, T, C, generator=torch.Generator().manual_seed(T + C + 1))
    dx = eng.interp_backward(dy, T)
    eng.check()
    assert rel(dx, interp_np.interp_backward(dy.numpy(), ri0, rlam, rn, T)) < 1e-6


# --------------------------------------------------------------------------------------------- 6: one engine across the 192-frame line
HISTORY = (96, 256, 200, 96, 256)


def _reset(eng, w):
    eng.load_weights(w)
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)


def test_engine_history_across_the_192_frame_line(E):
    """One Generator_3 engine (4 x 256) stepping at 96, 256, 200, 96, 256 frames (SS_STEP_BUCKET): every re-plan across 192 frames changes the
    GroupNorm kernels' instantiation and their LDS attribute in a live engine.  Each step starts from the same weights and a fresh Adam
    state (test_guarded_g3_train_step_buckets_and_back says why) and is compared with a fresh engine created for that T.  Then the same
    history under ss_tune("deterministic", 1): the two visits at 256 frames are bit-identical in loss, gradient arena and parameters."""
    B, Tm = 4, 256
    hp = W.default_hparams(max_len_pad=Tm)
    w = W.make_weights('G3', hp, WSEED['G3'])
    batches = {T: g3_batch(300 + T, B, T) for T in set(HISTORY)}
    eng = plain(E, 'G3', hp, B, Tm)
    fresh = {}
    for k, T in enumerate(HISTORY):
        if T not in fresh:
            fresh[T] = plain(E, 'G3', W.default_hparams(max_len_pad=T), B, T)
        ref = fresh[T]
        _reset(eng, w)
        _reset(ref, w)
        la, lb = g3_step(eng, batches[T], bucket=True), g3_step(ref, batches[T])
        eng.check()
        ref.check()
        compare_step(('history', k, T), types.SimpleNamespace(eng=eng), ref, la, lb, 1)
        assert eng.scratch_fallbacks() == 0 and ref.scratch_fallbacks() == 0
    del fresh
    E.tune('deterministic', 1)
    try:
        eng = plain(E, 'G3', hp, B, Tm)
        seen = []
        for T in HISTORY:
            _reset(eng, w)
            loss = float(g3_step(eng, batches[T], bucket=True))
            eng.check()
            if T == Tm:
                seen.append((loss, eng.grads.clone(), eng.params.clone()))
        (l0, g0, p0), (l1, g1, p1) = seen
        assert np.isfinite(l0) and l0 == l1 and bool(g0.any())
        assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)) and torch.equal(p0.view(torch.int32), p1.view(torch.int32))
        assert eng.scratch_fallbacks() == 0
    finally:
        E.tune('deterministic', 0)
