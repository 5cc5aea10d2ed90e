"""The pipelined k-loop of the fp16 x 2 GEMM (csrc/gemm_bf16x3.hip, PIPE; ss_tune("gemm_pipe"), pytest -m gpu).

It changes how a k-tile's loads are scheduled and nothing else: the same products reach every accumulator in the same order.  So
ss_tune("gemm_pipe", 1) must give the BITS of ss_tune("gemm_pipe", 0), and both the fp32 grade of the mode (5e-6 of max|C| against float64,
the bar of test_gemm_fp16x2_mode).

Isolated, through engine.gemm(..., f16x2=True):
  layouts  TN (ta, tb), NN with tb, NT;
  K        8, 32, 40, 64, 72, 96, 100, 160 -- 1, 2, 3 and 5 k-tiles of 32, with and without a partial last one;
  M x N    128 x 128, 130 x 132, 64 x 256, and 136 x 264 (two column blocks, the second with ONE valid group of eight columns);
  ksplit   1, 2, 3, 5 (5 at K = 96 leaves slices without a k-tile);
  launch   'plain': fp32 operands, split-K through atomics (ss_op_gemm);
           'img_b' / 'img_ab': as the engine's weight gradients -- the largest tile, B (and A) with its image, split-K through partial
           slabs (ss_op_gemm_pre).  The TN launches of these with M, N > 64 and N % 8 == 0 are the ones the pipelined loop takes: B's
           image by LDS-DMA, A through two register sets, the partial last tile through predicated register loads.
Bit identity is asserted wherever the launch is deterministic: everywhere with partial slabs, and for 'plain' up to ksplit 2 (three or more
fp32 atomics on one element commit in arrival order; two onto a zero commute).  The float64 bar holds for every case.
One case per launch kind runs with A, B, the images, the slabs and C flush against guard memory (tests/guarded.py).

Whole step: two fresh Generator_3 engines at B = 2, T = 8 and T = 128 under ss_tune("deterministic", 1), one step with gemm_pipe 0 and one with
1: loss, gradient arena and parameters bit-identical.  At B = 2, T = 128 the decoder's weight gradients are 128 x 128 TN tiles, ksplit 3, three
k-tiles per slice (the last of W_hh's a partial one) with the hidden-state image as B."""
import functools

import pytest
import torch

from oracle import weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from tests import guarded as G
from tests.test_gpu_engine_containment import plain, stack_draws

pytestmark = pytest.mark.gpu
BAR = 5e-6
LAYOUTS = {'TN': (True, True), 'NN_tb': (False, True), 'NT': (False, False)}
KS = (8, 32, 40, 64, 72, 96, 100, 160)
SHAPES = ((128, 128), (130, 132), (64, 256), (136, 264))
KSPLITS = (1, 2, 3, 5)
LAUNCHES = ('plain', 'img_b', 'img_ab')


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


@pytest.fixture
def pipe(E):
    """set(v): ss_tune("gemm_pipe", v); back at the default afterwards whatever happens."""
    try:
        yield lambda v: E.tune('gemm_pipe', v)
    finally:
        E.tune('gemm_pipe', 1)


def rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


@functools.lru_cache(maxsize=None)
def operands(layout, M, N, K):
    """(A, B, float64 product) on the GPU, made once per case and never changed."""
    ta, tb = LAYOUTS[layout]
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + (ta + 2 * tb))
    A = torch.randn((K, M) if ta else (M, K), generator=g).cuda()
    Bm = (torch.randn((K, N) if tb else (N, K), generator=g) * 0.05).cuda()
    ref = (A.t() if ta else A).double() @ (Bm if tb else Bm.t()).double()
    return A, Bm, ref


def image_of(E, x):
    """The image of an operand where it can have one (rows of whole groups of eight), else None."""
    return E.split_image(x) if x.shape[1] % 8 == 0 else None


def launch(E, how, layout, A, Bm, ks, imgs, part, out=None):
    ta, tb = LAYOUTS[layout]
    if how == 'plain':
        return E.gemm(A, Bm, None, ta, tb, ks, out=out, f16x2=True)
    return E.gemm(A, Bm, None, ta, tb, ks, out=out, f16x2=True, as_engine=True, a_img=imgs[0] if how == 'img_ab' else None, b_img=imgs[1],
                  part=part if ks > 1 else None)


@pytest.mark.parametrize('how', LAUNCHES)
@pytest.mark.parametrize('shape', SHAPES, ids=[f'{m}x{n}' for m, n in SHAPES])
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_pipe_matches_one_buffer_loop_and_float64(E, pipe, layout, shape, how):
    M, N = shape
    part = torch.empty(max(KSPLITS) * M * N, device='cuda')
    for K in KS:
        A, Bm, ref = operands(layout, M, N, K)
        imgs = (image_of(E, A), image_of(E, Bm))
        for ks in KSPLITS:
            got = []
            for v in (0, 1):
                pipe(v)
                part.fill_(float('nan'))
                got.append(launch(E, how, layout, A, Bm, ks, imgs, part))
            tag = (layout, shape, K, ks, how)
            e0, e1 = rel(got[0], ref), rel(got[1], ref)
            print(tag, f'gemm_pipe 0: {e0:.3g}  1: {e1:.3g}  equal: {torch.equal(got[0], got[1])}')
            assert e1 < BAR and e0 < BAR, (tag, e0, e1)
            # partial slabs exist in the kernel with the vector loads only (row strides that are multiples of 4 floats)
            slabs = how != 'plain' and A.stride(0) % 4 == 0 and Bm.stride(0) % 4 == 0
            if slabs or ks <= 2:
                assert torch.equal(got[0], got[1]), tag


@pytest.mark.parametrize('how', LAUNCHES)
@pytest.mark.parametrize('K', (96, 100))
def test_pipe_inside_guard_memory(E, pipe, how, K):
    """128 x 128 TN, ksplit 2 (K = 100: the second slice ends in a partial k-tile): every buffer of the launch ends where guard memory begins.
    A result computed from guard memory is a NaN, a write outside C or the slabs changes the guard."""
    layout, M, N, ks = 'TN', 128, 128, 2
    A, Bm, ref = operands(layout, M, N, K)
    res = []
    for v in (0, 1):
        pipe(v)
        ga, gb = G.inp(A, 'cuda', name='A'), G.inp(Bm, 'cuda', name='B')
        gia, gib = G.inp(E.split_image(A), 'cuda', name='A image'), G.inp(E.split_image(Bm), 'cuda', name='B image')
        gc = G.out((M, N), 'cuda', fill=0.0, name='C')
        gp = G.out((ks * M * N,), 'cuda', name='partial slabs')
        c = launch(E, how, layout, ga.t, gb.t, ks, (gia.t, gib.t), gp.t if how != 'plain' else None, out=gc.t)
        torch.cuda.synchronize()
        G.check_all([ga, gb, gia, gib, gc])
        gp.check(written=how != 'plain')
        G.assert_close(c, ref, BAR, (how, K, v))
        res.append(c.clone())
    assert torch.equal(res[0], res[1]), (how, K)


@pytest.mark.parametrize('T', (8, 128))
def test_train_step_is_bit_identical(E, pipe, T):
    B = 2
    hp = W.default_hparams(max_len_pad=T)
    mel, f0, emb, lens = synth_batch(40 + T, B, T, min(64, T))
    draws = stack_draws(draws_for(140 + T, B, 4))
    E.tune('deterministic', 1)
    try:
        res = []
        for v in (0, 1):
            pipe(v)
            eng = plain(E, 'G3', hp, B, T)
            loss = float(eng.g3_train_step(mel, f0, emb, lens, draws))
            eng.check()
            assert eng.scratch_fallbacks() == 0
            res.append((loss, eng.grads.clone(), eng.params.clone()))
    finally:
        E.tune('deterministic', 0)
    (l0, g0, p0), (l1, g1, p1) = res
    assert l0 == l0 and bool(g0.any()), (l0, 'the step computed nothing')
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)), float((g0 - g1).abs().max())
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)), float((p0 - p1).abs().max())
