"""Containment of the op hooks (pytest -m gpu): every kernel stays inside its declared outputs and its result does not depend on memory
around its declared inputs.  Operands are carved out of guarded allocations (tests/guarded.py: >= 1 MiB of quiet-NaN bit pattern before
and after, and in the ld - cols gap of every row; outputs start as the pattern too, so an element that is never written fails by itself),
placed at the offsets and strides the code documents and nothing more, results are compared with the float64 reference and the tolerance
of the op's existing test (named in each docstring -- nothing new is invented here), and afterwards every guard is compared bit for bit.

Placement rules and where they come from:
  ss_op_gemm         any base, any row stride: gemm_f32.hip has a vector path (16-byte aligned base, ld % 4 == 0, `vec_ok`) and scalar instances for
                     "unaligned / odd strides" -- operands are placed both ways, C with ldc in {N, N + 4, 2N, odd}.
  images             32-byte aligned base (bf16 single piece: 16-byte), ld % 8 == 0 (gemm_img.hip gemm_img_supported); the fp32 source of
                     ss_op_split_image: 16-byte aligned base, ld % 4 == 0 (gemm_img.hip split_image).  zeros_dev: ">= 1 KB of zero bytes" (header).
  haloed slabs       halo rows are zero where the contract says so (kernels.h: "two all-zero rows on either side of every utterance"; header,
                     ss_op_lstm_wgrad: "halo rows zero"): they are part of the input, not guard.
  small BLSTM slabs  rows lstm_small_ld(H) floats apart, "columns past 2H untouched" (header): the padding columns carry the pattern.
  persistent scratch the scratch of a persistent recurrence (H in {256, 512}, "persist" 1) holds sync words and tagged exchange tiles: its
                     extent is zero-filled as engine.blstm_layer does; only the bands around it carry the pattern.
Split-K of ss_op_gemm adds into C with atomics (GEMM_ACCUM) and ss_op_lstm_wgrad ACCUMULATES (header): those outputs are pre-filled as the
contract demands and only their guard carries the pattern."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import guarded as G
from oracle import interp_np, ref_model, weights as W

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = 1e-4
DEV = 'cuda'


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def pattern(shape):
    """float32 tensor on the GPU that holds the guard pattern everywhere (a pre-fill for slabs whose halo rows are then zeroed)."""
    return torch.full(tuple(shape), G.NAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------- ss_op_gemm
GEMM_SHAPES = [(128, 128, 64), (256, 512, 400), (100, 80, 164), (333, 257, 66), (1024, 512, 2560)]          # test_gemm_layouts
GEMM_EDGES = [(1, 257, 5), (3, 129, 1), (127, 1, 33), (129, 3, 66), (257, 127, 164), (1, 1, 1)]
LAYOUTS4 = [(False, False), (False, True), (True, True), (True, False)]


def _odd(n):
    return n + 5 if n % 2 == 0 else n + 4


# Operand placements (as functions of the operand's width).  launch_gemm (gemm_f32.hip) takes the vector kernels -- gemm_bf16x3_kernel in
# "gemm_mode" 1, the kernel the engine runs; the vector instances of gemm_f32_kernel in mode 0 and for A stored [K,M] with B stored [N,K] --
# only when BOTH operands pass vec_ok (16-byte aligned base, ld % 4 == 0); everything else runs gemm_f32_kernel's scalar instances.
ALIGNED = (lambda w: dict(ld=w + (-w) % 4 + 8, offset=64), lambda w: dict(ld=2 * w + (-2 * w) % 4, offset=4))
UNALIGNED = (lambda w: dict(ld=_odd(w), offset=3), lambda w: dict(ld=w + (-w) % 4 + 4, offset=65), lambda w: dict(ld=_odd(w), offset=64))
SCALAR_PAIRS = [(a, b) for a in (ALIGNED[0],) + UNALIGNED for b in UNALIGNED] + [(a, ALIGNED[1]) for a in UNALIGNED]
C_PLACES = (lambda N: dict(ld=N, offset=64), lambda N: dict(ld=N + 4, offset=64), lambda N: dict(ld=2 * N, offset=4), lambda N: dict(ld=_odd(N), offset=1))


def _vec_ok(t):
    return t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0


def _gemm_cases(E, shapes, mode_kw, make, tol_ref, use_bias):
    """Every (shape, layout, ksplit) runs five guarded calls: both operands on the vector path with EACH of the four C placements (ldc N,
    N + 4, 2N, odd; aligned and odd base), and one pair of operands that takes the scalar instances (the pair and its C placement walk
    through their lists with strides coprime to the loop periods, skewed by the shape index).  The placement is asserted to select the
    path it is meant to, and at the end every (layout, ksplit, C placement) must have run on the vector path."""
    vector, scalar, n = set(), set(), 0
    for si, (M, N, K) in enumerate(shapes):
        for li, (ta, tb) in enumerate(LAYOUTS4):
            if M * N * K > 5e8 and li not in (0, 2):
                continue                                                        # the largest shape: two layouts
            A, Bm, ref = make(M, N, K, ta, tb)
            bias = torch.randn(N, generator=torch.Generator().manual_seed(M + N)) if use_bias else None
            if use_bias:
                ref = ref + bias.double()
            wa, wb = A.shape[1], Bm.shape[1]
            for ks in (1, 4):
                cases = [(ALIGNED[c % 2](wa), ALIGNED[c // 2](wb), c, True) for c in range(4)]
                q = (7 * n + si) % len(SCALAR_PAIRS)
                cases.append((SCALAR_PAIRS[q][0](wa), SCALAR_PAIRS[q][1](wb), (3 * n + si) % 4, False))
                n += 1
                for pa, pb, c, vec in cases:
                    ga, gb = G.inp(A, DEV, name='A', **pa), G.inp(Bm, DEV, name='B', **pb)
                    gc = G.out((M, N), DEV, name='C', fill=0.0 if ks > 1 else None, **C_PLACES[c](N))   # split-K: atomics into C, zeroed by the caller
                    gbias = G.inp(bias, DEV, offset=(64, 3)[(c + ks // 4) % 2], name='bias') if use_bias else None
                    assert (_vec_ok(ga.t) and _vec_ok(gb.t)) == vec, (pa, pb)
                    E.gemm(ga.t, gb.t, gbias.t if use_bias else None, ta, tb, ks, out=gc.t, **mode_kw)
                    torch.cuda.synchronize()
                    G.assert_close(gc.t, ref, tol_ref, ('C', M, N, K, ta, tb, ks, pa, pb, c))
                    G.check_all([ga, gb, gc] + ([gbias] if use_bias else []))
                    (vector if vec else scalar).add((ta, tb, ks, c if vec else q))
    assert len(vector) == len(LAYOUTS4) * 2 * len(C_PLACES), sorted(vector)      # incl. (ta, not tb) on aligned operands, ksplit 4, every ldc
    assert len({s[:3] for s in scalar}) == len(LAYOUTS4) * 2 and len({s[3] for s in scalar}) == len(SCALAR_PAIRS)


def _randn_case(seed_off=0, b_scale=1.0, bf16=False, mixed=False):
    def make(M, N, K, ta, tb):
        g = torch.Generator().manual_seed(M + N + K + seed_off)
        A = torch.randn((K, M) if ta else (M, K), generator=g)
        Bm = torch.randn((K, N) if tb else (N, K), generator=g) * b_scale
        if mixed and A.numel() >= 7:
            A.view(-1)[:7] = torch.tensor([1e-3, 3e-5, 1e-6, 2e-8, 100.0, -250.0, 0.0])
        Ar, Br = (A.bfloat16().double(), Bm.bfloat16().double()) if bf16 else (A.double(), Bm.double())
        return A, Bm, (Ar.t() if ta else Ar) @ (Br if tb else Br.t())
    return make


@pytest.mark.parametrize('gemm_mode', [0, 1], ids=['fp32_mfma', 'bf16x3'])
def test_gemm_containment(E, gemm_mode):
    """ss_op_gemm in the fp32-MFMA and the default bf16 x 3 arithmetic: all four layouts (including A stored [K,M] with B stored [N,K]),
    ksplit 1 and 4, test_gemm_layouts' shapes plus M / N in {1, 3, 127, 129, 257} and K in {1, 5, 33, 66, 164}.  Reference and bound of
    test_gemm_layouts: float64 product + bias, relative max-norm 5e-6."""
    E.tune('gemm_mode', gemm_mode)
    try:
        _gemm_cases(E, GEMM_SHAPES + GEMM_EDGES, {}, _randn_case(), 5e-6, True)
    finally:
        E.tune('gemm_mode', 1)


def test_gemm_containment_bf16_operands(E):
    """GEMM_BF16 (operands rounded to bf16 inside the kernel).  Reference and bound of test_gemm_bf16_mode: float64 product of the
    bf16-rounded operands, 5e-6."""
    _gemm_cases(E, [(256, 512, 400), (384, 256, 1024), (1024, 512, 2560)] + GEMM_EDGES, dict(bf16=True), _randn_case(5, bf16=True), 5e-6, False)


def test_gemm_containment_fp16x2(E):
    """GEMM_F16X2.  Operands, reference and bound of test_gemm_fp16x2_mode: B scaled by 0.05, magnitudes from 2e-8 to 250 mixed into A,
    float64 product, 5e-6."""
    _gemm_cases(E, [(256, 512, 400), (384, 256, 1024), (1024, 512, 2560)] + GEMM_EDGES, dict(f16x2=True), _randn_case(6, 0.05, mixed=True), 5e-6,
                False)


# --------------------------------------------------------------------------------------------- ss_op_split_image + ss_op_gemm_img
IMG_SHAPES = [(264, 200, 96, 1), (1000, 520, 1024, 1), (512, 512, 4096, 4), (2048, 1024, 2112, 8)]         # test_image_gemm_against_fp64
IMG_SHAPES_TT = [(512, 264, 1027, 3), (256, 256, 8447, 8), (136, 128, 31, 1)]    # K tails of the reduction-major pair
_IMG_DATA = {}


def _img_data(M, N, K, bf16):
    key = (M, N, K, bf16)
    if key not in _IMG_DATA:
        g = torch.Generator().manual_seed(M + N + K)
        A = torch.randn(M, K, generator=g)
        Bm = torch.randn(N, K, generator=g) * 0.05
        if bf16:
            A, Bm = A.to(torch.bfloat16), Bm.to(torch.bfloat16)
        bias = torch.randn(N, generator=g)
        c0 = torch.randn(M, N, generator=g)
        prod = A.double() @ Bm.double().t() + bias.double()
        _IMG_DATA[key] = (A, Bm, bias, c0, prod)
    return _IMG_DATA[key]


def _img_operand(E, X, t, bf16, i, name):
    """X [rows, K] logical; stored transposed when t.  fp16 x 2: the fp32 source is a guarded input, its image a guarded output with
    ldi > cols that then serves as the GEMM's input; bf16: the matrix is its own image."""
    S = X.t().contiguous() if t else X
    cols = S.shape[1]
    if bf16:
        return [G.inp(S, DEV, ld=cols + 8 * (1 + i % 3), offset=8 * (1 + i % 5), name=name)]
    src = G.inp(S, DEV, ld=cols + 4 * (i % 3), offset=4 * (1 + i % 4), name=name + '.src')
    img = G.out(S.shape, DEV, ld=cols + 8 * (1 + i % 2), offset=8 * (1 + i % 7), name=name)
    E.split_image(src.t, out=img.t)
    torch.cuda.synchronize()
    img.check(written=False)                  # an image's bytes are fp16 pairs: not compared with the float32 pattern
    src.check()
    return [img, src]


def _img_cases(E, bf16, layouts):
    zeros = G.inp(torch.zeros(256), DEV, offset=8, name='zeros_dev')             # header: ">= 1 KB of zero bytes"
    i = 0
    try:
        for xcc in (0, 255, 0xF0):
            E.tune('img_xcc', xcc)
            for cfg in (0, 1, 2):
                for ta, tb in layouts:
                    shapes = IMG_SHAPES + (IMG_SHAPES_TT if ta and tb else [])
                    if xcc:
                        shapes = shapes[:1] + shapes[2:]                         # work-queue forms: one shape fewer
                    for M, N, K, ks in shapes:
                        if bf16 and not (ta and tb) and K % 64:
                            K = (K + 63) // 64 * 64                              # header: K % 64 == 0 for a K-contiguous bf16 operand
                        A, Bm, bias, c0, prod = _img_data(M, N, K, bf16)
                        acc = i % 2 == 0
                        ref = prod + c0.double() if acc else prod
                        ga = _img_operand(E, A, ta, bf16, i, 'A')
                        gb = _img_operand(E, Bm, tb, bf16, i + 1, 'B')
                        gbias = G.inp(bias, DEV, offset=64, name='bias')
                        gc = G.out((M, N), DEV, ld=(N + 4, 2 * N, N)[i % 3], offset=64, fill=c0 if acc else None, name='C')
                        part = G.out((ks * M * N,), DEV, offset=64, name='part') if ks > 1 else None     # exactly ksplit * M * N floats
                        E.gemm_img(ga[0].t, gb[0].t, ta, tb, gbias.t, ks, cfg, out=gc.t, accumulate=acc, part=part.t if part else None, zeros=zeros.t)
                        torch.cuda.synchronize()
                        what = (M, N, K, ks, ta, tb, cfg, xcc, acc)
                        G.assert_close(gc.t, ref, 5e-6, what)
                        G.check_all(ga + gb + [gbias, gc, zeros])
                        if part:
                            part.check(written=False)
                        # bit-identical to the plain contiguous call (partial slabs are added in a fixed order)
                        plain = [(x[0].t.contiguous()) for x in (ga, gb)]
                        c2 = E.gemm_img(plain[0], plain[1], ta, tb, bias.to(DEV), ks, cfg, out=c0.to(DEV).clone() if acc else None, accumulate=acc)
                        assert torch.equal(gc.t, c2), what
                        i += 1
    finally:
        E.tune('img_xcc', 0)


def test_image_gemm_containment_fp16x2(E):
    """ss_op_split_image + ss_op_gemm_img over fp16 x 2 images: layouts, tile configurations and work-queue forms of
    test_image_gemm_against_fp64, ragged M (multiples of 8) / N (multiples of 4), K tails of the reduction-major pair, ldc > N, images
    with ldi > cols, the split-K partial slabs in a guarded scratch of exactly ksplit * M * N floats.  Bound of that test: 5e-6 against
    float64, and bit-identical to the plain contiguous call."""
    _img_cases(E, False, [(False, False), (False, True), (True, True)])


def test_image_gemm_containment_bf16_single_piece(E):
    """The single-piece form (plain bf16 operands): test_image_gemm_bf16_single_piece's layouts and bound (5e-6 against float64 on the
    same bf16 operands, bit-identical repeat)."""
    _img_cases(E, True, LAYOUTS4)


def test_image_gemm_containment_conv_windows(E):
    """The segmented K axis over a haloed slab with images split at other scales (test_image_gemm_conv_windows_and_scales, 5e-6): the
    output starts as the pattern, is not accumulated into, and has ldc > N."""
    g = torch.Generator().manual_seed(5)
    B, T, Ci, Co = 3, 40, 64, 128
    TP = T + 4
    x = torch.zeros(B, TP, Ci)
    x[:, 2:2 + T] = torch.randn(B, T, Ci, generator=g)
    w = torch.randn(Co, 5, Ci, generator=g) * 0.05
    xs = x.reshape(B * TP, Ci)
    rows = B * TP - 4
    ref = torch.zeros(rows, Co, dtype=torch.float64)
    for tap in range(5):
        ref += xs[tap:tap + rows].double() @ w[:, tap].double().t()
    zeros = G.inp(torch.zeros(256), DEV, offset=8, name='zeros_dev')
    for cfg in (0, 1, 2):
        gx, gw = G.inp(xs, DEV, ld=Ci + 4, offset=4, name='x'), G.inp(w.reshape(Co, 5 * Ci), DEV, ld=5 * Ci + 8, offset=12, name='w')
        ix, iw = G.out(xs.shape, DEV, ld=Ci + 8, offset=8, name='x.img'), G.out((Co, 5 * Ci), DEV, ld=5 * Ci + 16, offset=24, name='w.img')
        E.split_image(gx.t, 4.0, out=ix.t)
        E.split_image(gw.t, 64.0, out=iw.t)
        gc = G.out((rows, Co), DEV, ld=Co + 4, offset=64, name='C')
        # the conv window reads Ci columns of five consecutive slab rows: the segment stride is the image's row stride
        E.gemm_img(ix.t, iw.t, cfg=cfg, scale_a=4.0, scale_b=64.0, a_seg=(Ci, ix.ld), M=rows, K=5 * Ci, out=gc.t, zeros=zeros.t)
        torch.cuda.synchronize()
        G.assert_close(gc.t, ref, 5e-6, cfg)
        G.check_all([gx, gw, gc, zeros])
        ix.check(written=False)
        iw.check(written=False)


# --------------------------------------------------------------------------------------------- ss_op_conv_block
def _conv_block_guarded(E, x, w, bias, gamma, beta, dy, i):
    """ss_op_conv_block zeroes its scratch and copies every operand into haloed slabs of its own inside it before a kernel runs
    (engine.hip), so guarded inputs and a NaN scratch check, at this level, the copies, the stores into the dense outputs and the documented
    scratch size -- NOT what the conv / GroupNorm kernels read; that is checked with the engine on guarded memory
    (test_gpu_engine_containment.py)."""
    lib = E._capi.lib()
    B, T, Ci = x.shape
    Co = w.shape[0]
    ins = [G.inp(t, DEV, offset=(64, 3, 1, 5, 7, 9)[(k + i) % 6], name=n)
           for k, (n, t) in enumerate((('x', x), ('w', w), ('bias', bias), ('gamma', gamma), ('beta', beta)) + ((('dy', dy),) if dy is not None else ()))]
    scratch = G.out((lib.ss_op_conv_block_scratch(B, T, Ci, Co),), DEV, offset=64, name='scratch')           # exactly the stated size
    outs = {'y': G.out((B, T, Co), DEV, offset=(64, 1)[i % 2], name='y')}
    if dy is not None:
        outs.update(dx=G.out((B, T, Ci), DEV, offset=(3, 64)[i % 2], name='dx'), gw=G.out((Co * Ci, 5), DEV, offset=64, name='gw'),
                    gb=G.out((Co,), DEV, offset=1, name='gb'), ggamma=G.out((Co,), DEV, offset=2, name='ggamma'), gbeta=G.out((Co,), DEV, offset=3, name='gbeta'))
    o = {k: (v.t.view(Co, Ci, 5) if k == 'gw' else v.t) for k, v in outs.items()}
    res = E.conv_block(*[g.t for g in ins[:5]], dy=ins[5].t if dy is not None else None, scratch=scratch.t, out=o)
    torch.cuda.synchronize()
    G.check_all(ins + list(outs.values()))
    scratch.check(written=False)
    return res


def _conv_ref(x, w, bias, gamma, beta, dy=None):
    P = {'b.0.conv.weight': w.double().requires_grad_(dy is not None), 'b.0.conv.bias': bias.double().requires_grad_(dy is not None),
         'b.1.weight': gamma.double().requires_grad_(dy is not None), 'b.1.bias': beta.double().requires_grad_(dy is not None)}
    xr = x.double().requires_grad_(dy is not None)
    y = ref_model.conv_gn_relu(xr.transpose(1, 2), P, 'b').transpose(1, 2)
    if dy is None:
        return (y.detach(),)
    y.backward(dy.double())
    return y.detach(), xr.grad, P['b.0.conv.weight'].grad, P['b.0.conv.bias'].grad, P['b.1.weight'].grad, P['b.1.bias'].grad


def test_conv_block_containment(E):
    """ss_op_conv_block forward + backward: the REFERENCE's vectors of test_conv_block_against_reference_vectors (blocks.npz, 1e-4), then
    B = 1, T = 8 at the layer-0 widths Ci = 80 / 337 against the float64 oracle block at the same 1e-4; every operand at an offset base,
    the scratch guarded at exactly ss_op_conv_block_scratch() floats."""
    z = np.load(os.path.join(GOLD, 'blocks.npz'))
    w = W.make_weights('G3', W.default_hparams(), 3)
    pre = 'encoder_2.convolutions.0'
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x, dy = t(z['conv_x'].transpose(0, 2, 1)), t(z['conv_gy'].transpose(0, 2, 1))
    res = _conv_block_guarded(E, x, t(w[pre + '.0.conv.weight']), t(w[pre + '.0.conv.bias']), t(w[pre + '.1.weight']), t(w[pre + '.1.bias']), dy, 0)
    refs = (z['conv_y'].transpose(0, 2, 1), z['conv_gx'].transpose(0, 2, 1), z['conv_gw'], z['conv_gb'], z['conv_ggamma'], z['conv_gbeta'])
    for name, a, b in zip(('y', 'dx', 'gw', 'gb', 'ggamma', 'gbeta'), res, refs):
        G.assert_close(a, np.ascontiguousarray(b), TOL, name)
    for i, (B, T, Ci, Co) in enumerate([(1, 8, 80, 128), (1, 8, 337, 512), (1, 8, 80, 512)]):
        g = torch.Generator().manual_seed(T + Ci + Co)
        x = torch.rand(B, T, Ci, generator=g) * 2 - 1 + 0.3
        wt, bias = torch.randn(Co, Ci, 5, generator=g) * 0.1, torch.randn(Co, generator=g) * 0.1
        gamma, beta = 1 + 0.2 * torch.randn(Co, generator=g), 0.1 * torch.randn(Co, generator=g)
        dy = torch.randn(B, T, Co, generator=g) * 0.1
        res = _conv_block_guarded(E, x, wt, bias, gamma, beta, dy, i + 1)
        for name, a, b in zip(('y', 'dx', 'gw', 'gb', 'ggamma', 'gbeta'), res, _conv_ref(x, wt, bias, gamma, beta, dy)):
            G.assert_close(a, b, TOL, (name, B, T, Ci, Co))


@pytest.mark.parametrize('case', [(264, 1, 256), (1000, 3, 512), (4096, 1, 512), (264, 3, 512)], ids=lambda c: 't%d_b%d_co%d' % c)
def test_conv_block_forward_long_containment(E, case):
    """Forward-only long T (the chunked GroupNorm): inputs and bound of test_conv_block_forward_long (float64 oracle block, 1e-4, run-to-run
    bit identity -- here: bit-identical to the plain call)."""
    T, B, Co = case
    g = torch.Generator().manual_seed(T + 7 * B + Co)
    Ci = 80
    x = torch.rand(B, T, Ci, generator=g) * 2 - 1 + 0.3
    w = torch.randn(Co, Ci, 5, generator=g) * 0.1
    bias = torch.randn(Co, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(Co, generator=g)
    beta = 0.1 * torch.randn(Co, generator=g)
    y = _conv_block_guarded(E, x, w, bias, gamma, beta, None, T)
    G.assert_close(y, _conv_ref(x, w, bias, gamma, beta)[0], TOL, case)
    plain = E.conv_block(*[v.to(DEV) for v in (x, w, bias, gamma, beta)])
    assert torch.equal(y, plain)


# --------------------------------------------------------------------------------------------- ss_op_lstm_fwd / ss_op_lstm_bwd
def _blstm_case(E, B, T, H, In, persistent, seed):
    """One layer forward + backward through engine.blstm_layer with every operand of the recurrences pre-placed; float64 torch.nn.LSTM as in
    test_persistent_blstm_layer_against_torch / test_small_blstm_layer_against_torch (1e-4 on output, input gradient, every weight / bias gradient)."""
    g = torch.Generator().manual_seed(seed)
    ref = torch.nn.LSTM(In, H, 1, batch_first=True, bidirectional=True).double()
    if H <= 32:
        with torch.no_grad():
            for p in ref.parameters():
                p.copy_(torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1)
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    d_out = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64) * 0.1
    xr = x.clone().requires_grad_(True)
    y_ref, _ = ref(xr)
    y_ref.backward(d_out)
    bufs = {}

    def place(name, shape):
        if name in ('out', 'csave', 'd_out'):
            pre = pattern(shape)                                   # real frames and padding columns: the pattern
            pre[:, :2, :2 * H] = 0                                 # halo rows: zero (kernels.h), part of the input
            pre[:, T + 2:, :2 * H] = 0
            fill = pre
        elif name == 'gates':
            fill = 0.0                                             # the hook writes every row of it
        else:
            fill = 0.0 if persistent else None                     # scratch: zero only where a persistent kernel's sync words live
        bufs[name] = G.out(shape, DEV, offset=(64, 4, 8, 12)[len(bufs) % 4], fill=fill, name=name)
        return bufs[name].t

    f = lambda n: getattr(ref, n).detach().float().to(DEV)
    y, dx, grads = E.blstm_layer(x.float().to(DEV), (f('weight_ih_l0'), f('weight_ih_l0_reverse')), (f('weight_hh_l0'), f('weight_hh_l0_reverse')),
                                 (f('bias_ih_l0'), f('bias_ih_l0_reverse')), (f('bias_hh_l0'), f('bias_hh_l0_reverse')), d_out.float().to(DEV), place=place)
    torch.cuda.synchronize()
    what = (B, T, H, persistent)
    G.assert_close(y, y_ref.detach(), TOL, ('y',) + what)
    G.assert_close(dx, xr.grad, TOL, ('dx',) + what)
    for d, sfx in enumerate(('', '_reverse')):
        for a, n in zip(grads[d], ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0')):
            G.assert_close(a, getattr(ref, n + sfx).grad, TOL, (n + sfx,) + what)
    for gb in bufs.values():
        gb.check(written=False)
    for name in ('out', 'csave', 'd_out'):
        s = bits(bufs[name].t)
        assert not bool(s[:, :2, :2 * H].any()) and not bool(s[:, T + 2:, :2 * H].any()), (name, 'halo rows changed') + what
        assert bool((s[:, :, 2 * H:] == G.NAN32).all()), (name, 'padding columns past 2H changed') + what
        if name != 'd_out':
            assert not bool((s[:, 2:T + 2, :2 * H] == G.NAN32).any()), (name, 'real frame never written') + what
    if H > 32:                                                    # the H <= 32 kernels take no scratch (lstm_scratch: 0 floats, one is placed)
        assert bufs['scratch_fwd'].t.numel() == E.lstm_scratch(B, H, False) and bufs['scratch_bwd'].t.numel() == E.lstm_scratch(B, H, True)


BT = [(1, 1), (7, 8), (16, 37), (33, 8), (1, 37), (33, 1)]


def test_small_blstm_containment(E):
    """ss_op_lstm_fwd / _bwd at H in {1, 3, 8, 17, 31, 32}, B in {1, 7, 16, 33}, T in {1, 8, 37}: results as in
    test_small_blstm_layer_against_torch (1e-4), and the lstm_small_ld(H) - 2H padding columns and all halo rows of out / csave / d_out keep
    their pre-call contents bit for bit (header: "columns past 2H untouched")."""
    for H in (1, 3, 8, 17, 31, 32):
        for B, T in BT:
            _blstm_case(E, B, T, H, 96, False, 40 + H + T + B)


@pytest.mark.parametrize('H', [256, 512])
@pytest.mark.parametrize('persist', [1, 0], ids=['persistent', 'per_step'])
def test_large_blstm_containment(E, H, persist):
    """The decoder-sized recurrences as one persistent launch and as one launch per time step ("persist" 0), scratch sized exactly by the
    header's formulas (engine.lstm_scratch); reference and bound of test_persistent_blstm_layer_against_torch (1e-4)."""
    E.tune('persist', persist)
    try:
        for B, T in ((1, 8), (7, 37), (16, 1), (33, 8)) if persist else ((7, 8), (33, 37)):
            _blstm_case(E, B, T, H, 96, bool(persist), 100 + B + T)
    finally:
        E.tune('persist', 1)


# --------------------------------------------------------------------------------------------- ss_op_lstm_wgrad
WGRAD = [(1, 128, 4 * 132), (8, 512, 8 * 132 + 3), (8, 16, 5 * 196), (32, 256, 6 * 196), (32, 100, 1000)] + [(H, 200, 8 * 132 + 3) for H in (3, 12, 17, 24, 31)]


def test_lstm_wgrad_containment(E):
    """csrc/lstm_wgrad.hip at the shapes of test_fused_encoder_blstm_weight_gradients and test_fused_wgrad_any_width: x a column view of a
    wider guarded matrix, hout rows 2H apart, outputs accumulated into (pre-filled with zeros, guard only), scratch of exactly the
    documented size (engine.lstm_wgrad_scratch).  Bound of those tests: 2e-6 against float64, bit-identical to the plain call."""
    for i, (H, In, R) in enumerate(WGRAD):
        g = torch.Generator().manual_seed(3 + H + In)
        dg = torch.randn(R, 8 * H, generator=g) * 1e-3
        dg[0] = 0
        dg[-1] = 0                   # halo rows of a gradient slab are zero
        x = torch.randn(R, In, generator=g)
        hout = torch.tanh(torch.randn(R, 2 * H, generator=g))
        hout[0] = 0
        hout[-1] = 0
        gdg, gh = G.inp(dg, DEV, offset=(64, 3)[i % 2], name='dg'), G.inp(hout, DEV, offset=(5, 64)[i % 2], name='hout')
        gx = G.inp(x, DEV, ld=In + 24 if i % 2 else In + 21, offset=8 if i % 2 else 3, name='x')
        outs = [G.out(s, DEV, offset=o, fill=0.0, name=n) for s, o, n in (((2 * 4 * H, In), 64, 'gw_ih'), ((2 * 4 * H, H), 1, 'gw_hh'), ((4, 4 * H), 2, 'gb'))]
        scratch = G.out((E.lstm_wgrad_scratch(H, In),), DEV, offset=64, name='scratch')
        o = (outs[0].t.view(2, 4 * H, In), outs[1].t.view(2, 4 * H, H), outs[2].t.view(2, 2, 4 * H))
        gwih, gwhh, gb = E.lstm_wgrad(gdg.t, gx.t, gh.t, scratch=scratch.t, out=o)
        torch.cuda.synchronize()
        d64, x64, h64 = dg.double(), x.double(), hout.double()
        for d in range(2):
            dd = d64[:, d * 4 * H:(d + 1) * 4 * H]
            G.assert_close(gwih[d], dd.t() @ x64, 2e-6, ('gw_ih', H, In, R, d))
            ref_hh = dd[1:].t() @ h64[:-1, :H] if d == 0 else dd[:-1].t() @ h64[1:, H:]
            G.assert_close(gwhh[d], ref_hh, 2e-6, ('gw_hh', H, In, R, d))
            G.assert_close(gb[d, 0], dd.sum(0), 2e-6, ('gb', H, In, R, d))
            assert torch.equal(gb[d, 0], gb[d, 1])
        G.check_all([gdg, gh, gx] + outs)
        scratch.check(written=False)
        plain = E.lstm_wgrad(dg.to(DEV), x.to(DEV), hout.to(DEV))
        assert all(torch.equal(a, b) for a, b in zip((gwih, gwhh, gb), plain)), (H, In, R)


# --------------------------------------------------------------------------------------------- ss_interp_forward / ss_interp_backward
def test_interp_containment(E):
    """The interp.npz cases of test_interp_bit_exact_against_reference with x / draws / dy as guarded inputs and y, i0, lam, counts, dx as
    guarded outputs: values bit-exact against the reference's output, plan bit-exact, backward within that test's 1e-6."""
    z = np.load(os.path.join(GOLD, 'interp.npz'))
    engines = {}
    for i in range(int(z['n'])):
        pad = int(z[f'c{i}_max_len_pad'])
        if pad not in engines:
            engines[pad] = E.Engine('interp', W.default_hparams(max_len_pad=pad), 16, pad)
        eng = engines[pad]
        x = torch.from_numpy(z[f'c{i}_x'])
        B, T, Cc = x.shape
        ins = [G.inp(x, DEV, offset=(3, 64)[i % 2], name='x'), G.inp(torch.as_tensor(z[f'c{i}_len_seq']).int(), DEV, offset=1, name='len_seq'),
               G.inp(torch.as_tensor(z[f'c{i}_scales']).float().reshape(-1), DEV, offset=5, name='scales'),
               G.inp(torch.as_tensor(z[f'c{i}_len_seg']).int().reshape(-1), DEV, offset=7, name='len_seg')]
        outs = [G.out((B, pad, Cc), DEV, offset=(64, 1)[i % 2], name='y'), G.out((B, pad), DEV, dtype=torch.int32, offset=3, name='i0'),
                G.out((B, pad), DEV, offset=5, name='lam'), G.out((B,), DEV, dtype=torch.int32, offset=9, name='counts')]
        y, i0, lam, cnt = eng.interp_forward(*[g.t for g in ins], want_plan=True, out=tuple(o.t for o in outs))
        torch.cuda.synchronize()
        ri0, rlam, rcnt, rn = interp_np.interp_plan(z[f'c{i}_scales'], z[f'c{i}_len_seg'], z[f'c{i}_len_seq'], max_len_pad=pad)
        assert np.array_equal(y.cpu().numpy(), z[f'c{i}_y']), i
        assert np.array_equal(i0.cpu().numpy(), ri0) and np.array_equal(cnt.cpu().numpy(), rcnt)
        assert np.array_equal(lam.cpu().numpy(), rlam)
        G.check_all(ins + outs)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(i))
        gdy, gdx = G.inp(dy, DEV, offset=(64, 3)[i % 2], name='dy'), G.out((B, T, Cc), DEV, offset=(1, 64)[i % 2], name='dx')
        dx = eng.interp_backward(gdy.t, T, out=gdx.t)
        torch.cuda.synchronize()
        G.assert_close(dx, interp_np.interp_backward(dy.numpy(), ri0, rlam, rn, T), 1e-6, ('dx', i))
        G.check_all([gdy, gdx])


# --------------------------------------------------------------------------------------------- ss_collate, ss_melspec, ss_f0_normalize
def _p(t):
    return C.c_void_p(t.data_ptr())


def test_feature_kernels_containment(E):
    """ss_melspec / ss_f0_normalize on the features.npz fixture with guarded float64 inputs and float32 outputs; bounds of
    test_mel_spectrogram_and_f0_normalisation_against_reference_fixture (2e-6 / 2e-7 absolute, same unvoiced frames)."""
    lib = E._capi.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = np.load(os.path.join(GOLD, 'features.npz'))
    for u in range(2):
        wav, mb = torch.from_numpy(np.ascontiguousarray(z[f'u{u}_wav'], dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(z['mel_basis'], dtype=np.float64))
        gw, gm = G.inp(wav, DEV, offset=(1, 64)[u], name='wav'), G.inp(mb, DEV, offset=(64, 3)[u], name='mel_basis')
        frames = lib.ss_melspec_frames(wav.numel())
        gs = G.out((frames, mb.shape[1]), DEV, offset=(3, 64)[u], name='S')
        E._capi.check(lib.ss_melspec(_p(gw.t), wav.numel(), _p(gm.t), mb.shape[1], _p(gs.t), s))
        torch.cuda.synchronize()
        S = gs.t.cpu().numpy()
        assert S.shape == z[f'u{u}_S'].shape and float(np.abs(S - z[f'u{u}_S']).max()) <= 2e-6, u
        G.check_all([gw, gm, gs])
        f0 = torch.from_numpy(np.ascontiguousarray(z[f'u{u}_f0'], dtype=np.float64))
        gf, gn = G.inp(f0, DEV, offset=(5, 64)[u], name='f0'), G.out((f0.numel(),), DEV, offset=(64, 1)[u], name='f0norm')
        E._capi.check(lib.ss_f0_normalize(_p(gf.t), f0.numel(), _p(gn.t), s))
        torch.cuda.synchronize()
        fn, ref = gn.t.cpu().numpy(), z[f'u{u}_f0norm']
        assert np.array_equal(fn == -1e10, ref == -1e10)
        assert float(np.abs(fn - ref)[ref != -1e10].max()) <= 2e-7, u
        G.check_all([gf, gn])


def test_collate_containment(E):
    """ss_collate on the collate.npz fixture (test_device_batcher_against_reference_collator_fixture: bit-equal to the REFERENCE collator's
    batch): the resident corpus, the crop tables and the three outputs all guarded.  The crops are drawn with the collator's generator
    calls, as DeviceBatcher.assemble draws them."""
    from speechsplit_amd import data_loader as DL, hparams as HPM
    lib = E._capi.lib()
    z = np.load(os.path.join(GOLD, 'collate.npz'))
    hp = HPM.default_hparams(batch_size=6)
    c = DL.DeviceCorpus(DL.SyntheticUtterances(int(z['corpus_n']), seed=int(z['corpus_seed'])), DEV)
    items = [int(i) for i in z['items']]
    np.random.seed(int(z['np_seed']))
    row0, lens = [], []
    for i in items:
        n = min(int(np.random.randint(hp.min_len_seq, hp.max_len_seq + 1, size=2)[0]), hp.max_len_pad)
        left = int(np.random.randint(0, max(int(c.lens[i]) - n, 1), size=2)[0])
        lens.append(min(n, int(c.lens[i]) - left))
        row0.append(int(c.starts[i]) + left)
    B, T, n_mel, emb_dim = len(items), hp.max_len_pad, c.mel.shape[1], c.emb.shape[1]
    ins = [G.inp(c.mel, DEV, offset=3, name='mel_cat'), G.inp(c.f0, DEV, offset=1, name='f0_cat'), G.inp(c.emb, DEV, offset=5, name='emb_tab'),
           G.inp(torch.tensor(row0, dtype=torch.int64), DEV, offset=1, name='row0'), G.inp(torch.tensor(lens, dtype=torch.int32), DEV, offset=3, name='len'),
           G.inp(torch.tensor(items, dtype=torch.int32), DEV, offset=7, name='item')]
    outs = [G.out((B, T, n_mel), DEV, offset=1, name='mel'), G.out((B, T), DEV, offset=3, name='f0'), G.out((B, emb_dim), DEV, offset=5, name='emb')]
    E._capi.check(lib.ss_collate(*[_p(g.t) for g in ins], B, T, n_mel, emb_dim, *[_p(o.t) for o in outs], C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].t.cpu().numpy(), z['mel']) and np.array_equal(outs[2].t.cpu().numpy(), z['emb'])
    assert np.array_equal(outs[1].t.cpu().numpy().reshape(z['f0'].shape), z['f0']) and np.array_equal(np.asarray(lens), z['len_org'])
    G.check_all(ins + outs)
