"""The wave-specialised form of the fp16 x 2 GEMM (csrc/gemm_bf16x3.hip, template flag WS; ss_tune("gemm_ws"), pytest -m gpu).

512 threads: waves 0-3 multiply, waves 4-7 stage (global loads two k-tiles ahead through two register sets, the split, the LDS stores), two
LDS buffers, ONE LDS-only barrier per k-tile.  Every launch here is a 128 x 128 tile (`want` = 1) of family f16x2 under gemm_ws = 2 unless
said otherwise, goes through ss_op_gemm_desc, and is judged per element by gemm_ref's SHARP and HONEST bars exactly as test_gpu_gemm_desc.py
judges the 256-thread kernels (its `problem` / `launch` / `Tuned` are used as they are; bars unchanged).  After every launch the text of
ss_debug_last_variant("gemm") must name the instance the case was meant to run (`variant_of` restates launch_cfg's choice).

Instances.  launch_cfg has a WS launch behind the transposing-read test and one behind its failure, per layout.  NN with tb and TN have both:
"tr ws" when gemm_tr allows it and every quad of the reduction-major operands is loadable (M % 4 for A^T, N % 4 for B^T), " ws" otherwise
(gemm_tr = 0, or the 130 x 132 shape for TN: M = 130).  NT has no reduction-major operand (CAN_TR is false), so gemm_tr 1 and 0 select the
SAME NT instance -- five distinct kernels, not six; NT is run under both values all the same and must say "NT f16x2 ws" twice.
A reduction-major A with a K-contiguous B (TA_only) never reaches this file's kernel (launch_gemm sends it to the fp32-MFMA kernel) and the
bf16 family is excluded from WS by its flag: under gemm_ws = 2 both must run what they run without it, and be right.
WS refuses none of the operand forms: a stager stores an image slot with the same 16-byte store as the 256-thread loop (sstore_one, `pre`),
so plain, img_b and img_ab all run "ws"; with gemm_ws = 2 it also takes precedence over the pipelined loop (TN / NN with B an image).  What
can be refused is the IMAGE (K % 8 for a K-contiguous operand, X % 8 and the transposing read for a reduction-major one): the kernel then
splits the fp32 operand in the loop with the same scale word, which gemm_ref judges as the same arithmetic.

Bit identity with the 256-thread one-buffer loop (gemm_ws = 0, gemm_pipe = 0, same gemm_tr) -- decided from the code: IDENTICAL, asserted.
Both kernels index everything by tid = threadIdx.x & 255: a stager thread loads, splits and stores exactly the slots the thread of the same
tid does in the one-buffer loop (setup / fetch / sstore_one are shared), a multiplier wave reads the same fragments (multiply() is shared)
and issues the same three MFMAs per fragment pair, k-tile after k-tile in ascending order into the same accumulators; the epilogue is shared.
The two buffers and the barrier change when a tile is staged, not what is multiplied or in which order.  So the bits must agree wherever the
launch itself is deterministic: ksplit 1, partial slabs at any ksplit, atomics up to ksplit 2 (two fp32 atomics onto a zero commute; three
or more commit in arrival order).  A missing wait between the stagers and the multipliers would show here as different bits AND against
float64: K = 8 .. 160 gives 1, 2, 3 and 5 k-tiles (odd and even counts for the two buffers, with and without a partial last tile), ksplit up
to 5 at K = 96 slices with no k-tile at all (the barrier count must still match: 1 + nk on both sides).

gemm_ws = 1 (the measured heuristic: not for TN, and at most 320 workgroups): NT 256 x 256 x 32 (4 tiles) says "ws", NT 2304 x 2304 x 32
(324 tiles) and TN do not.

Each launch prints `FIG <case> ... sharp=<worst ratio> honest=<worst ratio>` (1.0 = at the bar).  Worst over this file's 3734 launches on an
MI355X (profiles/r05/variant_knobs/test_figures.txt): fp16 x 2 sharp 0.24 (NN with tb, 130 x 132 x 8, ksplit 5), honest
0.12, the same for the 256-thread loop and the wave-specialised form in every case (the bits agree); bf16 x 3 0.07 / 0.07, bf16 honest 0.37; no
element outside a write set changed."""
import functools

import pytest

from tests import test_gpu_gemm_desc as D
from tests.test_gpu_gemm_desc import E, Tuned, problem  # noqa: F401  (E: the module fixture)

pytestmark = pytest.mark.gpu
LAYOUTS = ('NT', 'NN_tb', 'TN')
NAME = {'NT': 'NT', 'NN_tb': 'NN', 'TN': 'TN'}
KS = (8, 32, 40, 64, 72, 96, 100, 160)
SHAPES = ((72, 72), (128, 128), (130, 132), (136, 264))
KSPLITS = (1, 2, 3, 5)


def variant_of(layout, family, M, N, tr, ws):
    """launch_cfg's choice for a 128 x 128 tile over test_gpu_gemm_desc's dense geometries (16-byte aligned bases, strides % 4 == 0), no image
    taken by the pipelined loop (gemm_pipe = 0 or gemm_ws = 2 wherever an image is given)."""
    ta, tb = D.LAYOUTS[layout]
    quads = (not ta or M % 4 == 0) and (not tb or N % 4 == 0)
    use_tr = (ta or tb) and tr != 0 and (tr == 1 or not (ta and tb)) and family != 'bf16' and quads
    use_ws = family == 'f16x2' and ws
    return f'128x128 {NAME[layout]} {family}' + (' tr' if use_tr else '') + (' ws' if use_ws else '')


@functools.lru_cache(maxsize=None)
def reference(p, family, sa, sb):
    return D.reference_of(p, family, sa, sb)


def both(E, p, layout, tr, *, family='f16x2', part=False, tag='', same_bits=None, **kw):
    """Problem p on the 256-thread one-buffer loop, then under gemm_ws = 2: both judged against float64, the instance asserted, the bits
    compared where the launch is deterministic (same_bits=None: decided from ksplit and the slabs)."""
    d = p.d
    ref = reference(p, family, kw.get('sa', 16.0), kw.get('sb', 16.0))
    slabs = part and d.ksplit > 1 and d.row_mask[0] == 0 and d.N % 4 == 0 and p.bias is None       # launch_gemm_bf16x3 keeps the slabs
    if same_bits is None:
        same_bits = slabs or d.ksplit <= 2
    tag = f'ws {layout} tr={tr} {d.M}x{d.N}x{d.K} ks={d.ksplit}{" part" if part else ""} {tag}'
    with Tuned(E, gemm_ws=0, gemm_pipe=0, gemm_tr=tr):
        base = D.launch(E, p, family, want=1, part=part, tag=tag + ' [256 threads]', ref=ref, **kw)
        assert E.last_variant('gemm') == variant_of(layout, family, d.M, d.N, tr, False), (tag, E.last_variant('gemm'))
    with Tuned(E, gemm_ws=2, gemm_tr=tr):
        out = D.launch(E, p, family, want=1, part=part, tag=tag + ' [ws]', ref=ref, bits_of=base if same_bits else None, **kw)
        ran = E.last_variant('gemm')
    assert ran == variant_of(layout, family, d.M, d.N, tr, True), (tag, 'launched', ran)
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=[f'{m}x{n}' for m, n in SHAPES])
@pytest.mark.parametrize('tr', (1, 0), ids=['tr1', 'tr0'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_k_tiles_shapes_and_split_k(E, layout, tr, shape):
    """Every K x ksplit of the docstring on one M x N, split-K through atomics and through partial slabs."""
    M, N = shape
    for K in KS:
        for ks in KSPLITS:
            p = problem(M, N, K, layout, ksplit=ks)
            both(E, p, layout, tr, tag='atomics')
            if ks > 1:
                both(E, p, layout, tr, part=True)


@pytest.mark.parametrize('tr', (1, 0), ids=['tr1', 'tr0'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_batch_and_epilogue(E, layout, tr):
    """batch 2 (with and without a split), bias, accumulate onto a random C, the row mask over haloed slabs (halo rows keep their bits)."""
    both(E, problem(136, 132, 72, layout, batch=2, bias=True), layout, tr, tag='batch 2')
    both(E, problem(136, 132, 100, layout, batch=2, ksplit=3), layout, tr, part=True, tag='batch 2')
    both(E, problem(130, 136, 100, layout, bias=True), layout, tr, tag='bias')
    both(E, problem(130, 136, 100, layout, ksplit=2, bias=True), layout, tr, tag='bias')
    both(E, problem(130, 136, 100, layout, accum=True, c0='rand', bias=True), layout, tr, tag='accum onto C0')
    both(E, problem(136, 136, 160, layout, ksplit=3, c0='rand'), layout, tr, part=True, tag='onto C0')
    mask = (40, 2, 2, 38)
    both(E, problem(4 * 40 - 4, 72, 40, layout, row_mask=mask, bias=True), layout, tr, tag='row mask')
    both(E, problem(4 * 40 - 4, 136, 100, layout, row_mask=mask, accum=True, c0='rand'), layout, tr, tag='row mask accum')


@pytest.mark.parametrize('scale', (16.0, 4.0, 64.0), ids=['s16', 's4', 's64'])
@pytest.mark.parametrize('tr', (1, 0), ids=['tr1', 'tr0'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_operand_forms(E, layout, tr, scale):
    """plain (fp32 operands split in the loop with the scale word), img_b, img_ab: every form runs "ws"; where an image cannot be taken
    (K = 100 for a K-contiguous operand, 130 x 132 or gemm_tr = 0 for a reduction-major one) the in-loop split with the same word."""
    s = scale
    forms = {'plain': dict(pre_scale=(s, s), sa=s, sb=s), 'img_b': dict(pre_scale=(s, s), imgs=(None, s), sa=s, sb=s),
             'img_ab': dict(pre_scale=(s, s), imgs=(s, s), sa=s, sb=s)}
    for M, N in ((136, 264), (130, 132)):
        for K in (72, 100):
            for how, kw in forms.items():
                both(E, problem(M, N, K, layout), layout, tr, tag=f'{how} scale {s:g}', **kw)
                both(E, problem(M, N, K, layout, ksplit=3), layout, tr, part=True, tag=f'{how} scale {s:g}', **kw)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_ws_takes_precedence_over_the_pipelined_loop(E, layout):
    """gemm_pipe = 1 (default) and B an image: the pipelined loop without gemm_ws for TN and NN with tb, the wave-specialised form with
    gemm_ws = 2 -- same bits (both equal the one-buffer loop's), same bars."""
    p = problem(136, 264, 160, layout, ksplit=2)
    kw = dict(pre_scale=(16.0, 16.0), imgs=(16.0, 16.0), want=1, part=True, ref=reference(p, 'f16x2', 16.0, 16.0))
    piped = D.launch(E, p, 'f16x2', tag=f'ws {layout} default knobs', **kw)
    want = '128x128 NT f16x2' if layout == 'NT' else f'128x128 {NAME[layout]} f16x2 tr pipe apre'
    assert E.last_variant('gemm') == want, E.last_variant('gemm')
    with Tuned(E, gemm_ws=2):
        D.launch(E, p, 'f16x2', tag=f'ws {layout} gemm_ws=2 over gemm_pipe=1', bits_of=piped, **kw)
        assert E.last_variant('gemm') == variant_of(layout, 'f16x2', 136, 264, 1, True), E.last_variant('gemm')


def test_what_ws_does_not_serve_falls_back(E):
    """gemm_ws = 2 with a reduction-major A against a K-contiguous B (the fp32-MFMA kernel) and with the bf16 family (every layout): the
    kernels they run without it, the same bits, right."""
    for K in (40, 100):
        p = problem(136, 132, K, 'TA_only', ksplit=2)
        base = D.launch(E, p, 'f16x2', want=1, tag=f'ws TA_only K={K} gemm_ws=0')
        with Tuned(E, gemm_ws=2):
            D.launch(E, p, 'f16x2', want=1, tag=f'ws TA_only K={K} gemm_ws=2', bits_of=base)
            assert E.last_variant('gemm').endswith(' TA f32'), E.last_variant('gemm')
        for layout in LAYOUTS:
            for tr in (1, 0):
                both(E, problem(136, 132, K, layout, ksplit=2), layout, tr, family='bf16', part=True, tag='bf16 family')
                both(E, problem(136, 132, K, layout, bias=True), layout, tr, family='bf16x3', tag='bf16x3 family')


def test_ws1_heuristic(E):
    """gemm_ws = 1: NT below the limit of 320 workgroups runs "ws", NT above it (324 tiles) and TN do not; all three right."""
    cases = (('NT', 256, 256, True), ('TN', 256, 256, False), ('NT', 2304, 2304, False))
    for layout, M, N, ws in cases:
        p = problem(M, N, 32, layout)
        with Tuned(E, gemm_ws=1):
            D.launch(E, p, 'f16x2', want=1, tag=f'ws1 {layout} {M}x{N}x32')
            ran = E.last_variant('gemm')
        assert ran == variant_of(layout, 'f16x2', M, N, 1, ws), (layout, M, N, ran)
    with Tuned(E, gemm_ws=1):                               # 2 x 2 tiles x batch 2 x ksplit 2 = 16 workgroups: the grid counts them all
        D.launch(E, problem(256, 256, 100, 'NN_tb', batch=2, ksplit=2), 'f16x2', want=1, part=True, tag='ws1 NN_tb batch 2 ks=2')
        assert E.last_variant('gemm') == '128x128 NN f16x2 tr ws', E.last_variant('gemm')


@pytest.mark.parametrize('layout', LAYOUTS)
def test_inside_guard_memory(E, layout):
    """A, B, both images, the partial slabs and C end where guard memory begins (tests/guarded.py): K = 100, ksplit 2 -- the second slice
    ends in a partial k-tile, which the stagers fetch with predicated loads -- and 130 rows / 136 columns past the tile edge."""
    for tr in (1, 0):
        both(E, problem(136, 136, 100, layout, ksplit=2), layout, tr, part=True, guard=True, pre_scale=(16.0, 16.0), imgs=(16.0, 16.0), tag='guard images')
        both(E, problem(130, 132, 100, layout, ksplit=2, bias=True), layout, tr, guard=True, tag='guard plain')
