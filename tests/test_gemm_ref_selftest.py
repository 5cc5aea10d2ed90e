"""CPU self-test of tests/gemm_ref.py: a correct float32 restatement of every family passes both judgements at every descriptor feature, and
every wrong variant in gemm_ref.VARIANTS is reported, by the judgement that should see it.  No device, no library.

Separation (worst error / sharp bar, the inputs of `case('k8')`: K = 8, row magnitudes over 2^6): the dropped lo.hi product is reported at
>= 10x the bar and a single bf16 rounding where bf16 x 3 is expected at >= 1000x; the measured factors are printed by
test_sharp_check_separates_the_two_precision_mistakes (numpy, these inputs: 512x and 3.3e3x the sharp bar; 67x and 832x the honest bar)."""
import numpy as np
import pytest
import torch

import gemm_ref as R

F32 = np.float32


def _operand(rng, X, K, spread=6):
    """[X, K] float32, row x scaled by a power of two between 2^-spread and 1 -- a max-norm judgement would hide the small rows."""
    return (rng.standard_normal((X, K)) * 2.0 ** -rng.integers(0, spread + 1, (X, 1))).astype(F32)


def _place(flat, index, values):
    flat[index.reshape(-1)] = values.reshape(-1)


CASES = ('nt', 'tn', 'nn_tb', 'ta_only', 'k8', 'split3_bias', 'split5_empty', 'accum', 'conv_seg', 'wgrad_seg', 'batch3', 'shared_b', 'mask', 'rowmap',
         'scales')


def case(name, family='f32', seed=0):
    """(desc, a, b, c0, bias) of one feature; the buffers hold NaN wherever the descriptor does not point."""
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    M, N, K, batch, ta, tb = 40, 24, 72, 1, False, False
    kw, bias, ageom, bgeom = {}, None, None, None
    if name == 'tn':
        ta, tb = True, True
    elif name == 'nn_tb':
        tb = True
    elif name == 'ta_only':
        ta = True
    elif name == 'k8':
        K = 8
    elif name == 'split3_bias':
        kw['ksplit'], kw['accum'] = 3, True
        bias = (0.01 * rng.standard_normal(N)).astype(F32)
    elif name == 'split5_empty':
        kw['ksplit'], kw['accum'] = 5, True                 # 3 k-tiles over 5 slices: two are empty
    elif name == 'accum':
        kw['accum'] = True
    elif name == 'conv_seg':                                # k = 5 convolution over haloed slabs [3][T + 4][Ci] read as one matrix
        Ci, T = 32, 20
        M, K = 3 * (T + 4) - 4, 5 * Ci
        ageom = R.Geom(8, Ci + 8, 0, Ci, Ci + 8)
    elif name == 'wgrad_seg':                               # TN, A reduction-major with segmented columns: dW[tap * Ci + ci][co]
        Ci = 8
        ta, tb, M, K = True, True, 5 * Ci, 44
        ageom = R.Geom(0, Ci, 0, Ci, Ci)
    elif name == 'batch3':
        batch = 3
    elif name == 'shared_b':
        batch = 2
    elif name == 'mask':                                    # 4 utterances, T = 6, TP = 10
        M = 4 * 10 - 4
        kw['row_mask'] = (10, 2, 2, 8)
        bias = rng.standard_normal(N).astype(F32)
    elif name == 'rowmap':
        M = 4 * 6
        kw['rm'] = (6, 10)
    elif name == 'scales':                                  # A at 2^-20 with its measured scale, B with the fixed scale 4
        kw['sb'] = 4.0
    lda = (M if ta else K) + 4
    ldb = (N if tb else K) + 8
    ldc = N + 4
    if ageom is None:
        ageom = R.Geom(16, lda, (K if ta else M) * lda + 12 if batch > 1 else 0)
    if bgeom is None:
        bgeom = R.Geom(8, ldb, 0 if name == 'shared_b' or batch == 1 else (K if tb else N) * ldb + 4)
    rows_c = M if not kw.get('rm') else 4 * 10
    d = R.Desc(ageom, bgeom, 4, ldc, rows_c * ldc + 20 if batch > 1 else 0, M, N, K, batch, ta, tb, family=family, **kw)
    na, nb, nc = R.spans(d)
    if name == 'shared_b':
        nb = batch * N * ldb + 8                            # room for the variant that strides a shared B
    a, b = np.full(na + 8, np.nan, F32), (rng.standard_normal(nb + 8).astype(F32) if name == 'shared_b' else np.full(nb + 8, np.nan, F32))
    if name in ('conv_seg', 'wgrad_seg'):                   # overlapping rows: fill the slab itself
        a[:] = _operand(rng, 1, a.size, 0)[0]
    else:
        scale = 2.0 ** -20 if name == 'scales' else 1.0
        _place(a, R.a_index(d), np.stack([_operand(rng, M, K) for _ in range(batch)]) * F32(scale))
        if name == 'scales':
            d.sa = R.pow2_scale_of(np.nanmax(np.abs(a)))
    if name != 'shared_b':
        _place(b, R.b_index(d), np.stack([_operand(rng, N, K) for _ in range(batch if bgeom.bstride else 1)] * (1 if bgeom.bstride else batch)))
    c0 = (rng.standard_normal(nc + 8) * 3).astype(F32)
    c0[::7] = np.nan                                        # prior bits that must survive include NaNs
    if d.accum:
        c0[R.c_index(d).reshape(-1)] = rng.standard_normal(d.batch * M * N).astype(F32) if name == 'accum' else 0
    return d, a, b, c0, bias


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('name', CASES)
def test_correct_restatement_passes_every_feature(name, family):
    d, a, b, c0, bias = case(name, family)
    fails, fig = R.judge(R.reference(d, a, b, c0, bias), c0, R.simulate(d, a, b, c0, bias))
    assert not fails, (name, family, fails, fig)
    assert fig['untouched'] == 0 and fig['sharp'] <= 1.0 and fig['honest'] <= 1.0


# variant -> (case, family, the judgement that must report it)
WRONG = {
    'bias_every_slice': ('split3_bias', 'bf16x3', 'sharp'),
    'mask_shifted': ('mask', 'f32', 'untouched'),
    'mask_ignored_value': ('mask', 'f16x2', 'untouched'),
    'mask_ignored_zero': ('mask', 'bf16x3', 'untouched'),
    'segment_wrap_early': ('conv_seg', 'f32', 'sharp'),
    'segstride_not_on_image': ('conv_seg', 'f16x2', 'sharp'),
    'cstride_ignored': ('batch3', 'f32', 'sharp'),
    'shared_b_strided': ('shared_b', 'bf16x3', 'sharp'),
    'rm_TP_as_rm_T': ('rowmap', 'f16x2', 'untouched'),
    'accum_overwrites': ('accum', 'f32', 'sharp'),
    'scale_not_undone': ('scales', 'f16x2', 'sharp'),
    'lo_hi_dropped': ('k8', 'f16x2', 'sharp'),
    'k_tile_skipped': ('split3_bias', 'f32', 'sharp'),
    'bf16_single_rounding': ('k8', 'bf16x3', 'sharp'),
}


def test_every_variant_has_a_case():
    assert set(WRONG) == set(R.VARIANTS)


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_wrong_variant_is_reported(variant):
    name, family, kind = WRONG[variant]
    d, a, b, c0, bias = case(name, family)
    ref = R.reference(d, a, b, c0, bias)
    assert not R.judge(ref, c0, R.simulate(d, a, b, c0, bias))[0]
    fails, fig = R.judge(ref, c0, R.simulate(d, a, b, c0, bias, variant))
    assert kind in fails, (variant, fails, fig)


def test_small_rows_are_what_the_honest_check_adds():
    """A mistake confined to the rows of small magnitude passes the max-norm 5e-6 and fails the per-element honest bar."""
    d, a, b, c0, bias = case('nt', 'f32')
    ref = R.reference(d, a, b, c0, bias)
    out = R.simulate(d, a, b, c0, bias)
    idx = R.c_index(d)[0]
    small = int(np.abs(ref.honest[0]).max(1).argmin())
    out[idx[small]] *= F32(1.0 + 1e-4)
    got = out[idx].astype(np.float64)
    assert np.abs(got - ref.honest[0]).max() / np.abs(ref.honest[0]).max() < 5e-6
    fails, _ = R.judge(ref, c0, out)
    assert 'honest' in fails and 'sharp' in fails


def test_sharp_check_separates_the_two_precision_mistakes():
    for variant, least in (('lo_hi_dropped', 10.0), ('bf16_single_rounding', 1000.0)):
        name, family, _ = WRONG[variant]
        d, a, b, c0, bias = case(name, family)
        _, fig = R.judge(R.reference(d, a, b, c0, bias), c0, R.simulate(d, a, b, c0, bias, variant))
        print(f'{variant}: worst error = {fig["sharp"]:.3g} x the sharp bar, {fig["honest"]:.3g} x the honest bar')
        assert fig['sharp'] >= least, (variant, fig)


def test_scales_rounding_and_packers():
    assert [R.pow2_scale_of(m) for m in (1.0, 250.0, 128.0, 255.9, 2.0 ** -30, 2.0 ** 20, 0.0)] == \
        [128.0, 1.0, 1.0, 1.0, 2.0 ** 37, 2.0 ** -13, 2.0 ** 60]
    for m in (3e-7, 0.9, 17.0, 6e4):
        assert 128.0 <= m * R.pow2_scale_of(m) < 256.0
    x = np.random.default_rng(1).standard_normal(4096).astype(F32) * 100
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]      # ties: to even
    assert np.array_equal(R.bf16_rne(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert np.array_equal(R.pack_bf16(x), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    g = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -12, -0.3, 2.0 ** -20, 0.0, 100.0, 1e-9], F32)
    img = R.pack_image(g, 16.0)
    assert img.shape == (1, 16)
    hi, lo = img[0, :8].view(np.float16).astype(np.float64), img[0, 8:].view(np.float16).astype(np.float64)
    assert hi[0] == 16.0 and lo[0] == 0.0
    assert hi[1] == 16.0 and lo[1] == 2.0 ** -7              # the tie 16 + 2^-7 goes to the even 16; the residual is the lo piece
    assert hi[2] == 16.0 + 2.0 ** -6 and lo[2] == -2.0 ** -8
    assert np.abs(hi + lo - 16.0 * g.astype(np.float64)).max() <= 2.0 ** -25 + 2.0 ** -22 * 1600
    assert img.view(F32).size == g.size                     # the image has the fp32 buffer's geometry
    for s in (4.0, 64.0):
        h2, l2 = R.split_f16(g, s)
        assert np.array_equal(R.pack_image(g, s)[0, :8], h2.view(np.uint16)) and np.array_equal(R.pack_image(g, s)[0, 8:], l2.view(np.uint16))


def test_addressing_matches_the_operand_comment():
    g = R.Geom(5, 7, 100, 3, 11)
    idx = R.operand_index(g, 4, 8, 2, False)
    for bt, x, k in ((0, 0, 0), (1, 3, 7), (0, 2, 3), (1, 1, 5)):
        assert idx[bt, x, k] == 5 + bt * 100 + x * 7 + (k // 3) * 11 + k % 3
    idt = R.operand_index(g, 4, 8, 2, True)
    for bt, x, k in ((0, 0, 0), (1, 3, 7), (0, 2, 3)):
        assert idt[bt, x, k] == 5 + bt * 100 + k * 7 + (x // 3) * 11 + x % 3
    d = R.Desc(R.Geom(0, 8), R.Geom(0, 8), 3, 10, 1000, 12, 4, 8, 2, rm=(6, 10), row_mask=(0, 0, 0, 0))
    assert R.c_index(d)[1, 7, 2] == 3 + 1000 + (10 + 1) * 10 + 2
    assert R.a_index(d)[0, 7, 1] == (10 + 1) * 8 + 1
    dm = d.replace(rm=(0, 0), row_mask=(10, 2, 2, 8), M=16)
    assert R.written_rows(dm).tolist() == [(m + 2) % 10 in range(2, 8) for m in range(16)]
    assert R.Desc(R.Geom(), R.Geom(), 0, 1, 0, 1, 1, 100, ksplit=5, kt=32).slices() == [(0, 32), (32, 64), (64, 96), (96, 100), (100, 100)]
    assert R.Desc(R.Geom(), R.Geom(), 0, 1, 0, 1, 1, 100, ksplit=3, kt=32).k_len() == 64
