"""tests/relayout_ref.py proven on the CPU, without a GPU.  Every check of tests/test_gpu_relayout.py is exact (zero differing bits), so what
has to be shown is that the references are right and that bit equality tells a subtly wrong kernel from a right one:

1. The references equal an independent formulation: torch's permute / flip / pad for the packs and unpacks, torch's bfloat16 cast for
   bf16_bits, a brute-force search over the powers of two for act_scale_ref, exact rational arithmetic for the fused bound.
2. An EMULATION of each kernel's own index arithmetic / loop gives the reference's bits on the cases the GPU test runs.
3. Each MUTANT differs in at least one bit on those cases: taps not flipped; the padding columns of wf not zero; (ci, k) swapped in the
   unpack; a copy made as a + 0.f (the scalar path of prep_kernel as it was: -0.0 becomes +0.0); len not clamped to [0, T] in copy_rows;
   act_scales running a bound of +inf down to the floor (the loop as it was); param_guard with `> limit`, without its last float4, or
   writing the word instead of OR-ing it."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import relayout_ref as R

F32 = np.float32
SMALL_CONV = R.CONV_SHAPES[:3]                              # the element-by-element emulation is slow: the three small shapes


# ------------------------------------------------------------------------------------------------ 1. references
@pytest.mark.parametrize('shape', R.CONV_SHAPES)
def test_pack_refs_are_torch(shape):
    Co, Ci, Cp = shape
    w = R.conv_weight(Co, Ci)
    wf, wb = R.conv_pack_ref(w, Cp)
    tw = torch.from_numpy(w)
    twf = torch.nn.functional.pad(tw.permute(0, 2, 1), (0, Cp - Ci))
    twb = tw.flip(2).permute(1, 2, 0)
    assert R.same_bits(wf, twf.contiguous().numpy()) and R.same_bits(wb, twb.contiguous().numpy())
    assert not wf[:, :, Ci:].any() and not np.signbit(wf[:, :, Ci:]).any()                  # +0.0 in the padding columns
    assert np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all()                  # both zeros occur in the weight
    # the pack is what the convolution reads: y[t][co] = sum_k sum_c x[t + k - 2][c] wf[co][k][c], and wb gives its adjoint
    x = torch.randn(1, Ci, 9, dtype=torch.float64)
    y = torch.nn.functional.conv1d(x, tw.double(), padding=2)
    xp = torch.nn.functional.pad(x, (2, 2))
    y2 = sum(torch.einsum('oc,bct->bot', torch.from_numpy(wf[:, k, :Ci]).double(), xp[:, :, k:k + 9]) for k in range(5))
    assert torch.allclose(y, y2, rtol=1e-12, atol=1e-12)
    dy = torch.randn(1, Co, 9, dtype=torch.float64)
    dx = torch.nn.functional.conv_transpose1d(dy, tw.double(), padding=2)
    dyp = torch.nn.functional.pad(dy, (2, 2))
    dx2 = sum(torch.einsum('co,bot->bct', torch.from_numpy(wb[:, k, :]).double(), dyp[:, :, k:k + 9]) for k in range(5))
    assert torch.allclose(dx, dx2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('shape', R.CONV_SHAPES)
def test_unpack_ref_inverts_the_pack(shape):
    Co, Ci, Cp = shape
    w = R.conv_weight(Co, Ci)
    wf, _ = R.conv_pack_ref(w, Cp)
    wf[:, :, Ci:] = np.nan
    assert R.same_bits(R.conv_unpack_ref(wf, Ci), w)
    g0 = R.conv_weight(Co, Ci, seed=1) + F32(1)
    acc = R.conv_unpack_ref(wf, Ci, g0)
    assert R.same_bits(acc, (torch.from_numpy(g0) + torch.from_numpy(w)).numpy()) and np.all(np.isfinite(acc))


def test_bf16_bits_is_torch():
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096).astype(F32), (rng.standard_normal(4096) * 1e-3).astype(F32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38, 65504.0, 1e-40, np.inf, -np.inf], F32)])
    a[:64] = (np.arange(64, dtype=np.uint32) * 0x8000 + 0x3F800000).view(F32)               # exact ties and their neighbours
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(a), want)
    assert R.bf16_bits(np.array([np.nan], F32))[0] & 0x7FC0 == 0x7FC0


def test_f32_round_and_bound():
    rng = np.random.default_rng(6)
    for _ in range(2000):                                   # against the definition: no float32 is nearer
        x = Fraction(float(rng.uniform(0, 1e6))) * Fraction(float(F32(rng.uniform(0, 64)))) + Fraction(float(F32(rng.uniform(0, 4))))
        f = R.f32_round(x)
        for c in (np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))):
            assert abs(Fraction(float(f)) - x) <= abs(Fraction(float(c)) - x)
    top = Fraction(float(np.finfo(F32).max))
    assert R.f32_round(top + Fraction(2) ** 103 - 1) == np.finfo(F32).max and np.isinf(R.f32_round(top + Fraction(2) ** 103))
    # a fused bound that differs from the twice-rounded one exists, so the header's "one fused multiply-add" is a statement with content
    assert np.sqrt(F32(16 * 64), dtype=F32) == 32
    rt, differ = np.sqrt(F32(16 * 192), dtype=F32), 0
    for _ in range(500):
        g, b = F32(rng.uniform(0, 64)), F32(rng.uniform(0, 4))
        differ += R.act_bound(np.array([g], F32), np.array([b], F32), 192) != F32(F32(rt * g) + b)
    assert differ > 0
    assert R.act_bound(np.array([np.nan, 2.0], F32), np.array([np.nan], F32), 64) == 64      # NaN elements do not enter the maxima
    assert R.act_bound(np.zeros(0, F32), np.zeros(0, F32), 64) == 0
    assert np.isinf(R.act_bound(np.array([3e38], F32), np.array([0], F32), 64))


def test_act_scale_ref_is_brute_force():
    rng = np.random.default_rng(7)
    bounds = [F32(0), F32(2048), np.nextafter(F32(2048), F32(np.inf)), F32(4096), F32(32768), F32(65536), F32(3.4e38), F32(2.0 ** 35),
              np.nextafter(F32(2.0 ** 35), F32(np.inf))] + [F32(10.0 ** e) for e in rng.uniform(-3, 38, 300)]
    for bd in bounds:
        s = R.act_scale_ref(bd)
        ok = [F32(2.0 ** k) for k in range(-20, 5) if Fraction(float(bd)) * Fraction(2) ** k <= 32768]
        assert s == (max(ok) if ok else F32(2.0 ** -20)) and 2.0 ** -20 <= s <= 16
        assert R.act_scale_emulated(bd) == s, bd
    assert R.act_scale_ref(F32(2048)) == 16 and R.act_scale_ref(np.nextafter(F32(2048), F32(np.inf))) == 8
    assert R.act_scale_ref(F32(np.inf)) == 16 == R.act_scale_emulated(F32(np.inf))


# ------------------------------------------------------------------------------------------------ 2. emulations, 3. mutants
@pytest.mark.parametrize('shape', SMALL_CONV)
def test_pack_emulation_and_mutants(shape):
    Co, Ci, Cp = shape
    w = R.conv_weight(Co, Ci)
    wf, wb = R.conv_pack_ref(w, Cp)
    ef, eb = R.conv_pack_emulated(w, Cp)
    assert R.n_diff(ef, wf) == 0 and R.n_diff(eb, wb) == 0
    _, mb = R.conv_pack_emulated(w, Cp, flip=False)
    assert R.n_diff(mb, wb) > 0, 'taps not flipped'
    if Cp > Ci:
        mf, _ = R.conv_pack_emulated(w, Cp, pad_zero=False)
        assert R.n_diff(mf, wf) > 0, 'padding columns not zero'


@pytest.mark.parametrize('shape', SMALL_CONV)
def test_unpack_emulation_and_mutants(shape):
    Co, Ci, Cp = shape
    gp = R.packed_grad(Co, Ci, Cp, np.nan)
    g0 = R.conv_weight(Co, Ci, seed=2) + F32(1)
    for base in (None, g0):
        ref = R.conv_unpack_ref(gp, Ci, base)
        assert np.all(np.isfinite(ref)), 'a padding column was read'
        assert R.n_diff(R.conv_unpack_emulated(gp, Ci, base), ref) == 0
        if Ci > 1:
            assert R.n_diff(R.conv_unpack_emulated(gp, Ci, base, swapped=True), ref) > 0, '(ci, k) swapped'
    assert R.n_diff(R.conv_unpack_ref(gp, Ci, g0), R.conv_unpack_ref(gp, Ci)) > 0           # accumulating is not overwriting


def test_prep_copy_is_a_copy_of_the_bits():
    rng = np.random.default_rng(8)
    a = R.signed_zeros(rng.standard_normal(1003).astype(F32), rng)
    a[7] = np.array([0x7FC00123], np.uint32).view(F32)[0]                                   # a NaN payload travels too
    b = R.signed_zeros(rng.standard_normal(1003).astype(F32), rng)
    b[7] = 1
    assert np.signbit(a[a == 0]).any()
    for vec in (True, False):
        assert R.n_diff(R.prep_emulated(a, None, vec), R.prep_ref(a)) == 0
        assert R.n_diff(R.prep_emulated(a, b, vec), R.prep_ref(a, b)) == 0
    assert R.n_diff(R.prep_emulated(a, None, True, plus_zero=True), R.prep_ref(a)) == 0     # the float4 path always copied
    bad = R.prep_emulated(a, None, False, plus_zero=True)
    assert R.n_diff(bad, R.prep_ref(a)) == int(np.count_nonzero((a == 0) & np.signbit(a))), 'a + 0.f: exactly the -0.0 elements differ'
    assert R.n_diff(bad, R.prep_ref(a)) > 0
    assert R.prep_takes_vec(8, 32, 48) and not R.prep_takes_vec(6, 32, 48) and not R.prep_takes_vec(8, 36, 48)


def test_copy_rows_ref_and_mutant():
    B, T, C = 5, 9, 3
    src = np.random.default_rng(9).standard_normal((B, T, C)).astype(F32)
    lens = [0, 4, T, T + 5, -3]
    ref = R.copy_rows_ref(src, lens)
    for b, n in enumerate((0, 4, T, T, 0)):
        assert R.same_bits(ref[b, :n], src[b, :n]) and not ref[b, n:].any() and not np.signbit(ref[b, n:]).any()
    assert R.same_bits(R.copy_rows_ref(src), src)
    unclamped = src.copy()
    for b, n in enumerate(lens):                            # mutant: t >= len[b] with len taken as it is
        unclamped[b, max(n, 0):] = 0
    assert R.n_diff(unclamped, ref) == 0                    # (zeroing is the same: what differs is what is READ beyond T, a containment matter)
    assert [R.ragged_len(n, T) for n in lens] == [0, 4, T, T, 0]


def test_act_scale_cases_and_mutant():
    T = 64
    seen = set()
    for name, gmax, bmax in R.act_cases(T):
        for C in R.ACT_C:
            g, b = R.act_block(C, gmax, bmax, 0)
            bd = R.act_bound(g, b, T)
            assert not np.isnan(bd)
            s = R.act_scale_ref(bd)
            assert R.act_scale_emulated(bd) == s, name
            seen.add((name, float(s)))
            if np.isinf(bd):
                assert s == 16 and R.act_scale_emulated(bd, inf_keeps=False) == F32(2.0 ** -20), 'the loop as it was runs +inf down to the floor'
    want = {'bound=2048': 16, 'just-above': 8, 'above-by-beta': 8, 'ordinary': 16, 'below': 16, 'negative': 2, 'mid': 2.0 ** -10, 'huge': 2.0 ** -20,
            'overflow': 16, 'inf-gamma': 16, 'inf-beta': 16, 'nan-gamma': 16, 'nan-beta': 16, 'zero': 16, 'floor': 2.0 ** -20}
    assert seen == {(k, float(v)) for k, v in want.items()}, seen


def test_guard_ref_and_mutants():
    limit = 2048.0
    for n in R.GUARD_N[:2]:
        clean = R.guard_arena(n)
        assert np.abs(clean).max() < limit
        for word in (0, 1, 0x80000003, 4):
            assert R.guard_ref(clean, limit, word) == word == R.guard_emulated(clean, limit, word)
            for name, v, bad in R.guard_values(limit):
                for pos in (0, n // 2, n - 1):
                    p = clean.copy()
                    p[pos] = v
                    want = (word | 4) if bad else word
                    assert R.guard_ref(p, limit, word) == want == R.guard_emulated(p, limit, word), (name, pos)
    p = R.guard_arena(1024)
    p[500] = limit
    assert R.guard_emulated(p, limit, 0, strict=False) != R.guard_ref(p, limit, 0), '> limit lets the limit itself through'
    p = R.guard_arena(1024)
    p[1023] = np.inf
    assert R.guard_emulated(p, limit, 0, drop_last=True) != R.guard_ref(p, limit, 0), 'the last float4 not looked at'
    assert R.guard_emulated(p, limit, 0x80000003, set_word=True) != R.guard_ref(p, limit, 0x80000003), 'the word written, not OR-ed'
