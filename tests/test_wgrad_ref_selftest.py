"""tests/wgrad_ref.py proven on the CPU, without a GPU.

1. The float64 reference (matrix products over shifted rows) equals the header's four sums written as plain loops, on a small case.
2. An emulation of the kernel's own order (fp32 FMA chains per row group, float64 sums in group order, one rounding, one fp32 add onto the
   prefill) stays inside the budget on every case tests/test_gpu_wgrad_table.py runs.
3. Each wrong kernel falls outside it: W_hh paired with the same row instead of r +- 1; the last row of a row group dropped; directions
   swapped in a straddling block; the bias taken from column H instead of 32; one row group left out of the reduction.
4. The case list holds every value the tests are meant to cover."""
import numpy as np
import pytest

import wgrad_ref as R

F32 = np.float32


def ratio(got, ref, budget):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


def worst(got, s, m, pre, L):
    return max(ratio(g, p.astype(np.float64) + si, b) for g, si, p, b in zip(got, s, pre, R.wgrad_budget(s, m, pre, L)))


def test_reference_is_the_triple_loop():
    H, In, Rr = 3, 5, 7
    dG, X, Hout, pre = R.case_data(H, In, Rr)
    s, m = R.wgrad_ref(dG, X, Hout, H, pre)
    gwih, gwhh, gb = s[0].reshape(2, 4 * H, In), s[1].reshape(2, 4 * H, H), s[2].reshape(2, 2, 4 * H)
    d64, x64, h64 = dG.astype(np.float64), X.astype(np.float64), Hout.astype(np.float64)
    for d in range(2):
        for n in range(4 * H):
            for k in range(In):
                assert np.isclose(gwih[d, n, k], sum(d64[r, d * 4 * H + n] * x64[r, k] for r in range(Rr)), rtol=1e-13, atol=1e-14)
            for k in range(H):
                want = (sum(d64[r + 1, n] * h64[r, k] for r in range(Rr - 1)) if d == 0 else
                        sum(d64[r, 4 * H + n] * h64[r + 1, H + k] for r in range(Rr - 1)))
                assert np.isclose(gwhh[d, n, k], want, rtol=1e-13, atol=1e-14)
            assert np.isclose(gb[d, 0, n], d64[:, d * 4 * H + n].sum(), rtol=1e-13, atol=1e-14) and gb[d, 0, n] == gb[d, 1, n]
    assert all((mi >= np.abs(si) - 1e-12).all() for si, mi in zip(s, m))


def test_row_zero_must_be_zero():
    """the forward bias rides in the forward h tile (dG[r + 1]): with a non-zero row 0 the kernel's order misses it, and only it"""
    H, In, Rr, RG = 4, 5, 70, 2
    dG, X, Hout, pre = R.case_data(H, In, Rr)
    assert not dG[0].any()
    dG[0] = 1.5
    s, m = R.wgrad_ref(dG, X, Hout, H, pre)
    got = R.wgrad_emulated(dG, X, Hout, H, RG, pre)
    bud = R.wgrad_budget(s, m, pre, R.chain_len(Rr, RG))
    assert ratio(got[0], pre[0] + s[0], bud[0]) <= 1.0 and ratio(got[1], pre[1] + s[1], bud[1]) <= 1.0
    gb, want = got[2].reshape(2, 2, 4 * H), (pre[2] + s[2]).reshape(2, 2, 4 * H)
    assert np.allclose(want[0] - gb[0], 1.5, atol=1e-5) and np.allclose(want[1], gb[1], atol=1e-5)


def test_sizes():
    assert [R.small_ld(H) for H in (1, 2, 3, 4, 8, 16, 17, 31, 32)] == [2, 4, 8, 8, 16, 32, 36, 64, 64]
    assert R.tiles(32, 200) == 4 * (4 + 1) and R.tiles(8, 64) == 1 * (1 + 2) and R.tiles(17, 65) == 3 * (2 + 2) and R.tiles(1, 1) == 3
    assert R.chain_len(1059, 16) == 128 and R.chain_len(1, 1) == 64 and R.chain_len(1025, 16) == 128 and R.chain_len(1024, 16) == 64
    assert R.chain_len(1025, 7) == 192 and R.chain_len(63, 8) == 64


def test_cases_hold_every_value():
    Hs, Ins, Rs, RGs, modes = (set(c[i] for c in R.CASES) for i in range(5))
    assert Hs >= {1, 2, 4, 8, 16, 32, 3, 17, 31} and Ins >= {1, 3, 63, 64, 65, 200} and Rs >= {1, 2, 63, 64, 65, 1024, 1025}
    assert RGs >= {1, 7, 8, 9, 16} and modes == {'vec', 'odd', 'off'}
    assert any(m == 'vec' and In % 4 for _, In, _, _, m in R.CASES)                          # X aligned with In % 4 != 0
    assert any(Rr < 64 * RG for _, _, Rr, RG, _ in R.CASES)                                   # empty row groups
    assert any(In < 64 for _, In, _, _, _ in R.CASES)
    assert len(R.TABLE) == 3 and len({t[0] for t in R.TABLE}) == 3 and len({t[1] for t in R.TABLE}) == 3 and len({t[2] for t in R.TABLE}) == 3


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_emulation_stays_inside_the_budget(case):
    H, In, Rr, RG, _ = case
    dG, X, Hout, pre = R.case_data(H, In, Rr)
    s, m = R.wgrad_ref(dG, X, Hout, H, pre)
    q = worst(R.wgrad_emulated(dG, X, Hout, H, RG, pre), s, m, pre, R.chain_len(Rr, RG))
    assert q <= 1.0, q


@pytest.mark.parametrize('mutant', ('same_row', 'drop_last', 'swap_dir', 'bias_col', 'skip_group'))
@pytest.mark.parametrize('case', (R.CASES[1], R.CASES[3], R.CASES[6], R.CASES[9]), ids=lambda c: 'x'.join(map(str, c)))
def test_mutants_fall_outside(case, mutant):
    H, In, Rr, RG, _ = case
    dG, X, Hout, pre = R.case_data(H, In, Rr)
    s, m = R.wgrad_ref(dG, X, Hout, H, pre)
    q = worst(R.wgrad_emulated(dG, X, Hout, H, RG, pre, mutant=mutant), s, m, pre, R.chain_len(Rr, RG))
    assert q > 1.0, (mutant, q)
