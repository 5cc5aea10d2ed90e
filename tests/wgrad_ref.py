"""Float64 reference, budget, kernel-order emulation and cases for the fused encoder-BLSTM weight gradients (csrc/lstm_wgrad.hip) launched as
a table through ss_op_lstm_wgrad_table (tests/test_gpu_wgrad_table.py).

REFERENCE: the header's four sums in float64 over all R rows,
    dWih[d][n][k] = sum_r dG[r][d 4H + n] X[r][k]          dWhh[0][n][k] = sum_r dG[r + 1][n] Hout[r][k]
    db[d][n]      = sum_r dG[r][d 4H + n]                  dWhh[1][n][k] = sum_r dG[r][4H + n] Hout[r + 1][H + k]

PRECONDITION the first GPU run of these tests brought out (now in the header): the kernel computes the forward bias in the forward h tile, whose
dG operand is row r + 1, so db[0] = sum_r dG[r + 1] -- the flat sum only because row 0 of dG is a halo row, which is zero in every slab.  With
dG[0] != 0 the forward bias misses that row (measured: exactly dG[0] missing, every other output right).  The cases keep row 0 zero.

BUDGET per element: (L + 2) u sum|terms| + u |prefill + sum|, u = 2^-24, L = ceil(ceil(R / RG) / 64) 64 the longest fp32 chain (a row group).
Derivation: a row group's partial is one chain of at most L fused multiply-adds, each rounding once: to first order its error is at most
L u times the group's sum|terms| (the k-th rounding acts on a partial sum bounded by the terms so far), so all groups together stay inside
L u sum|terms|.  The float64 sum over the groups adds at most RG 2^-53 of that: nothing.  Rounding the total to fp32 adds u |sum| <= u sum|terms|
(the +1), adding it to the prefill in fp32 adds u |prefill + sum| (the last term), and the second +1 takes the second-order terms, (L u)^2 / 2 and
below, far under one u for L <= 2^11.  test_wgrad_ref_selftest.py shows the emulation of the kernel's order inside it and five wrong kernels
outside it."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
WGRAD_MAX = 8


def small_ld(H):
    """kernels.h lstm_small_ld: 2H for a power of two, else 2H rounded up to a multiple of 4"""
    return 2 * H if H > 32 or H & (H - 1) == 0 else (2 * H + 3) & ~3


def tiles(H, In):
    return -(-8 * H // 64) * (-(-In // 64) + (1 if (4 * H) % 64 == 0 else 2))


def chain_len(R, RG):
    return -(-(-(-R // RG)) // 64) * 64


# (H, In, R, row_groups, x_mode): every value the issue names occurs; x_mode 'vec' = X 16-byte aligned with x_ld % 4 == 0 (float4 loads with a
# scalar tail where In % 4 != 0), 'odd' = x_ld odd (scalar loads), 'off' = X at an odd element offset
CASES = ((1, 1, 1, 1, 'vec'), (2, 3, 2, 7, 'vec'), (4, 63, 63, 8, 'vec'), (8, 64, 64, 9, 'odd'), (16, 65, 65, 16, 'vec'), (32, 200, 1024, 16, 'vec'),
         (3, 200, 1025, 16, 'off'), (17, 64, 1025, 7, 'odd'), (31, 1, 1024, 9, 'vec'), (8, 3, 63, 16, 'odd'), (32, 65, 2, 1, 'off'))
TABLE = ((8, 64, 64, 'odd'), (3, 63, 65, 'vec'), (32, 200, 1024, 'vec'))      # the three-task table, row_groups 9
TABLE_RG = 9


def case_data(H, In, R, seed=0):
    rng = np.random.default_rng([31, H, In, R, seed])
    dG = rng.standard_normal((R, 8 * H)).astype(F32)
    dG[0] = 0               # row 0 of dg is a halo row and MUST be zero: the kernel takes the forward bias from the h tile, sum_r dg[r + 1]
    X = rng.standard_normal((R, In)).astype(F32)
    Hout = rng.uniform(-1, 1, (R, 2 * H)).astype(F32)
    pre = [(1.0 + rng.random(n)).astype(F32) * F32(-1) ** (i + 1) for i, n in enumerate((8 * H * In, 8 * H * H, 16 * H))]      # O(1) prefill
    return dG, X, Hout, pre


def _operands(dG, X, Hout, H):
    """per output family the (A [R][4H], B [R][cols]) whose row-wise outer products are summed; rows shifted for W_hh, zero beyond R"""
    R = dG.shape[0]
    z = lambda a: np.concatenate([a[1:], np.zeros((1,) + a.shape[1:], a.dtype)])      # noqa: E731  row r -> row r + 1, zero at the end
    ones = np.ones((R, 1), dG.dtype)
    return {('ih', 0): (dG[:, :4 * H], X), ('ih', 1): (dG[:, 4 * H:], X),
            ('hh', 0): (z(dG[:, :4 * H]), Hout[:, :H]), ('hh', 1): (dG[:, 4 * H:], z(Hout[:, H:])),
            ('b', 0): (dG[:, :4 * H], ones), ('b', 1): (dG[:, 4 * H:], ones)}


def _pack(fam, H, In):
    """family results -> the three flat outputs gwih [2][4H][In], gwhh [2][4H][H], gb [2][2][4H]"""
    gwih = np.stack([fam[('ih', 0)], fam[('ih', 1)]]).reshape(-1)
    gwhh = np.stack([fam[('hh', 0)], fam[('hh', 1)]]).reshape(-1)
    gb = np.stack([np.stack([fam[('b', d)][:, 0]] * 2) for d in (0, 1)]).reshape(-1)
    return [gwih, gwhh, gb]


def wgrad_ref(dG, X, Hout, H, pre):
    """float64: (prefill + sums, budgets) for gwih, gwhh, gb given the chain length L later: returns (sums, sum|terms|)"""
    ops = _operands(dG.astype(np.float64), X.astype(np.float64), Hout.astype(np.float64), H)
    In = X.shape[1]
    s = _pack({k: a.T @ b for k, (a, b) in ops.items()}, H, In)
    m = _pack({k: np.abs(a).T @ np.abs(b) for k, (a, b) in ops.items()}, H, In)
    return s, m


def wgrad_budget(s, m, pre, L):
    return [(L + 2) * U * mi + U * np.abs(p.astype(np.float64) + si) for si, mi, p in zip(s, m, pre)]


def wgrad_emulated(dG, X, Hout, H, RG, pre, mutant=None):
    """The kernel's own order: per row group one fp32 chain of fused multiply-adds in row order (a float64 product-and-sum rounded to fp32),
    the groups' partials added in float64 in group order, one rounding to fp32, one fp32 addition onto the prefill.
    Mutants: 'same_row' (W_hh paired with the same row instead of r +- 1), 'drop_last' (the last row of every row group left out),
    'swap_dir' (the h tile of a block that straddles the directions serves the other one: their W_hh rows come out exchanged between the
    pairings), 'bias_col' (the bias taken from column H of the h tile, which holds zero, instead of 32), 'skip_group' (one row group left
    out of the reduction)."""
    R, In = X.shape
    ops = _operands(dG, X, Hout, H)
    ops[('b', 0)] = (ops[('hh', 0)][0], ops[('b', 0)][1])  # the forward bias rides in the forward h tile: dg[r + 1] against the column of ones
    if mutant == 'same_row':
        ops[('hh', 0)] = (dG[:, :4 * H], Hout[:, :H])
        ops[('hh', 1)] = (dG[:, 4 * H:], Hout[:, H:])
    if mutant == 'swap_dir':
        z = lambda a: np.concatenate([a[1:], np.zeros((1,) + a.shape[1:], a.dtype)])      # noqa: E731
        ops[('hh', 0)] = (dG[:, :4 * H], z(Hout[:, H:]))
        ops[('hh', 1)] = (z(dG[:, 4 * H:]), Hout[:, :H])
    rpg = chain_len(R, RG)
    fam = {}
    for key, (a, b) in ops.items():
        total = np.zeros((a.shape[1], b.shape[1]), np.float64)
        for g in range(RG):
            lo, hi = g * rpg, min((g + 1) * rpg, R)
            if mutant == 'drop_last' and hi > lo:
                hi -= 1
            acc = np.zeros(total.shape, F32)
            for r in range(lo, hi):
                acc = (a[r].astype(np.float64)[:, None] * b[r].astype(np.float64)[None, :] + acc.astype(np.float64)).astype(F32)
            if mutant == 'skip_group' and g == 0:
                continue
            total += acc.astype(np.float64)
        if mutant == 'bias_col' and key[0] == 'b':
            total[:] = 0
        fam[key] = total.astype(F32)
    return [(p + v).astype(F32) for p, v in zip(pre, _pack(fam, H, In))]
