"""The fused encoder-BLSTM weight gradients (csrc/lstm_wgrad.hip) launched as the engine launches them -- a table of tasks with their own H, In,
R and strides, the caller's row_groups, scratch of exactly the stated size and caller-owned counters -- through ss_op_lstm_wgrad_table on
guarded buffers, judged PER ELEMENT against float64 with the budget of tests/wgrad_ref.py, (L + 2) u sum|terms| + u |prefill + sum|, which
tests/test_wgrad_ref_selftest.py proves (the kernel's own order stays inside, five wrong kernels do not).

  single tasks   H in {1, 2, 4, 8, 16, 32} and {3, 17, 31} with h_ld = lstm_small_ld(H) (padding columns hold the guard NaN); In in {1, 3, 63, 64,
                 65, 200}; X 16-byte aligned with In % 4 != 0, with an odd x_ld, and at an odd offset; R in {1, 2, 63, 64, 65, 1024, 1025}
                 (R below 64 row_groups: empty row groups); row_groups in {1, 7, 8, 9, 16} (the 8-unrolled and the tail half of the float64
                 reduction); outputs pre-filled with O(1) values
  table          three tasks with different H, In and R in one launch: the bits of the three single launches
  counters       two launches on the same counters: all-zero after each, the same bits

FINDING: run first on data with a non-zero row 0 of dG, every case measured 200 to 250000 budgets -- in the forward bias alone: the kernel
sums it beside the forward W_hh, over dG[r + 1], so row 0 never enters.  In a slab row 0 is a halo row (zero), so the engine's gradients are
the flat sums; the precondition is now stated in the header and in lstm_wgrad.hip, and the cases keep row 0 zero (tests/wgrad_ref.py).

Each test prints `FIG <test> <case> <worst error / budget>`."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import wgrad_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
ODD = 67


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def gin(a, name, ld=None, offset=64):
    a = np.ascontiguousarray(a)
    return G.inp(torch.from_numpy(a), 'cuda', ld=ld if ld is not None else a.shape[-1], name=name, offset=offset)


def gout(shape, name, fill=None, dtype=torch.float32, offset=64):
    if isinstance(fill, np.ndarray):
        fill = torch.from_numpy(np.ascontiguousarray(fill))
    return G.Guarded(shape, role='out', dtype=dtype, device='cuda', fill=fill, name=name, offset=offset)


def host(g):
    return g.t.contiguous().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ratio(got, ref, budget):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), 'a result is not finite: guard memory was read'
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


class Task:
    """one task's data, its guarded operands and fresh pre-filled outputs"""

    def __init__(self, H, In, Rr, mode, tag=''):
        self.H, self.In, self.R = H, In, Rr
        self.dG, self.X, self.Hout, self.pre = R.case_data(H, In, Rr)
        x_ld = {'vec': (In + 4) // 4 * 4, 'odd': In + 1 + In % 2, 'off': In + 4}[mode]
        h_ld = R.small_ld(H) if H & (H - 1) else 2 * H + 4
        self.gdg = gin(self.dG, 'dG' + tag)
        self.gx = gin(self.X, 'X' + tag, ld=x_ld, offset=ODD if mode == 'off' else 64)
        self.gh = gin(self.Hout, 'Hout' + tag, ld=h_ld, offset=ODD)
        assert self.gx.t.data_ptr() % 16 == (0 if mode != 'off' else 12) and (mode != 'vec' or x_ld % 4 == 0) and (mode != 'odd' or x_ld % 2)
        self.fresh(tag)

    def fresh(self, tag=''):
        self.outs = [gout((p.size,), n + tag, fill=p, offset=ODD) for n, p in zip(('gwih', 'gwhh', 'gb'), self.pre)]

    def args(self):
        return (self.gdg.t, self.gx.t, self.gh.t, *[o.t for o in self.outs])

    def check(self):
        G.check_all([self.gdg, self.gx, self.gh] + self.outs)
        return [host(o) for o in self.outs]

    def worst(self, got, RG):
        s, m = R.wgrad_ref(self.dG, self.X, self.Hout, self.H, self.pre)
        bud = R.wgrad_budget(s, m, self.pre, R.chain_len(self.R, RG))
        return max(ratio(g, p.astype(np.float64) + si, b) for g, si, p, b in zip(got, s, self.pre, bud))


def launch(E, tasks, RG, part=None, ctr=None):
    """one launch on scratch of exactly the stated size and zeroed counters (or the given ones); returns (part, ctr)"""
    args = [t.args() for t in tasks]
    floats, words = E.lstm_wgrad_table_sizes(args, RG)
    assert floats == sum(R.tiles(t.H, t.In) for t in tasks) * RG * 4096 and words == sum(R.tiles(t.H, t.In) for t in tasks)
    if part is None:
        part, ctr = gout((floats,), 'part'), gout((words,), 'ctr', fill=0, dtype=torch.int32, offset=ODD)
    E.lstm_wgrad_table(args, RG, part.t, ctr.t)
    torch.cuda.synchronize()
    part.check(written=False)                               # nothing outside the stated scratch changes
    ctr.check(written=False)
    assert not bool(ctr.t.any()), 'an arrival counter did not come back to zero'
    return part, ctr


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_single_task(E, case):
    H, In, Rr, RG, mode = case
    t = Task(H, In, Rr, mode)
    launch(E, [t], RG)
    q = t.worst(t.check(), RG)
    print(f'FIG wgrad_table H={H}/In={In}/R={Rr}/RG={RG}/{mode} {q:.4f}')
    assert q <= 1.0


def test_three_task_table_is_three_single_launches(E):
    RG = R.TABLE_RG
    tasks = [Task(H, In, Rr, mode, tag=str(i)) for i, (H, In, Rr, mode) in enumerate(R.TABLE)]
    launch(E, tasks, RG)
    together = [t.check() for t in tasks]
    worst = 0.0
    for t, tog in zip(tasks, together):
        worst = max(worst, t.worst(tog, RG))
        t.fresh()
        launch(E, [t], RG)
        alone = t.check()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(alone, tog)), 'a task in the table differs from its single launch'
    print(f'FIG wgrad_table three-task-table {worst:.4f}')
    assert worst <= 1.0


def test_counters_reused_without_zeroing(E):
    RG = 16
    t = Task(16, 65, 1025, 'vec')
    part, ctr = launch(E, [t], RG)
    first = t.check()
    t.fresh()
    launch(E, [t], RG, part, ctr)                           # the same counters and scratch, as they were left
    second = t.check()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, second)), 'the second launch on the same counters differs'
    q = t.worst(second, RG)
    print(f'FIG wgrad_table counters-reused {q:.4f}')
    assert q <= 1.0
