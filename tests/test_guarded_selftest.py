"""Self-test of tests/guarded.py on CPU tensors: deliberately wrong stand-in "kernels" written with plain torch indexing must each be
reported with the (row, column) of their fault, and the correct stand-in must pass.  This is the proof that the containment tests
(test_gpu_containment.py, test_gpu_engine_containment.py) can fail; no HIP kernel is ever built wrong for it."""
import pytest
import torch

from tests import guarded as G

ROWS, COLS, LD = 5, 6, 8


def _buffers(dtype=torch.float32, ld=LD, offset=3):
    x = torch.arange(1, ROWS * COLS + 1, dtype=torch.float32).reshape(ROWS, COLS).to(dtype)
    gin = G.inp(x, 'cpu', ld=ld + 3, offset=offset, name='x')
    gout = G.out((ROWS, COLS), 'cpu', ld=ld, offset=offset, dtype=dtype, name='y')
    return x, gin, gout


def _flat(g):
    """The whole allocation in the buffer's own type, and the index of the extent's first element: what a kernel's raw pointer sees."""
    return g.flat.view(g.dtype), g.base


def correct(gin, gout):
    gout.t.copy_(2 * gin.t)


def test_correct_stand_in_passes():
    for dtype in (torch.float32, torch.bfloat16, torch.float64, torch.int32):
        for ld, offset in ((LD, 3), (COLS, 64), (COLS + 1, 1)):
            x, gin, gout = _buffers(dtype, ld, offset)
            assert gout.t.shape == (ROWS, COLS) and gout.t.stride() == (ld, 1) and gout.t.storage_offset() == gout.base
            correct(gin, gout)
            gout.check()
            gin.check()
            assert torch.equal(gout.t, 2 * x)
            if dtype != torch.int32:
                G.assert_close(gout.t, 2 * x, 1e-6)


def test_bands_are_a_mebibyte_and_everything_starts_as_the_pattern():
    _, gin, gout = _buffers()
    assert gout.base * 4 >= G.BAND_BYTES + 3 * 4 and (gout.flat.numel() - gout.base - gout.span) * 4 >= G.BAND_BYTES
    assert bool((gout.flat == G.NAN32).all())                                 # role 'out': extent too
    assert bool(torch.isnan(gout.t).all()) and bool(torch.isnan(gout.flat.view(torch.float32)).all())
    assert int((gin.flat != G.NAN32).sum()) == ROWS * COLS                    # role 'in': exactly the extent differs
    assert bool(torch.isnan(G.Guarded((4,), dtype=torch.bfloat16).flat.view(torch.bfloat16)).all())
    assert bool(torch.isnan(G.Guarded((4,), dtype=torch.float64).flat.view(torch.float64)).all())
    g3 = G.out((2, ROWS, COLS), 'cpu', ld=LD)
    assert g3.t.stride() == (ROWS * LD, LD, 1)


def test_write_one_element_past_the_last_row_is_reported():
    _, gin, gout = _buffers()
    correct(gin, gout)
    flat, base = _flat(gout)
    flat[base + ROWS * LD] = 1.0                                              # element (ROWS, 0)
    with pytest.raises(G.GuardError) as e:
        gout.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('guard', ROWS, 0)


def test_write_into_the_row_gap_is_reported():
    _, gin, gout = _buffers()
    correct(gin, gout)
    flat, base = _flat(gout)
    flat[base + 2 * LD + COLS] = 0.0                                          # first gap column of row 2 (a plausible 0 is still a write)
    with pytest.raises(G.GuardError) as e:
        gout.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('guard', 2, COLS)


def test_write_one_element_before_the_base_is_reported():
    _, gin, gout = _buffers()
    correct(gin, gout)
    flat, base = _flat(gout)
    flat[base - 1] = 7.0
    with pytest.raises(G.GuardError) as e:
        gout.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('guard', -1, LD - 1)


def test_write_into_an_input_guard_is_reported():
    _, gin, gout = _buffers()
    correct(gin, gout)
    flat, base = _flat(gin)
    flat[base + COLS] = 0.0
    with pytest.raises(G.GuardError) as e:
        gin.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('guard', 0, COLS)


def test_batched_extent_gap_and_unwritten_element():
    g = G.out((2, ROWS, COLS), 'cpu', ld=LD, offset=5, name='y3')
    g.t.fill_(1.0)
    g.check()
    g.flat.view(torch.float32)[g.base + (ROWS + 1) * LD + COLS + 1] = 0.0     # batch 1, row 1, second gap column: flat row ROWS + 1
    with pytest.raises(G.GuardError) as e:
        g.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('guard', ROWS + 1, COLS + 1)


def test_unwritten_extent_element_is_reported():
    x, gin, gout = _buffers()
    correct(gin, gout)
    gout.t[3, 4] = float('nan')                                               # any NaN fails the value comparison ...
    with pytest.raises(G.GuardError) as e:
        G.assert_close(gout.t, 2 * x, 1e-6, 'y')
    assert (e.value.kind, e.value.row, e.value.col) == ('value', 3, 4)
    _, gin, gout = _buffers()
    gout.t[:3].copy_(2 * gin.t[:3])
    gout.t[3, :4].copy_(2 * gin.t[3, :4])                                     # ... and the stand-in that skips (3, 4) leaves the pattern there
    gout.t[3, 5:].copy_(2 * gin.t[3, 5:])
    gout.t[4].copy_(2 * gin.t[4])
    with pytest.raises(G.GuardError) as e:
        gout.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('extent', 3, 4)
    with pytest.raises(G.GuardError) as e:
        G.assert_close(gout.t, 2 * x, 1e-6, 'y')
    assert (e.value.row, e.value.col) == (3, 4)


def test_read_of_a_guard_element_is_reported():
    x, gin, gout = _buffers()
    flat, base = _flat(gin)
    correct(gin, gout)
    gout.t[1, 2] += 0 * flat[base + 1 * gin.ld + COLS]                        # "load the full tile and multiply the tail by zero"
    with pytest.raises(G.GuardError) as e:
        G.assert_close(gout.t, 2 * x, 1e-6, 'y')
    assert (e.value.kind, e.value.row, e.value.col) == ('value', 1, 2)
    with pytest.raises(G.GuardError) as e:                                    # the guard's NaN payload arrives in the output
        gout.check()
    assert (e.value.kind, e.value.row, e.value.col) == ('extent', 1, 2)


def test_accumulated_output_keeps_its_prefill_and_only_the_guard_is_checked():
    x, gin, _ = _buffers()
    c0 = torch.ones(ROWS, COLS)
    gout = G.out((ROWS, COLS), 'cpu', ld=LD, offset=3, fill=c0, name='c')
    assert torch.equal(gout.t, c0)
    gout.t.add_(gin.t)
    gout.check()
    G.assert_close(gout.t, x + 1, 1e-6)
    gout.flat.view(torch.float32)[gout.base + COLS] = 1.0
    with pytest.raises(G.GuardError) as e:
        gout.check()
    assert (e.value.row, e.value.col) == (0, COLS)


def test_wrong_value_is_reported_with_its_position():
    x, gin, gout = _buffers()
    correct(gin, gout)
    gout.t[4, 1] *= 1.001
    with pytest.raises(G.GuardError) as e:
        G.assert_close(gout.t, 2 * x, 1e-4, 'y')
    assert (e.value.row, e.value.col) == (4, 1)
