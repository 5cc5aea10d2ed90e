"""CPU-only checks of the ragged eval-mode interface: the new C symbols, their refusals on an engine that was never bound, the host-side
batch planner and the Python-side validation of the lengths.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

from speechsplit_amd import _capi, convert, hparams as HP
from speechsplit_amd.engine import check_lengths

_vp, _i, _l = C.c_void_p, C.c_int, C.c_long
SIGNATURES = {
    'ss_g3_forward_ragged': [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],      # e, x_f0, x_org, c_trg, len, B, T, training, out, stream
    'ss_g6_forward_ragged': [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],           # e, x_org, f0_trg, len, B, T, training, out, stream
    'ss_g3_rhythm_ragged': [_vp, _vp, _vp, _i, _i, _vp, _vp],                     # e, x_org, len, B, T, codes, stream
    'ss_op_conv_block_ragged': [_vp] * 8 + [_l, _i, _i, _i, _i, _vp],             # x, w, bias, gamma, beta, len, y, scratch, n, B, T, Ci, Co, stream
    'ss_op_lstm_fwd_ragged': [_vp] * 6 + [_l, _vp, _i, _i, _i, _vp],              # ss_op_lstm_fwd's arguments with len in front of B
}


def test_new_symbols_and_signatures():
    lib = _capi.lib()
    for name, args in SIGNATURES.items():
        assert name in _capi.SYMBOLS, name
        res, got = _capi.SYMBOLS[name]
        assert res is _i and list(got) == args, name
        fn = getattr(lib, name)
        assert fn.restype is _i and list(fn.argtypes) == args
    # the lstm hook is ss_op_lstm_fwd plus the length array
    plain = list(_capi.SYMBOLS['ss_op_lstm_fwd'][1])
    assert SIGNATURES['ss_op_lstm_fwd_ragged'] == plain[:7] + [_vp] + plain[7:]
    assert lib.ss_abi_version() == 2


def test_unbound_engine_refuses_every_ragged_entry_point():
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    g3, g6 = lib.ss_create(3, C.byref(hps), 2, 192), lib.ss_create(6, C.byref(hps), 2, 192)
    assert g3 and g6
    calls = {
        'g3 forward': lambda: lib.ss_g3_forward_ragged(g3, None, None, None, None, 2, 192, 0, None, None),
        'g6 forward': lambda: lib.ss_g6_forward_ragged(g6, None, None, None, 2, 192, 0, None, None),
        'g3 rhythm': lambda: lib.ss_g3_rhythm_ragged(g3, None, None, 2, 192, None, None),
    }
    for tag, call in calls.items():
        assert call() != 0, tag
        assert b'bound' in lib.ss_last_error(), (tag, lib.ss_last_error())
    # the wrong kind of engine, and training together with lengths, are refused by name
    assert lib.ss_g3_forward_ragged(g6, None, None, None, None, 2, 192, 0, None, None) != 0
    assert b'Generator_3' in lib.ss_last_error()
    assert lib.ss_g6_forward_ragged(g3, None, None, None, 2, 192, 0, None, None) != 0
    assert b'Generator_6' in lib.ss_last_error()
    assert lib.ss_g3_rhythm_ragged(g6, None, None, 2, 192, None, None) != 0
    dummy = C.c_void_p(16)
    assert lib.ss_g3_forward_ragged(g3, None, None, None, dummy, 2, 192, 1, None, None) != 0
    assert b'eval-only' in lib.ss_last_error()
    assert lib.ss_g6_forward_ragged(g6, None, None, dummy, 2, 192, 1, None, None) != 0
    assert b'eval-only' in lib.ss_last_error()
    # the hooks need no engine: null operands are an error with a message, nothing is launched
    assert lib.ss_op_conv_block_ragged(None, None, None, None, None, None, None, None, 0, 1, 8, 80, 256, None) != 0
    assert lib.ss_last_error()
    assert lib.ss_op_lstm_fwd_ragged(None, None, None, None, None, None, 0, None, 1, 8, 8, None) != 0
    assert lib.ss_last_error()
    lib.ss_destroy(g3)
    lib.ss_destroy(g6)


@pytest.mark.parametrize('max_rows', [1, 3, 16])
def test_plan_batches_properties(max_rows):
    rng = np.random.default_rng(7)
    lengths = [int(8 * n) for n in rng.integers(1, 129, 37)]
    plan = convert.plan_batches(lengths, max_rows)
    flat = [i for b in plan for i in b]
    assert sorted(flat) == list(range(len(lengths)))                                     # a permutation: every index exactly once
    assert all(1 <= len(b) <= max_rows for b in plan)
    assert len(plan) == -(-len(lengths) // max_rows)
    Ts = [max(lengths[i] for i in b) for b in plan]
    assert Ts == sorted(Ts)                                                              # batches non-decreasing in T
    assert all(lengths[b[-1]] == T for b, T in zip(plan, Ts))                            # a batch's T is its last member's
    assert [lengths[i] for i in flat] == sorted(lengths)                                 # sorted by length


def test_plan_batches_edge_cases():
    assert convert.plan_batches([96], 16) == [[0]]                                       # a single utterance
    assert convert.plan_batches([], 4) == []
    assert convert.plan_batches([64] * 5, 2) == [[0, 1], [2, 3], [4]]                    # equal lengths keep their order
    assert convert.plan_batches(np.array([24, 8, 16]), 8) == [[1, 2, 0]]
    with pytest.raises(ValueError):
        convert.plan_batches([8, 16], 0)


def test_lengths_are_validated_on_the_host():
    f = (8, 8, 8)
    ok = check_lengths([64, 8, 40, 24], 4, 64, f)
    assert ok.dtype == torch.int32 and ok.tolist() == [64, 8, 40, 24]
    assert check_lengths(np.array([16, 8]), 2, 16, f).tolist() == [16, 8]
    assert check_lengths(torch.tensor([16, 8]), 2, 16, f).dtype == torch.int32
    with pytest.raises(ValueError, match='multiple'):
        check_lengths([64, 12], 2, 64, f)                                                # not a multiple of the code factors
    with pytest.raises(ValueError, match='multiple'):
        check_lengths([64, 8], 2, 64, (8, 16, 8))                                        # ... of EVERY factor
    with pytest.raises(ValueError, match='outside'):
        check_lengths([64, 0], 2, 64, f)
    with pytest.raises(ValueError, match='outside'):
        check_lengths([72, 8], 2, 64, f)                                                 # > T
    with pytest.raises(ValueError, match='outside'):
        check_lengths([64, -8], 2, 64, f)
    with pytest.raises(ValueError, match='one entry per row'):
        check_lengths([64, 8, 8], 2, 64, f)                                              # a wrong count
    with pytest.raises(ValueError, match='one entry per row'):
        check_lengths([[64, 8]], 2, 64, f)
    with pytest.raises(ValueError, match='integers'):
        check_lengths([64.0, 8.0], 2, 64, f)
