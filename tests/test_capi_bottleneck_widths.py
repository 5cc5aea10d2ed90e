"""CPU-only checks of the bottleneck-width range: ss_create takes dim_neck, dim_neck_2 and dim_neck_3 anywhere in 1..32 and lays out
exactly the reference's state_dict for those hparams (oracle.weights.param_spec), and refuses widths outside the range with a message
that names it.  Nothing here touches a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import weights as W
from speechsplit_amd import _capi

KIND = {'G3': 3, 'G6': 6}

# name: (kind, (dim_neck, dim_neck_2, dim_neck_3), (freq, freq_2, freq_3)); tests/test_gpu_bottleneck_widths.py runs the same set
CONFIGS = {
    'W_odd': ('G3', (3, 2, 5), (8, 8, 8)),
    'W_mix': ('G3', (12, 3, 24), (4, 16, 8)),
    'W_top': ('G3', (31, 1, 17), (8, 8, 8)),
    'P_mix': ('G6', (8, 3, 20), (8, 8, 4)),
}


def hparams_of(name, T=192):
    _, (n1, n2, n3), (f1, f2, f3) = CONFIGS[name]
    return W.default_hparams(dim_neck=n1, dim_neck_2=n2, dim_neck_3=n3, freq=f1, freq_2=f2, freq_3=f3, max_len_pad=T)


def _create(kind, hp, B=4, T=192):
    lib = _capi.lib()
    hps = _capi.hparams_struct(hp)
    return lib, lib.ss_create(KIND[kind], C.byref(hps), B, T)


def _table(lib, h):
    name = C.create_string_buffer(256)
    off, nd, shp = C.c_long(), C.c_int(), (C.c_long * 3)()
    rows = []
    for i in range(lib.ss_num_params(h)):
        assert lib.ss_param_info(h, i, name, 256, C.byref(off), C.byref(nd), C.byref(shp)) == 0
        rows.append((name.value.decode(), tuple(shp[k] for k in range(nd.value)), off.value))
    return rows


def check_table(kind, hp):
    lib, h = _create(kind, hp)
    assert h, lib.ss_last_error().decode()
    try:
        rows = _table(lib, h)
        spec = [(n, tuple(s)) for n, s in W.param_spec(kind, hp)]
        assert [(n, s) for n, s, _ in rows] == spec
        prev_end = 0
        for n, s, off in rows:
            assert off % 4 == 0 and off >= prev_end, n                # 16-byte aligned, ordered, non-overlapping
            prev_end = off + int(np.prod(s))
        assert prev_end <= lib.ss_arena_numel(h) <= prev_end + 4 * len(rows) + 8     # alignment gaps and the status slot only
        assert lib.ss_workspace_bytes(h) > 0
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_configurations_are_accepted_with_the_reference_table(name):
    check_table(CONFIGS[name][0], hparams_of(name))


@pytest.mark.parametrize('kind', ['G3', 'G6'])
@pytest.mark.parametrize('H', list(range(1, 33)))
def test_every_width_in_range_is_accepted(kind, H):
    hp = W.default_hparams(dim_neck=H, dim_neck_2=3 if H != 3 else 5, dim_neck_3=33 - H)      # every triple holds an odd width
    check_table(kind, hp)


@pytest.mark.parametrize('field', ['dim_neck', 'dim_neck_2', 'dim_neck_3'])
@pytest.mark.parametrize('H', [0, 33, 64, -1])
def test_widths_outside_the_range_are_refused(field, H):
    for kind in ('G3', 'G6'):
        lib, h = _create(kind, W.default_hparams(**{field: H}))
        assert not h
        msg = lib.ss_last_error().decode()
        assert '1..32' in msg and 'bottleneck' in msg, msg

