"""CPU-only checks of the C ABI's entry guard: every entry point that takes an engine refuses a null engine, the wrong kind of engine and an
engine that is not bound -- in that order, by name, before its own argument checks and before the first HIP call (there is no device here,
and every pointer below is one that must never be dereferenced).  The table of entry points is parsed from include/speechsplit_amd.h, so a
call is tested from the day it is declared."""
import ctypes as C
import os
import re

import pytest

from speechsplit_amd import _capi, hparams as HP

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'speechsplit_amd.h')
FAKE = 4096                        # a non-null, 256-byte aligned address nobody may touch
MAX_B, MAX_T = 2, 192

# ---- the few things the header cannot say
# answered by the host on an engine that is not bound: getters of what ss_create built, switches of host-side state, and ss_bind itself
HOST_ONLY = {'ss_destroy', 'ss_num_params', 'ss_param_info', 'ss_arena_numel', 'ss_workspace_bytes', 'ss_plan_bytes', 'ss_bind', 'ss_side_stream',
             'ss_stream_report', 'ss_grad_split', 'ss_comm_destroy', 'ss_scratch_fallbacks', 'ss_dp_profile', 'ss_dp_profile_read',
             'ss_grad_accum_count', 'ss_status', 'ss_set_lockstep', 'ss_set_precision', 'ss_profile', 'ss_profile_sample', 'ss_profile_read',
             'ss_profile_timeline', 'ss_debug_buffer', 'ss_debug_names'}
# valid on an unbound engine too, but they synchronise the caller's stream first: not callable without a device
SYNCHRONISING = {'ss_check', 'ss_clear_abort'}
# the three clipping calls name a bad argument before a missing binding (tests/test_capi_grad_clip.py pins that order)
ARGUMENT_BEFORE_BINDING = {'ss_set_grad_clip', 'ss_grad_norm', 'ss_grad_clip_stats'}
# the backwards say that no forward has run before anything else about the engine, in a text pinned verbatim (tests/test_capi_input_grads.py)
NO_FORWARD = {'ss_g3_backward', 'ss_g3_backward_inputs', 'ss_g6_backward', 'ss_g6_backward_inputs'}
# documented values for a null engine where no error value exists
NULL_VALUE = {'ss_status': 0, 'ss_grad_accum_count': 0, 'ss_scratch_fallbacks': -1}
VALID_INT = {'B': MAX_B, 'T': MAX_T, 'world': 1, 'every_nth_step': 1, 'C': 4}      # every other integer (flags, index, rank, caps, switches): 0


def _declarations():
    """[(return type, name, [parameter names])] of every declaration whose first parameter is an engine"""
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r'^([A-Za-z_][\w \*]*?)\b(ss_\w+)\(((?:const )?ss_engine\s*\*[^;]*)\);', text, flags=re.M):
        names = [re.sub(r'\[\d*\]', '', p).split()[-1].lstrip('*') for p in params.split(',')]
        out.append((ret.strip(), name, names[1:]))
    return out


DECLS = _declarations()
NAMES = [d[1] for d in DECLS]
PARAMS = {d[1]: d[2] for d in DECLS}


def err(lib):
    return lib.ss_last_error().decode()


def args(name, valid=True):
    """the call's arguments behind the engine: valid small values, or (valid=False) zeros and null pointers"""
    out = []
    for typ, pname in zip(_capi.SYMBOLS[name][1][1:], PARAMS[name]):
        if typ in (C.c_int, C.c_uint, C.c_long):
            out.append(VALID_INT.get(pname, 0) if valid else 0)
        elif typ in (C.c_float, C.c_double):
            out.append(1.0)
        elif typ is C.c_void_p:
            out.append(C.c_void_p(FAKE) if valid else None)
        elif typ is C.c_char_p:
            out.append(b'x' if valid else None)
        else:                                    # a typed pointer to a host variable: every call takes NULL there or refuses it
            out.append(None)
    return out


def call(lib, name, engine, valid=True):
    return getattr(lib, name)(engine, *args(name, valid))


@pytest.fixture(scope='module')
def engines():
    lib = _capi.lib()
    hps = _capi.hparams_struct(HP.default_hparams())
    made = {kind: lib.ss_create(kind, C.byref(hps), MAX_B, MAX_T) for kind in (3, 6, 0)}
    assert all(made.values())
    yield lib, made
    for h in made.values():
        lib.ss_destroy(h)


def own_kind(name):
    return 3 if '_g3_' in name else 6 if '_g6_' in name else None


def test_the_table_comes_from_the_header_and_matches_the_binding():
    assert len(NAMES) > 60 and len(set(NAMES)) == len(NAMES)
    for probe in ('ss_destroy', 'ss_bind', 'ss_g3_forward', 'ss_g6_dp_train_step', 'ss_param_info', 'ss_stream_report', 'ss_debug_names'):
        assert probe in NAMES, probe
    text = open(HEADER).read()
    assert len(re.findall(r'\bss_\w+\((?:const )?ss_engine\s*\*', text)) == len(NAMES)        # no declaration the pattern above missed
    for name in NAMES:
        assert name in _capi.SYMBOLS, name
        assert len(_capi.SYMBOLS[name][1]) == 1 + len(PARAMS[name]), name
    assert (HOST_ONLY | SYNCHRONISING | ARGUMENT_BEFORE_BINDING | NO_FORWARD | set(NULL_VALUE)) <= set(NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_null_engine(name):
    lib = _capi.lib()
    res = _capi.SYMBOLS[name][0]
    rc = call(lib, name, None)
    if name in NULL_VALUE:
        assert rc == NULL_VALUE[name]
    elif res is None:
        assert name == 'ss_destroy'                           # a no-op
    else:
        if res in (C.c_void_p, C.c_char_p):
            assert rc is None, name
        elif res is C.c_long:
            assert rc == -1, name
        else:
            assert rc != 0, name
        assert name in err(lib) and 'null engine' in err(lib), (name, err(lib))


@pytest.mark.parametrize('name', [n for n in NAMES if own_kind(n)])
def test_wrong_kind(engines, name):
    lib, made = engines
    needs = 'Generator_3' if own_kind(name) == 3 else 'Generator_6'
    for kind in {3, 6, 0} - {own_kind(name)}:
        for valid in (True, False):                           # unbound AND bad arguments: the kind is still what is reported
            assert call(lib, name, made[kind], valid) != 0, (name, kind)
            assert name in err(lib) and 'is not a ' + needs in err(lib), (name, kind, err(lib))


@pytest.mark.parametrize('name', [n for n in NAMES if n.startswith('ss_interp_')])
def test_interp_calls_get_as_far_as_the_binding_on_every_kind(engines, name):
    lib, made = engines
    for kind, h in made.items():
        assert call(lib, name, h) != 0
        assert name in err(lib) and 'not bound' in err(lib), (name, kind, err(lib))


@pytest.mark.parametrize('name', [n for n in NAMES if n not in HOST_ONLY | SYNCHRONISING])
def test_unbound_engine_of_the_right_kind(engines, name):
    """everything that enqueues work or needs an arena: refused by name, also when its own arguments are bad as well (binding before arguments)"""
    lib, made = engines
    h = made[own_kind(name) or 3]
    for valid in (True,) if name in ARGUMENT_BEFORE_BINDING else (True, False):
        assert call(lib, name, h, valid) != 0, name
        if name in NO_FORWARD:
            assert err(lib) == 'backward without a preceding forward'
        else:
            assert name in err(lib) and 'not bound' in err(lib), (name, valid, err(lib))


def test_host_getters_answer_on_an_unbound_engine(engines):
    lib, made = engines
    for kind, h in made.items():
        n = lib.ss_num_params(h)
        assert (n > 0) == (kind != 0)
        assert lib.ss_arena_numel(h) >= 0 and lib.ss_workspace_bytes(h) > 0 and 0 <= lib.ss_grad_split(h) <= lib.ss_arena_numel(h)
        assert lib.ss_plan_bytes(h, MAX_B, MAX_T) == lib.ss_workspace_bytes(h)
        if n:
            assert call(lib, 'ss_param_info', h) == 0
        assert lib.ss_status(h) == 0 and lib.ss_grad_accum_count(h) == 0 and lib.ss_scratch_fallbacks(h) == 0
        assert lib.ss_side_stream(h) is None and lib.ss_stream_report(h) is not None
        for name in ('ss_set_precision', 'ss_profile', 'ss_profile_sample', 'ss_set_lockstep', 'ss_dp_profile', 'ss_dp_profile_read', 'ss_profile_read',
                     'ss_comm_destroy', 'ss_debug_names'):
            assert call(lib, name, h) == 0, (name, err(lib))
        for name in ('ss_profile_timeline', 'ss_debug_buffer', 'ss_bind'):      # these refuse their ARGUMENTS, by name, and say nothing about a binding
            assert call(lib, name, h) != 0
            assert name in err(lib) and 'not bound' not in err(lib), (name, err(lib))


def test_step_flags_equal_the_header():
    defines = dict(re.findall(r'#define (SS_STEP_\w+) (\d+)', open(HEADER).read()))
    assert set(defines) == {'SS_STEP_NO_ADAM', 'SS_STEP_SPLIT_BACKWARD', 'SS_STEP_SPLIT_NO_JOIN', 'SS_STEP_ACCUMULATE', 'SS_STEP_BUCKET'}
    for name, value in defines.items():
        assert getattr(_capi, name) == int(value), name
    from speechsplit_amd.engine import step_flags
    assert step_flags() == 0 and step_flags(True, True, True, True, True) == sum(int(v) for v in defines.values())
    assert step_flags(accumulate=True, bucket=True) == _capi.SS_STEP_ACCUMULATE | _capi.SS_STEP_BUCKET
