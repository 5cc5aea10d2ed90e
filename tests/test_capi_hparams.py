"""CPU-only checks of every ss_hparams field beyond the bottleneck widths (tests/test_capi_bottleneck_widths.py has those): what ss_create
accepts for dim_enc / dim_enc_2 / dim_enc_3, dim_freq, dim_spk_emb, dim_f0 and the InterpLnr fields is laid out exactly as the reference's
state_dict for those hparams (oracle.weights.param_spec), its workspace plan is positive and grows with the widths, and what it does not
accept is refused with a null handle and a message that names the field and the accepted set (include/speechsplit_amd.h, ss_create; the
audit behind each bound is DESIGN.md section 1, "Hyper-parameters").  Nothing here touches a device.

CONFIGS is shared with tests/test_gpu_hparams.py, which runs RUNNING on the GPU against the float64 oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import interp_np, weights as W
from oracle.gen_fixtures import draws_for
from speechsplit_amd import _capi
from speechsplit_amd.hparams import check_hparams
from tests.test_capi_bottleneck_widths import KIND, _create, check_table

SEGS10 = dict(min_len_seg=10, max_len_seg=24, max_len_seq=96)           # S = 10 segments, 48 candidate positions each
SEGS3 = dict(min_len_seg=31, max_len_seg=32, max_len_seq=64)            # S = 3 segments of 31 frames
# name: (kind, overrides of oracle.weights.default_hparams)
CONFIGS = {
    'H_narrow': ('G3', dict(dim_freq=36, dim_spk_emb=81, dim_enc=192, dim_enc_2=64, dim_enc_3=64)),
    'H_wide': ('G3', dict(dim_freq=100, dim_spk_emb=256, dim_enc=576, dim_enc_2=192, dim_enc_3=320)),
    'H_spk1': ('G3', dict(dim_spk_emb=1)),
    'H_oddmel': ('G3', dict(dim_freq=81)),
    'H_segs10': ('G3', dict(SEGS10)),
    'H_segs3': ('G3', dict(SEGS3)),
    'P_narrow': ('G6', dict(dim_freq=36, dim_enc_2=64, dim_enc_3=64, **SEGS10)),
    'P_f0_65': ('G6', dict(dim_f0=65)),
}
# refused by ss_create: name -> what the message must say.  H_oddmel: the mel slabs' rows are dim_freq floats apart while every tap of a
# layer-0 convolution reads align4(dim_freq) columns -- 3 floats past each row and, at the slab's last row, past the slab.
REFUSED = {'H_oddmel': ('dim_freq', 'multiple of 4 in 32..512')}
RUNNING = [n for n in CONFIGS if n not in REFUSED]
TRAIN_T = {n: 128 if 'segs' in n else 64 for n in CONFIGS}              # frames of the GPU train steps (B = 3)
CONV_WIDTHS = list(range(64, 1025, 64))


def hparams_of(name, T=64):
    return W.default_hparams(**CONFIGS[name][1], max_len_pad=T)


def nseg(hp):
    return hp.max_len_seq // hp.min_len_seg + 1                          # model.py:365


def draws_of(hp, seed, B, ncalls):
    """The reference's draws (oracle.gen_fixtures.draws_for) for the segment fields of hp."""
    return draws_for(seed, B, ncalls, lo=hp.min_len_seg, hi=hp.max_len_seg, nseg=nseg(hp))


def train_seeds(name, B):
    """(batch seed, draw seed of step 0) of the GPU train steps of a configuration; step `it` draws with dseed + it."""
    bseed = 300 + B + TRAIN_T[name] + 7 * list(CONFIGS).index(name)
    return bseed, bseed + 100


def test_every_configuration_runs_or_is_refused():
    assert set(RUNNING) | set(REFUSED) == set(CONFIGS) and not set(RUNNING) & set(REFUSED)
    assert {'H_narrow', 'H_wide', 'H_segs10', 'P_narrow'} <= set(RUNNING)


# --------------------------------------------------------------------------------------------- parameter table
@pytest.mark.parametrize('name', RUNNING)
def test_configurations_are_accepted_with_the_reference_table(name):
    check_table(CONFIGS[name][0], hparams_of(name, 192))


@pytest.mark.parametrize('field', ['dim_enc', 'dim_enc_2', 'dim_enc_3'])
@pytest.mark.parametrize('width', CONV_WIDTHS)
def test_every_conv_width_in_range_is_accepted(field, width):
    for kind in ('G3', 'G6'):
        check_table(kind, W.default_hparams(**{field: width}))


@pytest.mark.parametrize('field,values', [('dim_freq', (32, 36, 100, 512)), ('dim_spk_emb', (1, 81, 256, 1024))])
def test_free_input_widths_are_accepted(field, values):
    for v in values:
        check_table('G3', W.default_hparams(**{field: v}))
    for v in values if field == 'dim_freq' else ():
        check_table('G6', W.default_hparams(**{field: v}))


@pytest.mark.parametrize('dim_f0', [32, 65, 256, 512])
def test_generator_6_takes_other_f0_widths(dim_f0):
    check_table('G6', W.default_hparams(dim_f0=dim_f0))


# --------------------------------------------------------------------------------------------- workspace plan
def _plan(kind, hp, B, T):
    lib, h = _create(kind, hp, B, T)
    assert h, lib.ss_last_error().decode()
    try:
        n = lib.ss_plan_bytes(h, B, T)
        assert n == lib.ss_workspace_bytes(h)
        return n
    finally:
        lib.ss_destroy(h)


@pytest.mark.parametrize('name', RUNNING)
def test_workspace_plan_is_positive(name):
    kind = CONFIGS[name][0]
    for B, T in ((3, 64), (4, 128), (17, 64)):
        assert _plan(kind, hparams_of(name, T), B, T) > 0


@pytest.mark.parametrize('kind,field', [('G3', 'dim_enc'), ('G3', 'dim_enc_2'), ('G3', 'dim_enc_3'), ('G6', 'dim_enc_2'), ('G6', 'dim_enc_3')])
def test_workspace_plan_grows_with_every_conv_width(kind, field):
    sizes = [_plan(kind, W.default_hparams(**{field: c}, max_len_pad=64), 4, 64) for c in CONV_WIDTHS]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes


def test_workspace_plan_grows_with_the_speaker_width():
    sizes = [_plan('G3', W.default_hparams(dim_spk_emb=e, max_len_pad=64), 4, 64) for e in (1, 2, 3, 81, 82, 83, 256, 1023, 1024)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes          # the decoder's layer-0 W_ih alone adds 4096 floats per column to the arenas' scratch


# --------------------------------------------------------------------------------------------- refusals
# (kinds, overrides, what the message must name: the field and the accepted set)
REFUSALS = [
    (('G3', 'G6'), dict(dim_freq=81), ('dim_freq', 'multiple of 4 in 32..512')),
    (('G3', 'G6'), dict(dim_freq=82), ('dim_freq', 'multiple of 4 in 32..512')),
    (('G3', 'G6'), dict(dim_freq=28), ('dim_freq', 'multiple of 4 in 32..512')),
    (('G3', 'G6'), dict(dim_freq=516), ('dim_freq', 'multiple of 4 in 32..512')),
    (('G3', 'G6'), dict(dim_freq=0), ('dim_freq', 'multiple of 4 in 32..512')),
    (('G3', 'G6'), dict(dim_spk_emb=1025), ('dim_spk_emb', '1..1024')),
    (('G3', 'G6'), dict(dim_spk_emb=0), ('dim_spk_emb', '1..1024')),
    (('G3', 'G6'), dict(dim_spk_emb=-3), ('dim_spk_emb', '1..1024')),
    (('G3',), dict(dim_f0=65), ('dim_f0', '257', 'Generator_3')),
    (('G3',), dict(dim_f0=256), ('dim_f0', '257', 'Generator_3')),
    (('G3',), dict(dim_f0=264), ('dim_f0', '257', 'Generator_3')),
    (('G6',), dict(dim_f0=31), ('dim_f0', '32..512', 'Generator_6')),
    (('G6',), dict(dim_f0=513), ('dim_f0', '32..512', 'Generator_6')),
    (('G3', 'G6', 'interp'), dict(chs_grp=8), ('chs_grp', '16')),
    (('G3', 'G6', 'interp'), dict(chs_grp=32), ('chs_grp', '16')),
    (('G3', 'G6', 'interp'), dict(min_len_seg=0), ('min_len_seg', 'max_len_seg', '1 <= min_len_seg < max_len_seg <= 32')),
    (('G3', 'G6', 'interp'), dict(min_len_seg=-4), ('min_len_seg', 'max_len_seg', '1 <= min_len_seg < max_len_seg <= 32')),
    (('G3', 'G6', 'interp'), dict(min_len_seg=32), ('min_len_seg', 'max_len_seg', '1 <= min_len_seg < max_len_seg <= 32')),
    (('G3', 'G6', 'interp'), dict(min_len_seg=24, max_len_seg=24), ('min_len_seg', 'max_len_seg', '1 <= min_len_seg < max_len_seg <= 32')),
    (('G3', 'G6', 'interp'), dict(max_len_seg=33), ('min_len_seg', 'max_len_seg', '1 <= min_len_seg < max_len_seg <= 32')),
    (('G3', 'G6', 'interp'), dict(max_len_seq=0), ('max_len_seq', '1..512')),
    (('G3', 'G6', 'interp'), dict(max_len_seq=513), ('max_len_seq', '1..512')),
    (('G3', 'G6', 'interp'), dict(max_len_pad=0), ('max_len_pad', '1 <= max_len_pad <= 512')),
    (('G3', 'G6', 'interp'), dict(max_len_pad=513), ('max_len_pad', '1 <= max_len_pad <= 512')),
] + [(('G3', 'G6'), {f: c}, (f, 'multiples of 64 in 64..1024')) for f in ('dim_enc', 'dim_enc_2', 'dim_enc_3') for c in (0, -64, 32, 96, 1088)]
KINDS = dict(KIND, interp=0)


@pytest.mark.parametrize('kinds,over,says', REFUSALS, ids=[','.join(f'{k}={v}' for k, v in o.items()) for _, o, _ in REFUSALS])
def test_values_outside_the_accepted_sets_are_refused(kinds, over, says):
    lib = _capi.lib()
    for kind in kinds:
        hp = W.default_hparams(**over)
        hps = _capi.hparams_struct(hp)
        assert not lib.ss_create(KINDS[kind], C.byref(hps), 4, 192), (kind, over)
        msg = lib.ss_last_error().decode()
        assert all(s in msg for s in says), msg
        with pytest.raises(ValueError) as ei:                            # the Python side raises the library's message
            check_hparams(kind, hp, 4, 192)
        assert msg in str(ei.value)


@pytest.mark.parametrize('name', list(REFUSED))
def test_refused_configurations(name):
    kind = CONFIGS[name][0]
    lib, h = _create(kind, hparams_of(name, 192))
    assert not h
    msg = lib.ss_last_error().decode()
    assert all(s in msg for s in REFUSED[name]), msg


def test_refusals_leave_the_defaults_and_the_boundaries_alone():
    for kind in ('G3', 'G6', 'interp'):
        assert check_hparams(kind, W.default_hparams()) is not None
        assert check_hparams(kind, W.default_hparams(min_len_seg=1, max_len_seg=2, max_len_seq=1, max_len_pad=512), 1, 256)
        assert check_hparams(kind, W.default_hparams(min_len_seg=31, max_len_seg=32, max_len_seq=512, max_len_pad=8))
    assert check_hparams('interp', W.default_hparams(dim_freq=81, dim_f0=1, dim_spk_emb=0))       # a bare InterpLnr has no model widths


# --------------------------------------------------------------------------------------------- what the segment configurations reach
def _counts(hp, draw, lens):
    _, _, counts, nrows = interp_np.interp_plan(draw[0], draw[1], lens, hp.max_len_seg, hp.max_len_pad)
    return counts, nrows


@pytest.mark.parametrize('it', [0, 1])
def test_segment_configurations_reach_their_edges(it):
    """The draws the GPU train steps use (train_seeds), planned on the CPU: with H_segs3's three 31-frame segments no resampled slab of the
    encoders is live up to T = 128 (dead rows in every utterance of every call), with H_segs10's ten segments at least one utterance of
    each step is cut at T (counts >= T: pad_sequences' truncation, model.py:375)."""
    B = 3
    for name, check in (('H_segs3', lambda c: bool((c < 128).all())), ('H_segs10', lambda c: bool((c >= 128).any()))):
        T = TRAIN_T[name]
        hp = hparams_of(name, T)
        assert nseg(hp) == (3 if name == 'H_segs3' else 10)
        draws = draws_of(hp, train_seeds(name, B)[1] + it, B, 4)
        assert draws[0][0].shape == (B * nseg(hp),)
        counts = np.stack([_counts(hp, d, np.full(B, T))[0] for d in draws[1:]])     # the three encoder calls run with len = max_len_pad
        assert check(counts), (name, counts)
