"""Same-shape history independence (pytest -m gpu): what a call computes must not depend on what the engine ran before AT THE SAME (B, T).

Every slab of the workspace relies on zero halo rows and zero padding columns that no kernel writes; only the memset of engine.hip
geometry() establishes them, and geometry() returns early when the call arrives at the plan the engine already has.  The other history
tests (test_gpu_engine_containment.py, test_gpu_buckets_dp.py, test_gpu_frame_range.py) change the shape between history and compared
step, so there the memset always runs.  Here it never does because of the shape: every engine is created at exactly the shape it runs,
Engine(kind, hp, 6, 128) with max_len_pad = 128, no call changes B or T and none passes bucket=True.

Protocol, under ss_tune("deterministic", 1), for Generator_3 and Generator_6.  A FRESH engine has only ever been in the probe's precision
and has made no call before the probe.  The DIRTY engine (one per kind, reused) first runs a prefix at 6 x 128 on other batches, is then put
into the probe's precision and reset as test_history_independence_is_bit_exact_in_deterministic_mode resets: load_weights, Adam moments
zeroed, set_adam(step 0), zero_grads, every ss_tune knob at its default (tests/test_capi_host.py KEPT_TUNE_KEYS).  Both run the probe on
the same batch and draws; afterwards check() and scratch_fallbacks() == 0 on both.  Everything compared is compared bit for bit: == on the
loss, torch.equal on tensors.

Probes (PROBES): a fused train step in f32 and in bf16 (loss, gradient arena, parameter arena); an eval-mode forward (output); a ragged
eval-mode forward with lengths 128, 64, 8, 128, 72, 16 in f32 and in bf16 (the whole output, the zeros behind each row's end included); a
training forward + backward with every input gradient in f32 (gradient arena and each returned input gradient).
Prefixes (prefixes_of): every probe kind; a two-micro-batch accumulation cycle; a split-backward step; one step under each of the knobs the
suite toggles on its cached engines (persist, gn_gather, compact0, fwd_f16x2 + bwd_f16x2, gemm_mode, bf16_img in bf16, small_lds = 2);
two chained three-step prefixes f32 -> bf16 -> f32 and bf16 -> f32 -> bf16.
Cells: every (prefix, probe) pair with prefix != probe.  Absent, and only these: split_backward for Generator_6 (ss_g6_train_step has no
such flag), and each chained prefix with the probes of the other precision (it is probed in the mode of its last step; the switch into the
other mode is what the single-step prefixes cover).

Controls.  Reproducibility: for each probe two fresh engines agree bit for bit -- measured so for all six probes of both kinds, the bf16
ones included, so no probe needs anything weaker than bit identity.  The comparison can fail: a one written into one halo row of the
zero-haloed slab "in.f0" (inside the slab, so nothing faults) changes the train_f32 probe.

Default (non-deterministic) mode, the one people train in: at 16 x 128 an f32 step, ss_set_precision, a step of the other precision, against
a fresh engine of that precision from the same weights, with test_gpu_engine_containment.compare_step unchanged (1e-4 in f32,
test_gpu_configs.BF16_BOUNDS in bf16).

On the parent of the commit that added this file every cell whose prefix ends in the other precision than the probe was red: geometry()
did not know that the 16-bit data path lays the image buffers out differently (ss_engine::ioff)."""
import ctypes as C
import functools
import types

import pytest
import torch

from oracle import weights as W
from speechsplit_amd import _capi
from tests.test_capi_host import KEPT_TUNE_KEYS
from tests.test_gpu_engine_containment import LR, WSEED, compare_step, g3_batch, g3_step, g6_batch, g6_step, plain

pytestmark = pytest.mark.gpu
B, T = 6, 128
KINDS = ('G3', 'G6')
LENGTHS = [128, 64, 8, 128, 72, 16]
PROBES = ('train_f32', 'train_bf16', 'eval_f32', 'eval_ragged_f32', 'eval_ragged_bf16', 'input_grads_f32')
PROBE_SEED = 700
KNOBS = {'knob:persist=0': dict(persist=0), 'knob:gn_gather=0': dict(gn_gather=0), 'knob:compact0=0': dict(compact0=0),
         'knob:fwd_f16x2=0+bwd_f16x2=0': dict(fwd_f16x2=0, bwd_f16x2=0), 'knob:gemm_mode=0': dict(gemm_mode=0),
         'knob:bf16_img=0': dict(bf16_img=0), 'knob:small_lds=2': dict(small_lds=2)}
CHAINS = {'two_step:f32->bf16->f32': ('f32', 'bf16', 'f32'), 'two_step:bf16->f32->bf16': ('bf16', 'f32', 'bf16')}


def mode_of(probe):
    return 'bf16' if probe.endswith('bf16') else 'f32'


def prefixes_of(kind, probe):
    """The prefixes of the cells of one probe, in a fixed order (their position gives each its batch seeds)."""
    names = list(PROBES) + ['accum_cycle'] + (['split_backward'] if kind == 'G3' else []) + list(KNOBS) + list(CHAINS)
    return [n for n in names if n != probe and (n not in CHAINS or CHAINS[n][-1] == mode_of(probe))]


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


@pytest.fixture
def deterministic(E):
    E.tune('deterministic', 1)
    try:
        yield
    finally:
        E.tune('deterministic', 0)


HP = W.default_hparams(max_len_pad=T)


@functools.lru_cache(maxsize=None)
def train_batch(kind, seed):
    return (g3_batch if kind == 'G3' else g6_batch)(seed, B, T)


@functools.lru_cache(maxsize=None)
def forward_inputs(kind, seed):
    """(inputs of g3_forward / g6_forward without the draws, the draws, a fixed output gradient)."""
    mel, onehot, _, d3 = g6_batch(seed, B, T)
    g = torch.Generator().manual_seed(seed)
    if kind == 'G3':
        emb = torch.nn.functional.one_hot(torch.arange(B) % HP.dim_spk_emb, HP.dim_spk_emb).float()
        return (torch.cat((mel, onehot), -1), mel, emb), d3, torch.randn(B, T, HP.dim_freq, generator=g) * 0.1
    return (mel, onehot), d3, torch.randn(B, T, HP.dim_f0, generator=g) * 0.1


@functools.lru_cache(maxsize=None)
def weights(kind):
    return W.make_weights(kind, HP, WSEED[kind])


def train(kind, eng, seed, **kw):
    return float((g3_step if kind == 'G3' else g6_step)(eng, train_batch(kind, seed), **kw))


def run(E, kind, eng, call, seed):
    """One call of a probe's kind in the engine's current precision -> [(name, float or tensor copy)], what the probe compares."""
    if call.startswith('train'):
        loss = train(kind, eng, seed)
        return [('loss', loss), ('grads', eng.grads.clone()), ('params', eng.params.clone())]
    args, draws, d_out = forward_inputs(kind, seed)
    fwd, bwd = (eng.g3_forward, eng.g3_backward) if kind == 'G3' else (eng.g6_forward, eng.g6_backward)
    if call.startswith('eval'):
        return [('out', fwd(*args, lengths=LENGTHS if 'ragged' in call else None).clone())]
    assert call == 'input_grads_f32', call
    names = E.Engine.G3_INPUTS if kind == 'G3' else E.Engine.G6_INPUTS
    fwd(*args, draws, training=True)
    dx = bwd(d_out, inputs=names)
    return [('grads', eng.grads.clone())] + [('d' + n, t.clone()) for n, t in zip(names, dx)]


def run_prefix(E, kind, eng, name, seed):
    """History at 6 x 128, on batches of other seeds than the probe's.  Knobs are set back by reset()."""
    if name in PROBES:
        eng.set_precision(mode_of(name))
        run(E, kind, eng, name, seed)
    elif name == 'accum_cycle':                                    # the header's cycle of k = 2 micro-batches
        eng.set_precision('f32')
        train(kind, eng, seed, no_adam=True)
        train(kind, eng, seed + 1, accumulate=True, grad_scale=0.5)
    elif name == 'split_backward':
        eng.set_precision('f32')
        train(kind, eng, seed, no_adam=True, split_backward=True)
        eng.train_finish(no_adam=False)
    elif name in KNOBS:
        eng.set_precision('bf16' if 'bf16_img' in name else 'f32')
        for k, v in KNOBS[name].items():
            E.tune(k, v)
        train(kind, eng, seed)
    else:
        for i, mode in enumerate(CHAINS[name]):
            eng.set_precision(mode)
            train(kind, eng, seed + i)


def reset(E, kind, eng, mode):
    """Into the probe's precision, and the state a fresh engine starts from (as test_history_independence_is_bit_exact_in_deterministic_mode)."""
    if mode is not None:
        eng.set_precision(mode)
    eng.load_weights(weights(kind))
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    eng.zero_grads()
    for k, v in KEPT_TUNE_KEYS.items():
        if k != 'deterministic':
            E.tune(k, v)


def after(eng, tag):
    eng.check()
    assert eng.scratch_fallbacks() == 0, tag


def differing(a, b):
    """Names of the results that are not bit-identical."""
    assert [n for n, _ in a] == [n for n, _ in b]
    return [n for (n, x), (_, y) in zip(a, b) if not (x == y if isinstance(x, float) else torch.equal(x, y))]


def largest_difference(a, b):
    """Max-norm relative difference per result, for the assertion message only."""
    out = {}
    for (n, x), (_, y) in zip(a, b):
        x, y = torch.as_tensor(x, dtype=torch.float64).cpu(), torch.as_tensor(y, dtype=torch.float64).cpu()
        out[n] = float((x - y).abs().max() / y.abs().max().clamp_min(1e-300))
    return out


_fresh, _dirty = {}, {}


def fresh_result(E, kind, probe):
    """The probe on a fresh engine: computed once, shared by every test, never changed."""
    if (kind, probe) not in _fresh:
        eng = plain(E, kind, HP, B, T, mode_of(probe))
        res = run(E, kind, eng, probe, PROBE_SEED)
        after(eng, ('fresh', kind, probe))
        for n, x in res:
            assert bool(torch.isfinite(torch.as_tensor(x)).all()) and bool(torch.as_tensor(x).any()), ('fresh', kind, probe, n)
        _fresh[kind, probe] = res
    return _fresh[kind, probe]


def dirty_engine(E, kind):
    if kind not in _dirty:
        _dirty[kind] = plain(E, kind, HP, B, T)
    return _dirty[kind]


# --------------------------------------------------------------------------------------------- controls
@pytest.mark.parametrize('probe', PROBES)
@pytest.mark.parametrize('kind', KINDS)
def test_two_fresh_engines_agree_bit_for_bit(E, deterministic, kind, probe):
    """Without this a red cell could be run-to-run noise: two fresh engines give the same bits, in bf16 as in f32."""
    a = fresh_result(E, kind, probe)
    eng = plain(E, kind, HP, B, T, mode_of(probe))
    b = run(E, kind, eng, probe, PROBE_SEED)
    after(eng, ('second fresh', kind, probe))
    assert not differing(b, a), (kind, probe, largest_difference(b, a))


def slab(eng, name):
    """A named slab of the workspace, halo rows included, as a WRITABLE [B, T + 4, C] view (Engine.debug_buffer returns a copy)."""
    p, rows, cols = C.c_void_p(), C.c_long(), C.c_long()
    _capi.check(eng.lib.ss_debug_buffer(eng.h, name.encode(), C.byref(p), C.byref(rows), C.byref(cols)))
    assert rows.value == B * (T + 4), (name, rows.value)
    off = p.value - eng.ws.data_ptr()
    assert 0 <= off and off + 4 * rows.value * cols.value <= eng.ws.numel(), name
    return eng.ws[off:off + 4 * rows.value * cols.value].view(torch.float32).view(B, T + 4, cols.value)


@pytest.mark.parametrize('kind', KINDS)
def test_a_written_halo_row_changes_the_probe(E, deterministic, kind):
    """The comparison is not vacuous: after a train_f32 prefix and the reset (no precision switch, so nothing re-zeroes), ones in the first
    halo row of "in.f0" -- the k = 5 padding of the pitch stack's first convolution, read as fp32 -- change the train_f32 probe; the same
    engine without them does not.  The row lies inside the slab: nothing is provoked but a different result.  (An engine of its own: the
    shared dirty engine keeps its zeros.)"""
    ref = fresh_result(E, kind, 'train_f32')
    eng = plain(E, kind, HP, B, T)
    run_prefix(E, kind, eng, 'train_f32', PROBE_SEED + 1)
    reset(E, kind, eng, None)
    assert not differing(run(E, kind, eng, 'train_f32', PROBE_SEED), ref), 'an untouched engine already differs'
    reset(E, kind, eng, None)
    s = slab(eng, 'in.f0')
    assert not bool(s[:, :2].any()) and not bool(s[:, T + 2:].any())
    s[:, 0] = 1
    res = run(E, kind, eng, 'train_f32', PROBE_SEED)
    after(eng, ('written halo', kind))
    assert set(differing(res, ref)) == {'loss', 'grads', 'params'}, (kind, differing(res, ref), largest_difference(res, ref))


# --------------------------------------------------------------------------------------------- the cells
@pytest.mark.parametrize('probe', PROBES)
@pytest.mark.parametrize('kind', KINDS)
def test_probe_is_independent_of_same_shape_history(E, deterministic, kind, probe):
    """Every prefix of prefixes_of(kind, probe), then the reset, then the probe: bit-identical to the fresh engine's."""
    ref = fresh_result(E, kind, probe)
    eng = dirty_engine(E, kind)
    red = {}
    try:
        for i, prefix in enumerate(prefixes_of(kind, probe)):
            run_prefix(E, kind, eng, prefix, PROBE_SEED + 100 + 10 * i)
            reset(E, kind, eng, mode_of(probe))
            res = run(E, kind, eng, probe, PROBE_SEED)
            after(eng, (kind, prefix, probe))
            if differing(res, ref):
                red[prefix] = largest_difference(res, ref)
    finally:
        reset(E, kind, eng, 'f32')
    assert not red, f'{kind} {probe}: differs from a fresh engine after the prefixes {red}'


def test_every_cell_is_present():
    """The matrix the module docstring states: 6 probes x (5 other probes + accum_cycle + split_backward (Generator_3) + 7 knobs + the one
    chained prefix that ends in the probe's precision)."""
    for kind in KINDS:
        for probe in PROBES:
            ps = prefixes_of(kind, probe)
            assert len(ps) == len(set(ps)) == (15 if kind == 'G3' else 14) and probe not in ps, (kind, probe, ps)
            assert set(PROBES) - {probe} <= set(ps) and set(KNOBS) <= set(ps) and 'accum_cycle' in ps
            assert ('split_backward' in ps) == (kind == 'G3')
            assert [c for c in CHAINS if c in ps] == [c for c in CHAINS if c.endswith(mode_of(probe))]


# --------------------------------------------------------------------------------------------- the user-facing case, default mode
@pytest.mark.parametrize('first,then', [('f32', 'bf16'), ('bf16', 'f32')])
@pytest.mark.parametrize('kind', KINDS)
def test_precision_switch_between_steps_in_the_default_mode(E, kind, first, then):
    """16 x 128, atomic split-K (not deterministic): a step in one precision, ss_set_precision, a step in the other, against a fresh engine
    of that precision from the same weights and a fresh Adam state -- at compare_step's own bars."""
    Bu = 16
    step, mk = (g3_step, g3_batch) if kind == 'G3' else (g6_step, g6_batch)
    used, ref = plain(E, kind, HP, Bu, T, first), plain(E, kind, HP, Bu, T, then)
    step(used, mk(PROBE_SEED + 2, Bu, T))
    used.set_precision(then)
    used.load_weights(weights(kind))
    used.adam_m.zero_()
    used.adam_v.zero_()
    used.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    batch = mk(PROBE_SEED + 3, Bu, T)
    la, lb = float(step(used, batch)), float(step(ref, batch))
    for e in (used, ref):
        after(e, (kind, first, then))
    compare_step((kind, first, then), types.SimpleNamespace(eng=used), ref, la, lb, 1, bf16=then == 'bf16')


# --------------------------------------------------------------------------------------------- inside a forward / backward pair
@pytest.mark.parametrize('kind', KINDS)
def test_precision_change_discards_the_forward_in_flight(E, kind):
    """include/speechsplit_amd.h at ss_set_precision: a change between a training forward and its backward is refused (the backward finds no
    forward), setting the precision the engine already has changes nothing, and the engine goes on working after the refusal."""
    eng = plain(E, kind, HP, B, T)
    args, draws, d_out = forward_inputs(kind, PROBE_SEED)
    fwd, bwd = (eng.g3_forward, eng.g3_backward) if kind == 'G3' else (eng.g6_forward, eng.g6_backward)
    fwd(*args, draws, training=True)
    eng.set_precision('f32')                                       # unchanged: the forward stays
    bwd(d_out)
    fwd(*args, draws, training=True)
    eng.set_precision('bf16')
    with pytest.raises(RuntimeError, match='without a preceding forward'):
        bwd(d_out)
    eng.set_precision('f32')                                       # back again does not bring the forward back
    with pytest.raises(RuntimeError, match='without a preceding forward'):
        bwd(d_out)
    fwd(*args, draws, training=True)
    bwd(d_out)
    after(eng, kind)
    assert bool(torch.isfinite(eng.grads).all()) and bool(eng.grads.any())
