"""Refused calls leave no trace (pytest -m gpu): an engine that is sent every refusal reachable on a BOUND engine between the steps of a short
training run ends where an engine that never saw them ends -- same losses, same accumulation count, same parameters -- and nothing the
refused calls were given is written.  The smallest shapes the engine takes (B = 2, T = max_frames = max_len_pad = 8), both generators, both
precisions, SS_STEP_BUCKET off and on, and with the engine on its own main stream (ss_tune("own_streams", 1)), where a call's stream scope
records an event pair on the caller's stream and so must not be opened by a call that is refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import interp_np, weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from conftest import assert_same_trajectory
from speechsplit_amd import _capi

pytestmark = pytest.mark.gpu
B, T, LR, STEPS = 2, 8, 1e-4, 3
HP = W.default_hparams(max_len_pad=T)
_WEIGHTS = {}


@pytest.fixture(scope='module')
def E():
    from speechsplit_amd import engine
    return engine


def weights(kind):
    if kind not in _WEIGHTS:
        _WEIGHTS[kind] = W.make_weights(kind, HP, 3 if kind == 'G3' else 4)
    return _WEIGHTS[kind]


def batch(kind, it):
    """(arguments of the kind's train step, draws) of step `it`"""
    mel, f0, emb, lens = synth_batch(800 + it, B, T, T)
    draws = draws_for(900 + it, B, 4 if kind == 'G3' else 3)
    draws = (np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws]))
    if kind == 'G3':
        return (mel, f0, emb, lens), draws
    qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
    return (mel, torch.nn.functional.one_hot(qidx, 257).float(), qidx), draws


def make(E, kind, precision):
    eng = E.Engine(kind, HP, B, T)
    eng.load_weights(weights(kind))
    eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    eng.set_precision(precision)
    return eng


def refusals(E, eng, other, kind, p, stepped):
    """[(label, call, entry point named in the message, word in the message)]: every refusal reachable on this bound engine now"""
    lib, h, s, z = eng.lib, eng.h, E._stream(), None
    g3 = kind == 'G3'
    if g3:
        fwd_name, step_name, dec_name = 'ss_g3_forward', 'ss_g3_train_step', 'ss_g3_decode_backward'
        fwd = lambda b=B, t=T, x=p, e=h: lib.ss_g3_forward(e, x, p, p, z, z, b, t, 0, p, s)
        step = lambda b=B, t=T, flags=0, x=p: lib.ss_g3_train_step(h, x, p, p, p, p, p, b, t, 1.0, flags, p, s)
        dec_bwd = lambda d=p, flags=0: lib.ss_g3_decode_backward(h, d, z, z, z, z, flags, s)
        bwd = lambda: lib.ss_g3_backward(h, p, s)
    else:
        fwd_name, step_name, dec_name = 'ss_g6_forward', 'ss_g6_train_step', 'ss_g6_decode_backward'
        fwd = lambda b=B, t=T, x=p, e=h: lib.ss_g6_forward(e, x, p, z, z, b, t, 0, p, s)
        step = lambda b=B, t=T, flags=0, x=p: lib.ss_g6_train_step(h, x, p, p, p, p, b, t, 1.0, flags, p, s)
        dec_bwd = lambda d=p, flags=0: lib.ss_g6_decode_backward(h, d, z, z, flags, s)
        bwd = lambda: lib.ss_g6_backward(h, p, s)
    bucket = _capi.SS_STEP_BUCKET
    out = [('wrong kind', lambda: fwd(e=other), fwd_name, 'Generator_3' if g3 else 'Generator_6'),
           ('null input', lambda: fwd(x=z), fwd_name, 'null pointer'),
           ('B = 0', lambda: fwd(b=0), fwd_name, 'batch'),
           ('B = max_batch + 1', lambda: fwd(b=B + 1), fwd_name, 'batch'),
           ('T = 12', lambda: fwd(t=12), fwd_name, 'multiple'),
           ('T = 16', lambda: fwd(t=16), fwd_name, fwd_name),              # eval mode: above max_frames, and the plan does not fit the workspace
           ('step: null input', lambda: step(x=z), step_name, 'null pointer'),
           ('step: B = 0', lambda: step(b=0), step_name, 'batch'),
           ('step: B = 0, bucket', lambda: step(b=0, flags=bucket), step_name, 'batch'),
           ('step: B = max_batch + 1', lambda: step(b=B + 1), step_name, 'batch'),
           ('step: T = 12', lambda: step(t=12), step_name, 'max_frames'),
           ('step: T = 16', lambda: step(t=16), step_name, 'max_frames'),
           ('step: T = 12, bucket', lambda: step(t=12, flags=bucket), step_name, 'SS_STEP_BUCKET'),
           ('step: T = 16, bucket', lambda: step(t=16, flags=bucket), step_name, 'max_frames'),
           ('step: unknown flag', lambda: step(flags=32), step_name, 'flags'),
           ('decode backward: flag outside the set', lambda: dec_bwd(flags=_capi.SS_STEP_NO_ADAM), dec_name, 'flags'),
           ('decode backward: null d_out', lambda: dec_bwd(d=z), dec_name, 'null pointer'),
           ('nothing to wait for', lambda: lib.ss_wait_decoder_grads(h, s), 'ss_wait_decoder_grads', 'without a preceding')]
    if stepped:
        out.append(('decode backward after a full forward', dec_bwd, dec_name, 'full forward'))
    else:
        out += [('backward without a forward', bwd, 'backward', 'without a preceding forward'),
                ('decode backward without a forward', dec_bwd, dec_name, 'without a preceding'),
                ('train_finish with nothing pending', lambda: lib.ss_train_finish(h, 1.0, _capi.SS_STEP_NO_ADAM, s), 'ss_train_finish', 'without a preceding')]
    return out


def run(E, kind, precision, bucket, refuse):
    eng = make(E, kind, precision)
    # an engine of the other kind for the wrong-kind refusal: the kind is looked at before the binding, so it need not be bound
    other = eng.lib.ss_create(6 if kind == 'G3' else 3, C.byref(_capi.hparams_struct(HP)), B, T) if refuse else None
    buf = torch.full((B * 16 * 512,), float('nan'), device='cuda')           # what every refused call is given as inputs, outputs and loss
    p = C.c_void_p(buf.data_ptr())
    losses, counts = [], []
    for it in range(STEPS + 1):
        if refuse:
            torch.cuda.synchronize()
            for label, call, name, word in refusals(E, eng, other, kind, p, stepped=it > 0):
                rc = call()
                msg = eng.lib.ss_last_error().decode()
                assert rc != 0 and name in msg and word in msg, (label, rc, msg)
        if it == STEPS:
            break
        args, draws = batch(kind, it)
        loss = (eng.g3_train_step if kind == 'G3' else eng.g6_train_step)(*args, draws, bucket=bucket)
        losses.append(float(loss))
        counts.append(eng.grad_accum_count)
    eng.check()
    if refuse:
        eng.lib.ss_destroy(other)
        assert bool(torch.isnan(buf).all())                                 # nothing was enqueued on what the refused calls were given
    return losses, counts, eng.params.clone()


def compare(E, kind, precision, bucket):
    """Both runs under ss_tune("deterministic", 1), where two identical runs on fresh engines give the same bits (tests/test_gpu_robustness.py):
    the losses are then EQUAL step by step and the parameters bit-identical, on top of the standing trajectory bound."""
    E.tune('deterministic', 1)
    try:
        got, ref = run(E, kind, precision, bucket, True), run(E, kind, precision, bucket, False)
    finally:
        E.tune('deterministic', 0)
    print(f'[{kind} {precision} bucket={bucket}] losses with refusals {got[0]}  without {ref[0]}')
    assert got[1] == ref[1] == [1] * STEPS                                   # each step cleared the arena and counted one backward
    assert all(np.isfinite(a) for a in got[0]) and got[0] == ref[0], (got[0], ref[0])
    assert_same_trajectory(got[2], ref[2], LR, STEPS, f'{kind} {precision} bucket={bucket}')
    assert torch.equal(got[2], ref[2])


@pytest.mark.parametrize('bucket', [False, True], ids=['full', 'bucket'])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_refused_calls_leave_no_trace(E, kind, precision, bucket):
    compare(E, kind, precision, bucket)


@pytest.mark.parametrize('kind', ['G3', 'G6'])
def test_refused_calls_leave_no_trace_on_own_streams(E, kind):
    """own_streams is read by ss_bind: the engines of this test are created under it"""
    E.tune('own_streams', 1)
    try:
        compare(E, kind, 'f32', False)
    finally:
        E.tune('own_streams', 0)
