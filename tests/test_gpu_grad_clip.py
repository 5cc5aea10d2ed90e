"""Clipping by global norm and the non-finite guard of the optimiser step (ss_set_grad_clip / ss_grad_norm / ss_grad_clip_stats), on the
GPU (pytest -m gpu).

  1  the sum-of-squares kernel against float64 numpy over the parameter elements (gaps and status slot poisoned: same bits)
  2  the clipped step against the oracle: ref_model.g3_loss / g6_loss -> backward -> torch.nn.utils.clip_grad_norm_ -> Adam
  3  engine against engine in deterministic mode: coefficient 1 is bit-identical to clipping off; a clipped step's moments are c and c^2
     times the unclipped ones; every route to the optimiser gives the same coefficient and trajectory; toggling between steps
  4  a non-finite gradient skips that step only
  5  clipped steps on guarded memory
  6  the Solver's log line

Bounds.  1e-6 on the kernel: float64 accumulation leaves the final fp32 rounding and the square root, ~6e-8 each.  1e-4 on the reported norm
and on exp_avg (TOL of tests/test_gpu_parity.py through its grad_tolerances), twice that on exp_avg_sq (quadratic in g), 2e-5 on the losses
(test_fused_train_step_against_reference_fixture), 3e-2 (grad_tolerances' loose bound) on exp_avg after three steps.  Measured values are
printed.  Nothing here provokes a device fault: the non-finite cases store inf / NaN into the caller-owned gradient arena."""
import math

import numpy as np
import pytest
import torch

from conftest import assert_same_trajectory
from oracle import interp_np, ref_model, weights as W
from oracle.gen_fixtures import draws_for, synth_batch
from tests.test_gpu_engine_containment import Bound, g3_batch, g6_batch, g3_step, g6_step
from tests.test_gpu_parity import grad_tolerances, kink_margins, kink_safe_case, stack_draws

pytestmark = pytest.mark.gpu
TOL = 1e-4
LR = 1e-4
INF = float('inf')


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


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


def fresh(E, kind, hp, B, T, wseed, precision='f32'):
    eng = E.Engine(kind, hp, B, T)
    eng.set_precision(precision)
    eng.load_weights(W.make_weights(kind, hp, wseed))
    eng.set_adam(LR, 0.9, 0.999, 1e-8, 0)
    return eng


def param_mask(eng):
    """True for the arena's parameter elements; False for the alignment gaps and the four floats of the status slot."""
    m = torch.zeros(eng.grads.numel(), dtype=torch.bool)
    for _, o, s in eng.table:
        m[o:o + int(np.prod(s))] = True
    return m


def batch_of(kind, seed, B, T):
    return g3_batch(seed, B, T) if kind == 'G3' else g6_batch(seed, B, T)


def step(eng, kind, batch, **kw):
    return g3_step(eng, batch, **kw) if kind == 'G3' else g6_step(eng, batch, **kw)


def stats(eng):
    """(norm before clipping, coefficient, steps clipped, steps skipped) of the engine, as Python numbers."""
    s = eng.grad_clip_stats().cpu()
    return float(s[0]), float(s[1]), int(s[2]), int(s[3])


def coef_of(max_norm, norm):
    """clip_grad_norm_'s coefficient in float32 arithmetic."""
    return float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))


# --------------------------------------------------------------------------------------------- 1  the kernel
@pytest.mark.parametrize('kind,B,T', [('G3', 4, 128), ('G6', 4, 192), ('G3', 64, 128)], ids=['g3_4x128', 'g6_4x192', 'g3_64x128'])
def test_grad_norm_against_float64_and_blind_to_gaps(E, kind, B, T):
    hp = W.default_hparams(max_len_pad=T)
    eng = fresh(E, kind, hp, B, T, 3)
    step(eng, kind, batch_of(kind, 11, B, T), no_adam=True)
    eng.check()
    mask = param_mask(eng)
    # the status slot; Generator_6 also has the gap behind its 257-float head bias (Generator_3's tensors all end on float4 boundaries)
    assert int((~mask).sum()) >= (4 + 3 if kind == 'G6' else 4)
    g = eng.grads.cpu().double().numpy()
    ref = float(np.sqrt(np.sum(g[mask.numpy()] ** 2)))
    assert ref > 0
    got = {}
    for gs in (1.0, 0.25):
        got[gs] = float(eng.grad_norm(gs))
        err = abs(got[gs] - gs * ref) / (gs * ref)
        print(f'[{kind} {B}x{T}] grad_norm({gs}) = {got[gs]:.9g}, float64 {gs * ref:.9g}, relative error {err:.2e}')
        assert err <= 1e-6, (gs, got[gs], gs * ref)
    # two calls: the same bits
    a, b = eng.grad_norm(1.0).clone(), eng.grad_norm(1.0).clone()
    assert torch.equal(a, b) and float(a) == got[1.0]
    # a finite poison in every alignment gap and in the status slot: not counted, the same bits (nothing else reads the arena here)
    dev_mask = mask.to(eng.grads.device)
    eng.grads[~dev_mask] = 1e3
    try:
        for gs in (1.0, 0.25):
            assert float(eng.grad_norm(gs)) == got[gs], gs
    finally:
        eng.grads[~dev_mask] = 0.0
    # clipping on: the stand-alone call still answers, and leaves the clip state alone
    eng.set_grad_clip(0.5 * ref)
    assert float(eng.grad_norm(1.0)) == got[1.0]
    assert stats(eng) == (0.0, 0.0, 0, 0)


# --------------------------------------------------------------------------------------------- 2  against the oracle
def g6_kink_margins(P, hp, mel, onehot, qidx, draws):
    ref_model.TAP = {}
    with torch.no_grad():
        ref_model.g6_loss(P, hp, mel, onehot, qidx, draws)
    tap, ref_model.TAP = ref_model.TAP, None
    return {k[5:]: v for k, v in tap.items() if k.startswith('zmin:')}


@pytest.mark.parametrize('case', [('G3', 2, 64, 9, 46, True), ('G3', 4, 128, 9, 61, False), ('G6', 4, 192, 4, 51, False)],
                         ids=['g3_2x64_kink_safe', 'g3_4x128', 'g6_4x192'])
def test_clipped_steps_against_the_oracle(E, case):
    """Three clipped steps from zero moments, max_norm = half the oracle's first-step norm (so every step clips).  A single Adam step is nearly
    invariant to the gradient's scale: the moments, not the first step's parameters, are the evidence that the coefficient was applied."""
    kind, B, T, wseed, bseed, want_safe = case
    nsteps, ncalls = 3, 4 if kind == 'G3' else 3
    hp = W.default_hparams(max_len_pad=T)
    w = W.make_weights(kind, hp, wseed)
    if kind == 'G3':
        if want_safe:
            mel, f0, emb, lens, d0 = kink_safe_case(hp, w, B, T, bseed)
        else:
            mel, f0, emb, lens = synth_batch(bseed, B, T, 64 if T <= 128 else 96)
            d0 = draws_for(bseed + 100, B, 4)
        draws = [d0] + [draws_for(bseed + 200 + k, B, ncalls) for k in range(1, nsteps)]
        margins = kink_margins(ref_model.as_params(w, False), hp, mel, f0, emb, lens, d0)

        def oracle_loss(P, d):
            return ref_model.g3_loss(P, hp, mel, f0, emb, lens.numpy(), d)[0]

        def engine_step(eng, d):
            return eng.g3_train_step(mel, f0, emb, lens, stack_draws(d))
    else:
        mel, f0, _, _ = synth_batch(bseed, B, T, 96)
        qidx = torch.from_numpy(interp_np.quantize_f0(f0[:, :, 0].numpy()))
        onehot = torch.nn.functional.one_hot(qidx, 257).float()
        draws = [draws_for(bseed + 100 + k, B, ncalls) for k in range(nsteps)]
        margins = g6_kink_margins(ref_model.as_params(w, False), hp, mel, onehot, qidx, draws[0])

        def oracle_loss(P, d):
            return ref_model.g6_loss(P, hp, mel, onehot, qidx, d)[0]

        def engine_step(eng, d):
            return eng.g6_train_step(mel, onehot, qidx, stack_draws(d))

    # the oracle: loss -> backward -> clip_grad_norm_ -> Adam.  Its unclipped first-step norm n0 sets max_norm (the gradients of the first
    # step do not depend on whether they are clipped afterwards, so n0 is read off the same backward).
    st = ref_model.TrainState(w, LR)
    plist = list(st.P.values())
    o_loss, o_norm, o_m1, o_v1 = [], [], None, None
    max_norm = None
    for k in range(nsteps):
        lo = oracle_loss(st.P, draws[k])
        st.opt.zero_grad()
        lo.backward()
        if k == 0:
            n0 = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for p in plist])))
            max_norm = 0.5 * n0
        norm = float(torch.nn.utils.clip_grad_norm_(plist, max_norm))
        assert max_norm / (norm + 1e-6) < 1.0, (k, norm, max_norm)              # every step clips
        st.opt.step()
        o_loss.append(float(lo))
        o_norm.append(norm)
        if k == 0:
            o_m1 = {n: st.opt.state[p]['exp_avg'].clone() for n, p in st.P.items()}
            o_v1 = {n: st.opt.state[p]['exp_avg_sq'].clone() for n, p in st.P.items()}
    o_m3 = {n: st.opt.state[p]['exp_avg'].clone() for n, p in st.P.items()}
    print(f'[{kind} {B}x{T}] oracle norms {o_norm}, max_norm {max_norm:.6g}')

    eng = fresh(E, kind, hp, max(8, B), T, wseed)
    eng.set_grad_clip(max_norm)
    tol = grad_tolerances(list(st.P), margins)
    if want_safe:
        assert all(t == TOL for t in tol.values())
    for k in range(nsteps):
        loss = float(engine_step(eng, draws[k]))
        eng.check()
        norm, coef, clipped, skipped = stats(eng)
        lerr = abs(loss - o_loss[k]) / o_loss[k]
        nerr = abs(norm - o_norm[k]) / o_norm[k]
        print(f'[{kind} {B}x{T} step {k}] loss {loss:.8f} (oracle {o_loss[k]:.8f}, {lerr:.2e}); norm {norm:.8g} (oracle {o_norm[k]:.8g}, {nerr:.2e}); coef {coef:.6f}')
        assert coef < 1.0 and clipped == k + 1 and skipped == 0
        assert lerr <= 2e-5, (k, loss, o_loss[k])
        if k == 0:
            assert nerr <= TOL, (norm, o_norm[0])
            mv, vv = eng.views(eng.adam_m), eng.views(eng.adam_v)
            worst_m, worst_v = ('', 0.0), ('', 0.0)
            for n in st.P:
                em, ev = rel(mv[n], o_m1[n]), rel(vv[n], o_v1[n])
                worst_m, worst_v = max(worst_m, (n, em), key=lambda x: x[1]), max(worst_v, (n, ev), key=lambda x: x[1])
                assert em < tol[n], ('exp_avg', n, em, tol[n])
                assert ev < 2 * tol[n], ('exp_avg_sq', n, ev, 2 * tol[n])
            print(f'[{kind} {B}x{T}] after step one: worst exp_avg {worst_m[0]} {worst_m[1]:.2e}, worst exp_avg_sq {worst_v[0]} {worst_v[1]:.2e}')
    mv = eng.views(eng.adam_m)
    worst = max(((n, rel(mv[n], o_m3[n])) for n in st.P), key=lambda x: x[1])
    print(f'[{kind} {B}x{T}] after step three: worst exp_avg {worst[0]} {worst[1]:.2e}')
    for n in st.P:
        assert rel(mv[n], o_m3[n]) < 3e-2, (n,)


# --------------------------------------------------------------------------------------------- 3  engine against engine
def run_steps(E, kind, hp, B, T, batches, clip, precision='f32'):
    eng = fresh(E, kind, hp, B, T, 3, precision)
    if clip is not None:
        eng.set_grad_clip(clip)
    losses = [float(step(eng, kind, b)) for b in batches]
    eng.check()
    return eng, losses


@pytest.mark.parametrize('kind,B,T', [('G3', 4, 128), ('G6', 4, 192)], ids=['g3', 'g6'])
def test_coefficient_one_is_bit_identical_to_clipping_off(E, deterministic, kind, B, T):
    """max_norm = inf and max_norm = 1e6 against clipping off, three steps: only the schedule differs (no early update of the decoder range,
    the coefficient kernel), so parameters and both moments are bit-identical."""
    hp = W.default_hparams(max_len_pad=T)
    batches = [batch_of(kind, 21 + k, B, T) for k in range(3)]
    off, l_off = run_steps(E, kind, hp, B, T, batches, None)
    for clip in (INF, 1e6):
        on, l_on = run_steps(E, kind, hp, B, T, batches, clip)
        norm, coef, clipped, skipped = stats(on)
        assert coef == 1.0 and clipped == 0 and skipped == 0 and 0 < norm < 1e6
        assert l_on == l_off, clip
        assert torch.equal(on.params, off.params) and torch.equal(on.adam_m, off.adam_m) and torch.equal(on.adam_v, off.adam_v), clip


@pytest.mark.parametrize('kind,B,T', [('G3', 4, 128), ('G6', 4, 192)], ids=['g3', 'g6'])
def test_one_clipped_step_scales_the_moments(E, deterministic, kind, B, T):
    hp = W.default_hparams(max_len_pad=T)
    batch = batch_of(kind, 31, B, T)
    off, _ = run_steps(E, kind, hp, B, T, [batch], INF)
    n0 = stats(off)[0]
    max_norm = 0.5 * n0
    on, _ = run_steps(E, kind, hp, B, T, [batch], max_norm)
    norm, c, clipped, skipped = stats(on)
    assert norm == n0 and clipped == 1 and skipped == 0
    assert abs(c - coef_of(max_norm, norm)) <= 1e-6 * c and 0.49 < c < 0.51
    m_on, m_off = on.views(on.adam_m), off.views(off.adam_m)
    v_on, v_off = on.views(on.adam_v), off.views(off.adam_v)
    for n in m_on:
        assert rel(m_on[n], c * m_off[n].double()) <= 1e-6, ('adam_m', n)
        assert rel(v_on[n], c * c * v_off[n].double()) <= 1e-6, ('adam_v', n)


def _route(E, route, hp, Tmax, batch, max_norm, precision='f32'):
    """One clipped Generator_3 step from zero moments through one route to the optimiser; returns (engine, coefficient, norm)."""
    mel, f0, emb, lens, d = batch
    eng = fresh(E, 'G3', hp, 8, Tmax, 3, precision)
    eng.set_grad_clip(max_norm)
    if route == 'fused':
        eng.g3_train_step(mel, f0, emb, lens, d)
    elif route == 'no_adam':
        eng.g3_train_step(mel, f0, emb, lens, d, no_adam=True)
        eng.adam_step()
    elif route == 'split':
        eng.g3_train_step(mel, f0, emb, lens, d, no_adam=True, split_backward=True)
        eng.train_finish(no_adam=False)
    elif route == 'bucket':
        eng.g3_train_step(mel, f0, emb, lens, d, bucket=True)
    elif route == 'dp_native':
        eng.comm_init(0, 1)
        try:
            eng.dp_train_step_native(mel, f0, emb, lens, d)
            torch.cuda.synchronize()
        finally:
            eng.lib.ss_comm_destroy(eng.h)
    else:
        raise ValueError(route)
    eng.check()
    norm, c, clipped, skipped = stats(eng)
    assert clipped == 1 and skipped == 0, route
    return eng, c, norm


def test_every_route_to_the_optimiser_clips_alike(E, deterministic):
    """The same clipped step through the fused step, SS_STEP_NO_ADAM + ss_adam_step, the split backward + ss_train_finish, SS_STEP_BUCKET
    (T = 96 on a 192-frame engine) and the native data-parallel step on a one-rank communicator."""
    B, T = 4, 96
    hp96, hp192 = W.default_hparams(max_len_pad=T), W.default_hparams(max_len_pad=192)
    mel, f0, emb, lens = synth_batch(41, B, T, T - 7)
    batch = (mel, f0, emb, lens, stack_draws(draws_for(141, B, 4)))
    probe = fresh(E, 'G3', hp96, 8, T, 3)
    g3_step(probe, batch, no_adam=True)
    max_norm = 0.5 * float(probe.grad_norm())
    base, c0, n0 = _route(E, 'fused', hp96, T, batch, max_norm)
    assert abs(c0 - coef_of(max_norm, n0)) <= 1e-6 * c0 and 0.49 < c0 < 0.51
    for route in ('no_adam', 'split', 'bucket', 'dp_native'):
        eng, c, n = _route(E, route, hp192 if route == 'bucket' else hp96, 192 if route == 'bucket' else T, batch, max_norm)
        print(f'[route {route}] coefficient {c:.8f} (fused {c0:.8f}), norm {n:.8g}')
        assert abs(c - c0) <= 1e-6 * c0, (route, c, c0)
        assert_same_trajectory(eng.params, base.params, LR, 1, route)
        assert rel(eng.adam_m, base.adam_m) <= TOL, route


def test_routes_clip_alike_in_bf16(E, deterministic):
    B, T = 4, 128
    hp = W.default_hparams(max_len_pad=T)
    batch = g3_batch(43, B, T)
    probe = fresh(E, 'G3', hp, 8, T, 3, 'bf16')
    g3_step(probe, batch, no_adam=True)
    max_norm = 0.5 * float(probe.grad_norm())
    base, c0, n0 = _route(E, 'fused', hp, T, batch, max_norm, 'bf16')
    eng, c, n = _route(E, 'no_adam', hp, T, batch, max_norm, 'bf16')
    assert abs(c0 - coef_of(max_norm, n0)) <= 1e-6 * c0 and 0.49 < c0 < 0.51
    assert abs(c - c0) <= 1e-6 * c0
    assert_same_trajectory(eng.params, base.params, LR, 1, 'bf16')


def test_toggling_between_steps_matches_fresh_engines(E, deterministic):
    """Clipping on, off, on between the fused steps of ONE engine: each step is bit-identical to the same step on a fresh engine that starts
    from the toggling engine's state and has only ever been in that step's mode (the early range's bookkeeping carries nothing over)."""
    kind, B, T = 'G3', 4, 128
    hp = W.default_hparams(max_len_pad=T)
    batches = [batch_of(kind, 51 + k, B, T) for k in range(3)]
    probe = fresh(E, kind, hp, 8, T, 3)
    step(probe, kind, batches[0], no_adam=True)
    max_norm = 0.5 * float(probe.grad_norm())
    x = fresh(E, kind, hp, 8, T, 3)
    for k, clip in enumerate((max_norm, 0.0, max_norm)):
        f = fresh(E, kind, hp, 8, T, 3)
        for name in ('params', 'adam_m', 'adam_v'):
            getattr(f, name).copy_(getattr(x, name))
        f.set_adam(LR, 0.9, 0.999, 1e-8, k)
        if clip:
            f.set_grad_clip(clip)
        x.set_grad_clip(clip)
        lx, lf = float(step(x, kind, batches[k])), float(step(f, kind, batches[k]))
        x.check()
        f.check()
        assert lx == lf, k
        if clip:
            assert stats(x) == stats(f) and stats(x)[1] < 1.0
        for name in ('params', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(x, name), getattr(f, name)), (k, name)


# --------------------------------------------------------------------------------------------- 4  non-finite gradients
@pytest.mark.parametrize('bad', [INF, float('nan')], ids=['inf', 'nan'])
def test_a_non_finite_gradient_skips_that_step_only(E, deterministic, bad):
    kind, B, T = 'G3', 4, 128
    hp = W.default_hparams(max_len_pad=T)
    b0, b1 = batch_of(kind, 61, B, T), batch_of(kind, 62, B, T)
    eng = fresh(E, kind, hp, 8, T, 3)
    eng.set_grad_clip(INF)
    step(eng, kind, b0)                                            # one good step first: non-zero moments, step counter 1
    before = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
    step(eng, kind, b1, no_adam=True)
    _, off, shape = eng.table[len(eng.table) // 2]
    eng.grads[off + 1] = bad                                       # an ordinary store into the caller-owned gradient arena
    eng.adam_step()
    torch.cuda.synchronize()
    norm, coef, clipped, skipped = stats(eng)
    assert not math.isfinite(norm) and coef == 0.0 and clipped == 0 and skipped == 1
    for t, b in zip((eng.params, eng.adam_m, eng.adam_v), before):
        assert torch.equal(t, b)
    assert eng.status() == 0
    eng.check()                                                    # per step: nothing is refused afterwards
    # the next good step equals that of an engine that never saw the bad one: the step counter did not advance
    ref = fresh(E, kind, hp, 8, T, 3)
    ref.set_grad_clip(INF)
    step(ref, kind, b0)
    la, lb = float(step(eng, kind, b1)), float(step(ref, kind, b1))
    eng.check()
    assert la == lb
    for name in ('params', 'adam_m', 'adam_v'):
        assert torch.equal(getattr(eng, name), getattr(ref, name)), name
    assert stats(eng)[3] == 1 and stats(ref)[3] == 0
    # set_grad_clip starts the counters again
    eng.set_grad_clip(INF)
    assert stats(eng) == (0.0, 0.0, 0, 0)


# --------------------------------------------------------------------------------------------- 5  containment
@pytest.mark.parametrize('kind,B,T', [('G3', 16, 128), ('G6', 32, 192)], ids=['g3', 'g6'])
def test_clipped_steps_on_guarded_memory(E, kind, B, T):
    """Guarded arenas, a NaN-pre-filled workspace of exactly ss_workspace_bytes() (tests/test_gpu_engine_containment.py Bound): the partial
    sums and the clip state live in the planned, zeroed part; nothing outside the arenas is written, nothing unwritten is read."""
    hp = W.default_hparams(max_len_pad=T)
    b = Bound(E, kind, hp, B, T)
    probe_batch = batch_of(kind, 71, B, T)
    step(b, kind, probe_batch, no_adam=True)
    max_norm = 0.5 * float(b.eng.grad_norm())
    b.check((kind, 'probe'))
    b.eng.set_grad_clip(max_norm)
    ref = fresh(E, kind, hp, B, T, {'G3': 3, 'G6': 4}[kind])
    ref.set_grad_clip(max_norm)
    la, lb = step(b, kind, probe_batch), step(ref, kind, probe_batch)
    b.check((kind, 'clipped step'))
    st_b, st_r = stats(b.eng), stats(ref)
    b.check((kind, 'stats'))
    assert st_b[2] == 1 and st_b[3] == 0 and 0.49 < st_b[1] < 0.51
    assert abs(st_b[0] - st_r[0]) <= TOL * st_r[0]
    assert abs(float(la) - float(lb)) <= TOL * abs(float(lb))
    assert_same_trajectory(b.eng.params, ref.params, LR, 1, kind)
    assert rel(b.eng.adam_m, ref.adam_m) <= TOL
    step(b, kind, batch_of(kind, 72, B, T))
    b.check((kind, 'second clipped step'))
    assert b.eng.scratch_fallbacks() == 0


# --------------------------------------------------------------------------------------------- 6  the Solver
def _solver_lines(E, tmp_path, capsys, monkeypatch, grad_clip, env=None):
    from types import SimpleNamespace
    from speechsplit_amd import data_loader, hparams as HP, solver
    hp = HP.default_hparams(batch_size=4, max_len_pad=128)
    np.random.seed(0)
    torch.manual_seed(0)
    loader = data_loader.get_loader(hp, dataset=data_loader.SyntheticUtterances(16, seed=2))
    cfg = SimpleNamespace(num_iters=3, g_lr=1e-4, beta1=0.9, beta2=0.999, resume_iters=None, use_tensorboard=False,
                          device_id=0, log_dir=str(tmp_path), sample_dir=str(tmp_path), model_save_dir=str(tmp_path),
                          log_step=1, sample_step=1000, model_save_step=1000)
    if grad_clip != 'absent':
        cfg.grad_clip = grad_clip
    if env is not None:
        monkeypatch.setenv('SS_GRAD_CLIP', env)
    else:
        monkeypatch.delenv('SS_GRAD_CLIP', raising=False)
    capsys.readouterr()
    s = solver.Solver(loader, cfg, hp)
    capsys.readouterr()
    s.train()
    out = capsys.readouterr().out
    return s, [ln for ln in out.splitlines() if ln.startswith('Elapsed [')]


def _norms(lines):
    import re
    vals = []
    for ln in lines:
        m = re.fullmatch(r'Elapsed \[[^\]]*\], Iteration \[\d+/3\], G/loss_id: \d+\.\d{8}, G/grad_norm: (\d+\.\d{8})', ln)
        assert m, ln
        vals.append(float(m.group(1)))
    return vals


def test_solver_logs_the_norm_when_clipping_is_set(E, tmp_path, capsys, monkeypatch):
    import re
    # without it: the parent's line
    s, lines = _solver_lines(E, tmp_path, capsys, monkeypatch, 'absent')
    assert len(lines) == 3 and s.grad_clip == 0.0
    for ln in lines:
        assert re.fullmatch(r'Elapsed \[[^\]]*\], Iteration \[\d+/3\], G/loss_id: \d+\.\d{8}', ln), ln
    for off in (None, 0):
        s, lines = _solver_lines(E, tmp_path, capsys, monkeypatch, off)
        assert len(lines) == 3 and all('grad_norm' not in ln for ln in lines)
    # config.grad_clip: a finite positive norm at the end of every line; the engine clips
    s, lines = _solver_lines(E, tmp_path, capsys, monkeypatch, 0.01)
    vals = _norms(lines)
    assert len(vals) == 3 and all(math.isfinite(v) and v > 0 for v in vals)
    st = stats(s.eng)
    assert st[2] == 3 and st[3] == 0 and st[1] < 1.0
    # 'inf': measured, never clipped
    s, lines = _solver_lines(E, tmp_path, capsys, monkeypatch, INF)
    assert len(_norms(lines)) == 3 and stats(s.eng)[1:] == (1.0, 0, 0)
    # SS_GRAD_CLIP when the attribute is absent; the attribute wins when it is there
    s, lines = _solver_lines(E, tmp_path, capsys, monkeypatch, 'absent', env='0.01')
    assert s.grad_clip == 0.01 and len(_norms(lines)) == 3 and stats(s.eng)[2] == 3
    s, lines = _solver_lines(E, tmp_path, capsys, monkeypatch, None, env='0.01')
    assert s.grad_clip == 0.0 and all('grad_norm' not in ln for ln in lines)
