"""The Griffin-Lim vocoder on the GPU (csrc/vocoder.hip through the C ABI) against its float64 numpy restatement (griffinlim_ref.py, proven on
wrong stand-ins by test_griffinlim_ref_selftest.py): pytest -m gpu.  Shapes: 4, 5, 9 and 41 frames of features.npz's u1_wav and the ragged
batch [9, 4, 41, 5]; seconds in total.

Bounds.  STFT / ISTFT alone: 1e-12 of the largest element.  Griffin-Lim: per input, 100 x the disagreement of the reference's own two
transforms (numpy.fft against an explicit DFT matrix) over zero / seeded phases and momentum 0 / 0.99 at 32 iterations, measured when the
module is set up -- one factor of 10 for a third transform algorithm (radix-2 in LDS), one for fused multiply-add contraction -- capped at
1e-9 of max |x|.  Measured (MI355X; the fft-vs-dft column on the host the tests were written on):

    frames   fft vs dft   bound      GPU difference, worst of n_iter 0 / 1 / 32, momentum 0 / 0.99, zero / seeded phases
    4        1.27e-13     1.27e-11   8.51e-14
    5        6.78e-13     6.78e-11   1.23e-13
    9        1.67e-12     1.67e-10   9.95e-13
    41       3.67e-12     3.67e-10   3.94e-12

ss_op_stft 3e-16 of max |spec|, ss_op_istft 5.8e-16 and istft(stft(x)) - x 5.1e-16 of max |x|, ss_mel_to_linear 2e-16, end to end 5.9e-8 in
mel units.  Any fault of the self-test's wrong-variant list is larger than 1e-6."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import griffinlim_ref as R
from tests import guarded as G

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = 'cuda'
FRAMES = (4, 5, 9, 41)
RAGGED = [9, 4, 41, 5]
HOOK_TOL = 1e-12
NAN = float('nan')


@pytest.fixture(scope='module')
def V():
    from speechsplit_amd import vocoder
    return vocoder


@pytest.fixture(scope='module')
def lib():
    from speechsplit_amd import _capi
    return _capi.lib()


@pytest.fixture(scope='module')
def feats():
    return np.load(os.path.join(GOLD, 'features.npz'))


@pytest.fixture(scope='module')
def inputs(feats):
    """frames -> x (the slice cut to 256 (F - 1) samples), S, seeded phases, the Griffin-Lim bound"""
    out = {}
    for F in FRAMES:
        S, ph = R.parity_input(feats['u1_wav'], F)
        div = R.divergence(S, ph)
        assert div <= R.DIVERGENCE_CAP
        out[F] = dict(x=np.ascontiguousarray(feats['u1_wav'][:256 * (F - 1)]), S=S, ph=ph, div=div, bound=min(1e-9, 100.0 * div))
    return out


@functools.lru_cache(maxsize=None)
def _ref_gl_cached(key, n_iter, momentum, seeded):
    S, ph = _ref_gl_cached.inputs[key]['S'], _ref_gl_cached.inputs[key]['ph']
    return R.griffin_lim(S, n_iter, momentum, ph if seeded else None)


def ref_gl(inputs, F, n_iter, momentum, seeded):
    _ref_gl_cached.inputs = inputs
    return _ref_gl_cached(F, n_iter, momentum, seeded)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _check(lib, rc):
    assert rc == 0, lib.ss_last_error()


def _scratch(lib, B, T):
    return torch.empty(lib.ss_griffinlim_scratch_bytes(B, T), dtype=torch.uint8, device=DEV)


def gpu_stft(lib, wav, frames, T):
    """wav [B, 256 (T - 1)] -> complex128 numpy [B, T, 513]"""
    spec = torch.full((wav.shape[0], T, 513, 2), NAN, dtype=torch.float64, device=DEV)
    _check(lib, lib.ss_op_stft(_p(wav), _p(frames), wav.shape[0], T, _p(spec), _s()))
    s = spec.cpu().numpy()
    return s[..., 0] + 1j * s[..., 1]


def gpu_istft(lib, spec, frames, T):
    """spec float64 [B, T, 513, 2] -> numpy [B, 256 (T - 1)]"""
    B = spec.shape[0]
    wav = torch.full((B, 256 * (T - 1)), NAN, dtype=torch.float64, device=DEV)
    sc = _scratch(lib, B, T)
    _check(lib, lib.ss_op_istft(_p(spec), _p(frames), B, T, _p(wav), _p(sc), sc.numel(), _s()))
    return wav.cpu().numpy()


def _ri(z):
    return np.stack([z.real, z.imag], -1)


def _batch(rows, T, width, fill=NAN):
    """rows [F_b, width...] -> [B, T, width...] with `fill` behind every row's own frames"""
    out = np.full((len(rows), T) + tuple(width), fill)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


def _frames(fr):
    return torch.tensor(fr, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------- the two halves alone
@pytest.mark.parametrize('F', FRAMES)
def test_stft_matches_the_reference(lib, inputs, F):
    x = inputs[F]['x']
    ref = R.stft(x)
    got = gpu_stft(lib, _dev(x)[None], None, F)[0]
    err = R.rel_diff(got, ref)
    print(f'ss_op_stft, {F} frames: {err:.3g} of max |spec|')
    assert err <= HOOK_TOL


@pytest.mark.parametrize('F', FRAMES)
def test_istft_matches_the_reference_and_inverts_stft(lib, inputs, F):
    x = inputs[F]['x']
    spec = R.stft(x)
    got = gpu_istft(lib, _dev(_ri(spec))[None], None, F)[0]
    scale = np.abs(x).max()
    err = float(np.abs(got - R.istft(spec)).max() / scale)
    back = gpu_istft(lib, _dev(_ri(gpu_stft(lib, _dev(x)[None], None, F))), None, F)[0]
    rt = float(np.abs(back - x).max() / scale)
    print(f'ss_op_istft, {F} frames: {err:.3g} of max |x|; istft(stft(x)) - x: {rt:.3g}')
    assert err <= HOOK_TOL and rt <= HOOK_TOL


# ---------------------------------------------------------------------------------------------- Griffin-Lim parity
@pytest.mark.parametrize('F', FRAMES)
def test_griffinlim_parity(V, inputs, F):
    inp = inputs[F]
    mag, ph = _dev(inp['S'])[None], _dev(inp['ph'])[None]
    worst = 0.0
    for n_iter in (0, 1, 32):
        for momentum in R.MOMENTA:
            for seeded in (False, True):
                got = V.griffin_lim_mag(mag, ph if seeded else None, None, n_iter, momentum)[0].cpu().numpy()
                ref = ref_gl(inputs, F, n_iter, momentum, seeded)
                assert got.shape == ref.shape and np.isfinite(got).all()
                d = R.rel_diff(got, ref)
                worst = max(worst, d)
                print(f'{F} frames, n_iter {n_iter}, momentum {momentum}, {"seeded" if seeded else "zero"} phases: {d:.3g} (bound {inp["bound"]:.3g})')
                assert d <= inp['bound']
    print(f'{F} frames: fft vs dft {inp["div"]:.3g}, bound {inp["bound"]:.3g}, worst GPU difference {worst:.3g}')


# ---------------------------------------------------------------------------------------------- ragged batches, determinism
def _ragged_gl(V, inputs, n_iter, fill):
    T = max(RAGGED)
    mag = _dev(_batch([inputs[F]['S'] for F in RAGGED], T, (513,), fill))
    ph = _dev(_batch([inputs[F]['ph'] for F in RAGGED], T, (513,), fill))
    return V.griffin_lim_mag(mag, ph, _frames(RAGGED), n_iter, 0.99).cpu().numpy()


def test_ragged_batch_rows_are_the_utterances_alone(V, inputs):
    got = _ragged_gl(V, inputs, 32, NAN)                                 # NaN in every frame of mag and phase0 a row does not own
    clean = _ragged_gl(V, inputs, 32, 0.0)
    assert np.array_equal(got, clean)
    for b, F in enumerate(RAGGED):
        n = 256 * (F - 1)
        alone = V.griffin_lim_mag(_dev(inputs[F]['S'])[None], _dev(inputs[F]['ph'])[None], None, 32, 0.99)[0].cpu().numpy()
        assert np.array_equal(got[b, :n], alone), (b, F)                 # bit for bit
        assert not got[b, n:].any() and not np.signbit(got[b, n:]).any(), (b, F)
        assert R.rel_diff(got[b, :n], ref_gl(inputs, F, 32, 0.99, True)) <= inputs[F]['bound']


def test_ragged_hooks_rows_are_the_utterances_alone(lib, inputs):
    T, fr = max(RAGGED), _frames(RAGGED)
    wav = np.full((len(RAGGED), 256 * (T - 1)), NAN)
    for b, F in enumerate(RAGGED):
        wav[b, :256 * (F - 1)] = inputs[F]['x']
    spec = gpu_stft(lib, _dev(wav), fr, T)
    back = gpu_istft(lib, _dev(_batch([_ri(R.stft(inputs[F]['x'])) for F in RAGGED], T, (513, 2))), fr, T)
    for b, F in enumerate(RAGGED):
        x = inputs[F]['x']
        assert np.array_equal(spec[b, :F], gpu_stft(lib, _dev(x)[None], None, F)[0]) and not spec[b, F:].any()
        assert np.array_equal(back[b, :256 * (F - 1)], gpu_istft(lib, _dev(_ri(R.stft(x)))[None], None, F)[0]) and not back[b, 256 * (F - 1):].any()


def test_frame_counts_outside_the_contract_spoil_their_row_only(V, inputs):
    """every kernel clamps frames[b] into [4, max_frames]: rows 1 and 2 come out as they would alone whatever rows 0 and 3 claim"""
    T = 9
    S, ph = inputs[9]['S'], inputs[9]['ph']
    mag, p0 = _dev(np.stack([S] * 4)), _dev(np.stack([ph] * 4))
    got = V.griffin_lim_mag(mag, p0, _frames([-3, 9, 5, 1 << 30]), 2, 0.99).cpu().numpy()
    full = V.griffin_lim_mag(mag[:1], p0[:1], None, 2, 0.99)[0].cpu().numpy()
    five = V.griffin_lim_mag(mag[:1, :5].contiguous(), p0[:1, :5].contiguous(), None, 2, 0.99)[0].cpu().numpy()
    assert np.array_equal(got[1], full) and np.array_equal(got[3], full)          # above max_frames: max_frames
    assert np.array_equal(got[2, :1024], five) and not got[2, 1024:].any()
    assert np.isfinite(got[0]).all() and not got[0, 768:].any()                   # below 4: 4


def test_two_runs_give_the_same_bits(V, inputs):
    a, b = _ragged_gl(V, inputs, 32, NAN), _ragged_gl(V, inputs, 32, NAN)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    # a null phase0 is zero phases
    S = _dev(inputs[5]['S'])[None]
    assert np.array_equal(V.griffin_lim_mag(S, None, None, 3, 0.99).cpu().numpy(), V.griffin_lim_mag(S, torch.zeros_like(S), None, 3, 0.99).cpu().numpy())


# ---------------------------------------------------------------------------------------------- containment
CB, CT, CFR = 3, 9, [9, 4, 6]


def _guarded_scratch(lib):
    g = G.out((lib.ss_griffinlim_scratch_bytes(CB, CT) // 8,), DEV, dtype=torch.float64, offset=32, fill=0.0, name='scratch')
    assert g.t.data_ptr() % 256 == 0
    return g


def _rows(inputs, key):
    return [inputs[9][key][:F] for F in CFR]


def test_containment_stft(lib, inputs):
    wav = np.full((CB, 256 * (CT - 1)), NAN)
    for b, F in enumerate(CFR):
        wav[b, :256 * (F - 1)] = inputs[9]['x'][:256 * (F - 1)]
    gw, gf = G.inp(wav, DEV, name='wav'), G.inp(torch.tensor(CFR, dtype=torch.int32), DEV, name='frames')
    gs = G.out((CB, CT, 1026), DEV, dtype=torch.float64, name='spec')
    _check(lib, lib.ss_op_stft(_p(gw.t), _p(gf.t), CB, CT, _p(gs.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gw, gf, gs])
    got = gs.t.cpu().numpy().reshape(CB, CT, 513, 2)
    for b, F in enumerate(CFR):
        assert R.rel_diff(got[b, :F, :, 0] + 1j * got[b, :F, :, 1], R.stft(wav[b, :256 * (F - 1)])) <= HOOK_TOL and not got[b, F:].any()


def test_containment_istft(lib, inputs):
    specs = [R.stft(inputs[9]['x'][:256 * (F - 1)]) for F in CFR]
    gsp = G.inp(_batch([_ri(s) for s in specs], CT, (513, 2)).reshape(CB, CT, 1026), DEV, name='spec')
    gf = G.inp(torch.tensor(CFR, dtype=torch.int32), DEV, name='frames')
    gw, gsc = G.out((CB, 256 * (CT - 1)), DEV, dtype=torch.float64, name='wav'), _guarded_scratch(lib)
    _check(lib, lib.ss_op_istft(_p(gsp.t), _p(gf.t), CB, CT, _p(gw.t), _p(gsc.t), gsc.t.numel() * 8, _s()))
    torch.cuda.synchronize()
    G.check_all([gsp, gf, gw, gsc])
    got = gw.t.cpu().numpy()
    for b, F in enumerate(CFR):
        n = 256 * (F - 1)
        assert float(np.abs(got[b, :n] - R.istft(specs[b])).max() / np.abs(inputs[9]['x']).max()) <= HOOK_TOL and not got[b, n:].any()


def test_containment_griffinlim(lib, inputs):
    gm = G.inp(_batch(_rows(inputs, 'S'), CT, (513,)), DEV, name='mag')
    gp = G.inp(_batch(_rows(inputs, 'ph'), CT, (513,)), DEV, name='phase0')
    gf = G.inp(torch.tensor(CFR, dtype=torch.int32), DEV, name='frames')
    gw, gsc = G.out((CB, 256 * (CT - 1)), DEV, dtype=torch.float64, name='wav'), _guarded_scratch(lib)
    _check(lib, lib.ss_griffinlim(_p(gm.t), _p(gp.t), _p(gf.t), CB, CT, 2, 0.99, _p(gw.t), _p(gsc.t), gsc.t.numel() * 8, _s()))
    torch.cuda.synchronize()
    G.check_all([gm, gp, gf, gw, gsc])
    got = gw.t.cpu().numpy()
    for b, F in enumerate(CFR):
        n = 256 * (F - 1)
        ref = R.griffin_lim(inputs[9]['S'][:F], 2, 0.99, inputs[9]['ph'][:F])
        assert R.rel_diff(got[b, :n], ref) <= inputs[9]['bound'] and not got[b, n:].any()


def test_containment_mel_to_linear(lib, feats):
    inv = np.linalg.pinv(feats['mel_basis'])
    mels = [feats['u1_S'][:F] for F in CFR]
    gm = G.inp(_batch(mels, CT, (80,)).astype(np.float32), DEV, name='mel')
    gi, gf = G.inp(inv, DEV, name='inv_basis'), G.inp(torch.tensor(CFR, dtype=torch.int32), DEV, name='frames')
    go = G.out((CB, CT, 513), DEV, dtype=torch.float64, name='mag')
    _check(lib, lib.ss_mel_to_linear(_p(gm.t), _p(gi.t), _p(gf.t), CB, CT, 80, 1e-10, _p(go.t), _s()))
    torch.cuda.synchronize()
    G.check_all([gm, gi, gf, go])
    got = go.t.cpu().numpy()
    for b, F in enumerate(CFR):
        assert R.rel_diff(got[b, :F], R.mel_to_linear(mels[b], inv)) <= 1e-12 and not got[b, F:].any()


# ---------------------------------------------------------------------------------------------- mel -> linear, end to end, conversions
def test_mel_to_linear_matches_the_reference(V, feats):
    S, basis = feats['u1_S'], feats['mel_basis']
    inv = np.linalg.pinv(basis)
    got = V.mel_to_linear(S, basis).cpu().numpy()
    ref = R.mel_to_linear(S, inv)
    err = R.rel_diff(got, ref)
    print(f'ss_mel_to_linear on u1_S: {err:.3g} of max |mag| ({np.abs(ref).max():.3g}); floored elements {int((ref == 1e-10).sum())}')
    assert got.shape == (41, 513) and err <= 1e-12
    # the floor is applied: nothing below it, and it is reached where the pseudo-inverse goes negative
    assert got.min() == 1e-10 and (ref == 1e-10).any()
    hi = V.mel_to_linear(S, basis, floor=0.5).cpu().numpy()
    assert hi.min() == 0.5 and np.array_equal(hi, np.maximum(got, 0.5))


def test_end_to_end_mel_round_trip_agrees_with_numpy(V, feats):
    """griffin_lim(u1_S, 32 iterations) -> features.melspectrogram against the same pipeline in numpy: 1e-6 in mel units"""
    from speechsplit_amd import features
    S, basis = feats['u1_S'], feats['mel_basis']
    wav = V.griffin_lim(S, n_iter=32, generator=np.random.default_rng(5), mel_basis=basis)
    assert wav.dtype == np.float64 and wav.shape == (256 * 40,)
    mel = features.melspectrogram(wav, basis).cpu().numpy()
    ph = np.random.default_rng(5).uniform(-np.pi, np.pi, (41, 513))
    ref_wav = R.griffin_lim(R.mel_to_linear(S, np.linalg.pinv(np.asarray(basis, np.float64))), 32, 0.99, ph)
    ref_mel = R.melspec(ref_wav, basis)
    d = float(np.abs(mel - ref_mel).max())
    print(f'end to end: waveform {R.rel_diff(wav, ref_wav):.3g} of max |x|, mel {d:.3g}; round trip mean |mel - u1_S| {np.abs(mel - S).mean():.3g}')
    assert mel.shape == (41, 80) and d <= 1e-6


def test_result_does_not_depend_on_max_rows(V, feats):
    mels = [feats['u1_S'][:F] for F in RAGGED]
    runs = [V.griffin_lim(mels, n_iter=4, generator=np.random.default_rng(2), max_rows=r, mel_basis=feats['mel_basis']) for r in (1, 3, 16)]
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))
    assert [w.shape[0] for w in runs[0]] == [256 * (F - 1) for F in RAGGED]


def test_conversion_waveforms_names_and_lengths(gold_dir):
    from speechsplit_amd import convert
    z = np.load(os.path.join(gold_dir, 'demo_conversion.npz'))
    pairs = [[('p226_p231_u_' + c, z['out_' + c]) for c in ('R', 'F')], [('p231_p226_v_' + c, z['out_' + c][:40]) for c in ('U', 'RFU')]]
    out = convert.conversion_waveforms(pairs, n_iter=2, max_rows=3)
    assert [[n for n, _ in pair] for pair in out] == [[n for n, _ in pair] for pair in pairs]
    for pair_in, pair_out in zip(pairs, out):
        for (_, mel), (_, wav) in zip(pair_in, pair_out):
            assert wav.dtype == np.float64 and wav.shape == (256 * (mel.shape[0] - 1),) and np.isfinite(wav).all()
    flat = convert.conversion_waveforms(pairs[0], n_iter=2)
    assert [n for n, _ in flat] == [n for n, _ in pairs[0]] and [w.shape[0] for _, w in flat] == [256 * 104, 256 * 134]
